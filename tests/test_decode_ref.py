"""CPU: the decode reference (tests/decode_ref.py) and the synthetic decoder weights are pinned to the fixtures made
from transformers ``MimiModel.decode`` (tests/golden/make_decode_golden.py); plus the host-side pieces of the decode
path that need no GPU (length math, ``str_to_audio``'s reshaping, the up-conv weight re-layout)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_ref
from mimi_hip import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_TOL = 1e-5  # another host's BLAS (tests/test_oracle_golden.py uses the same bound for its stage tensors)


@pytest.fixture(scope="module")
def dgolden():
    with np.load(os.path.join(GOLDEN, "decode.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "decode_meta.json")) as f:
        meta = json.load(f)
    return arrays, meta


@pytest.fixture(scope="module")
def full_sd(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return decode_ref.as_tensors(sd)


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check(got, ref, what):
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):  # bit-equal on the CPU that made the fixtures
        return
    err = rel_err(got, ref)
    assert err < REL_TOL, (what, err)


def test_decoder_weights_reproduce_fixture_checkpoint(dgolden, golden, state_dict):
    _, meta = dgolden
    assert synthetic.state_dict_sha256(synthetic.make_decoder_state_dict(seed=0)) == meta["state_dict_sha256"]
    # make_state_dict is untouched: the encode fixtures' hash still holds
    assert synthetic.state_dict_sha256(state_dict) == golden[1]["weights_sha256"] == meta["encode_state_dict_sha256"]


def test_decoder_state_dict_names_and_shapes():
    sd = synthetic.make_decoder_state_dict(seed=0)
    assert sd["decoder.layers.0.conv.weight"].shape == (1024, 512, 7)
    for idx, shape in ((2, (1024, 512, 16)), (5, (512, 256, 12)), (8, (256, 128, 10)), (11, (128, 64, 8))):
        assert sd[f"decoder.layers.{idx}.conv.weight"].shape == shape
        assert sd[f"decoder.layers.{idx}.conv.bias"].shape == (shape[1],)
    for idx, c in ((3, 512), (6, 256), (9, 128), (12, 64)):
        assert sd[f"decoder.layers.{idx}.block.1.conv.weight"].shape == (c // 2, c, 3)
        assert sd[f"decoder.layers.{idx}.block.3.conv.weight"].shape == (c, c // 2, 1)
    assert sd["decoder.layers.14.conv.weight"].shape == (1, 64, 3)
    assert sd["upsample.conv.weight"].shape == (512, 1, 4)
    for q in ("semantic", "acoustic"):
        assert sd[f"quantizer.{q}_residual_vector_quantizer.output_proj.weight"].shape == (512, 256, 1)
    per_layer = [k for k in sd if k.startswith("decoder_transformer.layers.3.")]
    assert len(per_layer) == 12
    assert all(v.dtype == np.float32 for v in sd.values())


@pytest.mark.parametrize("T", [1, 2, 3, 13])
def test_decode_ref_matches_fixture(dgolden, full_sd, T):
    arrays, meta = dgolden
    for K in meta["ks"]:
        codes = torch.from_numpy(arrays[f"codes_T{T}"].astype(np.int64))[None, :K]
        y = decode_ref.decode(codes, full_sd)
        assert y.shape == (1, 1, 1920 * T)
        check(y[0, 0], arrays[f"wave_T{T}_K{K}"], f"T={T} K={K}")


def test_decode_ref_random_codes_and_taps(dgolden, full_sd):
    arrays, _ = dgolden
    y = decode_ref.decode(torch.from_numpy(arrays["codes_rand"].astype(np.int64))[None], full_sd)
    check(y[0, 0], arrays["wave_rand"], "random codes")
    taps = {}
    decode_ref.decode(torch.from_numpy(arrays["codes_T13"].astype(np.int64))[None, :8], full_sd, taps=taps)
    seen = set()
    for key, ref in arrays.items():
        if not key.startswith("tap_"):
            continue
        name, sub = key[len("tap_"):].rsplit("_sub", 1)
        check(taps[name][0][..., ::int(sub)], ref, name)
        seen.add(name)
    assert seen == set(decode_ref.TAP_NAMES)


def test_decode_ref_banded_window_fixture(dgolden, full_sd):
    """T = 129: 258 transformer frames, the reference's explicit sliding-window mask."""
    arrays, meta = dgolden
    T, sub = meta["long_frames"], meta["long_sub"]
    y = decode_ref.decode(torch.from_numpy(arrays[f"codes_T{T}"].astype(np.int64))[None], full_sd)
    assert y.shape == (1, 1, 1920 * T)
    check(y[0, 0, ::sub], arrays[f"wave_T{T}_K8_sub{sub}"], "T=129")


def test_decoded_length():
    from mimi_hip import _lib
    lib = _lib.load()
    for T in (0, 1, 2, 13, 125, 129, 100000):
        assert lib.mimi_decoded_length(T) == 1920 * T == decode_ref.decoded_length(T)
    assert lib.mimi_decoded_length(-1) == -1
    cfg = _lib.default_config()
    assert lib.mimi_decoded_length_cfg(ctypes.byref(cfg), 7) == 1920 * 7


def test_causal_prefix_property(dgolden, full_sd):
    """New codes in frame f leave samples [0, 1920 f) as they were (every conv, the upsample and the attention are
    causal): bit-identical where the fixtures were made, else within the cross-host bound."""
    arrays, _ = dgolden
    codes = torch.from_numpy(arrays["codes_T13"].astype(np.int64))[None, :8]
    y = decode_ref.decode(codes, full_sd)
    for f in (1, 6, 12):
        c2 = codes.clone()
        c2[:, :, f] = (c2[:, :, f] + 977) % 2048
        y2 = decode_ref.decode(c2, full_sd)
        n = 1920 * f
        check(y2[..., :n], y[..., :n], f"prefix of frame {f}")
        assert not torch.equal(y2[..., n:], y[..., n:])


def test_padding_mask_truncates(dgolden, full_sd):
    arrays, _ = dgolden
    codes = torch.from_numpy(arrays["codes_T2"].astype(np.int64))[None, :8]
    y = decode_ref.decode(codes, full_sd)
    yt = decode_ref.decode(codes, full_sd, padding_mask=torch.ones(1, 1, 3000))
    assert yt.shape[-1] == 3000 and torch.equal(yt, y[..., :3000])
    assert decode_ref.decode(codes, full_sd, padding_mask=torch.ones(1, 1, 5000)).shape[-1] == 3840


def test_str_to_audio_reshapes_like_the_reference(dgolden):
    """chars -> codes [8, T] -> model.decode(codes [1, 8, T] on `device`).audio_values[0] -> numpy."""
    from mimi_hip import codes as codes_mod
    from mimi_hip import str_to_audio
    arrays, _ = dgolden
    c8 = arrays["codes_T13"][:8].astype(np.int64)
    s = codes_mod.codes_to_chars(c8, codebook_size=2048)
    seen = {}

    class Out:
        def __init__(self, v):
            self.audio_values = v

    class Stub:
        def decode(self, codes):
            seen["codes"] = codes
            return Out(torch.arange(2 * 1 * 5, dtype=torch.float32).view(2, 1, 5))

    out = str_to_audio(s, Stub(), "cpu")
    assert tuple(seen["codes"].shape) == (1, 8, 13) and seen["codes"].dtype == torch.int64
    assert np.array_equal(seen["codes"][0].numpy(), c8)
    assert isinstance(out, np.ndarray) and out.shape == (1, 5) and np.array_equal(out[0], np.arange(5))


@pytest.mark.parametrize("r", [4, 5, 6, 8])
def test_upconv_relayout_is_conv_transpose(r):
    """The engine's weight re-layout (mimi_upconv_relayout, what mimi_finalize applies) turns the causal transposed
    conv into a causal k = 2 conv with r * Cout phase-major channels: checked against conv_transpose1d + trim."""
    from mimi_hip import _lib
    lib = _lib.load()
    cin, cout, T = 8, 8, 7
    g = torch.Generator().manual_seed(r)
    w = torch.randn(cin, cout, 2 * r, generator=g)
    b = torch.randn(cout, generator=g)
    x = torch.randn(1, cin, T, generator=g)
    ref = decode_ref.conv_transpose1d_causal(x, w, b, stride=r)                      # [1, cout, T r]
    wn = np.ascontiguousarray(w.numpy())
    out = np.empty((r * cout, 2 * cin), dtype=np.float32)
    assert lib.mimi_upconv_relayout(wn.ctypes.data, cin, cout, r, out.ctypes.data) == 0
    wk2 = torch.from_numpy(out).view(r * cout, 2, cin).permute(0, 2, 1).contiguous()   # conv1d weight [N][cin][2]
    y = F.conv1d(F.pad(x, (1, 0)), wk2, b.repeat(r))                                  # [1, r cout, T]
    y = y.view(1, r, cout, T).permute(0, 2, 3, 1).reshape(1, cout, T * r)             # [t r + p][co]
    assert y.shape == ref.shape
    assert float((y - ref).abs().max()) < 1e-5 * float(ref.abs().max())


def test_decode_before_enable_is_a_state_error_without_gpu_work():
    """mimi_enable_decode after finalize / decode entry points on a NULL engine fail cleanly (host-only checks)."""
    from mimi_hip import _lib
    lib = _lib.load()
    assert lib.mimi_enable_decode(None) == 1
    assert lib.mimi_decode(None, None, 1, 1, 1, None, None) == 1
    assert lib.mimi_rvq_decode(None, None, 1, 1, None, None) == 1
    assert lib.mimi_decode_workspace_bytes(None, 1, 1) == -1
