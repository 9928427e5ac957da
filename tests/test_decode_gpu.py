"""GPU parity of the decode path (codes -> waveform) against the fixtures made from transformers ``MimiModel.decode``
(tests/golden/decode.npz) and the on-box reference (tests/decode_ref.py).

Metric and tolerance are the project's own (tests/test_gpu_parity.py): ``rel_err`` = max-abs error over max-abs value,
``ACT_TOL`` = 1e-4.  Decode runs the fp32-MFMA GEMMs whatever the engine's precision mode.  Measured values go to
``parity_log`` (the session's parity_report.json).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_ref
from mimi_hip import synthetic

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dgolden():
    with np.load(os.path.join(GOLDEN, "decode.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "decode_meta.json")) as f:
        meta = json.load(f)
    return arrays, meta


@pytest.fixture(scope="module")
def full_np(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return sd


@pytest.fixture(scope="module")
def full_sd(full_np):
    return decode_ref.as_tensors(full_np)


@pytest.fixture(scope="module")
def dec(full_np):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(full_np, device="cuda:0", decode=True)


@pytest.fixture(scope="module")
def ref_cache(full_sd):
    """On-box reference decodes, computed once per code tensor and shared."""
    cache = {}

    def get(codes, taps=False):
        key = (tuple(codes.shape), codes.numpy().tobytes(), taps)
        if key not in cache:
            t = {} if taps else None
            y = decode_ref.decode(codes, full_sd, taps=t)
            cache[key] = (y, t)
        return cache[key]
    return get


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def log(parity_log, test, **kw):
    rec = {"test": test}
    rec.update(kw)
    parity_log.append(rec)
    print(json.dumps(rec))


def fixture_codes(arrays, T, K):
    return torch.from_numpy(arrays[f"codes_T{T}"].astype(np.int64))[None, :K]


def speech_codes(T, K, index, state_dict):
    """Codes a user would hold: the oracle's encode of a speech-like clip of T frames."""
    from oracle import mimi_ref
    x = synthetic.speech_like(1920 * T, 23, index)
    return mimi_ref.encode(torch.from_numpy(x)[None, None], state_dict, K)


# ---- end to end against the fixtures --------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8, 32])
@pytest.mark.parametrize("T", [1, 2, 3, 13])
def test_decode_matches_fixture(dec, dgolden, parity_log, T, K):
    """T = 1: only padding to the left in every conv, the depthwise upsample and the four up-convs; T = 2, 3: the first
    frames where x[t - 1] is real."""
    arrays, _ = dgolden
    out = dec.decode(fixture_codes(arrays, T, K))
    y = out.audio_values
    assert y.shape == (1, 1, 1920 * T) and y.dtype == torch.float32 and y.is_cuda
    assert out[0] is y and len(out) == 1
    err = rel_err(y[0, 0].cpu().numpy(), arrays[f"wave_T{T}_K{K}"])
    log(parity_log, f"decode_fixture_T{T}_K{K}", rel_err=err)
    assert err < ACT_TOL, err


def test_decode_random_codes_fixture(dec, dgolden, parity_log):
    arrays, _ = dgolden
    y = dec.decode(torch.from_numpy(arrays["codes_rand"].astype(np.int32))[None]).audio_values  # int32 input
    err = rel_err(y[0, 0].cpu().numpy(), arrays["wave_rand"])
    log(parity_log, "decode_fixture_random_codes", rel_err=err)
    assert err < ACT_TOL, err


def test_decode_stage_taps_match_fixture(dec, dgolden, parity_log):
    """Every stage of T = 13, K = 8 against the fixture: localises a wrong layer, phase order or tap swap in the
    up-conv re-layout.  (Fails on an engine without decode: there is no decode to tap.)"""
    arrays, _ = dgolden
    dec.set_taps(True)
    try:
        dec.decode(fixture_codes(arrays, 13, 8))
        errs = {}
        for key, ref in arrays.items():
            if not key.startswith("tap_"):
                continue
            name, sub = key[len("tap_"):].rsplit("_sub", 1)
            ref_t = torch.from_numpy(ref)
            if name.startswith("dres"):  # the fused block stores ELU(x + block(x)): the tap is that tensor
                tap, ref_t = dec.get_tap(name + "_elu"), F.elu(ref_t)
            else:
                tap = dec.get_tap(name)
            assert tap.shape[0] == 1
            got = tap[0].T[..., ::int(sub)]  # [time][channels] -> channel-first, subsampled as the fixture
            assert got.shape == tuple(ref_t.shape), (name, got.shape, ref_t.shape)
            errs[name] = rel_err(got, ref_t.numpy())
    finally:
        dec.set_taps(False)
    log(parity_log, "decode_stage_taps_T13_K8", rel_err=max(errs.values()), per_stage=errs)
    assert set(errs) == set(decode_ref.TAP_NAMES)
    for name, err in errs.items():
        assert err < ACT_TOL, (name, err, errs)


# ---- attention regimes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [125, 126, 129])
def test_decode_attention_regimes(dec, dgolden, state_dict, ref_cache, parity_log, T):
    """2T = 250 (the window exactly), 252 (mask active, still the <= 256-frame kernel), 258 (banded kernel; also pinned
    by the fixture)."""
    arrays, meta = dgolden
    codes = fixture_codes(arrays, 129, 8) if T == 129 else \
        torch.from_numpy(np.random.default_rng(T).integers(0, 2048, (1, 8, T)))
    y = dec.decode(codes).audio_values[0, 0].cpu().numpy()
    ref = ref_cache(codes)[0][0, 0].numpy()
    err = rel_err(y, ref)
    rec = {"rel_err": err}
    if T == 129:
        sub = meta["long_sub"]
        rec["rel_err_fixture"] = rel_err(y[::sub], arrays[f"wave_T129_K8_sub{sub}"])
    log(parity_log, f"decode_attention_T{T}", **rec)
    assert err < ACT_TOL, err
    assert rec.get("rel_err_fixture", 0.0) < ACT_TOL, rec


# ---- quantizer alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 32])
def test_dequantize_matches_reference(dec, dgolden, full_sd, parity_log, K):
    """K = 1: zero acoustic half; K = 2: the first acoustic level."""
    arrays, _ = dgolden
    codes = fixture_codes(arrays, 13, K)
    q = dec.dequantize(codes)
    assert q.shape == (1, 512, 13)
    ref = decode_ref.quantizer_decode(codes, full_sd, decode_ref.RefConfig())
    err = rel_err(q.cpu().numpy(), ref.numpy())
    log(parity_log, f"dequantize_K{K}", rel_err=err)
    assert err < ACT_TOL, err


# ---- batches --------------------------------------------------------------------------------------------------------
def test_batch_items_bitwise_equal_to_alone(dec, dgolden, state_dict):
    arrays, _ = dgolden
    items = [fixture_codes(arrays, 13, 8), speech_codes(13, 8, 1, state_dict), speech_codes(13, 8, 2, state_dict)]
    assert not torch.equal(items[0], items[1]) and not torch.equal(items[1], items[2])
    yb = dec.decode(torch.cat(items)).audio_values
    assert yb.shape == (3, 1, 1920 * 13)
    for i, c in enumerate(items):
        assert torch.equal(yb[i], dec.decode(c).audio_values[0]), i


def test_padded_batch_causality(dec, dgolden, ref_cache, parity_log):
    """Items of 5 and 13 frames padded to 13 with code 0: the short item's own 1920 * 5 samples are its own decode's."""
    arrays, _ = dgolden
    short = fixture_codes(arrays, 13, 8)[:, :, :5].clone()
    padded = torch.zeros(1, 8, 13, dtype=torch.int64)
    padded[:, :, :5] = short
    yb = dec.decode(torch.cat([padded, fixture_codes(arrays, 13, 8)])).audio_values
    ref = ref_cache(short)[0][0, 0].numpy()
    err = rel_err(yb[0, 0, :1920 * 5].cpu().numpy(), ref)
    log(parity_log, "decode_padded_batch_short_item", rel_err=err)
    assert err < ACT_TOL, err


def test_decode_is_deterministic(dec, dgolden):
    arrays, _ = dgolden
    c = fixture_codes(arrays, 13, 32)
    assert torch.equal(dec.decode(c).audio_values, dec.decode(c).audio_values)


def test_padding_mask_truncates(dec, dgolden):
    arrays, _ = dgolden
    c = fixture_codes(arrays, 2, 8)
    full = dec.decode(c).audio_values
    cut = dec.decode(c, padding_mask=torch.ones(1, 1, 3000)).audio_values
    assert cut.shape == (1, 1, 3000) and torch.equal(cut, full[..., :3000])
    assert dec.decode(c, padding_mask=torch.ones(1, 1, 9999)).audio_values.shape == (1, 1, 3840)
    assert isinstance(dec.decode(c, return_dict=False), tuple)


# ---- round trip through the public functions ------------------------------------------------------------------------
def test_str_round_trip(dec):
    from mimi_hip import audio_to_str, str_to_audio
    x = synthetic.speech_like(1920 * 5, 31, 0)
    s = audio_to_str(x, dec, "cuda:0")
    assert len(s) == 8 * 5
    y = str_to_audio(s, dec, "cuda:0")
    assert isinstance(y, np.ndarray) and y.shape == (1, 1920 * 5) and y.dtype == np.float32
    codes = dec.encode(torch.from_numpy(x)[None, None].cuda()).audio_codes[:, :8]
    assert np.array_equal(y, dec.decode(codes).audio_values[0].cpu().numpy())


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_encode_only_model_refuses_decode(state_dict, dgolden):
    from mimi_hip.model import MimiHipModel
    arrays, _ = dgolden
    m = MimiHipModel(state_dict, device="cuda:0")
    with pytest.raises(RuntimeError, match="decode=True"):
        m.decode(fixture_codes(arrays, 1, 8))
    with pytest.raises(RuntimeError, match="decode=True"):
        m.dequantize(fixture_codes(arrays, 1, 8))
    # the C entry itself: MIMI_ERR_STATE
    assert m._lib.mimi_decode(m._h, None, 1, 1, 1, None, None) == 7
    m.close()


def test_too_many_quantizers(dec):
    with pytest.raises(ValueError):
        dec.decode(torch.zeros(1, 33, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        dec.decode(torch.zeros(1, 0, 2, dtype=torch.int64))


@pytest.mark.parametrize("bad", [2048, -1])
def test_out_of_range_code_is_refused_and_engine_survives(dec, dgolden, bad):
    """The kernel checks a code against [0, codebook_size) before it forms an address (decode.hip rvq_decode_kernel:
    out-of-range -> flag + row 0), so this is an error return, never an out-of-bounds read."""
    arrays, _ = dgolden
    good = fixture_codes(arrays, 1, 1)
    before = dec.decode(good).audio_values.clone()
    with pytest.raises(ValueError, match="codebook_size"):
        dec.decode(torch.full((1, 1, 1), bad, dtype=torch.int64))
    with pytest.raises(ValueError, match="codebook_size"):
        dec.dequantize(torch.full((1, 1, 1), bad, dtype=torch.int64))
    assert torch.equal(dec.decode(good).audio_values, before)


# ---- encode untouched -----------------------------------------------------------------------------------------------
def test_encode_unchanged_on_a_decode_engine(dec, dgolden, state_dict, golden):
    from mimi_hip.model import MimiHipModel
    arrays, _ = dgolden
    _, gmeta = golden
    L = 240000
    x = torch.from_numpy(synthetic.speech_like(L, gmeta["audio_seed"], gmeta["lengths"].index(L)))[None, None].cuda()
    plain = MimiHipModel(state_dict, device="cuda:0")
    want = plain.encode(x).audio_codes
    plain.close()
    assert torch.equal(dec.encode(x).audio_codes, want)
    dec.decode(fixture_codes(arrays, 13, 8))
    assert torch.equal(dec.encode(x).audio_codes, want)


# ---- the C ABI without Python glue ----------------------------------------------------------------------------------
def write_checkpoint(sd, directory, drop=None):
    """An HF-layout checkpoint directory (model.safetensors + config.json) with the FULL decoder half."""
    import shutil

    from safetensors.numpy import save_file
    os.makedirs(directory, exist_ok=True)
    tensors = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items() if k != drop}
    save_file(tensors, os.path.join(directory, "model.safetensors"), metadata={"format": "pt"})
    shutil.copy(os.path.join(GOLDEN, "mimi_config.json"), os.path.join(directory, "config.json"))
    return directory


def test_c_abi_create_from_dir_flags(dec, dgolden, full_np, tmp_path):
    from mimi_hip import _lib
    lib = _lib.load()
    arrays, _ = dgolden
    codes = fixture_codes(arrays, 13, 8)
    want = dec.decode(codes).audio_values[0, 0]
    d = write_checkpoint(full_np, str(tmp_path / "full"))
    h = ctypes.c_void_p()
    assert lib.mimi_create_from_dir_flags(d.encode(), 0, _lib.CREATE_DECODE, ctypes.byref(h)) == 0, lib.mimi_last_error()
    try:
        c32 = codes.to(torch.int32).cuda().contiguous()
        n = lib.mimi_decoded_length(13)
        out = torch.empty(n, dtype=torch.float32, device="cuda:0")
        assert lib.mimi_decode_workspace_bytes(h, 1, 13) > 0
        torch.cuda.synchronize()
        assert lib.mimi_decode(h, ctypes.c_void_p(c32.data_ptr()), 1, 13, 8, ctypes.c_void_p(out.data_ptr()), None) == 0, \
            lib.mimi_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    finally:
        lib.mimi_destroy(h)
    # flags 0: the same directory loads and encodes as an encode-only engine (decode: MIMI_ERR_STATE)
    h = ctypes.c_void_p()
    assert lib.mimi_create_from_dir_flags(d.encode(), 0, 0, ctypes.byref(h)) == 0, lib.mimi_last_error()
    try:
        x = torch.from_numpy(synthetic.speech_like(1920 * 3, 5, 0)).cuda()
        got = torch.empty((1, 8, 3), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert lib.mimi_encode(h, ctypes.c_void_p(x.data_ptr()), 1, x.numel(), 8, ctypes.c_void_p(got.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(got.long(), dec.encode(x[None, None], num_quantizers=8).audio_codes)
        assert lib.mimi_decode(h, ctypes.c_void_p(got.data_ptr()), 1, 3, 8, ctypes.c_void_p(x.data_ptr()), None) == 7
    finally:
        lib.mimi_destroy(h)
    # one decoder tensor missing: finalize fails with MIMI_ERR_WEIGHTS naming it
    missing = "decoder.layers.8.conv.weight"
    d2 = write_checkpoint(full_np, str(tmp_path / "partial"), drop=missing)
    h = ctypes.c_void_p()
    assert lib.mimi_create_from_dir_flags(d2.encode(), 0, _lib.CREATE_DECODE, ctypes.byref(h)) == 4
    assert missing in lib.mimi_last_error().decode() and not h.value
    assert lib.mimi_create_from_dir_flags(d2.encode(), 0, 2, ctypes.byref(h)) == 1  # unknown flag
