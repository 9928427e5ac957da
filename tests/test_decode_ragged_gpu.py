"""Ragged decode on the GPU (mimi_decode_ragged / MimiHipModel.decode_ragged / strs_to_audio).

The contract under test: item b of a ragged decode is BITWISE ``decode`` of that item alone at its own length, whatever
its batch-mates; codes past an item's length are never read and samples past it never written.  Against the CPU
reference (tests/decode_ref.py) the metric and tolerance are the project's: ``rel_err < 1e-4``.  Everything else is
equality.

Batch A (K = 8, T = 13, 1, 129, 2, 64, 65, 5, 3): sum 282 -> 564 flat transformer rows on 64-row tiles; T = 129 is 258
rows, the banded attention, the others the <= 256-row kernel; T = 64 / 65 put up conv 1 at M = 1024 / 1040, either
side of the GEMM tile threshold; T = 1, 2, 3 are the frames where every x[t - 1] is the item's own left padding.
Batch B (40 items of 12 + b % 3 frames): sum 519 -> 1038 flat rows on 128-row tiles.
"""
import ctypes

import numpy as np
import pytest
import torch

from mimi_hip import synthetic
from test_decode_gpu import (ACT_TOL, dec, dgolden, fixture_codes, full_np, full_sd, log, ref_cache,  # noqa: F401
                             rel_err)

pytestmark = pytest.mark.gpu

T_A = [13, 1, 129, 2, 64, 65, 5, 3]
T_B = [12 + b % 3 for b in range(40)]
G64, G128 = "mimi::gemm_f32_kernel<64, 128,", "mimi::gemm_f32_kernel<128, 128,"
INT32_MAX = 2 ** 31 - 1


def item_codes(arrays, T, K=8, seed=None):
    if seed is None and f"codes_T{T}" in arrays:
        return fixture_codes(arrays, T, K)
    return torch.from_numpy(np.random.default_rng(T if seed is None else seed).integers(0, 2048, (1, K, T)))


def pad_batch(items, fill=0):
    """[1, K, T_b] items -> ([B, K, Tmax] int64 filled with `fill` past each length, lengths)."""
    lens = [int(c.shape[-1]) for c in items]
    out = torch.full((len(items), items[0].shape[1], max(lens)), fill, dtype=torch.int64)
    for b, c in enumerate(items):
        out[b, :, : lens[b]] = c[0]
    return out, lens


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def batch_a(dec, dgolden):
    """Batch A's items, each item's own B = 1 decode, and the ragged decode of the batch: computed once, never changed."""
    arrays, _ = dgolden
    items = [item_codes(arrays, T) for T in T_A]
    alone = [dec.decode(c).audio_values[0].clone() for c in items]
    codes, lens = pad_batch(items)
    ragged = [y.clone() for y in dec.decode_ragged(codes, lens)]
    return dict(items=items, alone=alone, codes=codes, lens=lens, ragged=ragged)


@pytest.fixture(scope="module")
def batch_b():
    items = [item_codes({}, T, seed=1000 + b) for b, T in enumerate(T_B)]
    codes, lens = pad_batch(items)
    return dict(items=items, codes=codes, lens=lens)


def profiled_ragged(m, codes, lens):
    m.set_profiling(1)
    try:
        y = m.decode_ragged(codes, lens)
        seq = m.profile_sequence()
    finally:
        m.set_profiling(0)
    assert seq and seq[0][0] == "dec_rvq" and seq[-1][0] == "dec_final", seq[:2]
    return y, seq


# ---- 1. bitwise vs alone ----------------------------------------------------------------------------------------------
def test_items_bitwise_equal_to_alone(dec, batch_a, ref_cache, parity_log):
    assert len(batch_a["ragged"]) == len(T_A)
    errs = {}
    for b, T in enumerate(T_A):
        y = batch_a["ragged"][b]
        assert y.shape == (1, 1920 * T) and y.dtype == torch.float32 and y.is_cuda
        assert same_bits(y, batch_a["alone"][b]), (b, T)
        errs[T] = rel_err(y[0].cpu().numpy(), ref_cache(batch_a["items"][b])[0][0, 0].numpy())
    log(parity_log, "decode_ragged_batch_a_vs_reference", rel_err=max(errs.values()), per_T=errs)
    for T, err in errs.items():
        assert err < ACT_TOL, (T, err)


def test_items_bitwise_in_reverse_order(dec, batch_a):
    codes, lens = pad_batch(batch_a["items"][::-1])
    ys = dec.decode_ragged(codes, lens)
    for b, y in enumerate(ys[::-1]):
        assert same_bits(y, batch_a["alone"][b]), (b, T_A[b])


# ---- 2. flat-row tile change ------------------------------------------------------------------------------------------
def test_flat_row_tile_change(dec, batch_b):
    ys = dec.decode_ragged(batch_b["codes"], batch_b["lens"])
    assert len(ys) == 40
    for b in (0, 17, 39):
        assert same_bits(ys[b], dec.decode(batch_b["items"][b]).audio_values[0]), b


# ---- 3. K -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 32])
def test_num_quantizers(dec, dgolden, K):
    """K = 1: the acoustic half stays zero."""
    arrays, _ = dgolden
    items = [item_codes(arrays, T, K) for T in (1, 3, 2)]
    codes, lens = pad_batch(items)
    for y, c in zip(dec.decode_ragged(codes, lens), items):
        assert same_bits(y, dec.decode(c).audio_values[0])


# ---- 4. padding is never read, the rest of a row never written -----------------------------------------------------------
@pytest.mark.parametrize("fill", [-1, 2048, INT32_MAX])
def test_padding_codes_are_never_read(dec, batch_a, fill):
    codes, lens = pad_batch(batch_a["items"], fill=fill)
    assert int((codes == fill).sum()) >= 8 * (129 * 8 - 282)
    for b, y in enumerate(dec.decode_ragged(codes, lens)):  # no ValueError: the bounds flag stays down
        assert same_bits(y, batch_a["ragged"][b]), (fill, b)


def test_rows_past_an_item_are_left_untouched(dec, batch_a):
    lib = dec._lib
    B, Tmax = len(T_A), max(T_A)
    codes = batch_a["codes"].to(device="cuda:0", dtype=torch.int32).contiguous()
    lens = np.asarray(T_A, dtype=np.int64)
    L = lib.mimi_decoded_length(Tmax)
    out = torch.full((B, L), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.mimi_decode_ragged(dec._h, ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(lens.ctypes.data), B, Tmax, 8,
                                ctypes.c_void_p(out.data_ptr()), None)
    assert rc == 0, lib.mimi_last_error()
    torch.cuda.synchronize()
    for b, T in enumerate(T_A):
        assert same_bits(out[b:b + 1, : 1920 * T], batch_a["ragged"][b]), b
        assert bool(torch.isnan(out[b, 1920 * T:]).all()), b
    # the same through the method's `out`
    out2 = torch.full((B, L), float("nan"), dtype=torch.float32, device="cuda:0")
    ys = dec.decode_ragged(batch_a["codes"], T_A, out=out2)
    assert all(y.data_ptr() == out2[b].data_ptr() for b, y in enumerate(ys))
    assert torch.equal(torch.isnan(out2), torch.isnan(out))


# ---- 5. errors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [2048, -1])
def test_bad_code_inside_an_item_is_refused_and_engine_survives(dec, batch_a, bad):
    codes = batch_a["codes"].clone()
    b = T_A.index(min(T_A))
    codes[b, 7, T_A[b] - 1] = bad  # the last valid frame of the shortest item
    uniform_before = dec.decode(batch_a["items"][0]).audio_values.clone()
    with pytest.raises(ValueError, match="codebook_size"):
        dec.decode_ragged(codes, T_A)
    for i, y in enumerate(dec.decode_ragged(batch_a["codes"], T_A)):
        assert same_bits(y, batch_a["ragged"][i]), i
    assert torch.equal(dec.decode(batch_a["items"][0]).audio_values, uniform_before)


def test_bad_lengths_are_refused_on_the_host(dec, batch_a):
    lib = dec._lib
    codes = batch_a["codes"][:3]
    for lens in ([1, 0, 2], [1, 130, 2], [1, 2], [[1, 2, 3]] * 2):
        with pytest.raises(ValueError, match="lengths"):
            dec.decode_ragged(codes, lens)
    # the C entry itself: refused on the host, before anything is launched
    c32 = codes.to(device="cuda:0", dtype=torch.int32).contiguous()
    out = torch.zeros((3, 1920 * 129), dtype=torch.float32, device="cuda:0")
    for lens in ([1, 0, 2], [1, 130, 2]):
        h = np.asarray(lens, dtype=np.int64)
        rc = lib.mimi_decode_ragged(dec._h, ctypes.c_void_p(c32.data_ptr()), ctypes.c_void_p(h.ctypes.data), 3, 129, 8,
                                    ctypes.c_void_p(out.data_ptr()), None)
        assert rc == 1 and b"lengths[1]" in lib.mimi_last_error()
        torch.cuda.synchronize()
        assert not bool(out.any())  # not one sample written
    with pytest.raises(ValueError):
        dec.decode_ragged(torch.zeros(2, 33, 2, dtype=torch.int64), [1, 2])
    with pytest.raises(ValueError):
        dec.decode_ragged(torch.zeros(2, 0, 2, dtype=torch.int64), [1, 2])


def test_encode_only_model_refuses_ragged_decode(state_dict):
    from mimi_hip.model import MimiHipModel
    m = MimiHipModel(state_dict, device="cuda:0")
    try:
        with pytest.raises(RuntimeError, match="decode=True"):
            m.decode_ragged(torch.zeros(1, 8, 1, dtype=torch.int64), [1])
        lens = np.asarray([1], dtype=np.int64)
        assert m._lib.mimi_decode_ragged(m._h, None, ctypes.c_void_p(lens.ctypes.data), 1, 1, 1, None, None) == 7
    finally:
        m.close()


# ---- 6. one pass ------------------------------------------------------------------------------------------------------
def test_one_pass_and_kernel_choices(dec, batch_a, batch_b):
    small = [item_codes({}, T, seed=50 + T) for T in (12, 13, 14)]
    _, seq_s = profiled_ragged(dec, *pad_batch(small))
    _, seq_b = profiled_ragged(dec, batch_b["codes"], batch_b["lens"])
    ya, seq_a = profiled_ragged(dec, batch_a["codes"], batch_a["lens"])
    for b, y in enumerate(ya):
        assert same_bits(y, batch_a["ragged"][b])
    names = lambda seq: [s for s, _ in seq]  # noqa: E731
    assert names(seq_s) == names(seq_b)  # 3 items or 40: the same launches
    layers = dec.config.num_hidden_layers
    assert len(seq_a) == len(seq_b) + layers  # the second attention kernel, once per layer
    assert [s for s in names(seq_a) if s != "dec_attention"] == [s for s in names(seq_b) if s != "dec_attention"]

    def kernels(seq, stage):
        return sorted({k for s, k in seq if s == stage})
    assert kernels(seq_a, "dec_attention") == ["mimi::attention_ragged_kernel", "mimi::attention_t256_ragged_kernel"]
    assert kernels(seq_b, "dec_attention") == ["mimi::attention_t256_ragged_kernel"]
    assert names(seq_a).count("dec_attention") == 2 * layers and names(seq_b).count("dec_attention") == layers
    for stage in ("dec_output_proj", "dec_o_proj", "dec_fc1", "dec_fc2"):
        for seq, prefix in ((seq_a, G64), (seq_b, G128)):
            # (output_proj runs on the 12.5 Hz rows: 282 and 519, both on 64-row tiles)
            want = G64 if stage == "dec_output_proj" else prefix
            syms = kernels(seq, stage)
            assert len(syms) == 1 and syms[0].startswith(want), (stage, syms, want)
    # the per-item stages run their ragged forms
    assert kernels(seq_a, "dec_rvq") == ["mimi::rvq_decode_ragged_kernel"]
    assert kernels(seq_a, "dec_upsample") == ["mimi::upsample_dw_ragged_kernel"]
    assert kernels(seq_a, "dec_final") == ["mimi::final_conv_ragged_kernel"]
    assert all(k.startswith("mimi::resblock_ragged_kernel<") for s, k in seq_a if s.startswith("dec_res_s"))
    # q/k/v always 64-row tiles; conv 0 and the up convs: the tile of the LONGEST item (258 .. rows: 128-row tiles)
    assert all(k.startswith(G64) and k.endswith(" 105>") for k in kernels(seq_a, "dec_qkv"))
    assert all(k.startswith(G64) for k in kernels(seq_b, "dec_conv0")) and \
        all(k.startswith(G64) for k in kernels(seq_a, "dec_conv0"))
    assert all(k.startswith(G128) for k in kernels(seq_a, "dec_up_s1"))  # M = 16 x 129 = 2064 > 1024


# ---- 7. taps ----------------------------------------------------------------------------------------------------------
def test_packed_taps_equal_each_items_own(dec, batch_a):
    names = ["quantized", "upsample", f"xfmr{dec.config.num_hidden_layers - 1}", "dconv0", "dconv0_elu", "audio"]
    for i in range(len(dec.config.upsampling_ratios)):
        names += [f"up{i}", f"dres{i}_elu"]
    S = sum(T_A)
    dec.set_taps(True)
    try:
        ys = dec.decode_ragged(batch_a["codes"], T_A)
        for b, y in enumerate(ys):
            assert same_bits(y, batch_a["ragged"][b])
        packed = {n: dec.get_tap(n) for n in names}
        off = 0
        for b, T in enumerate(T_A):
            dec.decode(batch_a["items"][b])
            for n in names:
                p = packed[n]
                assert p.shape[0] == 1 and p.shape[1] % S == 0, (n, p.shape)
                f = p.shape[1] // S
                own = dec.get_tap(n)
                assert own.shape == (1, f * T, p.shape[2]), (n, own.shape)
                got = p[0, f * off: f * (off + T)]
                assert np.array_equal(got.view(np.uint32), own[0].view(np.uint32)), (n, b, T)
            off += T
    finally:
        dec.set_taps(False)


# ---- 8. workspace -----------------------------------------------------------------------------------------------------
def test_workspace_grows_with_the_sum_of_lengths(dec, batch_a, batch_b):
    for lens in (T_A, T_B):
        need = dec.decode_ragged_workspace_bytes(lens)
        assert 0 < need <= dec.decode_workspace_bytes(1, sum(lens)) + 4096 + 256 * len(lens), (need, lens)
    assert dec.decode_ragged_workspace_bytes(T_A) < dec.decode_workspace_bytes(len(T_A), max(T_A)) // 3
    assert dec.decode_ragged_workspace_bytes([1, 0]) == -1


def test_workspace_shared_with_uniform_decode(full_np, batch_a):
    from mimi_hip.model import MimiHipModel
    m = MimiHipModel(full_np, device="cuda:0", decode=True)
    try:
        idx = [1, 7, 3]  # T = 1, 3, 2
        small, lens = pad_batch([batch_a["items"][i] for i in idx])
        want_u = None
        for _ in range(2):
            ys = m.decode_ragged(small, lens)  # 1st: grows the workspace; 2nd: after a larger uniform decode
            for i, y in zip(idx, ys):
                assert same_bits(y, batch_a["alone"][i]), i
            u = m.decode(torch.cat([batch_a["items"][0]] * 2)).audio_values  # B = 2 x 13 frames: a regrow the 1st time
            assert same_bits(u[0], batch_a["alone"][0]) and same_bits(u[1], batch_a["alone"][0])
            want_u = u.clone() if want_u is None else want_u
        big, blens = pad_batch([batch_a["items"][i] for i in (4, 0, 5)])  # 142 frames: the ragged pass regrows it
        for i, y in zip((4, 0, 5), m.decode_ragged(big, blens)):
            assert same_bits(y, batch_a["alone"][i]), i
        assert torch.equal(m.decode(torch.cat([batch_a["items"][0]] * 2)).audio_values, want_u)
    finally:
        m.close()


# ---- 9. neighbours ----------------------------------------------------------------------------------------------------
def test_encode_and_uniform_decode_unchanged(dec, batch_a, state_dict, golden, dgolden):
    from mimi_hip.model import MimiHipModel
    arrays, _ = dgolden
    _, gmeta = golden
    L = 240000
    x = torch.from_numpy(synthetic.speech_like(L, gmeta["audio_seed"], gmeta["lengths"].index(L)))[None, None].cuda()
    plain = MimiHipModel(state_dict, device="cuda:0")
    want = plain.encode(x).audio_codes
    plain.close()
    assert torch.equal(dec.encode(x).audio_codes, want)  # after batch A's ragged decodes (258 RoPE rows)
    assert torch.equal(dec.encode(x).audio_codes, want)
    c1 = dec.graph_captures
    small, lens = pad_batch([batch_a["items"][i] for i in (0, 6)])
    dec.decode_ragged(small, lens)  # 26 RoPE rows: the tables stay, and so does encode's graph
    assert torch.equal(dec.encode(x).audio_codes, want)
    assert dec.graph_captures == c1
    assert same_bits(dec.decode(fixture_codes(arrays, 13, 8)).audio_values[0], batch_a["alone"][0])


# ---- 10. public functions ---------------------------------------------------------------------------------------------
def test_strs_to_audio_equals_str_to_audio(dec, dgolden):
    from mimi_hip import codes_to_chars, str_to_audio, strs_to_audio
    arrays, _ = dgolden
    strs = []
    for i, T in enumerate([5, 0, 13, 2, 13]):
        c = item_codes({}, T, seed=700 + i)[0].numpy() if T else np.zeros((8, 0), dtype=np.int64)
        strs.append(codes_to_chars(c, codebook_size=2048))
    want = [str_to_audio(s, dec, "cuda:0") if s else np.zeros((1, 0), np.float32) for s in strs]
    for kw in ({}, {"max_batch_frames": 15}):  # one batch; then three: [5] | [13, 2] | [13]
        got = strs_to_audio(strs, dec, "cuda:0", **kw)
        assert len(got) == 5
        for g, w in zip(got, want):
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == w.shape
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
