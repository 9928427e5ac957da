"""GPU: the decode path kernel by kernel, in float64, at every shape where the dispatch picks another kernel.

* STAGE CHECKS: each stage's output tap against the float64 evaluation of that one stage on the engine's own input tap
  (tests/decode_stage_ref.py: q = max |got - ref64| / (2^-24 sum|a||w|), hard condition q <= n, working condition
  q <= 16 max(q_ref, 1) with q_ref torch-CPU's fp32 evaluation measured in the same test).  tests/test_decode_stage_ref.py
  shows on the CPU that one dropped weight, a missing zero row between items, swapped phases or taps, a missing bias
  and exchanged upsample weights each miss the working condition by >= 100 x.
* WHICH KERNEL RAN: every regime test reads the launch sequence of a profiled decode and asserts the tile family per
  stage (``gemm_f32_kernel<64, 128`` / ``<128, 128``, ``attention_t256_kernel`` / ``attention_kernel``).  A retune that
  moves a threshold fails that assertion: move the shape with it, so that both sides of the threshold stay tested.
* Each stage check appends {stage, case, q_engine, q_ref, n, kernel} to ``parity_log`` (parity_report.json).

Shapes (the smallest that reach their kernels; gemm.hip run_auto: 64-row tiles up to M = 1024 rows, 128-row above):
  B = 2 x T = 13     every stage; item 1's row 0 must see zeros; up2 / up3 (M = 1248 / 6240 per item) on 128-row tiles,
                     conv0, up0, up1 (M = 26, 26, 208) on 64-row; row tails 26, 208, 1248, 6240 inside a tile
  T = 64 / 65        up-conv 1 at M = 1024 (last 64-row shape) / 1040 (128-row, 16-row tail)
  T = 513            conv0 (both its forms: the ROLE_DOWN_ELU launch of the pass itself through the "dconv0_elu" tap, and
                     the taps-only ROLE_DOWN launch behind "dconv0") and up-conv 0 at M = 1026 (128-row, 2-row tail);
                     o_proj / fc1 / fc2 at 1026 flat rows; banded attention over 1026 rows (window 250)
  B = 40 x T = 13    o_proj / fc1 / fc2 at 1040 flat rows (128-row) while every per-item GEMM stays as at B = 1
  B = 2 x T = 129    banded attention with a batch
"""
import json

import numpy as np
import pytest
import torch

import decode_ref
import decode_stage_ref as dsr
from mimi_hip import synthetic

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
G64, G128 = "mimi::gemm_f32_kernel<64, 128,", "mimi::gemm_f32_kernel<128, 128,"
ATT256, ATTBAND = "mimi::attention_t256_kernel", "mimi::attention_kernel"
# the profiled stage(s) that produce each output tap
# ("dconv0" is the raw decoder.layers.0 output, which only taps compute, by a ROLE_DOWN launch of their own recorded as
# dec_conv0_tap; the pass itself runs the bias + ELU form, dec_conv0, whose output is the "dconv0_elu" tap)
STAGE_LAUNCHES = {"quantized": ("dec_rvq", "dec_output_proj"), "upsample": ("dec_upsample",),
                  "dconv0": ("dec_conv0_tap",), "dconv0_elu": ("dec_conv0",), "audio": ("dec_final",)}
RESBLOCK = ["mimi::resblock_kernel<512,", "mimi::resblock_kernel<256,", "mimi::resblock_kernel<128,",
            "mimi::resblock_kernel<64,"]
for _s in range(4):
    STAGE_LAUNCHES[f"up{_s}"] = (f"dec_up_s{_s}",)
    STAGE_LAUNCHES[f"dres{_s}_elu"] = (f"dec_res_s{_s}",)
XFMR_LAUNCHES = ("dec_layernorm", "dec_qkv", "dec_attention", "dec_o_proj", "dec_fc1", "dec_fc2")


@pytest.fixture(scope="module")
def full_np(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return sd


@pytest.fixture(scope="module")
def full_sd(full_np):
    return decode_ref.as_tensors(full_np)


def make_engine(full_np):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(full_np, device="cuda:0", decode=True)


@pytest.fixture(scope="module")
def dec(full_np):
    m = make_engine(full_np)
    yield m
    m.close()


def rand_codes(seed, B, K, T):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, (B, K, T)))


def profiled_decode(m, codes):
    """(waveform, {stage: set of kernel symbols}) of one decode with profiling on."""
    m.set_profiling(1)
    try:
        y = m.decode(codes).audio_values
        seq = m.profile_sequence()
    finally:
        m.set_profiling(0)
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    assert "dec_rvq" in kern and "dec_final" in kern, sorted(kern)  # the sequence is this decode's
    return y, kern


def assert_kernels(kern, want):
    """want: {stage: symbol prefix}; one symbol per stage, of that family."""
    for stage, prefix in want.items():
        assert stage in kern, (stage, sorted(kern))
        syms = sorted(kern[stage])
        assert len(syms) == 1 and syms[0].startswith(prefix), (stage, syms, prefix)


def symbols(kern, stages):
    return " + ".join(sorted(k for s in stages for k in kern.get(s, ())))


def tap_cf(m, name):
    """An engine tap [B][time][channels] as the channel-first tensor of decode_ref."""
    return torch.from_numpy(m.get_tap(name)).transpose(1, 2).contiguous()


def stage_input(m, name, codes):
    src = dsr.STAGES[name].source
    if src == "codes":
        return codes
    return tap_cf(m, src)


def check_stage(parity_log, case, name, x, got, sd, kern):
    rec = dsr.measure(name, x, sd, got)
    rec.update(test="decode_stage", case=case, kernel=symbols(kern, STAGE_LAUNCHES[name]))
    parity_log.append(rec)
    print(json.dumps(rec))
    assert not dsr.failures(rec), rec
    return rec


def check_transformer(parity_log, case, x, got, sd, kern):
    """The decoder transformer as a whole: project metric against float64, and against 16 x the error of torch-CPU's
    fp32 evaluation of the same input (floor 2^-24: one rounding of the largest element)."""
    ref64 = dsr.transformer(x, sd)
    rec = {"test": "decode_stage", "case": case, "stage": "xfmr7", "rel_err": dsr.rel_err(got, ref64),
           "rel_err_ref": dsr.rel_err(dsr.transformer(x, sd, torch.float32), ref64),
           "kernel": symbols(kern, XFMR_LAUNCHES)}
    parity_log.append(rec)
    print(json.dumps(rec))
    assert rec["rel_err"] < ACT_TOL, rec
    assert rec["rel_err"] <= dsr.WORKING_FACTOR * max(rec["rel_err_ref"], dsr.U), rec
    return rec


# ---- a. every stage at B = 2, T = 13, K = 8 -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dec):
    """One profiled taps-on decode of B = 2 x T = 13 x K = 8: (codes, waveform, kernels, {tap: channel-first})."""
    codes = rand_codes(13, 2, 8, 13)
    dec.set_taps(True)
    try:
        y, kern = profiled_decode(dec, codes)
        taps = {n: tap_cf(dec, n) for n in ("quantized", "upsample", "xfmr7", "dconv0", "dconv0_elu", "audio")}
        for s in range(4):
            taps[f"up{s}"] = tap_cf(dec, f"up{s}")
            taps[f"dres{s}_elu"] = tap_cf(dec, f"dres{s}_elu")
    finally:
        dec.set_taps(False)
    taps["codes"] = codes
    return codes, y, kern, taps


def test_small_shape_kernels(small):
    _, y, kern, taps = small
    assert_kernels(kern, {"dec_output_proj": G64, "dec_qkv": G64, "dec_attention": ATT256, "dec_o_proj": G64,
                          "dec_fc1": G64, "dec_fc2": G64, "dec_conv0": G64, "dec_conv0_tap": G64, "dec_up_s0": G64,
                          "dec_up_s1": G64, "dec_up_s2": G128, "dec_up_s3": G128, "dec_rvq": "mimi::rvq_decode_kernel",
                          "dec_upsample": "mimi::upsample_dw_kernel", "dec_final": "mimi::final_conv_kernel"})
    assert_kernels(kern, {f"dec_res_s{s}": RESBLOCK[s] for s in range(4)})
    assert torch.equal(taps["audio"][:, 0], y[:, 0].cpu())  # the tap is the returned waveform


@pytest.mark.parametrize("name", list(dsr.STAGES))
def test_stage_against_float64(small, full_sd, parity_log, name):
    _, _, kern, taps = small
    check_stage(parity_log, "B2_T13_K8", name, taps[dsr.STAGES[name].source], taps[name], full_sd, kern)


def test_transformer_against_float64(small, full_sd, parity_log):
    _, _, kern, taps = small
    check_transformer(parity_log, "B2_T13_K8", taps["upsample"], taps["xfmr7"], full_sd, kern)


# ---- b. up-conv 1 on either side of M = 1024 ------------------------------------------------------------------------
@pytest.mark.parametrize("T,tile", [(64, G64), (65, G128)])
def test_upconv1_tile_boundary(dec, full_sd, parity_log, T, tile):
    codes = rand_codes(T, 1, 8, T)
    dec.set_taps(True)
    try:
        y, kern = profiled_decode(dec, codes)
        assert_kernels(kern, {"dec_up_s1": tile, "dec_up_s0": G64, "dec_conv0": G64, "dec_up_s2": G128, "dec_up_s3": G128,
                              "dec_o_proj": G64, "dec_fc1": G64, "dec_fc2": G64, "dec_attention": ATT256,
                              "dec_res_s1": RESBLOCK[1]})
        for name in ("up1", "dres1_elu"):
            got = tap_cf(dec, name)
            assert got.shape[-1] == 96 * T
            check_stage(parity_log, f"B1_T{T}_K8", name, stage_input(dec, name, codes), got, full_sd, kern)
    finally:
        dec.set_taps(False)
    err = dsr.rel_err(y.cpu(), decode_ref.decode(codes, full_sd))
    parity_log.append({"test": f"decode_kernels_T{T}", "rel_err": err})
    assert err < ACT_TOL, err


# ---- c. T = 513: conv0 / up-conv 0 / the flat-row GEMMs on 128-row tiles, banded attention over many blocks ----------
def test_long_item_128_row_tiles(full_np, full_sd, parity_log):
    """An engine of its own: its tap buffers hold ~0.9 GB of device memory, freed on close.  Fetched: upsample,
    xfmr7, dconv0, up0 and dconv0_elu (the output of the ROLE_DOWN_ELU kernel that the pass itself runs)."""
    T = 513
    codes = rand_codes(T, 1, 8, T)
    m = make_engine(full_np)
    try:
        m.set_taps(True)
        y, kern = profiled_decode(m, codes)
        taps = {n: tap_cf(m, n) for n in ("upsample", "xfmr7", "dconv0", "dconv0_elu", "up0")}
        y = y.cpu()
    finally:
        m.close()
    assert_kernels(kern, {"dec_conv0": G128, "dec_conv0_tap": G128, "dec_up_s0": G128, "dec_up_s1": G128, "dec_up_s2": G128, "dec_up_s3": G128,
                          "dec_o_proj": G128, "dec_fc1": G128, "dec_fc2": G128, "dec_qkv": G64,
                          "dec_attention": ATTBAND, "dec_output_proj": G64})
    assert taps["xfmr7"].shape == (1, 512, 1026) and taps["up0"].shape == (1, 512, 8208)
    check_transformer(parity_log, "B1_T513_K8", taps["upsample"], taps["xfmr7"], full_sd, kern)
    check_stage(parity_log, "B1_T513_K8", "dconv0", taps["xfmr7"], taps["dconv0"], full_sd, kern)
    check_stage(parity_log, "B1_T513_K8", "dconv0_elu", taps["xfmr7"], taps["dconv0_elu"], full_sd, kern)
    check_stage(parity_log, "B1_T513_K8", "up0", taps["dconv0_elu"], taps["up0"], full_sd, kern)
    # decode is causal: the first 13 frames' samples are those of the 13-frame decode
    n = 1920 * 13
    err = dsr.rel_err(y[..., :n], decode_ref.decode(codes[..., :13], full_sd))
    parity_log.append({"test": "decode_kernels_T513_prefix13", "rel_err": err})
    assert err < ACT_TOL, err


# ---- d. B = 40 x T = 13: 1040 flat rows, and the bitwise claim across a tile change ----------------------------------
def test_batch_of_40_flat_rows_128_and_bitwise_items(dec, full_sd, parity_log):
    B, T = 40, 13
    codes = rand_codes(40, B, 8, T)
    assert len({codes[i].numpy().tobytes() for i in range(B)}) == B
    yb, kern = profiled_decode(dec, codes)
    per_item = {"dec_qkv": G64, "dec_attention": ATT256, "dec_conv0": G64, "dec_up_s0": G64, "dec_up_s1": G64,
                "dec_up_s2": G128, "dec_up_s3": G128}
    assert_kernels(kern, dict(per_item, dec_o_proj=G128, dec_fc1=G128, dec_fc2=G128, dec_output_proj=G64))
    refs = decode_ref.decode(codes[[0, 39]], full_sd)
    for i in (0, 17, 39):
        y1, k1 = profiled_decode(dec, codes[i:i + 1])
        assert_kernels(k1, dict(per_item, dec_o_proj=G64, dec_fc1=G64, dec_fc2=G64))  # the tiles did change
        assert torch.equal(yb[i], y1[0]), f"item {i} of the batch of 40 differs from its own B = 1 decode"
    for j, i in enumerate((0, 39)):
        err = dsr.rel_err(yb[i].cpu(), refs[j])
        parity_log.append({"test": f"decode_kernels_B40_item{i}", "rel_err": err})
        assert err < ACT_TOL, (i, err)


def test_benchmark_shape_items_bitwise(dec):
    """B = 32 x T = 125 (what tools/decode_bench.py times): 8000 flat rows on 128-row tiles, 250 rows per item on the
    <= 256-row attention.  Its items against their own B = 1 decodes (T = 125 alone is held to the reference by
    tests/test_decode_gpu.py)."""
    codes = rand_codes(125, 32, 8, 125)
    yb, kern = profiled_decode(dec, codes)
    assert_kernels(kern, {"dec_o_proj": G128, "dec_fc1": G128, "dec_fc2": G128, "dec_output_proj": G128, "dec_qkv": G64,
                          "dec_attention": ATT256, "dec_conv0": G64, "dec_up_s0": G64, "dec_up_s1": G128})
    for i in (0, 31):
        assert torch.equal(yb[i], dec.decode(codes[i:i + 1]).audio_values[0]), i


# ---- e. banded attention with a batch -------------------------------------------------------------------------------
def test_banded_attention_batch_items_bitwise(dec):
    codes = rand_codes(129, 2, 8, 129)
    yb, kern = profiled_decode(dec, codes)
    assert_kernels(kern, {"dec_attention": ATTBAND})
    for i in range(2):
        y1, k1 = profiled_decode(dec, codes[i:i + 1])
        assert_kernels(k1, {"dec_attention": ATTBAND})
        assert torch.equal(yb[i], y1[0]), i


# ---- f. settings that must not change a bit -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(dec):
    codes = rand_codes(7, 2, 8, 13)
    return codes, dec.decode(codes).audio_values.clone()


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "bf16x3", "f32"])
def test_precision_mode_does_not_move_decode(dec, base, mode):
    codes, want = base
    saved = dec.precision
    try:
        dec.set_precision(mode)
        y, kern = profiled_decode(dec, codes)
        assert dec.precision == mode
    finally:
        dec.set_precision(saved)
    assert torch.equal(y, want)
    assert all(next(iter(kern[s])).startswith("mimi::gemm_f32_kernel<") for s in
               ("dec_output_proj", "dec_qkv", "dec_o_proj", "dec_fc1", "dec_fc2", "dec_conv0", "dec_up_s0", "dec_up_s3")), kern


@pytest.mark.parametrize("rpw", [1, 2, 4, 8])
def test_ln_rpw_does_not_move_decode(dec, base, rpw):
    codes, want = base
    try:
        dec.set_option("ln_rpw", rpw)
        y, kern = profiled_decode(dec, codes)  # 52 rows: a tail of 4 at 8 rows per wave
    finally:
        dec.set_option("ln_rpw", 1)  # the engine's default
    assert kern["dec_layernorm"] == {f"mimi::layernorm_kernel<512, {rpw}>"}
    assert torch.equal(y, want)


def test_taps_profiling_and_stream_do_not_move_decode(dec, base):
    codes, want = base
    dec.set_taps(True)
    try:
        assert torch.equal(dec.decode(codes).audio_values, want)
    finally:
        dec.set_taps(False)
    assert torch.equal(dec.decode(codes).audio_values, want)
    y, _ = profiled_decode(dec, codes)
    assert torch.equal(y, want)
    side = torch.cuda.Stream(device=dec.device)
    assert side.cuda_stream != torch.cuda.current_stream(dec.device).cuda_stream
    with torch.cuda.stream(side):
        y = dec.decode(codes).audio_values
    side.synchronize()
    assert torch.equal(y, want)
    # a stream step and a slot step (the transformer's 40 per-layer taps are saved between their launches): taps on
    # moves no bit of the samples, and the per-layer taps are there
    sc = rand_codes(8, 2, 8, 5)
    outs = []
    for taps in (False, True):
        dec.set_taps(taps)
        try:
            with dec.decode_stream(batch=2, num_quantizers=8, max_step_frames=3) as st:
                ys = [st.step(sc[:, :, :2]).cpu()]
                if taps:
                    assert dec.get_tap("qkv3").shape == (2, 4, 1536) and dec.get_tap("ff7").shape == (2, 4, 2048)
                ys.append(st.step(sc[1:, :, 2:5], slots=[1]).cpu())
                if taps:
                    assert dec.get_tap("att0").shape == (1, 6, 512) and dec.get_tap("xfmr7").shape == (1, 6, 512)
                ys.append(st.step(sc[:1, :, 2:3], slots=[0]).cpu())
        finally:
            dec.set_taps(False)
        outs.append(ys)
    assert len(outs[0]) == len(outs[1]) == 3 and all(torch.equal(a, b) for a, b in zip(*outs))


def test_workspace_regrow_does_not_move_decode(full_np, base):
    """A fresh engine, so that the workspace does grow: T = 13, then B = 3 x T = 65 with taps on (another layout: the
    tap region), then T = 13 with taps off."""
    codes, want = base
    m = make_engine(full_np)
    try:
        small_bytes = m.decode_workspace_bytes(2, 13)
        assert torch.equal(m.decode(codes).audio_values, want)
        m.set_taps(True)
        big_bytes = m.decode_workspace_bytes(3, 65)
        assert big_bytes > small_bytes > 0
        big = rand_codes(65, 3, 8, 65)
        yb = m.decode(big).audio_values.clone()
        m.set_taps(False)
        assert m.decode_workspace_bytes(3, 65) < big_bytes  # taps change the layout
        assert torch.equal(m.decode(codes).audio_values, want)
        assert torch.equal(m.decode(big).audio_values, yb)
    finally:
        m.close()


# ---- g. encode's captured graphs survive decode's RoPE regrow --------------------------------------------------------
def test_encode_graphs_survive_decode_rope_regrow(full_np, golden):
    _, gmeta = golden
    L = 240000  # 10 s: 250 transformer rows, inside the first 256-row RoPE table
    x = torch.from_numpy(synthetic.speech_like(L, gmeta["audio_seed"], gmeta["lengths"].index(L)))[None].cuda()
    m = make_engine(full_np)
    try:
        r0, c0 = m.graph_replays, m.graph_captures
        outs = [m.encode_int32(x, 8).cpu() for _ in range(3)]
        r1, c1 = m.graph_replays, m.graph_captures
        assert r1 > r0 and c1 == c0 + 1
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        m.decode(rand_codes(13, 1, 8, 13))  # 26 rows: the tables stay, and so does the graph
        assert torch.equal(m.encode_int32(x, 8).cpu(), outs[0])
        assert m.graph_captures == c1 and m.graph_replays == r1 + 1
        m.decode(rand_codes(129, 1, 8, 129))  # 258 rows: the tables are freed and rebuilt at other addresses
        assert torch.equal(m.encode_int32(x, 8).cpu(), outs[0])
        r2 = m.graph_replays
        assert m.graph_captures == c1 + 1, "the graph that held the freed tables' addresses was replayed"
        assert torch.equal(m.encode_int32(x, 8).cpu(), outs[0])
        assert m.graph_replays > r2 > r1 and m.graph_captures == c1 + 1
    finally:
        m.close()


# ---- h. the quantizer kernel's edges through dequantize ---------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8, 9, 31, 32])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 3), (3, 9)])
def test_dequantize_against_float64(dec, full_sd, parity_log, B, T, K):
    """B T = 1, 3, 27 frames: odd counts, the half-filled last workgroup (two frames per workgroup)."""
    codes = rand_codes(100 * B * T + K, B, K, T)
    dec.set_profiling(1)
    try:
        got = dec.dequantize(codes).cpu()
        kern = {}
        for stage, kernel in dec.profile_sequence():
            kern.setdefault(stage, set()).add(kernel)
    finally:
        dec.set_profiling(0)
    assert_kernels(kern, {"dec_rvq": "mimi::rvq_decode_kernel", "dec_output_proj": G64})
    assert got.shape == (B, 512, T)
    check_stage(parity_log, f"dequantize_B{B}_T{T}_K{K}", "quantized", codes, got, full_sd, kern)


@pytest.mark.parametrize("bad", [-1, 2048, 2 ** 31 - 1, -2 ** 31])
def test_out_of_range_code_at_the_last_position(dec, bad):
    """The last level of the last frame of the last item: the last word the kernel reads.  An error return by design
    (decode.hip rvq_decode_kernel checks the code before it forms an address)."""
    good = rand_codes(5, 3, 32, 5)
    before = dec.decode(good).audio_values.clone()
    codes = good.clone()
    codes[2, 31, 4] = bad
    with pytest.raises(ValueError, match="codebook_size"):
        dec.decode(codes)
    with pytest.raises(ValueError, match="codebook_size"):
        dec.dequantize(codes)
    assert torch.equal(dec.decode(good).audio_values, before)
