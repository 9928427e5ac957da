"""GPU: streaming decode (``MimiHipModel.decode_stream``), codes to audio chunk by chunk on a KV cache.

What a stream promises, and what these tests hold it to:

1. CHUNKING DOES NOT MOVE A BIT: the concatenated steps of any split of a sequence are ``torch.equal`` to one another,
   and within ``ACT_TOL`` = 1e-4 (the project's ``rel_err``) of ``decode_ref.decode`` of the whole sequence.
2. the sliding window, eviction and the ring's wrap at the real window (T = 130: 260 rows against 250), with the
   smallest ring (``max_step_frames`` = 1), a mid-sized one and one chunk that holds the whole sequence;
3. the window comes from the config (``sliding_window`` = 5: odd, its edge inside a frame's pair of rows);
4. stage by stage in float64 on the per-step taps concatenated in time (tests/decode_stage_ref.py), and the kernels a
   step runs;
5. items of a batch and streams of an engine do not see one another, nor the decodes / encodes run between their steps;
6. the life cycle: reset, constant state size, bad arguments, bad codes, an encode-only model, the ``out`` buffer.

tests/test_decode_stream_ref.py shows on the CPU that these inputs tell the likely mistakes apart (window off by one,
RoPE restarted per chunk, a short or unshifted carry, a dropped upsample carry) by >= 10 x the tolerance.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import decode_ref
import decode_stage_ref as dsr
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = 1920
G64 = "mimi::gemm_f32_kernel<64, 128,"
SPLITS_13 = ([13], [1] * 13, [2, 3, 1, 7], [12, 1])
TAPS = ["quantized", "upsample", "xfmr7", "dconv0", "dconv0_elu", "audio"] + [f"up{s}" for s in range(4)] + \
       [f"dres{s}_elu" for s in range(4)]
XFMR_LAUNCHES = ("dec_layernorm", "dec_qkv", "dec_attention", "dec_o_proj", "dec_fc1", "dec_fc2")
STAGE_LAUNCHES = {"quantized": ("dec_rvq", "dec_output_proj"), "upsample": ("dec_upsample",),
                  "dconv0": ("dec_conv0_tap",), "dconv0_elu": ("dec_conv0",), "audio": ("dec_final",)}
for _s in range(4):
    STAGE_LAUNCHES[f"up{_s}"] = (f"dec_up_s{_s}",)
    STAGE_LAUNCHES[f"dres{_s}_elu"] = (f"dec_res_s{_s}",)


@pytest.fixture(scope="module")
def full_np(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return sd


@pytest.fixture(scope="module")
def full_sd(full_np):
    return decode_ref.as_tensors(full_np)


def make_engine(full_np, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(full_np, device="cuda:0", decode=True, **kw)


@pytest.fixture(scope="module")
def dec(full_np):
    m = make_engine(full_np)
    yield m
    m.close()


def rand_codes(seed, B, K, T):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, (B, K, T)))


def steps_of(codes, split):
    assert sum(split) == codes.shape[2]
    at = 0
    for n in split:
        yield codes[:, :, at:at + n]
        at += n


def run_stream(m, codes, split, max_step_frames=None):
    """The concatenated steps of one fresh stream, on the host."""
    B, K, _ = codes.shape
    with m.decode_stream(batch=B, num_quantizers=K, max_step_frames=max_step_frames or max(split)) as st:
        out = []
        for c in steps_of(codes, split):
            y = st.step(c)
            assert y.shape == (B, 1, FRAME * c.shape[2]) and y.dtype == torch.float32 and y.is_cuda
            out.append(y.cpu())
        assert st.position == codes.shape[2]
    return torch.cat(out, dim=-1)


def log(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


# ---- 1. chunking does not move a bit --------------------------------------------------------------------------------
def test_chunking_does_not_move_a_bit(dec, full_sd, parity_log):
    codes = rand_codes(13, 1, 8, 13)
    want = decode_ref.decode(codes, full_sd)
    outs = [run_stream(dec, codes, split) for split in SPLITS_13]
    for split, y in zip(SPLITS_13, outs):
        err = dsr.rel_err(y, want)
        log(parity_log, "decode_stream_T13_K8", split=list(split), rel_err=err)
        assert err < ACT_TOL, (split, err)
    for split, y in zip(SPLITS_13[1:], outs[1:]):
        assert torch.equal(y, outs[0]), f"split {split} differs from one step of 13 frames"


@pytest.mark.parametrize("K", [1, 32])
def test_chunking_other_level_counts(dec, full_sd, parity_log, K):
    codes = rand_codes(100 + K, 1, K, 13)
    y = run_stream(dec, codes, [2, 3, 1, 7])
    err = dsr.rel_err(y, decode_ref.decode(codes, full_sd))
    log(parity_log, f"decode_stream_T13_K{K}", split=[2, 3, 1, 7], rel_err=err)
    assert err < ACT_TOL, err
    assert torch.equal(y, run_stream(dec, codes, [13]))


# ---- 2. window, eviction and ring wrap at the real window -----------------------------------------------------------
@pytest.fixture(scope="module")
def t130(dec):
    """T = 130 three ways; the 1-frame stream's state size after its first and after its last step."""
    codes = rand_codes(130, 1, 8, 130)
    with dec.decode_stream(batch=1, num_quantizers=8, max_step_frames=1) as st:
        out, sizes = [], []
        for c in steps_of(codes, [1] * 130):
            out.append(st.step(c).cpu())
            sizes.append(st.state_bytes)
        assert st.position == 130
    ones = torch.cat(out, dim=-1)
    sevens = run_stream(dec, codes, [7] * 18 + [4], max_step_frames=7)
    whole = run_stream(dec, codes, [130], max_step_frames=130)
    return codes, ones, sevens, whole, sizes


def test_window_eviction_and_ring_wrap(t130, full_sd, parity_log):
    codes, ones, sevens, whole, _ = t130
    want = decode_ref.decode(codes, full_sd)
    for name, y in (("1x130", ones), ("7x18+4", sevens), ("130", whole)):
        err = dsr.rel_err(y, want)
        log(parity_log, "decode_stream_T130", split=name, rel_err=err)
        assert err < ACT_TOL, (name, err)
    assert torch.equal(ones, whole), "130 steps of 1 frame (the smallest ring) differ from one step of 130"
    assert torch.equal(sevens, whole), "steps of 7 frames differ from one step of 130"


# ---- 3. the window comes from the config ----------------------------------------------------------------------------
def test_window_from_the_config(full_np, full_sd, parity_log):
    from mimi_hip.config import MimiConfig
    codes = rand_codes(9, 1, 8, 9)
    want = decode_ref.decode(codes, full_sd, RefConfig(sliding_window=5))
    assert dsr.rel_err(decode_ref.decode(codes, full_sd), want) > 10 * ACT_TOL  # the window shows in these samples
    m = make_engine(full_np, config=MimiConfig(sliding_window=5))
    try:
        outs = {}
        for split in ([1] * 9, [4, 4, 1], [9]):
            y = run_stream(m, codes, split)
            err = dsr.rel_err(y, want)
            log(parity_log, "decode_stream_T9_window5", split=list(split), rel_err=err)
            assert err < ACT_TOL, (split, err)
            outs[len(split)] = y
    finally:
        m.close()
    assert torch.equal(outs[9], outs[1]) and torch.equal(outs[3], outs[1])


# ---- 4. stage by stage, in float64 ----------------------------------------------------------------------------------
def tap_cf(m, name):
    """An engine tap [B][time][channels] as the channel-first tensor of decode_ref."""
    return torch.from_numpy(m.get_tap(name)).transpose(1, 2).contiguous()


def symbols(kern, stages):
    return " + ".join(sorted(k for s in stages for k in kern.get(s, ())))


def assert_kernels(kern, want):
    """want: {stage: symbol prefix}; one symbol per stage, of that family."""
    for stage, prefix in want.items():
        assert stage in kern, (stage, sorted(kern))
        syms = sorted(kern[stage])
        assert len(syms) == 1 and syms[0].startswith(prefix), (stage, syms, prefix)


def check_stage(parity_log, case, name, x, got, sd, kern):
    rec = dsr.measure(name, x, sd, got)
    rec.update(test="decode_stream_stage", case=case, kernel=symbols(kern, STAGE_LAUNCHES[name]))
    parity_log.append(rec)
    print(json.dumps(rec))
    assert not dsr.failures(rec), rec


def check_transformer(parity_log, case, x, got, sd, kern):
    """The two conditions of tests/test_decode_kernels.py: the project metric against float64, and against 16 x the
    error of torch-CPU's fp32 evaluation of the same input (floor 2^-24)."""
    ref64 = dsr.transformer(x, sd)
    rec = {"test": "decode_stream_stage", "case": case, "stage": "xfmr7", "rel_err": dsr.rel_err(got, ref64),
           "rel_err_ref": dsr.rel_err(dsr.transformer(x, sd, torch.float32), ref64),
           "kernel": symbols(kern, XFMR_LAUNCHES)}
    parity_log.append(rec)
    print(json.dumps(rec))
    assert rec["rel_err"] < ACT_TOL, rec
    assert rec["rel_err"] <= dsr.WORKING_FACTOR * max(rec["rel_err_ref"], dsr.U), rec


@pytest.fixture(scope="module")
def staged(dec):
    """B = 2 x T = 13 in steps [1, 1, 1, 1, 1, 3, 5] with taps on: every tap concatenated in time, the kernels of the
    last step, and the taps of a one-shot decode of the same codes."""
    codes = rand_codes(13, 2, 8, 13)
    split = [1, 1, 1, 1, 1, 3, 5]
    parts = {n: [] for n in TAPS}
    dec.set_taps(True)
    try:
        with dec.decode_stream(batch=2, num_quantizers=8, max_step_frames=5) as st:
            ys = []
            for i, c in enumerate(steps_of(codes, split)):
                last = i == len(split) - 1
                if last:
                    dec.set_profiling(1)
                try:
                    ys.append(st.step(c).cpu())
                    if last:
                        seq = dec.profile_sequence()
                finally:
                    if last:
                        dec.set_profiling(0)
                for n in TAPS:
                    parts[n].append(tap_cf(dec, n))
                    assert parts[n][-1].shape[0] == 2 and parts[n][-1].shape[2] % c.shape[2] == 0, (n, parts[n][-1].shape)
        taps = {n: torch.cat(v, dim=-1) for n, v in parts.items()}
        one = dec.decode(codes).audio_values.cpu()
        oneshot = {n: tap_cf(dec, n) for n in ("quantized", "upsample")}
    finally:
        dec.set_taps(False)
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    taps["codes"] = codes
    return codes, torch.cat(ys, dim=-1), taps, kern, one, oneshot


def test_step_kernels(staged):
    _, y, taps, kern, _, _ = staged
    assert_kernels(kern, {"dec_attention": "mimi::attention_stream_kernel", "dec_upsample": "mimi::upsample_dw_hist_kernel",
                          "dec_res_s0": "mimi::resblock_hist_kernel<512,", "dec_res_s1": "mimi::resblock_hist_kernel<256,",
                          "dec_res_s2": "mimi::resblock_hist_kernel<128,", "dec_res_s3": "mimi::resblock_hist_kernel<64,",
                          "dec_final": "mimi::final_conv_hist_kernel", "dec_rvq": "mimi::rvq_decode_kernel",
                          "dec_output_proj": G64, "dec_qkv": G64, "dec_o_proj": G64, "dec_fc1": G64, "dec_fc2": G64,
                          "dec_conv0": G64, "dec_conv0_tap": G64, "dec_up_s0": G64, "dec_up_s1": G64, "dec_up_s2": G64,
                          # the profiled step brings 5 frames: up conv 3 has 2400 rows per item, past run_auto's 1024
                          "dec_up_s3": "mimi::gemm_f32_kernel<128, 128,"})
    assert torch.equal(taps["audio"][:, 0], y[:, 0])  # the tap is the returned waveform


def test_taps_concatenate_to_the_sequence(staged, full_sd, parity_log):
    codes, y, taps, _, one, oneshot = staged
    assert taps["upsample"].shape == (2, 512, 26) and taps["audio"].shape == (2, 1, FRAME * 13)
    # the same per-row arithmetic on the same input: the bits of a one-shot decode
    assert torch.equal(taps["quantized"], oneshot["quantized"])
    assert torch.equal(taps["upsample"], oneshot["upsample"])
    err = dsr.rel_err(y, decode_ref.decode(codes, full_sd))
    log(parity_log, "decode_stream_B2_T13_steps_1x5_3_5", rel_err=err, rel_err_to_one_shot=dsr.rel_err(y, one))
    assert err < ACT_TOL, err


@pytest.mark.parametrize("name", list(dsr.STAGES))
def test_stage_against_float64(staged, full_sd, parity_log, name):
    _, _, taps, kern, _, _ = staged
    check_stage(parity_log, "stream_B2_T13", name, taps[dsr.STAGES[name].source], taps[name], full_sd, kern)


def test_transformer_against_float64(staged, full_sd, parity_log):
    _, _, taps, kern, _, _ = staged
    check_transformer(parity_log, "stream_B2_T13", taps["upsample"], taps["xfmr7"], full_sd, kern)


# ---- 5. items and streams are their own -----------------------------------------------------------------------------
def test_items_are_their_own(dec):
    codes = torch.cat([rand_codes(50 + i, 1, 8, 13) for i in range(3)])
    assert len({codes[i].numpy().tobytes() for i in range(3)}) == 3
    yb = run_stream(dec, codes, [2, 3, 1, 7])
    for i in range(3):
        assert torch.equal(yb[i], run_stream(dec, codes[i:i + 1], [2, 3, 1, 7])[0]), i


def test_streams_and_interleaved_calls_are_their_own(full_np):
    """A fresh engine, so that the decode between the steps does regrow the workspace the steps run in."""
    split = [2, 3, 1, 7]
    ca, cb = rand_codes(61, 1, 8, 13), rand_codes(62, 2, 8, 13)
    big = rand_codes(63, 2, 8, 65)
    rag, lens = rand_codes(64, 2, 8, 9), [9, 4]
    x = torch.from_numpy(np.stack([synthetic.speech_like(12000, 5, i) for i in range(2)]))
    m = make_engine(full_np)
    try:
        # the same calls with no stream present, and each stream alone
        want_big = m.decode(big).audio_values.cpu()
        want_rag = [t.cpu() for t in m.decode_ragged(rag, lens)]
        want_enc = m.encode_int32(x.cuda(), 8).cpu()
        alone_a, alone_b = run_stream(m, ca, split), run_stream(m, cb, split)
    finally:
        m.close()
    m = make_engine(full_np)
    try:
        sa = m.decode_stream(batch=1, num_quantizers=8, max_step_frames=7)
        sb = m.decode_stream(batch=2, num_quantizers=8, max_step_frames=7)
        ya, yb = [], []
        between = [lambda: m.decode(big).audio_values.cpu(), lambda: [t.cpu() for t in m.decode_ragged(rag, lens)],
                   lambda: m.encode_int32(x.cuda(), 8).cpu(), lambda: m.decode(big).audio_values.cpu()]
        got = []
        for a, b, call in zip(steps_of(ca, split), steps_of(cb, split), between):
            ya.append(sa.step(a).cpu())
            got.append(call())
            yb.append(sb.step(b).cpu())
        sa.close()
        sb.close()
    finally:
        m.close()
    assert torch.equal(torch.cat(ya, dim=-1), alone_a)
    assert torch.equal(torch.cat(yb, dim=-1), alone_b)
    assert torch.equal(got[0], want_big) and torch.equal(got[3], want_big)
    assert all(torch.equal(g, w) for g, w in zip(got[1], want_rag))
    assert torch.equal(got[2], want_enc)


# ---- 6. life cycle --------------------------------------------------------------------------------------------------
def test_reset_gives_the_same_bits(dec):
    codes = rand_codes(71, 1, 8, 13)
    with dec.decode_stream(batch=1, num_quantizers=8, max_step_frames=7) as st:
        first = torch.cat([st.step(c).cpu() for c in steps_of(codes, [2, 3, 1, 7])], dim=-1)
        assert st.position == 13
        st.reset()
        assert st.position == 0
        again = torch.cat([st.step(c).cpu() for c in steps_of(codes, [2, 3, 1, 7])], dim=-1)
    assert torch.equal(first, again)


def test_state_bytes_constant(t130):
    sizes = t130[4]
    assert len(sizes) == 130 and sizes[0] > 0 and sizes[0] == sizes[129] and len(set(sizes)) == 1


def test_bad_step_lengths_leave_the_state_untouched(dec):
    codes = rand_codes(72, 1, 8, 13)
    want = run_stream(dec, codes, [2, 3, 8], max_step_frames=8)
    with dec.decode_stream(batch=1, num_quantizers=8, max_step_frames=8) as st:
        out = [st.step(codes[:, :, :2]).cpu()]
        with pytest.raises(ValueError):
            st.step(codes[:, :, :0])
        with pytest.raises(ValueError):
            st.step(codes[:, :, :9])
        # and through the C entry itself
        c = codes[:, :, :9].to(device=dec.device, dtype=torch.int32).contiguous()
        buf = torch.empty(FRAME * 9, device=dec.device)
        for n in (0, 9, -1):
            assert dec._lib.mimi_decode_stream_step(st._h, ctypes.c_void_p(c.data_ptr()), n,
                                                    ctypes.c_void_p(buf.data_ptr()), dec._stream()) == 1
        assert st.position == 2
        out.append(st.step(codes[:, :, 2:5]).cpu())
        out.append(st.step(codes[:, :, 5:]).cpu())
    assert torch.equal(torch.cat(out, dim=-1), want)


@pytest.mark.parametrize("bad", [2048, -1])
def test_bad_code_fails_the_step_until_reset(dec, bad):
    codes = rand_codes(73, 1, 8, 13)
    want = run_stream(dec, codes, [2, 3, 1, 7])
    before = dec.decode(codes).audio_values.clone()
    with dec.decode_stream(batch=1, num_quantizers=8, max_step_frames=7) as st:
        st.step(codes[:, :, :2])
        poisoned = codes[:, :, 2:5].clone()
        poisoned[0, 7, 2] = bad
        with pytest.raises(ValueError, match="codebook_size"):
            st.step(poisoned)
        with pytest.raises(_lib.MimiHipError, match="reset"):
            st.step(codes[:, :, 2:5])
        assert torch.equal(dec.decode(codes).audio_values, before)  # the engine is unharmed
        st.reset()
        again = torch.cat([st.step(c).cpu() for c in steps_of(codes, [2, 3, 1, 7])], dim=-1)
    assert torch.equal(again, want)


def test_encode_only_model_refuses(state_dict):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    m = MimiHipModel(state_dict, device="cuda:0")
    try:
        with pytest.raises(RuntimeError, match="decode=True"):
            m.decode_stream()
        h = ctypes.c_void_p()
        assert m._lib.mimi_decode_stream_create(m._h, 1, 8, 1, ctypes.byref(h)) == 7  # MIMI_ERR_STATE, as mimi_decode
        assert not h.value
    finally:
        m.close()


def test_out_is_fully_overwritten_and_nothing_past_it(dec):
    codes = rand_codes(74, 1, 8, 3)
    want = run_stream(dec, codes, [3])
    n = FRAME * 3
    buf = torch.full((n + 4096,), float("nan"), device=dec.device)
    out = buf[:n].view(1, 1, n)
    with dec.decode_stream(batch=1, num_quantizers=8, max_step_frames=3) as st:
        y = st.step(codes, out=out)
    assert y.data_ptr() == buf.data_ptr()
    host = buf.cpu()
    assert not torch.isnan(host[:n]).any() and torch.equal(host[:n].view(1, 1, n), want)
    assert torch.isnan(host[n:]).all()
