"""GPU: a decode-stream step in which every listed slot brings its own number of frames
(``DecodeStream.step(codes, slots=..., frames=...)``, ``mimi_decode_stream_step_ragged``).

The oracle for BITS is the ``batch = 1`` stream on the same engine, stepped in lock-step: a path this feature leaves as
it was.  The oracle for VALUES is ``decode_ref.decode`` of a session's whole sequence, within ``ACT_TOL`` = 1e-4 (the
project's ``rel_err``).  The ragged path is never its own oracle.

1. the schedule of tests/stream_ragged_ref.py at ``sliding_window`` = 5 (tests/test_stream_ragged_ref.py shows on the
   CPU that it tells the likely mistakes apart by >= 1000 x the tolerance);
2. calls whose longest item moves the conv GEMMs to the 128-row tile while the short item's own stream runs 64-row tiles;
3. the real window: a slot 133 frames in, its ring wrapped, steps 7 frames beside a fresh slot that steps 1;
4. poisoned input padding; 5. the output past an item's length; 6. a bad code inside an item;
7. equal counts are the slot step (launch for launch); 8. unequal counts: the same number of launches, ragged kernels;
9. the packed taps of a mixed-count step; 10. other calls between ragged steps; 11. the C entry and every ValueError.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import decode_ref
import decode_stage_ref as dsr
import stream_ragged_ref as rag
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = 1920
K = 8
INT32_MAX = 2 ** 31 - 1


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


def rand_codes(seed, T, B=1):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, (B, K, T)))


def solo(m, codes, split, max_step_frames=7):
    """The oracle for bits: ``codes [1, K, T]`` through a fresh batch = 1 stream in lock-step steps of ``split``."""
    assert codes.shape[0] == 1 and sum(split) == codes.shape[2]
    out, at = [], 0
    with m.decode_stream(batch=1, num_quantizers=K, max_step_frames=max_step_frames) as st:
        for n in split:
            out.append(st.step(codes[:, :, at:at + n]).cpu())
            at += n
        assert st.positions == [at]
    return torch.cat(out, dim=-1)


def log(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


def padded(chunks, nmax, fill=0):
    """[1, K, f_i] chunks -> codes [m, K, nmax] with ``fill`` past each item's frames, and the counts."""
    codes = torch.full((len(chunks), K, nmax), fill, dtype=torch.int64)
    for i, c in enumerate(chunks):
        codes[i, :, :c.shape[2]] = c[0]
    return codes, [int(c.shape[2]) for c in chunks]


class Feed:
    """Sessions on the slots of one stream: ``open(slot, codes)``, then ``step({slot: frames}, nmax)`` feeds every listed
    slot its next frames in one ragged call, in the order listed; the samples are kept per slot and the positions
    checked after every call."""

    def __init__(self, st):
        self.st, self.codes, self.at, self.out = st, {}, {}, {}
        self.pos = [0] * st.batch

    def open(self, slot, codes):
        self.codes[slot], self.at[slot], self.out[slot] = codes, 0, []

    def step(self, counts, nmax=None, fill=0, **kw):
        slots = list(counts)
        nmax = nmax or max(counts.values())
        c, frames = padded([self.codes[s][:, :, self.at[s]:self.at[s] + counts[s]] for s in slots], nmax, fill)
        assert frames == [counts[s] for s in slots]
        y = self.st.step(c, slots=slots, frames=frames, **kw)
        assert y.shape == (len(slots), 1, FRAME * nmax) and y.dtype == torch.float32 and y.is_cuda
        for i, s in enumerate(slots):
            self.out[s].append(y[i:i + 1, :, :FRAME * counts[s]].cpu())
            self.at[s] += counts[s]
            self.pos[s] += counts[s]
        assert self.st.positions == self.pos and self.st.position == max(self.pos)
        return y

    def samples(self, slot):
        return torch.cat(self.out[slot], dim=-1)


def profiled(m, step):
    m.set_profiling(1)
    try:
        step()
        return m.profile_sequence()
    finally:
        m.set_profiling(0)


def kernels_of(seq):
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, []).append(kernel)
    return kern


# ---- 1. the schedule ------------------------------------------------------------------------------------------------
def test_schedule(full_np, full_sd, parity_log):
    from mimi_hip.config import MimiConfig
    sessions = rag.make_sessions()
    split = rag.splits()
    cfg = RefConfig(sliding_window=rag.WINDOW)
    m = make_engine(full_np, config=MimiConfig(sliding_window=rag.WINDOW))
    try:
        with m.decode_stream(batch=rag.BATCH, num_quantizers=K, max_step_frames=rag.MAX_STEP_FRAMES) as st:
            size = st.state_bytes
            got = rag.play(sessions, lambda slots, codes, frames: st.step(codes, slots=slots, frames=frames), st.reset,
                           lambda: st.positions)
            assert st.state_bytes == size
        alone = {name: solo(m, codes, split[name]) for name, codes in sessions.items()}
    finally:
        m.close()
    for name, codes in sessions.items():
        err = dsr.rel_err(got[name], decode_ref.decode(codes, full_sd, cfg))
        log(parity_log, "decode_stream_ragged_schedule", session=name, split=split[name], rel_err=err)
        assert err < ACT_TOL, (name, err)
        assert torch.equal(got[name], alone[name]), f"session {name} differs from its own batch = 1 stream"


# ---- 2. the longest item picks the tile -----------------------------------------------------------------------------
@pytest.mark.parametrize("short,long,stage", [(1, 3, "dec_up_s3"), (2, 11, "dec_up_s2")])
def test_tile_is_picked_from_the_longest_item(dec, short, long, stage):
    a, b = rand_codes(600 + short, short + 1), rand_codes(610 + long, long)
    with dec.decode_stream(batch=2, num_quantizers=K, max_step_frames=12) as st:
        f = Feed(st)
        f.open(0, a)
        f.open(1, b)
        f.step({0: 1})
        seq = profiled(dec, lambda: f.step({1: long, 0: short}))
        got_a, got_b = f.samples(0), f.samples(1)
    with dec.decode_stream(batch=1, num_quantizers=K, max_step_frames=12) as sx:
        sx.step(a[:, :, :1])
        seq_short = profiled(dec, lambda: sx.step(a[:, :, 1:]))
    up, up_short = kernels_of(seq)[stage], kernels_of(seq_short)[stage]
    assert len(up) == len(up_short) == 1
    assert up[0].startswith("mimi::gemm_f32_kernel<128, 128,") and up[0].endswith(", 214>"), up
    assert up_short[0].startswith("mimi::gemm_f32_kernel<64, 128,") and up_short[0].endswith(", 14>"), up_short
    assert torch.equal(got_a, solo(dec, a, [1, short], 12)), "the short item differs from its own stream"
    assert torch.equal(got_b, solo(dec, b, [long], 12))


# ---- 3. the real window ---------------------------------------------------------------------------------------------
def test_wrapped_ring_beside_a_fresh_slot(dec, full_sd, parity_log):
    long_codes, short_codes = rand_codes(500, 140), rand_codes(501, 4)
    with dec.decode_stream(batch=2, num_quantizers=K, max_step_frames=7) as st:
        f = Feed(st)
        f.open(1, long_codes)
        for _ in range(19):  # 133 frames = 266 rows: past the window of 250 rows and the ring's 263
            st.step(long_codes[:, :, f.at[1]:f.at[1] + 7], slots=[1])
            f.at[1] += 7
            f.pos[1] += 7
        f.open(0, short_codes)
        f.step({1: 7, 0: 1})
        f.step({0: 3})
        tail, short = f.samples(1), f.samples(0)
    want = solo(dec, long_codes, [7] * 20)
    assert torch.equal(tail, want[..., FRAME * 133:]), "the wrapped slot differs from its own batch = 1 stream"
    assert torch.equal(short, solo(dec, short_codes, [1, 3]))
    err = dsr.rel_err(tail, decode_ref.decode(long_codes, full_sd)[..., FRAME * 133:])
    log(parity_log, "decode_stream_ragged_window250", rel_err=err)
    assert err < ACT_TOL, err


# ---- 4. poisoned input padding --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [-1, 2048, INT32_MAX])
def test_input_padding_is_never_read(dec, fill):
    a, b = rand_codes(620, 5), rand_codes(621, 8)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=7) as st:
        f = Feed(st)
        f.open(2, a)
        f.open(0, b)
        f.step({2: 2, 0: 1}, nmax=3, fill=fill)
        f.step({0: 7, 2: 3}, fill=fill)
        got_a, got_b = f.samples(2), f.samples(0)
    assert torch.equal(got_a, solo(dec, a, [2, 3])) and torch.equal(got_b, solo(dec, b, [1, 7]))


# ---- 5. the output past an item's length ----------------------------------------------------------------------------
def test_output_past_an_item_is_untouched(dec):
    a, b = rand_codes(630, 3), rand_codes(631, 1)
    n = 2 * FRAME * 3
    buf = torch.full((n + 4096,), float("nan"), device=dec.device)
    out = buf[:n].view(2, 1, FRAME * 3)
    with dec.decode_stream(batch=2, num_quantizers=K, max_step_frames=3) as st:
        c, frames = padded([b, a], 3)
        y = st.step(c, slots=[1, 0], frames=frames, out=out)
        assert st.positions == [3, 1]
        with pytest.raises(ValueError):
            st.step(c[:1], slots=[0], frames=[1], out=out)  # [2, 1, L] for one slot
        fresh = rand_codes(632, 2)
        st.reset(1)
        z = st.step(padded([fresh[:, :, :1], fresh[:, :, 1:]], 2)[0][:1], slots=[1], frames=[1])  # allocated by the call
    assert y.data_ptr() == buf.data_ptr()
    host = buf.cpu()
    rows = host[:n].view(2, FRAME * 3)
    assert torch.isnan(host[n:]).all() and torch.isnan(rows[0, FRAME:]).all()
    assert not torch.isnan(rows[0, :FRAME]).any() and not torch.isnan(rows[1]).any()
    assert torch.equal(rows[0, :FRAME], solo(dec, b, [1], 3)[0, 0]) and torch.equal(rows[1], solo(dec, a, [3], 3)[0, 0])
    assert z.shape == (1, 1, FRAME * 2) and (z[..., FRAME:] == 0).all()  # zero past the item when the call allocates


# ---- 6. a bad code inside an item -----------------------------------------------------------------------------------
def test_bad_code_fails_the_listed_slots_only(dec):
    c0, c1, c2 = rand_codes(640, 6), rand_codes(641, 9), rand_codes(642, 6)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:
        f = Feed(st)
        for s, c in ((0, c0), (1, c1), (2, c2)):
            f.open(s, c)
        f.step({1: 2, 0: 1, 2: 3})
        poisoned, frames = padded([c0[:, :, 1:2], c2[:, :, 3:6]], 3)
        poisoned[1, 7, 2] = 2048  # inside item 1's three frames
        with pytest.raises(ValueError, match="codebook_size"):
            st.step(poisoned, slots=[0, 2], frames=frames)
        assert st.positions == [1, 2, 3]
        for slots in ([0], [2], [1, 2]):
            good, fr = padded([f.codes[s][:, :, f.at[s]:f.at[s] + 1] for s in slots], 2)
            with pytest.raises(_lib.MimiHipError, match="reset"):
                st.step(good, slots=slots, frames=fr)
        assert st.positions == [1, 2, 3]
        f.step({1: 3})  # the unlisted slot goes on
        st.reset(0)
        f.pos[0] = 0
        f.open(0, c0)
        f.step({1: 1, 0: 3})
        got1, got0 = f.samples(1), f.samples(0)
    assert torch.equal(got1, solo(dec, c1[:, :, :6], [2, 3, 1], 3))
    assert torch.equal(got0, solo(dec, c0[:, :, :3], [3], 3))


# ---- 7. / 8. the launches -------------------------------------------------------------------------------------------
def test_equal_counts_are_the_slot_step(dec):
    x = rand_codes(650, 6, B=2)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as a, \
            dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as b:
        a.step(x[:1, :, :1], slots=[2])
        b.step(x[:1, :, :1], slots=[2])
        ya, yb = [None], [None]
        seq_r = profiled(dec, lambda: ya.__setitem__(0, a.step(x[:, :, 1:4], slots=[2, 0], frames=[3, 3])))
        seq_s = profiled(dec, lambda: yb.__setitem__(0, b.step(x[:, :, 1:4], slots=[2, 0])))
        assert a.positions == b.positions == [3, 0, 4]
    assert seq_r == seq_s and not any("ragged" in k for _, k in seq_r)
    assert torch.equal(ya[0], yb[0])


def test_unequal_counts_keep_the_launch_count(dec):
    x = rand_codes(651, 6, B=2)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as a, \
            dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as b:
        seq_r = profiled(dec, lambda: a.step(x[:, :, :3], slots=[2, 0], frames=[3, 1]))
        seq_s = profiled(dec, lambda: b.step(x[:, :, :3], slots=[2, 0]))
        seq_r1 = profiled(dec, lambda: a.step(x[:, :, 3:5], slots=[0, 2], frames=[2, 1]))
        assert a.positions == [3, 0, 4]
    assert len(seq_r) == len(seq_s) == len(seq_r1)
    assert [stage for stage, _ in seq_r] == [stage for stage, _ in seq_s] == [stage for stage, _ in seq_r1]
    kern = kernels_of(seq_r)
    assert set(kern["dec_attention"]) == {"mimi::attention_stream_ragged_kernel"}
    assert set(kern["dec_kv_append"]) == {"mimi::attention_stream_append_ragged_kernel"}
    assert set(kern["dec_carry"]) == {"mimi::stream_carry_ragged_kernel"}
    assert kern["dec_rvq"] == ["mimi::rvq_decode_ragged_kernel"]
    assert kern["dec_upsample"] == ["mimi::upsample_dw_hist_ragged_kernel"]
    assert kern["dec_final"] == ["mimi::final_conv_hist_ragged_kernel"]
    for s in range(4):
        assert kern[f"dec_res_s{s}"][0].startswith("mimi::resblock_hist_ragged_kernel<"), kern
        assert kern[f"dec_up_s{s}"][0].endswith(", 214>"), kern
    assert kern["dec_conv0"][0].endswith(", 103>") and kern["dec_output_proj"][0].endswith(", 110>"), kern
    # the flat-row stages run what they always ran
    flat = kernels_of(seq_s)
    for stage in ("dec_layernorm", "dec_qkv", "dec_o_proj", "dec_fc1", "dec_fc2"):
        assert kern[stage] == flat[stage], stage


# ---- 9. the packed taps ---------------------------------------------------------------------------------------------
# every kind of stage: a carried stage at 12.5 Hz, the flat rows, the raw layer-0 output (a GEMM of its own), the
# carried stages of the SEANet at three rates, the padded waveform
TAPS = ["quantized", "upsample", "xfmr7", "dconv0", "dconv0_elu", "up0", "dres1_elu", "dres3_elu", "audio"]


def tapped(m, step):
    m.set_taps(True)
    try:
        step()
        return {n: torch.from_numpy(m.get_tap(n)).clone() for n in TAPS}
    finally:
        m.set_taps(False)


def test_packed_taps_of_a_mixed_count_step(dec):
    x, y = rand_codes(660, 6), rand_codes(661, 1)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:
        st.step(x[:, :, :3], slots=[0])
        c, frames = padded([y, x[:, :, 3:]], 3)
        taps = tapped(dec, lambda: st.step(c, slots=[2, 0], frames=frames))
        assert st.positions == [6, 0, 1]
    with dec.decode_stream(batch=1, num_quantizers=K, max_step_frames=3) as sx:
        sx.step(x[:, :, :3])
        taps_x = tapped(dec, lambda: sx.step(x[:, :, 3:]))
    with dec.decode_stream(batch=1, num_quantizers=K, max_step_frames=3) as sy:
        taps_y = tapped(dec, lambda: sy.step(y))
    for n in TAPS:  # packed [1][f (1 + 3)][C]: item 0's f rows, then item 1's 3 f
        f = taps_y[n].shape[1]
        assert taps_y[n].shape[0] == taps_x[n].shape[0] == 1 and taps_x[n].shape[1] == 3 * f, n
        assert tuple(taps[n].shape) == (1, 4 * f, taps_y[n].shape[2]), (n, tuple(taps[n].shape))
        assert torch.equal(taps[n][0, :f], taps_y[n][0]), f"{n}: item 0 (slot 2, 1 frame) differs"
        assert torch.equal(taps[n][0, f:], taps_x[n][0]), f"{n}: item 1 (slot 0, 3 frames at frame 3) differs"
    assert taps_y["quantized"].shape[1] == 1 and taps_y["upsample"].shape[1] == 2 and taps_y["audio"].shape[1] == FRAME


# ---- 10. neighbours between the calls -------------------------------------------------------------------------------
def test_calls_between_ragged_steps(dec, full_np):
    ca, cb = rand_codes(670, 13), rand_codes(671, 11)
    big = rand_codes(672, 65, B=2)
    rg, lens = rand_codes(673, 9, B=2), [9, 4]
    x = torch.from_numpy(np.stack([synthetic.speech_like(12000, 5, i) for i in range(2)]))
    want_big = dec.decode(big).audio_values.cpu()
    want_rag = [t.cpu() for t in dec.decode_ragged(rg, lens)]
    want_enc = dec.encode_int32(x.cuda(), 8).cpu()
    want_a, want_b = solo(dec, ca, [2, 3, 1, 7]), solo(dec, cb, [1, 2, 7, 1])
    m = make_engine(full_np)  # a fresh engine: the decode between the steps regrows the workspace they run in
    try:
        with m.decode_stream(batch=3, num_quantizers=K, max_step_frames=7) as st:
            f = Feed(st)
            f.open(2, ca)
            f.open(0, cb)
            f.step({2: 2, 0: 1})
            got = [m.decode(big).audio_values.cpu()]
            f.step({0: 2, 2: 3})
            got.append([t.cpu() for t in m.decode_ragged(rg, lens)])
            f.step({2: 1, 0: 7})
            got.append(m.encode_int32(x.cuda(), 8).cpu())
            f.step({0: 1, 2: 7})
            got.append(m.decode(big).audio_values.cpu())
            got_a, got_b = f.samples(2), f.samples(0)
    finally:
        m.close()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    assert torch.equal(got[0], want_big) and torch.equal(got[3], want_big)
    assert all(torch.equal(g, w) for g, w in zip(got[1], want_rag))
    assert torch.equal(got[2], want_enc)


# ---- 11. the C entry and every ValueError ---------------------------------------------------------------------------
def test_c_entry_and_bad_arguments(dec):
    ca, cb = rand_codes(680, 9), rand_codes(681, 7)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=4) as st, \
            dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=4) as sc:
        f = Feed(st)
        f.open(0, ca)
        f.open(2, cb)
        f.step({0: 2, 2: 1})
        one = ca[:, :, :2]
        two = torch.cat([one, one])
        for slots, c, frames in (([0], one, []), ([0], one, [1, 1]), ([0], one, [0]), ([0], one, [3]), ([0], one, [-1]),
                                 ([0, 0], two, [1, 2]), ([3], one, [1]), ([], ca[:0, :, :2], []),
                                 ([0, 2], two[:, :, :0], [1, 1]), ([0], ca[:, :, :5], [5])):
            with pytest.raises(ValueError):
                st.step(c, slots=slots, frames=frames)
        with pytest.raises(ValueError):
            st.step(torch.cat([one] * 3), frames=[1, 2])  # all slots: three counts
        assert st.positions == [2, 0, 1]

        # the C entry itself: the same call as frames=, then MIMI_ERR_INVALID_ARGUMENT whatever else is valid
        c, frames = padded([ca[:, :, :2], cb[:, :, :1]], 2)
        dev = c.to(device=dec.device, dtype=torch.int32).contiguous()
        buf = torch.zeros(2, 1, FRAME * 2, device=dec.device)
        cp, bp = ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(buf.data_ptr())

        def call(slots, frames, m, nmax, codes=cp, audio=bp):
            tab = (ctypes.c_int32 * max(len(slots), 1))(*slots) if slots is not None else None
            fr = (ctypes.c_int32 * max(len(frames), 1))(*frames) if frames is not None else None
            return dec._lib.mimi_decode_stream_step_ragged(sc._h, tab, fr, m, nmax, codes, audio, dec._stream())

        assert call([0, 2], frames, 2, 2) == 0 and sc.positions == [2, 0, 1]
        want = torch.cat([f.out[0][0], torch.cat([f.out[2][0], torch.zeros(1, 1, FRAME)], dim=-1)])
        assert torch.equal(buf.cpu(), want), "the C entry differs from frames="
        for slots, fr, m, nmax in (([0], [1], 0, 1), ([0], [1], -1, 1), ([0, 1, 2, 0], [1] * 4, 4, 1), ([-1], [1], 1, 1),
                                   ([3], [1], 1, 1), ([0, 0], [1, 1], 2, 1), ([0], [0], 1, 1), ([0], [2], 1, 1),
                                   ([0], [-1], 1, 1), ([0], [1], 1, 0), ([0], [1], 1, 5), ([0], [5], 1, 5)):
            assert call(slots, fr, m, nmax) == 1, (slots, fr, m, nmax)
        assert call(None, [1], 1, 1) == 1 and call([0], None, 1, 1) == 1
        assert call([0], [1], 1, 1, codes=None) == 1 and call([0], [1], 1, 1, audio=None) == 1
        assert sc.positions == [2, 0, 1]
        f.step({2: 4, 0: 3})
        got_a, got_b = f.samples(0), f.samples(2)
    assert torch.equal(got_a, solo(dec, ca[:, :, :5], [2, 3], 4))
    assert torch.equal(got_b, solo(dec, cb[:, :, :5], [1, 4], 4))
