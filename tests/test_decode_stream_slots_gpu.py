"""GPU: a decode stream as a pool of slots (``DecodeStream.step(codes, slots=...)``, ``reset(slot)``, ``positions``).

The oracle for BITS is the ``batch = 1`` stream on the same engine, stepped in lock-step: the path this feature leaves
as it was (tests/test_decode_stream_gpu.py holds it to the reference on its own).  The oracle for VALUES is
``decode_ref.decode`` of a session's whole sequence, within ``ACT_TOL`` = 1e-4 (the project's ``rel_err``).  The slot
path is never its own oracle.

1. staggered sessions at ``sliding_window`` = 5: the schedule of tests/decode_stream_slots_ref.py (four sessions that
   start and end at different times, 1 - 3 slots per call in ascending and permuted order, n over 1, 2, 3, 7, one slot
   reset and reused, one never used); tests/test_decode_stream_slots_ref.py shows on the CPU that this schedule tells
   the likely mistakes apart by >= 10 x the tolerance;
2. the real window: one slot past 250 rows with its ring wrapped (133 frames in steps of 7), beside a fresh slot, then
   reset and replayed over what its ring still holds;
3. the taps, kernels and launch count of a mixed-position step;
4. ``step`` and ``step(slots=all)`` agree, ``step`` after the positions have diverged;
5. bad arguments leave the state alone; 6. a bad code is the problem of the slots of that call only;
7. decodes and encodes between the calls; 8. the ``out`` buffer.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import decode_ref
import decode_stage_ref as dsr
import decode_stream_slots_ref as slots_ref
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = 1920
K = 8


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
        assert st.positions == [at] and st.position == at
    return torch.cat(out, dim=-1)


def log(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


class Feed:
    """Sessions on the slots of one stream: ``open(slot, codes)``, then ``step(slots, n)`` feeds every listed slot its
    next n frames, in the order listed; the samples are kept per slot, the positions checked after every call."""

    def __init__(self, st):
        self.st, self.codes, self.at, self.out = st, {}, {}, {}
        self.pos = [0] * st.batch

    def open(self, slot, codes):
        self.codes[slot], self.at[slot], self.out[slot] = codes, 0, []

    def step(self, slots, n, **kw):
        c = torch.cat([self.codes[s][:, :, self.at[s]:self.at[s] + n] for s in slots])
        assert c.shape[2] == n
        y = self.st.step(c, slots=slots, **kw)
        assert y.shape == (len(slots), 1, FRAME * n) and y.dtype == torch.float32 and y.is_cuda
        for i, s in enumerate(slots):
            self.out[s].append(y[i:i + 1].cpu())
            self.at[s] += n
            self.pos[s] += n
        assert self.st.positions == self.pos and self.st.position == max(self.pos)
        return y

    def reset(self, slot):
        self.st.reset(slot)
        self.pos[slot] = 0
        assert self.st.positions == self.pos

    def samples(self, slot):
        return torch.cat(self.out[slot], dim=-1)


# ---- 1. staggered sessions ------------------------------------------------------------------------------------------
def test_staggered_sessions(full_np, full_sd, parity_log):
    from mimi_hip.config import MimiConfig
    sessions = slots_ref.make_sessions()
    split = slots_ref.splits()
    cfg = RefConfig(sliding_window=slots_ref.WINDOW)
    m = make_engine(full_np, config=MimiConfig(sliding_window=slots_ref.WINDOW))
    try:
        with m.decode_stream(batch=slots_ref.BATCH, num_quantizers=K,
                             max_step_frames=slots_ref.MAX_STEP_FRAMES) as st:
            size = st.state_bytes
            got = slots_ref.play(sessions, lambda slots, codes: st.step(codes, slots=slots), st.reset,
                                 lambda: st.positions)
            assert st.state_bytes == size
        alone = {name: solo(m, codes, split[name]) for name, codes in sessions.items()}
    finally:
        m.close()
    for name, codes in sessions.items():
        err = dsr.rel_err(got[name], decode_ref.decode(codes, full_sd, cfg))
        log(parity_log, "decode_stream_slots_staggered", session=name, split=split[name], rel_err=err)
        assert err < ACT_TOL, (name, err)
        assert torch.equal(got[name], alone[name]), f"session {name} differs from its own batch = 1 stream"


# ---- 2. the real window: a wrapped ring beside a fresh slot ---------------------------------------------------------
def test_wrapped_ring_beside_a_fresh_slot(dec, full_sd, parity_log):
    long_codes, short_codes = rand_codes(500, 137), rand_codes(501, 17)
    with dec.decode_stream(batch=2, num_quantizers=K, max_step_frames=7) as st:
        f = Feed(st)
        f.open(1, long_codes)
        # 133 frames = 266 rows alone: past the window of 250 rows at frame 126, and past the ring's 263 rows (250 - 1 +
        # 2 x 7), so the step that brings rows 259 .. 272 wraps it
        for _ in range(19):
            f.step([1], 7)
        f.open(0, short_codes)
        f.step([0, 1], 1)
        f.step([1, 0], 3)
        first = f.samples(1)
        f.reset(1)
        f.open(1, long_codes[:, :, :13])  # the slot's first 13 frames again, over what its ring still holds
        f.step([1, 0], 7)
        f.step([0, 1], 3)
        f.step([1, 0], 3)
        replay, short = f.samples(1), f.samples(0)
    want_long = decode_ref.decode(long_codes, full_sd)
    for name, y, bits, want in (
            ("long", first, solo(dec, long_codes, [7] * 19 + [1, 3]), want_long),
            ("short", short, solo(dec, short_codes, [1, 3, 7, 3, 3]), decode_ref.decode(short_codes, full_sd)),
            ("replay", replay, solo(dec, long_codes[:, :, :13], [7, 3, 3]), want_long[..., :FRAME * 13])):
        err = dsr.rel_err(y, want)
        log(parity_log, "decode_stream_slots_window250", segment=name, rel_err=err)
        assert err < ACT_TOL, (name, err)
        assert torch.equal(y, bits), f"{name} differs from its own batch = 1 stream"
    assert torch.equal(replay, first[..., :FRAME * 13])  # (the same bits as the slot's first life, then)


# ---- 3. taps, kernels and launch count of a mixed-position step -----------------------------------------------------
TAPS = ["quantized", "upsample", "xfmr7", "dres1_elu", "audio"]


def tapped_step(m, step):
    """One step with taps and profiling on: (the taps, the recorded (stage, kernel) sequence)."""
    m.set_taps(True)
    m.set_profiling(1)
    try:
        step()
        seq = m.profile_sequence()
        taps = {n: torch.from_numpy(m.get_tap(n)).clone() for n in TAPS}
    finally:
        m.set_profiling(0)
        m.set_taps(False)
    return taps, seq


def test_taps_of_a_mixed_position_step(dec):
    x, y = rand_codes(510, 6), rand_codes(511, 3)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:
        st.step(x[:, :, :2], slots=[0])
        st.step(x[:, :, 2:3], slots=[0])
        assert st.positions == [3, 0, 0]
        taps, seq = tapped_step(dec, lambda: st.step(torch.cat([y, x[:, :, 3:]]), slots=[2, 0]))
        assert st.positions == [6, 0, 3]
    with dec.decode_stream(batch=1, num_quantizers=K, max_step_frames=3) as sx:
        sx.step(x[:, :, :2])
        sx.step(x[:, :, 2:3])
        taps_x, _ = tapped_step(dec, lambda: sx.step(x[:, :, 3:]))
    with dec.decode_stream(batch=1, num_quantizers=K, max_step_frames=3) as sy:
        taps_y, _ = tapped_step(dec, lambda: sy.step(y))
    with dec.decode_stream(batch=2, num_quantizers=K, max_step_frames=3) as sl:
        _, seq_lock = tapped_step(dec, lambda: sl.step(torch.cat([y, x[:, :, 3:]])))
    for n in TAPS:
        assert taps[n].shape[0] == 2 and taps_x[n].shape[0] == taps_y[n].shape[0] == 1, n
        assert torch.equal(taps[n][0], taps_y[n][0]), f"{n}: item 0 (slot 2, at frame 0) differs"
        assert torch.equal(taps[n][1], taps_x[n][0]), f"{n}: item 1 (slot 0, at frame 3) differs"
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    assert len(kern["dec_attention"]) == 1 and next(iter(kern["dec_attention"])).startswith("mimi::attention_stream"), kern
    # the same launches as a lock-step step of the same n, stage for stage
    assert len(seq) == len(seq_lock)
    assert [stage for stage, _ in seq] == [stage for stage, _ in seq_lock]


# ---- 4. step and step(slots=all) ------------------------------------------------------------------------------------
def test_step_and_step_slots_agree(dec):
    codes = torch.cat([rand_codes(520 + i, 8) for i in range(3)])
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as a, \
            dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as b:
        for lo, hi in ((0, 2), (2, 3)):
            ya, yb = a.step(codes[:, :, lo:hi]), b.step(codes[:, :, lo:hi], slots=[0, 1, 2])
            assert torch.equal(ya, yb)
        assert a.positions == b.positions == [3, 3, 3]
        # the positions diverge (slot 1 runs ahead), then all slots in one step()
        ahead = [b.step(codes[1:2, :, 3:5], slots=[1]).cpu()]
        assert b.positions == [3, 5, 3] and b.position == 5
        rest = b.step(torch.cat([codes[0:1, :, 3:6], codes[1:2, :, 5:8], codes[2:3, :, 3:6]])).cpu()
        assert b.positions == [6, 8, 6]
    want = [solo(dec, codes[i:i + 1, :, :sum(split)], split, 3)
            for i, split in enumerate(([2, 1, 3], [2, 1, 2, 3], [2, 1, 3]))]
    assert torch.equal(rest[0], want[0][0, :, FRAME * 3:])
    assert torch.equal(torch.cat([ahead[0][0], rest[1]], dim=-1), want[1][0, :, FRAME * 3:])
    assert torch.equal(rest[2], want[2][0, :, FRAME * 3:])


# ---- 5. validation leaves the state alone ---------------------------------------------------------------------------
def test_bad_arguments_leave_the_state_alone(dec):
    ca, cb = rand_codes(530, 9), rand_codes(531, 7)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=4) as st:
        f = Feed(st)
        f.open(0, ca)
        f.open(2, cb)
        f.step([0], 2)
        f.step([2, 0], 3)
        one = ca[:, :, :1]
        for slots, c in (([], ca[:0, :, :1]), ([0, 1, 2, 0], torch.cat([one] * 4)), ([-1], one), ([3], one),
                         ([0, 0], torch.cat([one] * 2)), ([0], ca[:, :, :0]), ([0], ca[:, :, :5])):
            with pytest.raises(ValueError):
                st.step(c, slots=slots)
        with pytest.raises(ValueError):
            st.reset(3)
        # and through the C entries themselves: MIMI_ERR_INVALID_ARGUMENT, whatever else is valid
        c = torch.cat([ca[:, :, :5]] * 4).to(device=dec.device, dtype=torch.int32).contiguous()
        buf = torch.empty(4 * FRAME * 5, device=dec.device)
        cp, bp = ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(buf.data_ptr())

        def call(slots, m, n, codes=cp, audio=bp):
            tab = (ctypes.c_int32 * max(len(slots), 1))(*slots) if slots is not None else None
            return dec._lib.mimi_decode_stream_step_slots(st._h, tab, m, codes, n, audio, dec._stream())

        for slots, m, n in (([0], 0, 1), ([0], -1, 1), ([0, 1, 2, 0], 4, 1), ([-1], 1, 1), ([3], 1, 1), ([0, 0], 2, 1),
                            ([1, 2, 1], 3, 1), ([0], 1, 0), ([0], 1, 5), ([0], 1, -1)):
            assert call(slots, m, n) == 1, (slots, m, n)
        assert call(None, 1, 1) == 1 and call([0], 1, 1, codes=None) == 1 and call([0], 1, 1, audio=None) == 1
        assert dec._lib.mimi_decode_stream_reset_slot(st._h, 3) == 1
        assert dec._lib.mimi_decode_stream_reset_slot(st._h, -1) == 1
        assert dec._lib.mimi_decode_stream_slot_position(st._h, 3) == -1
        assert dec._lib.mimi_decode_stream_slot_position(st._h, -1) == -1
        assert st.positions == [5, 0, 3]
        f.step([0, 2], 4)
        got_a, got_b = f.samples(0), f.samples(2)
    assert torch.equal(got_a, solo(dec, ca, [2, 3, 4], 4))
    assert torch.equal(got_b, solo(dec, cb, [3, 4], 4))


# ---- 6. a bad code is its callers' problem only ---------------------------------------------------------------------
def test_bad_code_fails_the_listed_slots_only(dec):
    c0, c1, c2, fresh = rand_codes(540, 6), rand_codes(541, 9), rand_codes(542, 6), rand_codes(543, 5)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:
        f = Feed(st)
        for s, c in ((0, c0), (1, c1), (2, c2)):
            f.open(s, c)
        f.step([1], 2)
        f.step([0, 1, 2], 2)
        poisoned = torch.cat([c0[:, :, 2:4], c2[:, :, 2:4]]).clone()
        poisoned[1, 7, 1] = 2048
        with pytest.raises(ValueError, match="codebook_size"):
            st.step(poisoned, slots=[0, 2])
        assert st.positions == [2, 4, 2]
        for slots in ([0], [2], [1, 2]):
            good = torch.cat([f.codes[s][:, :, 2:3] for s in slots])
            with pytest.raises(_lib.MimiHipError, match="reset"):
                st.step(good, slots=slots)
        with pytest.raises(_lib.MimiHipError, match="reset"):
            st.step(torch.cat([c0[:, :, :1]] * 3))  # all slots: two of them refuse
        assert st.positions == [2, 4, 2]
        f.step([1], 3)  # the unlisted slot goes on
        f.reset(0)
        f.open(0, fresh)
        f.step([1, 0], 2)
        f.step([0], 3)
        with pytest.raises(_lib.MimiHipError, match="reset"):
            st.step(c2[:, :, 2:3], slots=[2])  # still refuses: only slot 0 was reset
        f.reset(2)
        f.open(2, c2)
        f.step([2], 3)
        f.step([2], 3)
        got1, got0, got2 = f.samples(1), f.samples(0), f.samples(2)
    assert torch.equal(got1, solo(dec, c1, [2, 2, 3, 2], 3))
    assert torch.equal(got0, solo(dec, fresh, [2, 3], 3))
    assert torch.equal(got2, solo(dec, c2, [3, 3], 3))


# ---- 7. neighbours between the calls --------------------------------------------------------------------------------
def test_calls_between_slot_steps(dec, full_np):
    """A fresh engine for the slot steps, so that the decode between them does regrow the workspace they run in; every
    oracle comes from the module's engine, with no slot step anywhere near."""
    ca, cb = rand_codes(550, 13), rand_codes(551, 11)
    big = rand_codes(552, 65, B=2)
    rag, lens = rand_codes(553, 9, B=2), [9, 4]
    x = torch.from_numpy(np.stack([synthetic.speech_like(12000, 5, i) for i in range(2)]))
    want_big = dec.decode(big).audio_values.cpu()
    want_rag = [t.cpu() for t in dec.decode_ragged(rag, lens)]
    want_enc = dec.encode_int32(x.cuda(), 8).cpu()
    want_a, want_b = solo(dec, ca, [2, 3, 1, 7]), solo(dec, cb, [3, 1, 7])
    m = make_engine(full_np)
    try:
        with m.decode_stream(batch=3, num_quantizers=K, max_step_frames=7) as st:
            f = Feed(st)
            f.open(2, ca)
            f.open(0, cb)
            f.step([2], 2)
            got = [m.decode(big).audio_values.cpu()]
            f.step([0, 2], 3)
            got.append([t.cpu() for t in m.decode_ragged(rag, lens)])
            f.step([2, 0], 1)
            got.append(m.encode_int32(x.cuda(), 8).cpu())
            f.step([0, 2], 7)
            got.append(m.decode(big).audio_values.cpu())
            got_a, got_b = f.samples(2), f.samples(0)
    finally:
        m.close()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    assert torch.equal(got[0], want_big) and torch.equal(got[3], want_big)
    assert all(torch.equal(g, w) for g, w in zip(got[1], want_rag))
    assert torch.equal(got[2], want_enc)


# ---- 8. the out buffer ----------------------------------------------------------------------------------------------
def test_out_is_fully_overwritten_and_nothing_past_it(dec):
    ca, cb = rand_codes(560, 5), rand_codes(561, 3)
    n = 2 * FRAME * 3
    buf = torch.full((n + 4096,), float("nan"), device=dec.device)
    out = buf[:n].view(2, 1, FRAME * 3)
    with dec.decode_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:
        f = Feed(st)
        f.open(1, ca)
        f.open(2, cb)
        f.step([1], 2)
        y = f.step([2, 1], 3, out=out)
        with pytest.raises(ValueError):
            st.step(ca[:, :, :3], slots=[0], out=out)  # [2, 1, L] for one slot
    assert y.data_ptr() == buf.data_ptr()
    host = buf.cpu()
    assert not torch.isnan(host[:n]).any() and torch.isnan(host[n:]).all()
    assert torch.equal(host[:n].view(2, 1, -1)[1:2], solo(dec, ca, [2, 3], 3)[..., FRAME * 2:])
    assert torch.equal(host[:n].view(2, 1, -1)[0:1], solo(dec, cb, [3], 3))
