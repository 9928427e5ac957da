"""GPU: an encode stream as a pool of SLOTS (``EncodeStream.step(audio, slots=...)``, ``reset(slot)``), and hostile audio.

The contract (tests/encode_stream_ref.py ``SlotPool``): slot ``s`` IS a ``batch = 1`` stream, and a step that lists it
feeds that stream its item -- whatever the other slots are, where they stand, in which order the step lists them,
whatever was called in between.  Held here to the bit:

* the schedule of ``encode_stream_ref.SCHEDULE`` (the decode slots schedule's shape: four sessions of 9 - 13 frames that
  start and end at different times on four slots at ``sliding_window`` = 5, 1 - 3 slots per call in ascending and
  permuted order, ``n`` over 1, 2, 3, 7, one slot reset and reused -- its downsample carry must be the new session's
  first row, not the old session's --, one never used): every session is its own ``batch = 1`` stream;
* at the real window a slot 133 frames in (its ring wrapped) beside a fresh one, then reset and replayed;
* ``step(audio)`` = ``step(audio, slots=all)``, and the slot-form kernels of a mixed-position step;
* every bad argument, through Python and the C entry, with the sessions continuing to the same bits;
* HOSTILE AUDIO: a slot fed NaN, then Inf, then 1e30 beside a clean slot -- the clean slot is bitwise its own stream, the
  hostile slot's codes stay in ``[0, 2048)``, and after ``reset(slot)`` it equals a fresh stream.

tests/test_encode_stream_ref.py shows on the CPU that the schedule tells a table indexed by the item's place, and a
reset that keeps the downsample carry, from the right answer.
"""
import ctypes
import json

import pytest
import torch

import encode_stream_ref as esr
from conftest import assert_codes_in_range
from mimi_hip import _lib
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = esr.FRAME


@pytest.fixture(scope="module")
def sd(state_dict):
    return esr.as_tensors(state_dict)


def make_engine(state_dict, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(state_dict, device="cuda:0", **kw)


@pytest.fixture(scope="module")
def enc(state_dict):
    m = make_engine(state_dict)
    yield m
    m.close()


@pytest.fixture(scope="module")
def enc5(state_dict):
    from mimi_hip.config import MimiConfig
    m = make_engine(state_dict, config=MimiConfig(sliding_window=esr.WINDOW))
    yield m
    m.close()


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def solo(m, x, split, max_step_frames=None):
    """The codes of a batch = 1 stream fed x in steps of ``split``."""
    with m.encode_stream(batch=1, num_quantizers=8, max_step_frames=max_step_frames or max(split)) as st:
        out = [st.step(a).cpu() for a in esr.chunks(x, split)]
    return torch.cat(out, dim=-1)


def checked(st):
    def step(slots, audio):
        c = st.step(audio, slots=slots)
        assert_codes_in_range(c)
        return c
    return step


# ---- the schedule ---------------------------------------------------------------------------------------------------
def test_schedule_every_session_is_its_own_stream(enc5, sd):
    sessions = {name: esr.clip(name) for name in esr.SESSION_FRAMES}
    cut = esr.splits()
    cfg = RefConfig(sliding_window=esr.WINDOW)
    embs = {name: [] for name in sessions}
    enc5.set_taps(True)
    try:
        with enc5.encode_stream(batch=esr.BATCH, num_quantizers=esr.K, max_step_frames=esr.MAX_STEP_FRAMES) as st:
            size = st.state_bytes
            order = [[name for _, name in op[1]] for op in esr.SCHEDULE if op[0] == "step"]
            calls = iter(order)

            def step(slots, audio):
                c = st.step(audio, slots=slots)
                assert_codes_in_range(c)
                e = torch.from_numpy(enc5.get_tap("downsample").copy()).transpose(1, 2)
                for i, name in enumerate(next(calls)):
                    embs[name].append(e[i:i + 1])
                return c
            got = esr.play(sessions, step, st.reset, lambda: st.positions)
            assert st.state_bytes == size
            assert st.positions[2] == 0  # never used
    finally:
        enc5.set_taps(False)
    for name, x in sessions.items():
        assert torch.equal(got[name], solo(enc5, x, cut[name])), f"session {name} is not its own batch = 1 stream"
        err = rel_err(torch.cat(embs[name], dim=-1), mimi_ref.pre_quantizer(x, sd, cfg))
        print(json.dumps(dict(test="encode_stream_slots", session=name, rel_err=err)))
        assert err < ACT_TOL, (name, err)  # D: the slot A left -- its first row, not A's carry


# ---- the real window: a wrapped ring beside a fresh one -------------------------------------------------------------
def test_wrapped_slot_beside_a_fresh_one_then_replayed(enc):
    long_x, short_x = esr.clip("t133"), esr.clip("t13")
    split = [7] * 19
    alone_long = solo(enc, long_x, split)
    alone_short = solo(enc, short_x, [7, 6], max_step_frames=7)
    with enc.encode_stream(batch=2, num_quantizers=8, max_step_frames=7) as st:
        long_out = [st.step(a, slots=[1]).cpu() for a in esr.chunks(long_x[..., :126 * FRAME], [7] * 18)]
        assert st.positions == [0, 126]
        # slot 1 at frame 126 (252 rows: past the window, its ring wrapped) beside slot 0 at frame 0, listed after it
        y = st.step(torch.cat([long_x[..., 126 * FRAME:], short_x[..., :7 * FRAME]]), slots=[1, 0]).cpu()
        long_out.append(y[:1])
        short_out = [y[1:]]
        assert st.positions == [7, 133]
        short_out.append(st.step(short_x[..., 7 * FRAME:], slots=[0]).cpu())
        assert torch.equal(torch.cat(long_out, dim=-1), alone_long)
        assert torch.equal(torch.cat(short_out, dim=-1), alone_short)
        # the wrapped slot reset and replayed: a fresh stream again (its ring is not cleared, and need not be)
        st.reset(1)
        assert st.positions == [13, 0]
        again = [st.step(a, slots=[1]).cpu() for a in esr.chunks(long_x, split)]
        assert torch.equal(torch.cat(again, dim=-1), alone_long)
        assert st.positions == [13, 133]


# ---- step = step(slots = all), and the kernels of a slot step -------------------------------------------------------
def test_step_means_all_slots_and_slot_kernels(enc):
    xs = [esr.clip(n) for n in ("t13", "t13b", "t13c")]
    alone = [solo(enc, x[..., :9 * FRAME], [2, 3, 4]) for x in xs[:2]] + [solo(enc, xs[2][..., :7 * FRAME], [3, 4])]
    with enc.encode_stream(batch=3, num_quantizers=8, max_step_frames=4) as st:
        out = [[], [], []]
        y = st.step(torch.cat([xs[1][..., :2 * FRAME], xs[0][..., :2 * FRAME]]), slots=[1, 0]).cpu()
        out[1].append(y[:1])
        out[0].append(y[1:])
        assert st.positions == [2, 2, 0]
        # positions differ: step() is the slot step over 0, 1, 2, under the slot-form names
        enc.set_profiling(1)
        try:
            y = st.step(torch.cat([xs[0][..., 2 * FRAME:5 * FRAME], xs[1][..., 2 * FRAME:5 * FRAME],
                                   xs[2][..., :3 * FRAME]])).cpu()
            seq = enc.profile_sequence()
        finally:
            enc.set_profiling(0)
        for i in range(3):
            out[i].append(y[i:i + 1])
        assert st.positions == [5, 5, 3]
        y = st.step(torch.cat([x[..., p * FRAME:(p + 4) * FRAME] for x, p in zip(xs, (5, 5, 3))]), slots=[0, 1, 2]).cpu()
        for i in range(3):
            out[i].append(y[i:i + 1])
        assert st.positions == [9, 9, 7]
    for i in range(3):
        assert torch.equal(torch.cat(out[i], dim=-1), alone[i]), i
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    assert kern["encs_carry"] == {"mimi::stream_carry_slots_kernel"}
    assert kern["encs_attention"] == {"mimi::attention_stream_slots_kernel"}
    assert kern["encs_kv_append"] == {"mimi::attention_stream_append_slots_kernel"}
    assert kern["encs_ds_rows"] == {"mimi::stream_ds_rows_slots_kernel"}
    assert kern["encs_conv0"] == {"mimi::conv0_hist_kernel<64, 7>"}
    assert all(next(iter(kern[f"encs_res_s{s}"])).startswith("mimi::resblock_hist_kernel<") for s in range(4))


# ---- bad arguments --------------------------------------------------------------------------------------------------
def test_bad_arguments_touch_nothing(enc):
    xa, xb = esr.clip("t13"), esr.clip("t13d")
    alone_a, alone_b = solo(enc, xa, [2, 3, 8], 8), solo(enc, xb, [2, 3, 8], 8)
    lib = enc._lib
    with enc.encode_stream(batch=2, num_quantizers=8, max_step_frames=8) as st:
        out = [st.step(torch.cat([xb[..., :2 * FRAME], xa[..., :2 * FRAME]]), slots=[1, 0]).cpu()]
        two = torch.cat([xa[..., 2 * FRAME:5 * FRAME], xb[..., 2 * FRAME:5 * FRAME]])
        for slots, audio in (([], two[:0]), ([0, 1, 0], torch.cat([two, two[:1]])), ([2], two[:1]), ([-1], two[:1]),
                             ([0, 0], two), ([0], two), ([0, 1], two[..., :FRAME - 1]),
                             ([0, 1], torch.cat([two] * 3, dim=-1))):
            with pytest.raises(ValueError):
                st.step(audio, slots=slots)
        with pytest.raises(ValueError):
            st.reset(2)
        with pytest.raises(ValueError):
            st.reset(-1)
        # the C entry itself
        a = two.to(enc.device)[:, 0].contiguous()
        buf = torch.full((2 * 8 * 9,), -7, dtype=torch.int32, device=enc.device)
        ap, bp, s = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(buf.data_ptr()), enc._stream()

        def tab(*v):
            return (ctypes.c_int32 * len(v))(*v)
        h = st._h
        for slots, m, n, audio, codes in ((tab(0, 1), 0, 3, ap, bp), (tab(0, 1), 3, 3, ap, bp), (tab(0, 2), 2, 3, ap, bp),
                                          (tab(-1, 1), 2, 3, ap, bp), (tab(1, 1), 2, 3, ap, bp), (tab(0, 1), 2, 0, ap, bp),
                                          (tab(0, 1), 2, 9, ap, bp), (None, 2, 3, ap, bp), (tab(0, 1), 2, 3, None, bp),
                                          (tab(0, 1), 2, 3, ap, None)):
            assert lib.mimi_encode_stream_step_slots(h, slots, m, audio, n, codes, s) == 1, (list(slots or ()), m, n)
        assert lib.mimi_encode_stream_reset_slot(h, 2) == 1
        assert lib.mimi_encode_stream_slot_position(h, 2) == -1 and lib.mimi_encode_stream_slot_position(h, -1) == -1
        assert bool((buf.cpu() == -7).all())  # nothing was launched
        assert st.positions == [2, 2]
        out.append(st.step(two, slots=[0, 1]).cpu()[[1, 0]])
        out.append(st.step(torch.cat([xb[..., 5 * FRAME:], xa[..., 5 * FRAME:]]), slots=[1, 0]).cpu())
    got = torch.cat(out, dim=-1)
    assert torch.equal(got[1:], alone_a) and torch.equal(got[:1], alone_b)
    with pytest.raises(_lib.MimiHipError):
        _lib.check(lib.mimi_encode_stream_reset_slot(None, 0))


# ---- hostile audio --------------------------------------------------------------------------------------------------
def test_hostile_audio_stays_in_its_slot(enc):
    clean, other = esr.clip("t13"), esr.clip("t13d")
    split = [2, 3, 1, 7]
    alone_clean = solo(enc, clean, split)
    alone_other = solo(enc, other, split)
    poison = [float("nan"), float("inf"), 1e30, -float("inf")]
    with enc.encode_stream(batch=2, num_quantizers=8, max_step_frames=7) as st:
        got = []
        for a, v in zip(esr.chunks(clean, split), poison):
            bad = a.clone()
            bad[..., ::3] = v
            y = st.step(torch.cat([bad, a]), slots=[0, 1])
            assert_codes_in_range(y)  # the hostile slot's codes are unspecified, but they are codes
            got.append(y[1:].cpu())
        assert torch.equal(torch.cat(got, dim=-1), alone_clean), "the clean slot saw its neighbour's NaN / Inf"
        assert st.positions == [13, 13]
        # the carries and the ring of slot 0 hold non-finite rows: clean audio there stays unspecified, in range
        assert_codes_in_range(st.step(other[..., :FRAME], slots=[0]))
        st.reset(0)
        again = [st.step(a, slots=[0]).cpu() for a in esr.chunks(other, split)]
    assert torch.equal(torch.cat(again, dim=-1), alone_other), "reset(slot) left something of the hostile session"
