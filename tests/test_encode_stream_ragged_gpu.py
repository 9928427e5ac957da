"""GPU: an encode-stream step in which every listed slot brings its own number of frames
(``EncodeStream.step(audio, slots=..., frames=...)``, ``mimi_encode_stream_step_ragged``).

The oracle for BITS is the ``batch = 1`` stream on the same engine, stepped in lock-step: a path this feature leaves as
it was.  The oracle for VALUES is ``mimi_ref.pre_quantizer`` of a session's whole clip, within ``ACT_TOL`` = 1e-4.  The
ragged path is never its own oracle.

1. the schedule of tests/stream_ragged_ref.py at ``sliding_window`` = 5 on the encode stream's clips, every item's
   padding NaN (tests/test_stream_ragged_ref.py shows on the CPU that it tells the likely mistakes apart);
2. calls whose longest item moves the conv GEMMs to the 128-row tile while the short item's own stream runs 64-row tiles;
3. the real window: a slot 126 frames in, its ring wrapped, steps 7 frames beside a fresh slot that steps 1 (the
   replicate fill is the fresh slot's own first row);
4. input padding of NaN and Inf; 5. the codes past an item's length; 7. equal counts are the slot step;
8. unequal counts: the same number of launches, ragged kernels; 9. the packed taps; 10. other calls between ragged
   steps; 11. the C entry and every ValueError.
"""
import ctypes
import json

import pytest
import torch

import encode_stream_ref as esr
import stream_ragged_ref as rag
from conftest import assert_codes_in_range
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = esr.FRAME
K = 8
SENTINEL = -7


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


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def solo(m, x, split, max_step_frames=None):
    """The codes of a batch = 1 stream fed x [1, 1, 1920 T] in lock-step steps of ``split``."""
    with m.encode_stream(batch=1, num_quantizers=K, max_step_frames=max_step_frames or max(split)) as st:
        out = [st.step(a).cpu() for a in esr.chunks(x, split)]
    return torch.cat(out, dim=-1)


def padded(chunks, nmax, fill=float("nan")):
    """[1, 1, 1920 f_i] chunks -> audio [m, 1920 nmax] with ``fill`` past each item's samples, and the counts."""
    audio = torch.full((len(chunks), FRAME * nmax), fill, dtype=torch.float32)
    for i, c in enumerate(chunks):
        audio[i, :c.shape[-1]] = c[0, 0]
    return audio, [int(c.shape[-1]) // FRAME for c in chunks]


class Feed:
    """Sessions on the slots of one stream: ``open(slot, audio)``, then ``step({slot: frames}, nmax)`` feeds every listed
    slot its next frames in one ragged call, in the order listed; the codes are kept per slot, the positions checked."""

    def __init__(self, st):
        self.st, self.audio, self.at, self.out = st, {}, {}, {}
        self.pos = [0] * st.batch

    def open(self, slot, audio):
        self.audio[slot], self.at[slot], self.out[slot] = audio, 0, []

    def step(self, counts, nmax=None, fill=float("nan"), **kw):
        slots = list(counts)
        nmax = nmax or max(counts.values())
        a, frames = padded([self.audio[s][..., FRAME * self.at[s]:FRAME * (self.at[s] + counts[s])] for s in slots],
                           nmax, fill)
        assert frames == [counts[s] for s in slots]
        y = self.st.step(a, slots=slots, frames=frames, **kw)
        assert y.shape == (len(slots), K, nmax) and y.dtype == torch.int32 and y.is_cuda
        for i, s in enumerate(slots):
            self.out[s].append(y[i:i + 1, :, :counts[s]].cpu())
            assert_codes_in_range(self.out[s][-1])
            self.at[s] += counts[s]
            self.pos[s] += counts[s]
        assert self.st.positions == self.pos and self.st.position == max(self.pos)
        return y

    def codes(self, slot):
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
def test_schedule(state_dict, sd):
    from mimi_hip.config import MimiConfig
    sessions = {name: esr.clip(name) for name in rag.SESSION_FRAMES}
    cut = rag.splits()
    cfg = RefConfig(sliding_window=rag.WINDOW)
    embs = {name: [] for name in sessions}
    calls = iter([[(name, f) for _, name, f in op[1]] for op in rag.SCHEDULE if op[0] == "step"])
    m = make_engine(state_dict, config=MimiConfig(sliding_window=rag.WINDOW))
    m.set_taps(True)
    try:
        with m.encode_stream(batch=rag.BATCH, num_quantizers=K, max_step_frames=rag.MAX_STEP_FRAMES) as st:
            size = st.state_bytes

            def step(slots, audio, frames):
                c = st.step(audio, slots=slots, frames=frames)
                e = torch.from_numpy(m.get_tap("downsample").copy())  # packed [1][sum][512], or [m][n][512] (equal counts)
                e = e.reshape(-1, e.shape[-1])
                at = 0
                equal = all(f == audio.shape[-1] // FRAME for f in frames)
                for i, (name, f) in enumerate(next(calls)):
                    embs[name].append(e[at:at + f].t()[None])
                    at += f if not equal else audio.shape[-1] // FRAME
                return c
            got = rag.play_encode(sessions, step, st.reset, lambda: st.positions)
            assert st.state_bytes == size and st.positions[2] == 0
        m.set_taps(False)
        alone = {name: solo(m, x, cut[name]) for name, x in sessions.items()}
    finally:
        m.set_taps(False)
        m.close()
    for name, x in sessions.items():
        assert_codes_in_range(got[name])
        assert torch.equal(got[name], alone[name]), f"session {name} is not its own batch = 1 stream"
        err = rel_err(torch.cat(embs[name], dim=-1), mimi_ref.pre_quantizer(x, sd, cfg))
        print(json.dumps(dict(test="encode_stream_ragged_schedule", session=name, split=cut[name], rel_err=err)))
        assert err < ACT_TOL, (name, err)


# ---- 2. the longest item picks the tile -----------------------------------------------------------------------------
@pytest.mark.parametrize("short,long,stage", [(1, 3, "encs_down_s0"), (2, 11, "encs_down_s1")])
def test_tile_is_picked_from_the_longest_item(enc, short, long, stage):
    a, b = esr.clip("t13")[..., :FRAME * (short + 1)], esr.clip("t13b")[..., :FRAME * long]
    with enc.encode_stream(batch=2, num_quantizers=K, max_step_frames=12) as st:
        f = Feed(st)
        f.open(0, a)
        f.open(1, b)
        f.step({0: 1})
        seq = profiled(enc, lambda: f.step({1: long, 0: short}))
        got_a, got_b = f.codes(0), f.codes(1)
    with enc.encode_stream(batch=1, num_quantizers=K, max_step_frames=12) as sx:
        sx.step(a[..., :FRAME])
        seq_short = profiled(enc, lambda: sx.step(a[..., FRAME:]))
    down, down_short = kernels_of(seq)[stage], kernels_of(seq_short)[stage]
    assert len(down) == len(down_short) == 1
    assert down[0].startswith("mimi::gemm_f32_kernel<128, 128,") and down[0].endswith(", 102>"), down
    assert down_short[0].startswith("mimi::gemm_f32_kernel<64, 128,") and down_short[0].endswith(", 2>"), down_short
    assert torch.equal(got_a, solo(enc, a, [1, short], 12)), "the short item differs from its own stream"
    assert torch.equal(got_b, solo(enc, b, [long], 12))


# ---- 3. the real window ---------------------------------------------------------------------------------------------
def test_wrapped_ring_beside_a_fresh_slot(enc):
    long_x, short_x = esr.clip("t133"), esr.clip("t13")[..., :FRAME * 4]
    with enc.encode_stream(batch=2, num_quantizers=K, max_step_frames=7) as st:
        f = Feed(st)
        f.open(1, long_x)
        for a in esr.chunks(long_x[..., :126 * FRAME], [7] * 18):  # 252 rows: past the window, the ring wrapped
            st.step(a, slots=[1])
        f.at[1] = f.pos[1] = 126
        f.open(0, short_x)
        f.step({1: 7, 0: 1})
        f.step({0: 3})
        tail, short = f.codes(1), f.codes(0)
    assert torch.equal(tail, solo(enc, long_x, [7] * 19)[..., 126:]), "the wrapped slot differs from its own stream"
    assert torch.equal(short, solo(enc, short_x, [1, 3], 7)), "the fresh slot differs (its replicate fill is its own row)"


# ---- 4. poisoned input padding --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [float("nan"), float("inf"), -float("inf")])
def test_input_padding_is_never_read(enc, fill):
    a, b = esr.clip("t13")[..., :FRAME * 5], esr.clip("t13c")[..., :FRAME * 8]
    with enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=7) as st:
        f = Feed(st)
        f.open(2, a)
        f.open(0, b)
        f.step({2: 2, 0: 1}, nmax=3, fill=fill)
        f.step({0: 7, 2: 3}, fill=fill)
        got_a, got_b = f.codes(2), f.codes(0)
    assert torch.equal(got_a, solo(enc, a, [2, 3], 7)) and torch.equal(got_b, solo(enc, b, [1, 7], 7))


# ---- 5. the output past an item's length ----------------------------------------------------------------------------
def test_output_past_an_item_is_untouched(enc):
    a, b = esr.clip("t13")[..., :FRAME * 3], esr.clip("t13d")[..., :FRAME]
    n = 2 * K * 3
    buf = torch.full((n + 1024,), SENTINEL, dtype=torch.int32, device=enc.device)
    out = buf[:n].view(2, K, 3)
    with enc.encode_stream(batch=2, num_quantizers=K, max_step_frames=3) as st:
        x, frames = padded([b, a], 3)
        y = st.step(x, slots=[1, 0], frames=frames, out=out)
        assert st.positions == [3, 1]
        with pytest.raises(ValueError):
            st.step(x[:1], slots=[0], frames=[1], out=out)  # [2, K, 3] for one slot
        st.reset(1)
        z = st.step(padded([b], 2)[0], slots=[1], frames=[1])  # allocated by the call: zero past the item
    assert y.data_ptr() == buf.data_ptr()
    host = buf.cpu()
    rows = host[:n].view(2, K, 3)
    assert (host[n:] == SENTINEL).all() and (rows[0, :, 1:] == SENTINEL).all()
    assert torch.equal(rows[0, :, :1], solo(enc, b, [1], 3)[0]) and torch.equal(rows[1], solo(enc, a, [3], 3)[0])
    assert z.shape == (1, K, 2) and (z[..., 1:] == 0).all() and torch.equal(z[..., :1].cpu(), solo(enc, b, [1], 3))


# ---- 7. / 8. the launches -------------------------------------------------------------------------------------------
def test_equal_counts_are_the_slot_step(enc):
    x = torch.cat([esr.clip("t13")[0, :, :FRAME * 4], esr.clip("t13b")[0, :, :FRAME * 4]])
    with enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=3) as a, \
            enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=3) as b:
        a.step(x[:1, :FRAME], slots=[2])
        b.step(x[:1, :FRAME], slots=[2])
        ya, yb = [None], [None]
        seq_r = profiled(enc, lambda: ya.__setitem__(0, a.step(x[:, FRAME:], slots=[2, 0], frames=[3, 3])))
        seq_s = profiled(enc, lambda: yb.__setitem__(0, b.step(x[:, FRAME:], slots=[2, 0])))
        assert a.positions == b.positions == [3, 0, 4]
    assert seq_r == seq_s and not any("ragged" in k for _, k in seq_r)
    assert torch.equal(ya[0], yb[0])


def test_unequal_counts_keep_the_launch_count(enc):
    x = torch.cat([esr.clip("t13")[0, :, :FRAME * 5], esr.clip("t13b")[0, :, :FRAME * 5]])
    with enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=3) as a, \
            enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=3) as b:
        seq_r = profiled(enc, lambda: a.step(x[:, :FRAME * 3], slots=[2, 0], frames=[3, 1]))
        seq_s = profiled(enc, lambda: b.step(x[:, :FRAME * 3], slots=[2, 0]))
        assert a.positions == [1, 0, 3]
    assert len(seq_r) == len(seq_s)
    assert [stage for stage, _ in seq_r] == [stage for stage, _ in seq_s]
    kern, flat = kernels_of(seq_r), kernels_of(seq_s)
    assert set(kern["encs_attention"]) == {"mimi::attention_stream_ragged_kernel"}
    assert set(kern["encs_kv_append"]) == {"mimi::attention_stream_append_ragged_kernel"}
    assert set(kern["encs_carry"]) == {"mimi::stream_carry_ragged_kernel"}
    assert kern["encs_conv0"] == ["mimi::conv0_hist_ragged_kernel<64, 7>"]
    assert kern["encs_ds_rows"] == ["mimi::stream_ds_rows_ragged_kernel"]
    for s in range(4):
        assert kern[f"encs_res_s{s}"][0].startswith("mimi::resblock_hist_ragged_kernel<"), kern
        assert kern[f"encs_down_s{s}"][0].endswith(", 103>" if s == 3 else ", 102>"), kern
    assert kern["encs_final"][0].endswith(", 104>") and kern["encs_downsample"][0].endswith(", 109>"), kern
    # the flat-row stages and the RVQ run what they always ran
    for stage in ("encs_layernorm", "encs_qkv", "encs_o_proj", "encs_fc1", "encs_fc2", "encs_input_proj", "encs_rvq"):
        assert kern[stage] == flat[stage], stage


# ---- 9. the packed taps ---------------------------------------------------------------------------------------------
TAPS = ["conv0", "res0_elu", "down0", "res3_elu", "down3_elu", "encoder", "xfmr7", "downsample", "proj"]


def tapped(m, step):
    m.set_taps(True)
    try:
        step()
        return {n: torch.from_numpy(m.get_tap(n)).clone() for n in TAPS}
    finally:
        m.set_taps(False)


def test_packed_taps_of_a_mixed_count_step(enc):
    x, y = esr.clip("t13")[..., :FRAME * 6], esr.clip("t13b")[..., :FRAME]
    with enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:
        st.step(x[..., :FRAME * 3], slots=[0])
        a, frames = padded([y, x[..., FRAME * 3:]], 3)
        taps = tapped(enc, lambda: st.step(a, slots=[2, 0], frames=frames))
        assert st.positions == [6, 0, 1]
    with enc.encode_stream(batch=1, num_quantizers=K, max_step_frames=3) as sx:
        sx.step(x[..., :FRAME * 3])
        taps_x = tapped(enc, lambda: sx.step(x[..., FRAME * 3:]))
    with enc.encode_stream(batch=1, num_quantizers=K, max_step_frames=3) as sy:
        taps_y = tapped(enc, lambda: sy.step(y))
    for n in TAPS:  # packed [1][f (1 + 3)][C]: item 0's f rows, then item 1's 3 f
        f = taps_y[n].shape[1]
        assert taps_y[n].shape[0] == taps_x[n].shape[0] == 1 and taps_x[n].shape[1] == 3 * f, n
        assert tuple(taps[n].shape) == (1, 4 * f, taps_y[n].shape[2]), (n, tuple(taps[n].shape))
        assert torch.equal(taps[n][0, :f], taps_y[n][0]), f"{n}: item 0 (slot 2, 1 frame, fresh) differs"
        assert torch.equal(taps[n][0, f:], taps_x[n][0]), f"{n}: item 1 (slot 0, 3 frames at frame 3) differs"
    assert taps_y["conv0"].shape[1] == FRAME and taps_y["encoder"].shape[1] == 2 and taps_y["proj"].shape[1] == 1


# ---- 10. neighbours between the calls -------------------------------------------------------------------------------
def test_calls_between_ragged_steps(enc, state_dict):
    xa, xb = esr.clip("t13"), esr.clip("t13c")[..., :FRAME * 11]
    big = torch.cat([esr.clip("t133")[0, :, :FRAME * 60], esr.clip("t133")[0, :, FRAME * 60:FRAME * 120]])
    want_big = enc.encode_int32(big.cuda(), K).cpu()
    want_a, want_b = solo(enc, xa, [2, 3, 1, 7]), solo(enc, xb, [1, 2, 7, 1])
    m = make_engine(state_dict)  # a fresh engine: the encode between the steps grows what they share
    try:
        with m.encode_stream(batch=3, num_quantizers=K, max_step_frames=7) as st:
            f = Feed(st)
            f.open(2, xa)
            f.open(0, xb)
            f.step({2: 2, 0: 1})
            got = [m.encode_int32(big.cuda(), K).cpu()]
            f.step({0: 2, 2: 3})
            f.step({2: 1, 0: 7})
            got.append(m.encode_int32(big.cuda(), K).cpu())
            f.step({0: 1, 2: 7})
            got_a, got_b = f.codes(2), f.codes(0)
    finally:
        m.close()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    assert torch.equal(got[0], want_big) and torch.equal(got[1], want_big)


# ---- 11. the C entry and every ValueError ---------------------------------------------------------------------------
def test_c_entry_and_bad_arguments(enc):
    xa, xb = esr.clip("t13")[..., :FRAME * 9], esr.clip("t13b")[..., :FRAME * 7]
    with enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=4) as st, \
            enc.encode_stream(batch=3, num_quantizers=K, max_step_frames=4) as sc:
        f = Feed(st)
        f.open(0, xa)
        f.open(2, xb)
        f.step({0: 2, 2: 1})
        one = xa[0, :, :FRAME * 2]
        two = torch.cat([one, one])
        for slots, a, frames in (([0], one, []), ([0], one, [1, 1]), ([0], one, [0]), ([0], one, [3]), ([0], one, [-1]),
                                 ([0, 0], two, [1, 2]), ([3], one, [1]), ([0], one[:, :FRAME + 7], [1]),
                                 ([0], xa[0, :, :FRAME * 5], [5])):
            with pytest.raises(ValueError):
                st.step(a, slots=slots, frames=frames)
        with pytest.raises(ValueError):
            st.step(torch.cat([one] * 3), frames=[1, 2])  # all slots: three counts
        assert st.positions == [2, 0, 1]

        # the C entry itself: the same call as frames=, then MIMI_ERR_INVALID_ARGUMENT whatever else is valid
        a, frames = padded([xa[..., :FRAME * 2], xb[..., :FRAME]], 2)
        dev = a.to(enc.device).contiguous()
        buf = torch.zeros(2, K, 2, dtype=torch.int32, device=enc.device)
        ap, bp = ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(buf.data_ptr())

        def call(slots, frames, m, nmax, audio=ap, codes=bp):
            tab = (ctypes.c_int32 * max(len(slots), 1))(*slots) if slots is not None else None
            fr = (ctypes.c_int32 * max(len(frames), 1))(*frames) if frames is not None else None
            return enc._lib.mimi_encode_stream_step_ragged(sc._h, tab, fr, m, nmax, audio, codes, enc._stream())

        assert call([0, 2], frames, 2, 2) == 0 and sc.positions == [2, 0, 1]
        want = torch.zeros(2, K, 2, dtype=torch.int32)
        want[0], want[1, :, :1] = f.out[0][0][0], f.out[2][0][0]
        assert torch.equal(buf.cpu(), want), "the C entry differs from frames="
        for slots, fr, m, nmax in (([0], [1], 0, 1), ([0], [1], -1, 1), ([0, 1, 2, 0], [1] * 4, 4, 1), ([-1], [1], 1, 1),
                                   ([3], [1], 1, 1), ([0, 0], [1, 1], 2, 1), ([0], [0], 1, 1), ([0], [2], 1, 1),
                                   ([0], [-1], 1, 1), ([0], [1], 1, 0), ([0], [1], 1, 5), ([0], [5], 1, 5)):
            assert call(slots, fr, m, nmax) == 1, (slots, fr, m, nmax)
        assert call(None, [1], 1, 1) == 1 and call([0], None, 1, 1) == 1
        assert call([0], [1], 1, 1, audio=None) == 1 and call([0], [1], 1, 1, codes=None) == 1
        assert sc.positions == [2, 0, 1]
        f.step({2: 4, 0: 3})
        got_a, got_b = f.codes(0), f.codes(2)
    assert torch.equal(got_a, solo(enc, xa[..., :FRAME * 5], [2, 3], 4))
    assert torch.equal(got_b, solo(enc, xb[..., :FRAME * 5], [1, 4], 4))
