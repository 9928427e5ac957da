"""GPU: decode-stream steps at serving scale -- 128 and 129 slots in one call, 1022 and 1030 flat rows: the two sides of
the fp32 GEMM's ``M > 1024`` tile boundary, which no other stream test reaches -- and the small boundaries below it.

The oracle for BITS is a ``batch = 1`` stream on the same engine stepped in lock-step (``reset()`` between sessions), for
EVERY session of every test: a session's samples do not depend on its step-mates, on its place in the step, or on the
tile family.  The oracle for VALUES is ``decode_ref.decode`` of the whole session within ``ACT_TOL`` = 1e-4, for the 8
sessions of ``stream_scale_ref.value_sample`` (the big step's first and last item, the items at flat rows 63 / 64 and
1023 / 1024, a session that ends with the big step and one that starts on a reset slot); all 131 would take the CPU
minutes.  The path under test is never its own oracle.

1. the schedule of tests/stream_scale_ref.py (tests/test_stream_scale_ref.py shows on the CPU that it tells a table
   indexed by the wrong thing apart by >= 500 x the tolerance) at m = 128 and 129, ``sliding_window`` = 5;
2. the kernels of its big step; 3. the packed taps of the 1030-row step, stage by stage, for the four items at its
   ends and around row 1024; 4. equal counts at 128 and 129 slots x 4 frames (1024 and 1032 rows): the slot step and the
   lock-step step;
5. 32, 33, 64 and 65 slots x 1 frame, slot form and ragged form; 6. the real window once: 65 slots, three of them
   wrapped; 7. poisoned padding and the output past every item; a bad code in item 100.
"""
import json

import numpy as np
import pytest
import torch

import decode_ref
import decode_stage_ref as dsr
import stream_ragged_ref as rag
import stream_scale_ref as sc
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = 1920
K = sc.K
NMAX = sc.MAX_STEP_FRAMES
INT32_MAX = 2 ** 31 - 1
T64, T128 = "mimi::gemm_f32_kernel<64, 128,", "mimi::gemm_f32_kernel<128, 128,"


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
def dec5(full_np):
    """The engine at ``sliding_window`` = 5: rings of 18 rows, a state of a few KB per slot."""
    from mimi_hip.config import MimiConfig
    m = make_engine(full_np, config=MimiConfig(sliding_window=sc.WINDOW))
    yield m
    m.close()


@pytest.fixture(scope="module")
def dec(full_np):
    m = make_engine(full_np)
    yield m
    m.close()


def rand_codes(seed, T):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, (1, K, T)))


def log(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


def solos(m, jobs, max_step_frames=NMAX):
    """The oracle for bits: name -> (codes [1, K, T], split) through ONE batch = 1 stream in lock-step steps, reset
    between the sessions.  name -> samples [1, 1, 1920 T]."""
    out = {}
    with m.decode_stream(batch=1, num_quantizers=K, max_step_frames=max_step_frames) as st:
        for name, (codes, split) in jobs.items():
            assert sum(split) == codes.shape[2], (name, split, tuple(codes.shape))
            st.reset()
            parts, at = [], 0
            for n in split:
                parts.append(st.step(codes[:, :, at:at + n]))
                at += n
            assert st.positions == [at]
            out[name] = torch.cat(parts, dim=-1).cpu()
    return out


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


def padded(chunks, nmax, fill=0):
    codes = torch.full((len(chunks), K, nmax), fill, dtype=torch.int64)
    for i, c in enumerate(chunks):
        codes[i, :, :c.shape[2]] = c[0]
    return codes, [int(c.shape[2]) for c in chunks]


class Feed:
    """Sessions on the slots of one stream: ``open(slot, codes)``; ``step({slot: frames})`` feeds the listed slots in the
    order listed -- one ragged call, or with ``form`` = "slots" / "all" (equal counts) the slot step / the lock-step
    step.  The samples are kept per slot and the positions checked after every call."""

    def __init__(self, st):
        self.st, self.codes, self.at, self.out = st, {}, {}, {}
        self.pos = [0] * st.batch

    def open(self, slot, codes):
        self.codes[slot], self.at[slot], self.out[slot] = codes, 0, []

    def step(self, counts, form="ragged", fill=0, **kw):
        slots = list(counts)
        nmax = max(counts.values())
        c, frames = padded([self.codes[s][:, :, self.at[s]:self.at[s] + counts[s]] for s in slots], nmax, fill)
        assert frames == [counts[s] for s in slots]
        if form == "ragged":
            y = self.st.step(c, slots=slots, frames=frames, **kw)
        else:
            assert set(frames) == {nmax} and (form == "slots" or slots == list(range(self.st.batch)))
            y = self.st.step(c, slots=slots, **kw) if form == "slots" else self.st.step(c, **kw)
        assert y.shape == (len(slots), 1, FRAME * nmax) and y.dtype == torch.float32 and y.is_cuda
        host = y.cpu()
        for i, s in enumerate(slots):
            self.out[s].append(host[i:i + 1, :, :FRAME * counts[s]])
            self.at[s] += counts[s]
            self.pos[s] += counts[s]
        assert self.st.positions == self.pos and self.st.position == max(self.pos)
        return y

    def samples(self, slot):
        return torch.cat(self.out[slot], dim=-1)


def assert_all_equal(got, want, what):
    bad = [name for name in want if not torch.equal(got[name], want[name])]
    assert not bad, f"{what}: {len(bad)} of {len(want)} sessions differ from their own batch = 1 stream: {bad[:12]}"


# ---- 1. / 2. the schedule, and the kernels of its big step ----------------------------------------------------------
@pytest.fixture(scope="module")
def played(dec5):
    """m -> the schedule run once on a batch = m stream (the big step under the profiler, which changes no bits) and
    every session through the batch = 1 oracle."""
    cache = {}

    def run(m):
        if m in cache:
            return cache[m]
        sessions, sched, split = sc.make_sessions(m), sc.schedule(m), sc.splits(m)
        big = [s for s, _, _ in sched[sc.BIG][1]]
        seq = []
        with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
            size = st.state_bytes

            def step(slots, codes, frames):
                if slots != big or seq:
                    return st.step(codes, slots=slots, frames=frames)
                y = [None]
                seq.extend(profiled(dec5, lambda: y.__setitem__(0, st.step(codes, slots=slots, frames=frames))))
                return y[0]
            got = rag.play(sessions, step, st.reset, lambda: st.positions, schedule=sched, batch=m)
            assert st.state_bytes == size
        alone = solos(dec5, {name: (codes, split[name]) for name, codes in sessions.items()})
        cache[m] = dict(sessions=sessions, got=got, alone=alone, seq=seq, split=split)
        return cache[m]
    return run


@pytest.mark.parametrize("m", sc.M_GPU)
def test_schedule(dec5, played, full_sd, parity_log, m):
    p = played(m)
    assert len(p["got"]) == m + 3
    assert_all_equal(p["got"], p["alone"], f"schedule at m = {m}")
    cfg = RefConfig(sliding_window=sc.WINDOW)
    for name in sc.value_sample(m):
        err = dsr.rel_err(p["got"][name], decode_ref.decode(p["sessions"][name], full_sd, cfg))
        log(parity_log, "decode_stream_scale_schedule", m=m, session=name, split=p["split"][name], rel_err=err)
        assert err < ACT_TOL, (name, err)


@pytest.mark.parametrize("m", sc.M_GPU)
def test_kernels_of_the_big_step(dec5, played, m):
    kern = kernels_of(played(m)["seq"])
    rows = 2 * sum(f for _, _, f in sc.schedule(m)[sc.BIG][1])
    assert rows == {128: 1022, 129: 1030}[m]
    tile = T64 if rows <= 1024 else T128
    # o_proj, fc1 and fc2 run over the flat rows: gemm.hip's run_auto moves them to the 128-row tile at M > 1024
    for stage in ("dec_o_proj", "dec_fc1", "dec_fc2"):
        assert len(kern[stage]) == 8 and all(k.startswith(tile) for k in kern[stage]), (stage, kern[stage])
    # q/k/v runs over the same flat rows but its RoPE epilogue exists on the 64-row tile only: gemm.hip's dispatch
    # launches ROLE_QKV as run<64, 128, ...> whatever M is
    assert len(kern["dec_qkv"]) == 8 and all(k.startswith(T64) for k in kern["dec_qkv"]), kern["dec_qkv"]
    # output_proj of a ragged step is a GEMM per item (tag 110): its M is the longest item's 7 frames
    assert len(kern["dec_output_proj"]) == 1
    assert kern["dec_output_proj"][0].startswith(T64) and kern["dec_output_proj"][0].endswith(", 110>"), kern
    assert set(kern["dec_attention"]) == {"mimi::attention_stream_ragged_kernel"}
    assert set(kern["dec_kv_append"]) == {"mimi::attention_stream_append_ragged_kernel"}
    assert set(kern["dec_carry"]) == {"mimi::stream_carry_ragged_kernel"}
    assert kern["dec_rvq"] == ["mimi::rvq_decode_ragged_kernel"]
    assert kern["dec_upsample"] == ["mimi::upsample_dw_hist_ragged_kernel"]
    assert kern["dec_final"] == ["mimi::final_conv_hist_ragged_kernel"]
    for s in range(4):
        assert kern[f"dec_res_s{s}"][0].startswith("mimi::resblock_hist_ragged_kernel<"), kern
        assert kern[f"dec_up_s{s}"][0].endswith(", 214>"), kern
    assert kern["dec_conv0"][0].endswith(", 103>"), kern
    # as many launches, stage for stage, as a 3-slot ragged step
    x = rand_codes(700, 3)
    with dec5.decode_stream(batch=3, num_quantizers=K, max_step_frames=NMAX) as st:
        seq3 = profiled(dec5, lambda: st.step(torch.cat([x, x]), slots=[2, 0], frames=[3, 1]))
    assert [stage for stage, _ in played(m)["seq"]] == [stage for stage, _ in seq3]


# ---- 3. the packed taps of the 1030-row step ------------------------------------------------------------------------
# the carried stage at 12.5 Hz, every flat-row stage of layer 0 (q/k/v, attention, o_proj, fc1, fc2), the last layer,
# the carried stages of the SEANet at three rates, the padded waveform
TAPS = ["quantized", "upsample", "qkv0", "att0", "oproj0", "ff0", "xfmr0", "att7", "xfmr7", "dconv0_elu", "up0",
        "dres3_elu", "audio"]


def test_packed_taps_of_the_1030_row_step(dec5):
    m = 129
    sessions, sched = sc.make_sessions(m), sc.schedule(m)
    big = sched[sc.BIG][1]
    items = sc.tap_items(m)
    assert items == [0, 126, 127, 128]
    off = [sum(f for _, _, f in big[:j]) for j in range(m)]
    total = sum(f for _, _, f in big)
    cut = {n: sessions[n][:, :, :sum(sc.splits(m)[n][:-1]) if n not in sc.reset_sessions(m) else None] for n in range(m)}
    got = {}
    with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        def step(slots, codes, frames):
            if len(slots) < m:
                return st.step(codes, slots=slots, frames=frames)
            dec5.set_taps(True)
            try:
                y = st.step(codes, slots=slots, frames=frames)
                for n in TAPS:  # only the four items' rows are kept: dres3_elu is 250 MB
                    t = torch.from_numpy(dec5.get_tap(n))
                    assert t.shape[0] == 1 and t.shape[1] % total == 0, (n, tuple(t.shape))
                    f = t.shape[1] // total
                    got[n] = {j: t[0, f * off[j]:f * (off[j] + big[j][2])].clone() for j in items}
            finally:
                dec5.set_taps(False)
            return y
        rag.play(cut, step, st.reset, lambda: st.positions, schedule=sched[:sc.BIG + 1], batch=m)
    assert set(got) == set(TAPS)
    with dec5.decode_stream(batch=1, num_quantizers=K, max_step_frames=NMAX) as sx:
        for j in items:
            _, name, f = big[j]
            codes, split = cut[name], sc.splits(m)[name]
            split = split if name in sc.reset_sessions(m) else split[:-1]
            assert split[-1] == f and sum(split) == codes.shape[2]
            sx.reset()
            at = 0
            for n in split[:-1]:
                sx.step(codes[:, :, at:at + n])
                at += n
            dec5.set_taps(True)
            try:
                sx.step(codes[:, :, at:])
                for n in TAPS:
                    want = torch.from_numpy(dec5.get_tap(n))
                    assert want.shape[0] == 1 and tuple(want.shape[1:]) == tuple(got[n][j].shape), (n, j)
                    assert torch.equal(got[n][j], want[0]), f"{n}: item {j} (slot {big[j][0]}, {f} frames) differs"
            finally:
                dec5.set_taps(False)


# ---- 4. equal counts at 128 and 129 slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", sc.M_GPU)
def test_equal_counts_at_scale(dec5, m):
    """m slots x 4 frames: 1024 flat rows at 128 -- the last M of run_auto's ``M <= 1024``, the 64-row tile -- and 1032
    at 129, the 128-row tile; as a slot step from staggered positions, then as the lock-step step of a fresh stream."""
    n = 4
    tile = T64 if 2 * m * n <= 1024 else T128
    assert (m, tile) in ((128, T64), (129, T128))
    warm = [sc.warm_position(s) for s in range(m)]
    codes = {s: rand_codes(1000 + s, warm[s] + n) for s in range(m)}
    perm = [s for s, _, _ in sc.schedule(m)[sc.BIG][1]]
    with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st)
        for s in range(m):
            f.open(s, codes[s])
        f.step({s: min(warm[s], NMAX) for s in range(m) if warm[s]})
        f.step({s: warm[s] - NMAX for s in reversed(range(m)) if warm[s] > NMAX})
        seq = profiled(dec5, lambda: f.step({s: n for s in perm}, form="slots"))
        got = {s: f.samples(s) for s in range(m)}
    split = {s: [x for x in (min(warm[s], NMAX), warm[s] - NMAX) if x > 0] + [n] for s in range(m)}
    assert_all_equal(got, solos(dec5, {s: (codes[s], split[s]) for s in range(m)}), f"the slot step at {m} x 4")
    names = [k for _, k in seq]
    kern = kernels_of(seq)
    assert not any("ragged" in k for k in names)
    assert set(kern["dec_attention"]) == {"mimi::attention_stream_slots_kernel"}
    assert set(kern["dec_kv_append"]) == {"mimi::attention_stream_append_slots_kernel"}
    assert set(kern["dec_carry"]) == {"mimi::stream_carry_slots_kernel"}
    for stage in ("dec_o_proj", "dec_fc1", "dec_fc2"):
        assert len(kern[stage]) == 8 and all(k.startswith(tile) for k in kern[stage]), (stage, kern[stage])
    assert all(k.startswith(T64) for k in kern["dec_qkv"])

    # the lock-step step of a fresh batch = m stream: one RoPE image for all items
    fresh = {s: codes[s][:, :, :n] for s in range(m)}
    with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st)
        for s in range(m):
            f.open(s, fresh[s])
        seq = profiled(dec5, lambda: f.step({s: n for s in range(m)}, form="all"))
        got = {s: f.samples(s) for s in range(m)}
    assert_all_equal(got, solos(dec5, {s: (fresh[s], [n]) for s in range(m)}), f"the lock-step step at {m} x 4")
    names = [k for _, k in seq]
    kern = kernels_of(seq)
    assert not any("ragged" in k or "slots" in k for k in names), names
    assert set(kern["dec_attention"]) == {"mimi::attention_stream_kernel"}
    for stage in ("dec_o_proj", "dec_fc1", "dec_fc2"):
        assert len(kern[stage]) == 8 and all(k.startswith(tile) for k in kern[stage]), (stage, kern[stage])


# ---- 5. the small boundaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [32, 33, 64, 65])
def test_small_boundaries(dec5, m):
    """m slots x 1 frame = 64, 66, 128 and 130 flat rows (one and two 64-row tiles, exactly and with a remainder) from
    staggered positions: the slot step, then the ragged step (every count 1 but one 2, which forces the ragged kernels)."""
    warm = [(3 * s) % 7 for s in range(m)]
    two = (5 * m) // 7
    last = {s: 2 if s == two else 1 for s in range(m)}
    codes = {s: rand_codes(2000 + 100 * m + s, warm[s] + 1 + last[s]) for s in range(m)}
    perm = [(31 * j + 1) % m for j in range(m)]
    assert sorted(perm) == list(range(m)) and all(p != j for j, p in enumerate(perm))
    with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st)
        for s in range(m):
            f.open(s, codes[s])
        f.step({s: warm[s] for s in range(m) if warm[s]})
        seq_s = profiled(dec5, lambda: f.step({s: 1 for s in perm}, form="slots"))
        seq_r = profiled(dec5, lambda: f.step({s: last[s] for s in reversed(perm)}))
        got = {s: f.samples(s) for s in range(m)}
    assert not any("ragged" in k for _, k in seq_s)
    assert set(kernels_of(seq_s)["dec_attention"]) == {"mimi::attention_stream_slots_kernel"}
    assert set(kernels_of(seq_r)["dec_attention"]) == {"mimi::attention_stream_ragged_kernel"}
    for seq in (seq_s, seq_r):  # 64 .. 132 flat rows: the 64-row tile in both forms
        for stage in ("dec_o_proj", "dec_fc1", "dec_fc2", "dec_qkv"):
            k = kernels_of(seq)[stage]
            assert len(k) == 8 and all(x.startswith(T64) for x in k), (stage, k)
    split = {s: ([warm[s]] if warm[s] else []) + [1, last[s]] for s in range(m)}
    assert_all_equal(got, solos(dec5, {s: (codes[s], split[s]) for s in range(m)}), f"{m} slots x 1 frame")


# ---- 6. the real window once ----------------------------------------------------------------------------------------
def test_real_window_at_65_slots(dec, full_sd, parity_log):
    m = 65
    wrapped = {7: 7, 40: 3, 64: 1}  # slot -> its count in the big step, 133 frames in (266 rows: the ring has wrapped)
    warm = {s: (3 * s) % 7 for s in range(m) if s not in wrapped}
    count = {s: wrapped.get(s, 1 + (5 * s) % 7) for s in range(m)}
    codes = {s: rand_codes(3000 + s, (133 if s in wrapped else warm[s]) + count[s]) for s in range(m)}
    order = [(11 * j + 5) % m for j in range(m)]
    with dec.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        assert 0.5e9 < st.state_bytes < 0.6e9, st.state_bytes
        f = Feed(st)
        for s in range(m):
            f.open(s, codes[s])
        for s in wrapped:
            for _ in range(19):
                f.step({s: 7}, form="slots")
        f.step({s: w for s, w in warm.items() if w})
        f.step({s: count[s] for s in order})
        got = {s: f.samples(s) for s in range(m)}
    split = {s: ([7] * 19 if s in wrapped else [warm[s]] if warm[s] else []) + [count[s]] for s in range(m)}
    assert_all_equal(got, solos(dec, {s: (codes[s], split[s]) for s in range(m)}), "65 slots at the real window")
    err = dsr.rel_err(got[7][..., FRAME * 133:], decode_ref.decode(codes[7], full_sd)[..., FRAME * 133:])
    log(parity_log, "decode_stream_scale_window250", slots=m, rel_err=err)
    assert err < ACT_TOL, err


# ---- 7. neighbours --------------------------------------------------------------------------------------------------
def test_padding_is_never_read_and_output_past_an_item_is_untouched(dec5, played):
    """The big step at m = 129 with every item's padding poisoned (2048, -1 and INT32_MAX in turn) into a caller's
    NaN-filled buffer."""
    m = 129
    p = played(m)
    sched = sc.schedule(m)
    big = sched[sc.BIG][1]
    fills = (2048, -1, INT32_MAX)
    n = m * FRAME * NMAX
    buf = torch.full((n + 4096,), float("nan"), device=dec5.device)
    cut = {name: p["sessions"][name][:, :, :sum(p["split"][name][:(None if name in sc.reset_sessions(m) else -1)])]
           for name in range(m)}
    with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        def step(slots, codes, frames):
            for i, f in enumerate(frames):
                codes[i, :, f:] = fills[i % 3]
            if len(slots) < m:
                return st.step(codes, slots=slots, frames=frames)
            y = st.step(codes, slots=slots, frames=frames, out=buf[:n].view(m, 1, FRAME * NMAX))
            assert y.data_ptr() == buf.data_ptr()
            return y
        got = rag.play(cut, step, st.reset, lambda: st.positions, schedule=sched[:sc.BIG + 1], batch=m)
    want = {name: p["alone"][name][..., :FRAME * cut[name].shape[2]] for name in range(m)}
    assert_all_equal(got, want, "poisoned padding")
    host = buf.cpu()
    assert torch.isnan(host[n:]).all()
    rows = host[:n].view(m, FRAME * NMAX)
    for i, (_, name, f) in enumerate(big):
        assert torch.isnan(rows[i, FRAME * f:]).all() and not torch.isnan(rows[i, :FRAME * f]).any(), (i, name, f)


def test_bad_code_in_item_100_fails_the_listed_slots_only(dec5):
    m = 129
    warm = [sc.warm_position(s) for s in range(m)]
    order = [s for s, _, _ in sc.schedule(m)[sc.BIG][1]]
    unlisted = [order[1], order[64], order[127]]
    listed = [s for s in order if s not in unlisted]
    count = {s: 1 + (5 * s) % 7 for s in range(m)}
    codes = {s: rand_codes(4000 + s, warm[s] + count[s]) for s in range(m)}
    fresh = rand_codes(4200, 4)
    with dec5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st)
        for s in range(m):
            f.open(s, codes[s])
        f.step({s: min(warm[s], NMAX) for s in range(m) if warm[s]})
        f.step({s: warm[s] - NMAX for s in reversed(range(m)) if warm[s] > NMAX})
        poisoned, frames = padded([codes[s][:, :, warm[s]:] for s in listed], NMAX)
        poisoned[100, 5, frames[100] - 1] = 2048  # inside item 100's own frames
        with pytest.raises(ValueError, match="codebook_size"):
            st.step(poisoned, slots=listed, frames=frames)
        assert st.positions == warm
        for s in listed:  # exactly the listed slots refuse: all 126 of them, and (below) none of the other three
            with pytest.raises(_lib.MimiHipError, match="reset"):
                st.step(codes[s][:, :, warm[s]:warm[s] + 1], slots=[s], frames=[1])
        assert st.positions == warm
        st.reset(listed[100])
        f.pos[listed[100]] = 0
        f.open(listed[100], fresh)
        f.step({unlisted[2]: count[unlisted[2]], listed[100]: 4, unlisted[0]: count[unlisted[0]],
                unlisted[1]: count[unlisted[1]]})  # the unlisted slots go on, beside a new session on a reset slot
        got = {s: f.samples(s) for s in unlisted}
        got["fresh"] = f.samples(listed[100])
    jobs = {s: (codes[s], [x for x in (min(warm[s], NMAX), warm[s] - NMAX) if x > 0] + [count[s]]) for s in unlisted}
    jobs["fresh"] = (fresh, [4])
    assert_all_equal(got, solos(dec5, jobs), "the slots a failed step did not list")
