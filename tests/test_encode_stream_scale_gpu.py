"""GPU: encode-stream steps at serving scale -- 128 and 129 slots in one call, 1022 and 1030 flat rows: the two sides of
the fp32 GEMM's ``M > 1024`` tile boundary -- and the small boundaries below it.  The encode twin of
tests/test_decode_stream_scale_gpu.py, on the same schedule (tests/stream_scale_ref.py).

Codes are quantised and can hide a small error, so the oracle for BITS is the ``proj`` tap (the RVQ's input) and the
``downsample`` tap (the pre-quantizer embedding) of a ``batch = 1`` stream on the same engine stepped in lock-step, for
EVERY session of every test; the codes must be equal as well.  The oracle for VALUES is ``mimi_ref.pre_quantizer`` of the
whole clip within ``ACT_TOL`` = 1e-4, for the 8 sessions of ``stream_scale_ref.value_sample``.  The path under test is
never its own oracle.

1. the schedule at m = 128 and 129, ``sliding_window`` = 5, every item's padding NaN; 2. the kernels of its big step;
3. the packed taps of the 1030-row step for the four items at its ends and around row 1024; 4. equal counts at 128
and 129 slots x 4 frames (1024 and 1032 rows); 5. 32, 33, 64 and 65 slots x 1 frame; 6. the real window once: 65
slots, three of them 133 frames in, their rings wrapped; 7. NaN / Inf padding and the codes past every item; 8. the 12
fresh slots inside the big step (the replicate fill is each item's own first row); 9. the round trip: the big step's
codes through the decode stream's big step.
"""
import json

import pytest
import torch

import encode_stream_ref as esr
import stream_ragged_ref as rag
import stream_scale_ref as sc
from conftest import assert_codes_in_range
from mimi_hip import synthetic
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = esr.FRAME
K = sc.K
NMAX = sc.MAX_STEP_FRAMES
SENTINEL = -7
T64, T128 = "mimi::gemm_f32_kernel<64, 128,", "mimi::gemm_f32_kernel<128, 128,"


@pytest.fixture(scope="module")
def full_np(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return sd


def make_engine(full_np, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(full_np, device="cuda:0", decode=True, **kw)


@pytest.fixture(scope="module")
def enc5(full_np):
    """The engine at ``sliding_window`` = 5 (with the decoder, for the round trip)."""
    from mimi_hip.config import MimiConfig
    m = make_engine(full_np, config=MimiConfig(sliding_window=sc.WINDOW))
    yield m
    m.close()


@pytest.fixture(scope="module")
def enc(full_np):
    m = make_engine(full_np)
    yield m
    m.close()


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def speech(frames, seed, index):
    return torch.from_numpy(synthetic.speech_like(FRAME * frames, seed, index))[None, None]


def item_taps(m, frames, nmax):
    """The ``downsample`` and ``proj`` taps of the step just run, cut per item: [(ds [f, 512], proj [f, 512])].  A ragged
    step packs them ([1][sum][C]); a step of equal counts holds [m][n][C]."""
    cut = []
    for name in ("downsample", "proj"):
        t = torch.from_numpy(m.get_tap(name).copy())
        t = t.reshape(-1, t.shape[-1])
        packed = t.shape[0] == sum(frames)
        assert packed or t.shape[0] == len(frames) * nmax, (name, tuple(t.shape), sum(frames), nmax)
        rows, at = [], 0
        for f in frames:
            rows.append(t[at:at + f])
            at += f if packed else nmax
        cut.append(rows)
    return list(zip(*cut))


def solos(m, jobs, max_step_frames=NMAX, taps_from=0):
    """The oracle for bits: name -> (audio [1, 1, 1920 T], split) through ONE batch = 1 stream in lock-step steps, reset
    between the sessions.  name -> dict(codes [1, K, T], ds [T, 512], proj [T, 512]); with ``taps_from`` = -1 the taps
    are those of the last step only."""
    out = {}
    with m.encode_stream(batch=1, num_quantizers=K, max_step_frames=max_step_frames) as st:
        for name, (audio, split) in jobs.items():
            st.reset()
            codes, ds, proj = [], [], []
            chunks = list(esr.chunks(audio, split))
            for i, a in enumerate(chunks):
                tap = taps_from == 0 or i == len(chunks) - 1
                m.set_taps(tap)
                try:
                    codes.append(st.step(a).cpu())
                    if tap:
                        (d, p), = item_taps(m, [split[i]], split[i])
                        ds.append(d)
                        proj.append(p)
                finally:
                    m.set_taps(False)
            assert st.positions == [sum(split)]
            out[name] = dict(codes=torch.cat(codes, dim=-1), ds=torch.cat(ds), proj=torch.cat(proj))
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


def padded(chunks, nmax, fill=float("nan")):
    audio = torch.full((len(chunks), FRAME * nmax), fill, dtype=torch.float32)
    for i, c in enumerate(chunks):
        audio[i, :c.shape[-1]] = c[0, 0]
    return audio, [int(c.shape[-1]) // FRAME for c in chunks]


class Feed:
    """Sessions on the slots of one stream: ``open(slot, audio)``; ``step({slot: frames})`` feeds the listed slots in the
    order listed -- one ragged call, or with ``form`` = "slots" / "all" (equal counts) the slot step / the lock-step
    step; with ``taps`` the step's downsample and proj taps are kept per slot beside the codes."""

    def __init__(self, st, model):
        self.st, self.m, self.audio, self.at, self.out, self.ds, self.proj = st, model, {}, {}, {}, {}, {}
        self.pos = [0] * st.batch

    def open(self, slot, audio):
        self.audio[slot], self.at[slot], self.out[slot], self.ds[slot], self.proj[slot] = audio, 0, [], [], []

    def step(self, counts, form="ragged", fill=float("nan"), taps=True, **kw):
        slots = list(counts)
        nmax = max(counts.values())
        a, frames = padded([self.audio[s][..., FRAME * self.at[s]:FRAME * (self.at[s] + counts[s])] for s in slots],
                           nmax, fill)
        assert frames == [counts[s] for s in slots]
        self.m.set_taps(taps)
        try:
            if form == "ragged":
                y = self.st.step(a, slots=slots, frames=frames, **kw)
            else:
                assert set(frames) == {nmax} and (form == "slots" or slots == list(range(self.st.batch)))
                y = self.st.step(a, slots=slots, **kw) if form == "slots" else self.st.step(a, **kw)
            cut = item_taps(self.m, frames, nmax) if taps else None
        finally:
            self.m.set_taps(False)
        assert y.shape == (len(slots), K, nmax) and y.dtype == torch.int32 and y.is_cuda
        host = y.cpu()
        for i, s in enumerate(slots):
            self.out[s].append(host[i:i + 1, :, :counts[s]])
            assert_codes_in_range(self.out[s][-1])
            if taps:
                self.ds[s].append(cut[i][0])
                self.proj[s].append(cut[i][1])
            self.at[s] += counts[s]
            self.pos[s] += counts[s]
        assert self.st.positions == self.pos and self.st.position == max(self.pos)
        return y

    def result(self, slot):
        return dict(codes=torch.cat(self.out[slot], dim=-1), ds=torch.cat(self.ds[slot]), proj=torch.cat(self.proj[slot]))


def assert_all_equal(got, want, what):
    for key in ("proj", "ds", "codes"):
        bad = [name for name in want if not torch.equal(got[name][key], want[name][key])]
        assert not bad, (f"{what}: {key} of {len(bad)} of {len(want)} sessions differs from their own batch = 1 "
                         f"stream: {bad[:12]}")


def log(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


# ---- 1. the schedule ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def played(enc5):
    """m -> the schedule run once on a batch = m stream with the taps on, and every session through the batch = 1
    oracle."""
    cache = {}

    def run(m):
        if m in cache:
            return cache[m]
        clips, sched, split = sc.make_clips(m), sc.schedule(m), sc.splits(m)
        calls = iter([op[1] for op in sched if op[0] == "step"])
        ds, proj, big_codes = {n: [] for n in clips}, {n: [] for n in clips}, []
        enc5.set_taps(True)
        try:
            with enc5.encode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
                size = st.state_bytes

                def step(slots, audio, frames):
                    items = next(calls)
                    c = st.step(audio, slots=slots, frames=frames)
                    for (_, name, _), (d, p) in zip(items, item_taps(enc5, frames, audio.shape[-1] // FRAME)):
                        ds[name].append(d)
                        proj[name].append(p)
                    if items is sched[sc.BIG][1]:
                        big_codes.append(c.clone())
                    return c
                codes = rag.play_encode(clips, step, st.reset, lambda: st.positions, schedule=sched, batch=m)
                assert st.state_bytes == size
        finally:
            enc5.set_taps(False)
        got = {n: dict(codes=codes[n], ds=torch.cat(ds[n]), proj=torch.cat(proj[n])) for n in clips}
        alone = solos(enc5, {n: (x, split[n]) for n, x in clips.items()})
        cache[m] = dict(clips=clips, got=got, alone=alone, split=split, big_codes=big_codes[0])
        return cache[m]
    return run


@pytest.mark.parametrize("m", sc.M_GPU)
def test_schedule(played, state_dict, parity_log, m):
    p = played(m)
    assert len(p["got"]) == m + 3
    for name, g in p["got"].items():
        assert_codes_in_range(g["codes"])
    assert_all_equal(p["got"], p["alone"], f"schedule at m = {m}")
    sd, cfg = esr.as_tensors(state_dict), RefConfig(sliding_window=sc.WINDOW)
    for name in sc.value_sample(m):
        err = rel_err(p["got"][name]["ds"].t()[None], mimi_ref.pre_quantizer(p["clips"][name], sd, cfg))
        log(parity_log, "encode_stream_scale_schedule", m=m, session=name, split=p["split"][name], rel_err=err)
        assert err < ACT_TOL, (name, err)


# ---- 2. the kernels of the big step ---------------------------------------------------------------------------------
def to_the_big_step(eng, m, clips, big_step, pad=float("nan")):
    """The schedule up to and with the big step on a fresh batch = m stream; ``big_step(st, slots, audio, frames)`` runs
    the big one.  name -> the codes so far."""
    sched, split = sc.schedule(m), sc.splits(m)
    ends = sc.reset_sessions(m)
    cut = {n: clips[n][..., :FRAME * sum(split[n][:(None if n in ends else -1)])] for n in range(m)}
    with eng.encode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        def step(slots, audio, frames):
            if len(slots) < m:
                return st.step(audio, slots=slots, frames=frames)
            return big_step(st, slots, audio, frames)
        return rag.play_encode(cut, step, st.reset, lambda: st.positions, schedule=sched[:sc.BIG + 1], batch=m, pad=pad)


@pytest.mark.parametrize("m", sc.M_GPU)
def test_kernels_of_the_big_step(enc5, played, m):
    seq = []

    def big_step(st, slots, audio, frames):
        y = [None]
        seq.extend(profiled(enc5, lambda: y.__setitem__(0, st.step(audio, slots=slots, frames=frames))))
        return y[0]
    to_the_big_step(enc5, m, played(m)["clips"], big_step)
    kern = kernels_of(seq)
    frames = sum(f for _, _, f in sc.schedule(m)[sc.BIG][1])
    assert frames == {128: 511, 129: 515}[m]
    tile = T64 if 2 * frames <= 1024 else T128
    # o_proj, fc1 and fc2 run over the 2 x frames flat rows: gemm.hip's run_auto moves them to the 128-row tile at M > 1024
    for stage in ("encs_o_proj", "encs_fc1", "encs_fc2"):
        assert len(kern[stage]) == 8 and all(k.startswith(tile) for k in kern[stage]), (stage, kern[stage])
    # q/k/v: its RoPE epilogue exists on the 64-row tile only (gemm.hip's dispatch, ROLE_QKV), whatever M is
    assert len(kern["encs_qkv"]) == 8 and all(k.startswith(T64) for k in kern["encs_qkv"]), kern["encs_qkv"]
    # input_proj runs over the flat FRAMES (511 and 515: both under 1025); the final conv and the downsample of a
    # ragged step are GEMMs per item (tags 104 and 109) whose M is the longest item's rows: 64-row tiles on both sides
    assert len(kern["encs_input_proj"]) == 1 and kern["encs_input_proj"][0].startswith(T64), kern["encs_input_proj"]
    assert kern["encs_final"][0].startswith(T64) and kern["encs_final"][0].endswith(", 104>"), kern["encs_final"]
    assert kern["encs_downsample"][0].startswith(T64) and kern["encs_downsample"][0].endswith(", 109>"), kern
    # the RVQ launcher (ops.hip launch_rvq) has one form boundary: its small-batch form while ceil(frames / 32) * 8 <
    # 256, that is up to 992 frames.  511 and 515 frames are on the same side of it, and the nearest frame count at
    # which the form changes (993) is beyond what a step of 129 x 7 frames can hold: the same kernel as a 3-slot step
    x = speech(3, 41, 0)[0]
    with enc5.encode_stream(batch=3, num_quantizers=K, max_step_frames=NMAX) as st:
        seq3 = profiled(enc5, lambda: st.step(padded([x[None], x[None, ..., :FRAME]], 3)[0], slots=[2, 0], frames=[3, 1]))
    assert len(kern["encs_rvq"]) == 1 and kern["encs_rvq"] == kernels_of(seq3)["encs_rvq"]
    assert "rvq_level" in kern["encs_rvq"][0] and ", 32, 8, 32, " in kern["encs_rvq"][0], kern["encs_rvq"]
    assert [stage for stage, _ in seq] == [stage for stage, _ in seq3]  # as many launches, stage for stage
    assert set(kern["encs_attention"]) == {"mimi::attention_stream_ragged_kernel"}
    assert set(kern["encs_kv_append"]) == {"mimi::attention_stream_append_ragged_kernel"}
    assert set(kern["encs_carry"]) == {"mimi::stream_carry_ragged_kernel"}
    assert kern["encs_conv0"] == ["mimi::conv0_hist_ragged_kernel<64, 7>"]
    assert kern["encs_ds_rows"] == ["mimi::stream_ds_rows_ragged_kernel"]
    for s in range(4):
        assert kern[f"encs_res_s{s}"][0].startswith("mimi::resblock_hist_ragged_kernel<"), kern
        assert kern[f"encs_down_s{s}"][0].endswith(", 103>" if s == 3 else ", 102>"), kern


# ---- 3. the packed taps of the 1030-row step ------------------------------------------------------------------------
TAPS = ["conv0", "res0_elu", "down3_elu", "encoder", "qkv0", "att0", "xfmr7", "downsample", "proj"]


def test_packed_taps_of_the_1030_row_step(enc5, played):
    m = 129
    clips, split = played(m)["clips"], sc.splits(m)
    big = sc.schedule(m)[sc.BIG][1]
    items = sc.tap_items(m)
    assert items == [0, 126, 127, 128]
    off = [sum(f for _, _, f in big[:j]) for j in range(m)]
    total = sum(f for _, _, f in big)
    got = {}

    def big_step(st, slots, audio, frames):
        enc5.set_taps(True)
        try:
            y = st.step(audio, slots=slots, frames=frames)
            for n in TAPS:  # only the four items' rows are kept: conv0 is 250 MB
                t = torch.from_numpy(enc5.get_tap(n))
                assert t.shape[0] == 1 and t.shape[1] % total == 0, (n, tuple(t.shape))
                f = t.shape[1] // total
                got[n] = {j: t[0, f * off[j]:f * (off[j] + big[j][2])].clone() for j in items}
        finally:
            enc5.set_taps(False)
        return y
    to_the_big_step(enc5, m, clips, big_step)
    assert set(got) == set(TAPS)
    ends = sc.reset_sessions(m)
    with enc5.encode_stream(batch=1, num_quantizers=K, max_step_frames=NMAX) as sx:
        for j in items:
            _, name, f = big[j]
            cut = split[name] if name in ends else split[name][:-1]
            assert cut[-1] == f
            sx.reset()
            chunks = list(esr.chunks(clips[name][..., :FRAME * sum(cut)], cut))
            for a in chunks[:-1]:
                sx.step(a)
            enc5.set_taps(True)
            try:
                sx.step(chunks[-1])
                for n in TAPS:
                    want = torch.from_numpy(enc5.get_tap(n))
                    assert want.shape[0] == 1 and tuple(want.shape[1:]) == tuple(got[n][j].shape), (n, j)
                    assert torch.equal(got[n][j], want[0]), f"{n}: item {j} (slot {big[j][0]}, {f} frames) differs"
            finally:
                enc5.set_taps(False)


# ---- 4. equal counts at 128 and 129 slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", sc.M_GPU)
def test_equal_counts_at_scale(enc5, m):
    """m slots x 4 frames: 1024 flat rows at 128 -- the last M of run_auto's ``M <= 1024``, the 64-row tile -- and 1032
    at 129, the 128-row tile; as a slot step from staggered positions, then as the lock-step step of a fresh stream."""
    n = 4
    tile = T64 if 2 * m * n <= 1024 else T128
    assert (m, tile) in ((128, T64), (129, T128))
    warm = [sc.warm_position(s) for s in range(m)]
    audio = {s: speech(warm[s] + n, 43, s) for s in range(m)}
    perm = [s for s, _, _ in sc.schedule(m)[sc.BIG][1]]
    with enc5.encode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st, enc5)
        for s in range(m):
            f.open(s, audio[s])
        f.step({s: min(warm[s], NMAX) for s in range(m) if warm[s]})
        f.step({s: warm[s] - NMAX for s in reversed(range(m)) if warm[s] > NMAX})
        seq = profiled(enc5, lambda: f.step({s: n for s in perm}, form="slots"))
        got = {s: f.result(s) for s in range(m)}
    split = {s: [x for x in (min(warm[s], NMAX), warm[s] - NMAX) if x > 0] + [n] for s in range(m)}
    assert_all_equal(got, solos(enc5, {s: (audio[s], split[s]) for s in range(m)}), f"the slot step at {m} x 4")
    kern = kernels_of(seq)
    assert not any("ragged" in k for _, k in seq)
    assert set(kern["encs_attention"]) == {"mimi::attention_stream_slots_kernel"}
    assert set(kern["encs_kv_append"]) == {"mimi::attention_stream_append_slots_kernel"}
    assert set(kern["encs_carry"]) == {"mimi::stream_carry_slots_kernel"}
    assert kern["encs_ds_rows"] == ["mimi::stream_ds_rows_slots_kernel"]
    for stage in ("encs_o_proj", "encs_fc1", "encs_fc2"):
        assert len(kern[stage]) == 8 and all(k.startswith(tile) for k in kern[stage]), (stage, kern[stage])
    assert all(k.startswith(T64) for k in kern["encs_qkv"])

    # the lock-step step of a fresh batch = m stream
    fresh = {s: audio[s][..., :FRAME * n] for s in range(m)}
    with enc5.encode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st, enc5)
        for s in range(m):
            f.open(s, fresh[s])
        seq = profiled(enc5, lambda: f.step({s: n for s in range(m)}, form="all"))
        got = {s: f.result(s) for s in range(m)}
    assert_all_equal(got, solos(enc5, {s: (fresh[s], [n]) for s in range(m)}), f"the lock-step step at {m} x 4")
    kern = kernels_of(seq)
    assert not any("ragged" in k or "slots" in k for _, k in seq), seq
    assert set(kern["encs_attention"]) == {"mimi::attention_stream_kernel"}
    for stage in ("encs_o_proj", "encs_fc1", "encs_fc2"):
        assert len(kern[stage]) == 8 and all(k.startswith(tile) for k in kern[stage]), (stage, kern[stage])


# ---- 5. the small boundaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [32, 33, 64, 65])
def test_small_boundaries(enc5, m):
    """m slots x 1 frame = 64, 66, 128 and 130 flat rows from staggered positions: the slot step, then the ragged step
    (every count 1 but one 2, which forces the ragged kernels)."""
    warm = [(3 * s) % 7 for s in range(m)]
    two = (5 * m) // 7
    last = {s: 2 if s == two else 1 for s in range(m)}
    audio = {s: speech(warm[s] + 1 + last[s], 47 + m, s) for s in range(m)}
    perm = [(31 * j + 1) % m for j in range(m)]
    assert sorted(perm) == list(range(m)) and all(p != j for j, p in enumerate(perm))
    with enc5.encode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        f = Feed(st, enc5)
        for s in range(m):
            f.open(s, audio[s])
        f.step({s: warm[s] for s in range(m) if warm[s]})
        seq_s = profiled(enc5, lambda: f.step({s: 1 for s in perm}, form="slots"))
        seq_r = profiled(enc5, lambda: f.step({s: last[s] for s in reversed(perm)}))
        got = {s: f.result(s) for s in range(m)}
    assert not any("ragged" in k for _, k in seq_s)
    assert set(kernels_of(seq_s)["encs_attention"]) == {"mimi::attention_stream_slots_kernel"}
    assert set(kernels_of(seq_r)["encs_attention"]) == {"mimi::attention_stream_ragged_kernel"}
    for seq in (seq_s, seq_r):  # 64 .. 132 flat rows: the 64-row tile in both forms
        for stage in ("encs_o_proj", "encs_fc1", "encs_fc2", "encs_qkv"):
            k = kernels_of(seq)[stage]
            assert len(k) == 8 and all(x.startswith(T64) for x in k), (stage, k)
    split = {s: ([warm[s]] if warm[s] else []) + [1, last[s]] for s in range(m)}
    assert_all_equal(got, solos(enc5, {s: (audio[s], split[s]) for s in range(m)}), f"{m} slots x 1 frame")


# ---- 6. the real window once ----------------------------------------------------------------------------------------
def test_real_window_at_65_slots(enc, state_dict, parity_log):
    m = 65
    # slot -> its count in the big step, 133 frames in: 266 rows against the ring's cap = 249 + 14 = 263, so the big
    # step's keys are read across the wrap (rows 263 .. 265 sit at ring rows 0 .. 2)
    wrapped = {7: 7, 40: 3, 64: 1}
    warm = {s: (3 * s) % 7 for s in range(m) if s not in wrapped}
    count = {s: wrapped.get(s, 1 + (5 * s) % 7) for s in range(m)}
    audio = {s: speech(warm[s] + count[s], 53, s) for s in warm}
    for s, f in wrapped.items():
        audio[s] = speech(133 + f, 53, s)
    assert 2 * 133 > enc.config.sliding_window - 1 + 2 * NMAX == 263
    order = [(11 * j + 5) % m for j in range(m)]
    with enc.encode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        assert 0.5e9 < st.state_bytes < 0.6e9, st.state_bytes
        f = Feed(st, enc)
        for s in range(m):
            f.open(s, audio[s])
        for s in wrapped:
            for _ in range(19):
                f.step({s: 7}, form="slots", taps=False)
        f.step({s: w for s, w in warm.items() if w}, taps=False)
        f.step({s: count[s] for s in order})
        got = {s: dict(codes=torch.cat(f.out[s], dim=-1), ds=f.ds[s][-1], proj=f.proj[s][-1]) for s in range(m)}
    split = {s: ([7] * 19 if s in wrapped else [warm[s]] if warm[s] else []) + [count[s]] for s in range(m)}
    assert_all_equal(got, solos(enc, {s: (audio[s], split[s]) for s in range(m)}, taps_from=-1),
                     "65 slots at the real window")
    want = mimi_ref.pre_quantizer(audio[7], esr.as_tensors(state_dict), RefConfig())[..., 133:]
    err = rel_err(got[7]["ds"].t()[None], want)
    log(parity_log, "encode_stream_scale_window250", slots=m, rel_err=err)
    assert err < ACT_TOL, err


# ---- 7. padding and the codes past an item --------------------------------------------------------------------------
def test_padding_is_never_read_and_codes_past_an_item_are_untouched(enc5, played):
    """The big step at m = 129 with every item's padding NaN, +Inf and -Inf in turn, into a caller's buffer of
    sentinels."""
    m = 129
    p = played(m)
    big = sc.schedule(m)[sc.BIG][1]
    fills = (float("nan"), float("inf"), -float("inf"))
    n = m * K * NMAX
    buf = torch.full((n + 1024,), SENTINEL, dtype=torch.int32, device=enc5.device)

    def big_step(st, slots, audio, frames):
        for i, f in enumerate(frames):
            audio[i, :, FRAME * f:] = fills[i % 3]
        y = st.step(audio, slots=slots, frames=frames, out=buf[:n].view(m, K, NMAX))
        assert y.data_ptr() == buf.data_ptr()
        return y
    got = to_the_big_step(enc5, m, p["clips"], big_step)
    for name in range(m):
        want = p["alone"][name]["codes"][..., :got[name].shape[-1]]
        assert torch.equal(got[name], want), f"session {name} differs from its own batch = 1 stream"
    host = buf.cpu()
    assert (host[n:] == SENTINEL).all()
    rows = host[:n].view(m, K, NMAX)
    for i, (_, name, f) in enumerate(big):
        assert (rows[i, :, f:] == SENTINEL).all() and (rows[i, :, :f] >= 0).all(), (i, name, f)


# ---- 8. the fresh slots inside the big step -------------------------------------------------------------------------
@pytest.mark.parametrize("m", sc.M_GPU)
def test_fresh_slots_inside_the_big_step(played, m):
    """12 of the big step's items find their slot at position 0, none of them the step's first item: the downsample's
    replicate fill must be each item's own first row (``stream_ds_rows_ragged_kernel``)."""
    p = played(m)
    big = sc.schedule(m)[sc.BIG][1]
    fresh = [(j, name, f) for j, (s, name, f) in enumerate(big) if sc.warm_position(s) == 0]
    assert len(fresh) == 12 and all(j > 0 for j, _, _ in fresh)
    for j, name, f in fresh:
        assert p["split"][name][0] == f
        for key in ("ds", "proj"):
            assert torch.equal(p["got"][name][key][:f], p["alone"][name][key][:f]), (key, j, name)
        assert torch.equal(p["got"][name]["codes"][..., :f], p["alone"][name]["codes"][..., :f]), (j, name)


# ---- 9. the round trip ----------------------------------------------------------------------------------------------
def test_round_trip_of_the_big_step(enc5, played):
    """The big step's codes, as the encode stream left them on the device, through the decode stream's big step: same
    slots, same counts.  Every item's audio is bitwise that of a batch = 1 decode stream fed its codes."""
    m = 129
    p = played(m)
    big = sc.schedule(m)[sc.BIG][1]
    slots, frames = [s for s, _, _ in big], [f for _, _, f in big]
    codes = p["big_codes"]
    assert tuple(codes.shape) == (m, K, NMAX) and codes.is_cuda
    with enc5.decode_stream(batch=m, num_quantizers=K, max_step_frames=NMAX) as st:
        y = st.step(codes, slots=slots, frames=frames).cpu()
        assert st.positions == [frames[slots.index(s)] for s in range(m)]
    host = codes.cpu()
    with enc5.decode_stream(batch=1, num_quantizers=K, max_step_frames=NMAX) as sx:
        bad = []
        for i, f in enumerate(frames):
            sx.reset()
            if not torch.equal(y[i:i + 1, :, :FRAME * f], sx.step(host[i:i + 1, :, :f]).cpu()):
                bad.append(i)
    assert not bad, f"{len(bad)} items differ from their own batch = 1 decode stream: {bad[:12]}"
