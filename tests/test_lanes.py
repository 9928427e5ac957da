"""Engine lanes (mimi_set_option "lanes"): encodes kept in flight run side by side on the engine's two lane streams,
each lane with its own workspace, maxima buffers and captured graphs.  Lanes are kernel-agnostic, so the shapes are
tiny; ``rvq_chain = 0`` lets the default rule (uniform f16x3 batches on the per-level RVQ kernels) engage on these
small grids.  Every case compares bitwise with the same encodes run synchronously under ``lanes = 0``."""
import numpy as np
import pytest
import torch

from mimi_hip import synthetic

pytestmark = pytest.mark.gpu

SMALL, OTHER, BIG = (2, 24000), (3, 13440), (2, 96000)
LONG = (1, 252000)  # 263 transformer rows: past the 256-row RoPE table the 10 s calibration leaves behind
LOUD = 3e4          # the amplitude of tests/test_gpu_parity.py::test_f16_overflow_fallback


def make_engine(sd, lanes, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    m = MimiHipModel(sd, device="cuda:0", **kw)
    m.set_option("rvq_chain", 0)
    m.set_option("lanes", lanes)
    return m


@pytest.fixture(scope="module")
def eng(state_dict):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    m = make_engine(state_dict, 1)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ref(state_dict):
    """clip -> its codes from a synchronous encode on an engine with lanes off (computed once per clip)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    m = make_engine(state_dict, 0)
    cache = {}

    def get(x):
        key = (tuple(x.shape), x.cpu().numpy().tobytes())
        if key not in cache:
            cache[key] = m.encode_int32(x, 8).cpu()
            assert m.lane_encodes[1] == 0
        return cache[key]
    get.quantize = lambda emb: m.quantize(emb, 8).cpu()  # (the quantizer alone, on the same engine)
    yield get
    m.close()


def clip(shape, seed):
    return torch.from_numpy(synthetic.clip_batch(shape[0], shape[1], seed=seed)).cuda()


def submit(m, x, log=None):
    """encode_async, noting which lane took it and whether it was a graph replay."""
    l0, r0 = m.lane_encodes, m.graph_replays
    t = m.encode_async(x, 8)
    l1 = m.lane_encodes
    assert sum(l1) == sum(l0) + 1
    if log is not None:
        log.append((0 if l1[0] > l0[0] else 1, tuple(x.shape), m.graph_replays > r0))
    return t


def run_in_flight(m, xs, depth, log):
    """Every clip of xs through encode_async with `depth` encodes kept in flight; the codes, in order."""
    out, fly = [], []
    for x in xs:
        fly.append(submit(m, x, log))
        if len(fly) == depth:
            out.append(fly.pop(0).wait().cpu())
    out += [t.wait().cpu() for t in fly]
    return out


def test_no_cross_talk_and_graphs_on_both_lanes(eng, ref):
    xs = [clip(SMALL if i % 2 == 0 else OTHER, 100 + i) for i in range(16)]
    log = []
    got = run_in_flight(eng, xs[:8], 2, log) + run_in_flight(eng, xs[8:], 4, log)
    for i, (g, x) in enumerate(zip(got, xs)):
        assert torch.equal(g, ref(x)), i
    assert min(eng.lane_encodes) > 0, eng.lane_encodes
    uses, replayed = {}, {0: 0, 1: 0}
    for lane, shape, rep in log:
        uses[lane, shape] = uses.get((lane, shape), 0) + 1
        if uses[lane, shape] >= 3:
            assert rep, (lane, shape, uses[lane, shape])
            replayed[lane] += 1
    assert replayed[0] > 0 and replayed[1] > 0, (replayed, log)


def test_out_of_order_waits_and_ticket_limit(eng, ref):
    from mimi_hip import _lib
    x1, x2 = clip(SMALL, 201), clip(OTHER, 202)
    t1, t2 = submit(eng, x1), submit(eng, x2)
    c2 = t2.wait().cpu()
    c1 = t1.wait().cpu()
    assert torch.equal(c1, ref(x1)) and torch.equal(c2, ref(x2))
    xs = [clip(SMALL, 210 + i) for i in range(16)]
    fly = [submit(eng, x) for x in xs]
    with pytest.raises(_lib.MimiHipError) as ei:
        eng.encode_async(xs[0], 8)
    assert ei.value.status == 7  # MIMI_ERR_STATE
    for t, x in zip(fly, xs):
        assert torch.equal(t.wait().cpu(), ref(x))


def test_workspace_and_rope_growth_beside_an_encode_in_flight(state_dict, ref):
    m = make_engine(state_dict, 1)
    try:
        for big, seed in ((BIG, 300), (LONG, 310)):
            a, b, c, d = clip(SMALL, seed), clip(big, seed + 1), clip(big, seed + 2), clip(SMALL, seed + 3)
            log = []
            ta = submit(m, a, log)  # lane 0
            tb = submit(m, b, log)  # lane 1: its workspace grows (the RoPE tables: both lanes drained)
            assert [l for l, _, _ in log] == [0, 1]
            assert torch.equal(ta.wait().cpu(), ref(a))
            tc = submit(m, c, log)  # lane 0 grows while lane 1's encode is in flight
            td = submit(m, d, log)
            assert log[2][0] == 0
            for t, x in ((tb, b), (tc, c), (td, d)):
                assert torch.equal(t.wait().cpu(), ref(x))
    finally:
        m.close()


def test_overflow_rerun_beside_an_encode_in_flight(eng, ref):
    quiet = clip(SMALL, 400)
    loud = torch.from_numpy(synthetic.speech_like(48000, 5, 1) * np.float32(LOUD))[None].cuda()
    for first, second in ((quiet, loud), (loud, quiet)):
        before = eng.f16_reruns
        log = []
        t1, t2 = submit(eng, first, log), submit(eng, second, log)
        assert [l for l, _, _ in log] == [0, 1]
        tl, tq = (t2, t1) if first is quiet else (t1, t2)
        cl = tl.wait().cpu()  # the re-run goes through the loud ticket's lane while the other lane may still run
        assert eng.f16_reruns == before + 1
        cq = tq.wait().cpu()
        assert torch.equal(cl, ref(loud)) and torch.equal(cq, ref(quiet))


@pytest.mark.parametrize("gate", ["rvq_chain", "taps", "profiling"])
def test_lane_gating(eng, ref, gate):
    """Encodes that may launch the persistent RVQ chain, taps and per-stage profiling keep every encode in lane 0."""
    m = eng
    try:
        if gate == "rvq_chain":
            m.set_option("rvq_chain", 1)
        elif gate == "taps":
            m.set_taps(True)
        else:
            m.set_profiling(1)
        l0, r0 = m.lane_encodes, m.rvq_chain_reruns
        xs = [clip(SMALL, 500 + i) for i in range(4)]
        got = run_in_flight(m, xs, 2, None)
        assert m.lane_encodes == (l0[0] + 4, l0[1])
        assert m.rvq_chain_reruns == r0 == 0
        for g, x in zip(got, xs):
            assert torch.equal(g, ref(x))
    finally:
        m.set_option("rvq_chain", 0)
        m.set_taps(False)
        m.set_profiling(0)
        m.profile_reset()


def test_sync_encodes_stay_in_lane_0(state_dict, ref):
    m = make_engine(state_dict, 1)
    try:
        x = clip(SMALL, 600)
        for _ in range(2):
            assert torch.equal(m.encode_int32(x, 8).cpu(), ref(x))
        assert m.graph_captures == 1
        assert m.lane_encodes == (2, 0)
    finally:
        m.close()


def test_quantize_between_encodes_in_flight(eng, ref):
    """``quantize`` (mimi_rvq_encode) borrows lane 0's workspace: beside an encode in flight in each lane it gives its
    own bits and leaves theirs alone."""
    emb = torch.from_numpy(np.random.default_rng(11).standard_normal((1, 512, 13)).astype(np.float32)).cuda()
    want = ref.quantize(emb)
    x1, x2 = clip(SMALL, 800), clip(OTHER, 801)
    chain0, f160 = eng.rvq_chain_reruns, eng.f16_reruns
    log = []
    t1, t2 = submit(eng, x1, log), submit(eng, x2, log)
    assert [l for l, _, _ in log] == [0, 1]
    got = eng.quantize(emb, 8).cpu()
    c1, c2 = t1.wait().cpu(), t2.wait().cpu()
    assert torch.equal(got, want)
    assert torch.equal(c1, ref(x1)) and torch.equal(c2, ref(x2))
    assert (eng.rvq_chain_reruns, eng.f16_reruns) == (chain0, f160)


def test_decode_between_encodes_in_flight(state_dict, ref):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    m = make_engine(sd, 1, decode=True)
    try:
        codes = torch.from_numpy(np.random.default_rng(7).integers(0, 2048, (1, 8, 13))).cuda()
        want = m.decode(codes).audio_values.cpu()
        xs = [clip(SMALL if i % 2 == 0 else OTHER, 700 + i) for i in range(8)]
        run_in_flight(m, xs[:6], 2, None)  # three uses of its shape per lane: both lanes hold a graph
        r0, c0 = m.graph_replays, m.graph_captures
        log = []
        t1, t2 = submit(m, xs[6], log), submit(m, xs[7], log)
        wave = m.decode(codes).audio_values.cpu()
        assert torch.equal(t1.wait().cpu(), ref(xs[6])) and torch.equal(t2.wait().cpu(), ref(xs[7]))
        assert torch.equal(wave, want)
        assert [(l, r) for l, _, r in log] == [(0, True), (1, True)]
        assert m.graph_replays == r0 + 2 and m.graph_captures == c0
    finally:
        m.close()
