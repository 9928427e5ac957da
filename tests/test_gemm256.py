"""The 256 x 256 staggered planes-GEMM tile (gemm_planes256.h, engine option "gemm256": bit 0 fc1, bit 1 the k = 2s down
convs, bit 2 both on any grid) against the tiles it replaces: the same K-step order, product order per K step and
epilogue code, so every tap downstream of it and all 32 codebooks must be equal BITWISE between option 0 and the forced
form -- on both sides of a tile edge, on one N tile and several, in graph replays, run after run (the barrier structure
is new), and never on ragged batches (TF/modeling_mimi.py:210-347 MimiConv1d, :602-615 MimiMLP)."""
import numpy as np
import pytest
import torch

from mimi_hip import synthetic

pytestmark = pytest.mark.gpu

DEFAULT = 3   # the engine's default "gemm256": the roles adopted by measurement (bit 0 fc1, bit 1 down convs)
FORCED = 7    # every role, any grid size
LAYERS = 8
NEW = "gemm_planes256_kernel"


@pytest.fixture(scope="module")
def engine(state_dict):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    m = MimiHipModel(state_dict, device="cuda:0")
    yield m
    m.set_option("gemm256", DEFAULT)


def batch(B, L, seed):
    return torch.from_numpy(np.stack([synthetic.speech_like(L, seed, i) for i in range(B)])).cuda()


def run(engine, opt, x, names, K=32):
    """(codes, [taps]) of one encode under gemm256 = opt."""
    engine.set_option("gemm256", opt)
    engine.set_taps(bool(names))
    try:
        c = engine.encode_int32(x, K).cpu().numpy()
        return c, [engine.get_tap(n).copy() for n in names]
    finally:
        engine.set_taps(False)
        engine.set_option("gemm256", DEFAULT)


def profiled(engine, opt, encode):
    """{stage: set of kernel symbols} of one profiled encode under gemm256 = opt."""
    engine.set_option("gemm256", opt)
    engine.set_profiling(1)
    try:
        encode()
        seq = engine.profile_sequence()
    finally:
        engine.set_profiling(0)
        engine.set_option("gemm256", DEFAULT)
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    return kern


def assert_same(names, t0, t1, what):
    for n, a, b in zip(names, t0, t1):
        assert a.shape == b.shape, (what, n)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, n, int((a != b).sum()))


DOWN_TAPS = ["down1", "down2", "res2_elu", "res3_elu"]


# rows of down_s1 per item (L / 20): 256 = one tile, 257 = a 1-row tail tile, 1, 8401 = 32 tiles + a 209-row tail
@pytest.mark.parametrize("B,L", [(2, 5120), (3, 5121), (2, 1), (2, 24000 * 7 + 11)])
def test_down_convs_bitwise(engine, B, L):
    x = batch(B, L, 511)
    c0, t0 = run(engine, 0, x, DOWN_TAPS)
    c1, t1 = run(engine, FORCED, x, DOWN_TAPS)
    assert_same(DOWN_TAPS, t0, t1, (B, L))
    assert np.array_equal(c0, c1), (B, L, int((c0 != c1).sum()))


def test_forced_form_runs_the_new_kernel(engine):
    x = batch(2, 5121, 512)
    kern = profiled(engine, FORCED, lambda: engine.encode_int32(x, 32))
    for stage in ("down_s1", "down_s2", "fc1"):
        assert stage in kern and all(NEW in k for k in kern[stage]), (stage, kern.get(stage))


FC1_TAPS = [f"ff{l}" for l in range(LAYERS)]


# flat rows of fc1 (B x frames, 960 samples per frame): 39, 256 = one tile, 258
@pytest.mark.parametrize("B,frames", [(3, 13), (2, 128), (2, 129)])
def test_fc1_bitwise(engine, B, frames):
    x = batch(B, 960 * frames, 513)
    c0, t0 = run(engine, 0, x, FC1_TAPS)
    c1, t1 = run(engine, FORCED, x, FC1_TAPS)
    assert t0[0].shape[0] * t0[0].shape[1] == B * frames
    assert_same(FC1_TAPS, t0, t1, (B, frames))
    assert np.array_equal(c0, c1), (B, frames, int((c0 != c1).sum()))


def test_ragged_batch_keeps_the_old_kernels(engine):
    lengths = [1, 5121, 24000 * 7 + 11, 122880, 61234]
    x = np.zeros((len(lengths), max(lengths)), np.float32)
    for i, L in enumerate(lengths):
        x[i, :L] = synthetic.speech_like(L, 514, i)
    xt = torch.from_numpy(x).cuda()
    engine.set_option("gemm256", 0)
    ref = engine.encode_ragged(xt, lengths, 32).cpu().numpy()
    got = []
    kern = profiled(engine, FORCED, lambda: got.append(engine.encode_ragged(xt, lengths, 32).cpu().numpy()))
    assert np.array_equal(ref, got[0]), int((ref != got[0]).sum())
    for stage in ("down_s1", "down_s2", "fc1"):
        assert stage in kern, sorted(kern)
    for stage, names in kern.items():
        assert not any(NEW in k for k in names), (stage, names)


def test_graph_replay(engine):
    x = torch.from_numpy(synthetic.clip_batch(8, 240000, seed=515)).cuda()
    ref, _ = run(engine, 0, x, [])
    engine.set_option("gemm256", FORCED)
    try:
        before = engine.graph_replays
        outs = [engine.encode_int32(x, 32).cpu().numpy() for _ in range(3)]
        assert engine.graph_replays > before
    finally:
        engine.set_option("gemm256", DEFAULT)
    for o in outs:
        assert np.array_equal(o, ref)


def test_deterministic(engine):
    names = ["down1", "down2", f"ff{LAYERS - 1}"]
    x = batch(3, 24000 * 7 + 11, 516)
    _, first = run(engine, FORCED, x, names)
    for i in range(29):
        _, t = run(engine, FORCED, x, names)
        assert_same(names, first, t, i + 1)


def test_default_dispatch(engine):
    """B = 32 x 10 s at the default option: the new kernel runs for exactly the adopted roles."""
    x = torch.from_numpy(synthetic.clip_batch(32, 240000, seed=517)).cuda()
    kern = profiled(engine, DEFAULT, lambda: engine.encode_int32(x, 8))
    want = {"fc1": bool(DEFAULT & 1), "down_s1": bool(DEFAULT & 2), "down_s2": bool(DEFAULT & 2)}
    for stage, names in kern.items():
        for k in names:
            assert (NEW in k) == want.get(stage, False), (stage, k)
    for stage in want:
        assert stage in kern, sorted(kern)
