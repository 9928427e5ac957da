"""The fused stage-0 kernel's deferred y epilogue (stage0_fused.hip, S0F_DEFER): a block wave keeps z of its round-n
block in registers and writes that block's y -- ELU, plane split, LDS stores -- in the MFMA gaps of round n + 1's
GEMM1; the conv waves, the y-halo copy and the descriptors follow one round later and every wave runs one more round.

Two parts:
  * a pure-Python model of the round schedule (no GPU): which role writes and reads which y buffer, halo and
    descriptor in which round, by buffer parity, for per-wave block counts 0..5 with and without the recompute
    round -- everything read is complete at the barrier before the round that reads it, nothing is overwritten
    before it has been read, and all 12 waves pass the same number of barriers;
  * GPU cases at the smallest shapes where the deferral can go wrong, each bitwise against the two-kernel path
    ("stage0_fused" 0, an independent implementation) on x1 (tap "down0"), y (tap "res0_elu") and all 32 codebooks.
"""
import itertools

import numpy as np
import pytest
import torch

from mimi_hip import synthetic
from mimi_hip.config import encoded_length

NA = 4  # block waves per CU (s0f::NA); 8 conv waves, two per section
EMPTY = "empty"


# ------------------------------------------------------------------------------------------------------------------
# The schedule model.  One CU: block wave w owns section w of both y buffers.  `defer` is s0f::DS (1: the shipped
# order, 0: the epilogue inside its own round); the buffer indices are the kernel's expressions.
# ------------------------------------------------------------------------------------------------------------------
def simulate(counts, recompute, defer, item_starts=(), conv_defer=None):
    """counts[w]: blocks of wave w's range; recompute[w]: the range starts inside an item (one more block first, its
    y feeding only the halo, nothing stored); item_starts: block indices (> 0) at which a wave's walk enters a new item
    (t0 == 0: zero halo); conv_defer: the conv waves' shift where it is not the block waves' (a broken kernel, for
    the model's own test).  Returns (down-conv results [(wave, block)], barriers per wave [12])."""
    DS, DSC = defer, defer if conv_defer is None else conv_defer
    hstart = [1 if recompute[w] and counts[w] > 0 else 0 for w in range(NA)]
    Rw = [counts[w] + hstart[w] for w in range(NA)]
    barriers = [0] * (NA + 8)
    # prologue: the block waves publish their round counts and empty descriptors in buffer 1, one barrier; the audio
    # images of round 0, a second one (S0F_HELP)
    desc = {(1, w): dict(val=EMPTY, round=-1, read=True) for w in range(NA)}
    ybuf, halo = {}, {}
    for w in range(NA + 8):
        barriers[w] += 2
    R = {w: max(Rw) for w in range(NA + 8)}  # every wave reads the same shared counts after the first barrier
    done = []

    def t0_zero(w, k):  # block k of wave w starts its item
        return (k == 0 and not hstart[w]) or (k in item_starts and k >= 1 + hstart[w])

    for n in range(max(R.values()) + max(DS, DSC) + 1):
        reads, writes = [], []  # (kind, buffer, section) ; (kind, buffer, section, value)
        cur, prev = (n + DS) & 1, (n + DS + 1) & 1
        for w in range(NA):  # ---- block waves ----
            if n > R[w] + DS:
                continue
            k = n - DS  # the block whose y this round writes
            if DS:
                writes.append(("desc", cur, w, k if 0 <= k < Rw[w] else EMPTY))
                if 0 <= k < Rw[w]:
                    writes.append(("y", cur, w, k))
                elif n < Rw[w]:
                    writes.append(("y", cur, w, "zeros"))  # round 0's GEMM1 carries an epilogue without a block
            else:
                writes.append(("desc", cur, w, k if k < Rw[w] else EMPTY))
                if k < Rw[w]:
                    writes.append(("y", cur, w, k))
            barriers[w] += 1
        for c in range(8):  # ---- conv waves: sections (c >> 1) for the helper work, all four for the conv ----
            wv = NA + c
            if n > R[wv] + DSC:
                continue
            hw, hrole = c >> 1, c & 1
            k = n - DSC
            ccur, cprev = (n + DSC) & 1, (n + DSC + 1) & 1
            if hrole == 1 and n >= DSC and k < Rw[hw]:
                if t0_zero(hw, k):
                    writes.append(("halo", ccur, hw, (k, "zeros")))
                else:
                    reads.append(("ytail", cprev, hw, None if k == 0 else k - 1))  # (k == 0: the recompute block)
                    writes.append(("halo", ccur, hw, (k, "copy")))
            if n > DSC and c == 0:  # (all 8 conv waves read the same four sections: model them once)
                for w in range(NA):
                    reads.append(("conv", cprev, w, n - DSC - 1))
            barriers[wv] += 1
        # reads of this round see only what earlier rounds wrote
        touched = {(kind if kind != "ytail" else "y", b, s) for kind, b, s, _ in reads}
        touched |= {("halo", b, s) for kind, b, s, _ in reads if kind == "conv"}
        touched |= {("desc", b, s) for kind, b, s, _ in reads if kind == "conv"}
        touched |= {("y", b, s) for kind, b, s, _ in reads if kind == "conv"}
        for kind, b, s, _ in writes:
            assert (kind, b, s) not in touched, f"round {n}: {kind} of buffer {b} section {s} written while it is read"
        for kind, b, s, want in reads:
            if kind == "ytail":
                if want is not None:
                    e = ybuf.get((b, s))
                    assert e and e["val"] == want and e["round"] < n, (n, "halo source", b, s, want, e)
                continue
            d = desc.get((b, s))
            assert d is not None and d["round"] < n, (n, "descriptor never written", b, s)
            d["read"] = True
            if want < Rw[s]:
                assert d["val"] == want, (n, "descriptor of another block", b, s, want, d)
                y, h = ybuf.get((b, s)), halo.get((b, s))
                assert y and y["val"] == want and y["round"] < n, (n, "y incomplete", b, s, want, y)
                assert h and h["val"][0] == want and h["round"] < n, (n, "halo incomplete", b, s, want, h)
                y["read"] = h["read"] = True
                done.append((s, want))
            else:
                assert d["val"] == EMPTY, (n, "a stale descriptor would store", b, s, d)
        for kind, b, s, val in writes:
            store = {"desc": desc, "y": ybuf, "halo": halo}[kind]
            old = store.get((b, s))
            if old is not None and not old["read"] and old["val"] not in (EMPTY, "zeros"):
                raise AssertionError(f"round {n}: {kind} {old} of buffer {b} section {s} overwritten before it was read")
            store[(b, s)] = dict(val=val, round=n, read=False)
    for store in (ybuf, desc):
        for key, e in store.items():
            assert e["read"] or e["val"] in (EMPTY, "zeros"), ("written and never read", key, e)
    return done, barriers


@pytest.mark.parametrize("defer", [1, 0])
def test_schedule_model(defer):
    """Block counts 0..5 per wave (all 6^4 combinations), with and without the recompute round, and with an item
    boundary inside the ranges: every block's y, halo and descriptor reach the down conv complete, exactly once and in
    order; no buffer is written while read or overwritten unread; one barrier count for all 12 waves."""
    for counts in itertools.product(range(6), repeat=NA):
        for rc, starts in ((False, ()), (True, ()), (True, (2,)), (False, (1, 3))):
            recompute = [rc] * NA
            done, barriers = simulate(counts, recompute, defer, starts)
            assert len(set(barriers)) == 1, (counts, rc, barriers)
            extra = [1 if rc and c > 0 else 0 for c in counts]
            assert barriers[0] == 2 + max(c + e for c, e in zip(counts, extra)) + defer + 1
            want = [(w, k) for w in range(NA) for k in range(counts[w] + extra[w])]
            assert sorted(done) == want, (counts, rc, starts)
            for w in range(NA):  # a section's blocks in order
                ks = [k for s, k in done if s == w]
                assert ks == sorted(ks)


def test_schedule_model_rejects_a_one_sided_shift():
    """The model is not vacuous: block waves that defer beside conv waves that do not (or the reverse) fail it."""
    for d, dc in ((1, 0), (0, 1)):
        with pytest.raises(AssertionError):
            done, barriers = simulate((2, 1, 0, 3), [False] * NA, d, conv_defer=dc)
            assert len(set(barriers)) == 1


# ------------------------------------------------------------------------------------------------------------------
# GPU cases
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(state_dict):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    m = MimiHipModel(state_dict, device="cuda:0")
    yield m
    m.set_option("stage0_fused", 1)


@pytest.fixture(scope="module")
def waves():
    """Block waves of the launch: 4 per CU, one workgroup per CU."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return NA * torch.cuda.get_device_properties(0).multi_processor_count


def run(engine, variant, fn):
    engine.set_option("stage0_fused", variant)
    engine.set_taps(True)
    try:
        codes = fn()
        return codes, engine.get_tap("down0").copy(), engine.get_tap("res0_elu").copy()
    finally:
        engine.set_taps(False)


def uniform_case(engine, B, L, seed):
    x = torch.from_numpy(np.stack([synthetic.speech_like(L, seed, i) for i in range(B)])).cuda()
    (c0, x0, y0), (c1, x1, y1) = [run(engine, v, lambda: engine.encode_int32(x, 32).cpu().numpy()) for v in (0, 1)]
    assert x0.shape == (B, (L + 3) // 4, 128)
    assert np.array_equal(x1, x0), (B, L, int((x1 != x0).sum()), x0.size)
    assert np.array_equal(y1, y0), (B, L, int((y1 != y0).sum()))
    assert np.array_equal(c1, c0), (B, L, int((c1 != c0).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 65])
def test_defer_few_blocks(engine, L):
    """B = 1: block waves with 0, 1 and 2 blocks (the range split puts them on different waves), most waves idle."""
    uniform_case(engine, 1, L, 71)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_defer_one_block_per_wave(engine, waves, delta):
    """Total blocks = 4 CUs - 1, 4 CUs, 4 CUs + 1: one block per wave (one wave with none), then one wave with two --
    the other waves retire their kept epilogue in a round without a block."""
    uniform_case(engine, 1, 32 * (waves + delta), 72)


@pytest.mark.gpu
def test_defer_ranges_start_mid_item(engine, waves):
    """B = 2, 2 CUs blocks each + 5 steps: most ranges start inside an item (the recompute round, nothing stored for
    it, followed by a deferred epilogue)."""
    uniform_case(engine, 2, 32 * (waves // 2) + 5, 73)


@pytest.mark.gpu
def test_defer_ranges_cross_items(engine):
    """B = 3 x (341 blocks + 5 steps): ranges cross an item boundary -- the kept epilogue of item b's last block
    (zeros past the item's end) retired while block 0 of item b + 1, with its zero halo, is built."""
    uniform_case(engine, 3, 32 * 341 + 5, 74)


@pytest.mark.gpu
def test_defer_ragged(engine, waves):
    lengths = [1, 33, 961, 1921, 32 * waves + 7]
    clips = [synthetic.speech_like(L, 75, i) for i, L in enumerate(lengths)]
    x = np.zeros((len(clips), max(lengths)), np.float32)
    for i, c in enumerate(clips):
        x[i, :len(c)] = c
    xt = torch.from_numpy(x).cuda()
    (c0, x0, y0), (c1, x1, y1) = [run(engine, v, lambda: engine.encode_ragged(xt, lengths, 32).cpu().numpy())
                                  for v in (0, 1)]
    for i, L in enumerate(lengths):  # each item's valid rows
        T1, F = (L + 3) // 4, encoded_length(L)
        assert np.array_equal(x1[i, :T1], x0[i, :T1]), (i, L, int((x1[i, :T1] != x0[i, :T1]).sum()))
        assert np.array_equal(y1[i, :L], y0[i, :L]), (i, L)
        assert np.array_equal(c1[i, :, :F], c0[i, :, :F]), (i, L)


@pytest.mark.gpu
def test_defer_graph_replay_and_determinism(engine, waves):
    """Taps off (graph-captured on the 2nd encode of a shape, replayed from the 3rd): five repeated encodes give the
    taps-on two-kernel codes, every time."""
    L = 32 * (waves // 2) + 5
    x = torch.from_numpy(np.stack([synthetic.speech_like(L, 76, i) for i in range(2)])).cuda()
    ref, _, _ = run(engine, 0, lambda: engine.encode_int32(x, 32).cpu().numpy())
    engine.set_option("stage0_fused", 1)
    before = engine.graph_replays
    outs = [engine.encode_int32(x, 32).cpu().numpy() for _ in range(5)]
    assert engine.graph_replays > before
    for o in outs:
        assert np.array_equal(o, ref)
