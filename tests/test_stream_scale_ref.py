"""The serving-scale stream schedule without a GPU (tests/stream_scale_ref.py), decode and encode.

* THE SCHEDULE IS WHAT THE GPU TESTS NEED.  At ``m`` = 128 the big step has 511 frames = 1022 flat rows, at 129 it has
  515 = 1030: the two sides of the fp32 GEMM's ``M > 1024`` tile boundary.  No item of it sits in the slot of its own
  index, no two neighbours stand at the same position, fresh, mid-ring and wrapped slots meet in it, and every session
  has 4 .. 18 frames.
* POOL = WHOLE at ``m`` = 17 (seconds, not minutes): every session comes out of the pool of float64-checked ``batch = 1``
  reference streams within ``ACT_TOL`` = 1e-4 (the project's ``rel_err``) of ``decode_ref.decode`` /
  ``mimi_ref.pre_quantizer`` of its whole sequence.
* MUTANTS.  Each mistake that only shows past the first few items -- item i on slot i's state, the position of item
  i >= 8 read from item i - 8, the RoPE rows of the item listed before, a reset that keeps the position -- moves at least
  one session beyond ``MISS`` = 500 x ``ACT_TOL``.  ``MISS`` was set after measuring, not before: the factors on this
  CPU reference are 1830 .. 10630 x the tolerance (CHANGELOG; the smallest is the decode stream's
  ``position_from_8_back``), and 500 is the round number at least 2 x below the smallest.  A condition on the schedule.
"""
import json

import pytest

import decode_ref
import stream_ragged_ref as rag
import stream_scale_ref as sc
from decode_stage_ref import rel_err
from mimi_hip import synthetic
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

ACT_TOL = 1e-4
MISS = 500 * ACT_TOL
M = sc.M_CPU
CFG5 = RefConfig(sliding_window=sc.WINDOW)
MUTANTS = ("state_by_item", "position_from_8_back", "rope_of_previous_item", "reset_keeps_position")


def record(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


@pytest.mark.parametrize("m,frames", [(128, 511), (129, 515), (M, 67)])
def test_schedule_is_what_the_gpu_tests_need(m, frames):
    total, own = sc.check(m)
    assert total == frames  # 1022 and 1030 flat rows: the tile boundary is the point
    assert (2 * total <= 1024) == (m != 129)
    assert own == ([] if m > M else [5])  # no item of the big step sits in the slot of its own index
    sample = sc.value_sample(m)
    assert len(sample) == len(set(sample)) == 8 and all(0 <= i < m + 3 for i in sample)
    big = sc.schedule(m)[sc.BIG][1]
    held = {name for _, name, _ in big}
    assert {big[0][1], big[m - 1][1]} <= set(sample) and set(sample) - {m} <= held
    rows = sc.flat_rows(m)
    assert [f for _, _, f in big] == [1 + (5 * ((13 * j + 16) % m)) % 7 for j in range(m)]  # (the layout test's counts)
    if m == 129:  # rows 1023 / 1024 meet between items 126 and 127, and one more item follows
        assert sc.tap_items(m) == [0, 126, 127, 128] and rows[127][0] == 1024 and rows[126][0] + rows[126][1] == 1024
    if m >= 128:  # rows 63 / 64 meet between items 7 and 8
        assert sc.items_at_row(m, 64) == [7, 8] and rows[8][0] == 64
        assert {big[j][1] for j in (7, 8, 126, 127)} <= set(sample)
        fresh = [j for j, (s, _, _) in enumerate(big) if sc.warm_position(s) == 0]
        assert len(fresh) == 12 and 0 not in fresh  # (the encode stream's replicate fill is per item)


# ---- decode ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_sd(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return decode_ref.as_tensors(sd)


@pytest.fixture(scope="module")
def sessions():
    return sc.make_sessions(M)


@pytest.fixture(scope="module")
def whole(full_sd, sessions):
    """session -> decode_ref.decode of its whole sequence; computed once, never written."""
    return {name: decode_ref.decode(codes, full_sd, CFG5) for name, codes in sessions.items()}


def run_pool(full_sd, sessions, mutant=None, pool=None):
    pool = pool or sc.decode_pool(full_sd, M, CFG5, mutant)
    return rag.play(sessions, pool.step_ragged, pool.reset, lambda: pool.positions, schedule=sc.schedule(M), batch=M)


def test_pool_equals_whole(full_sd, sessions, whole, parity_log):
    """The existing float64-checked pool (``stream_ragged_ref.RaggedPool`` on ``SlotPool``'s states) on this schedule;
    the pool the mutants live in is that pool bit for bit when no mutant is on."""
    import torch
    got = run_pool(full_sd, sessions, pool=rag.RaggedPool(full_sd, M, CFG5))
    same = run_pool(full_sd, sessions)
    assert all(torch.equal(got[name], same[name]) for name in got)
    errs = {}
    for name, y in got.items():
        assert y.shape == whole[name].shape
        errs[name] = rel_err(y, whole[name])
        assert errs[name] < ACT_TOL, (name, errs[name])
    record(parity_log, "decode_stream_scale_ref", m=M, sessions=len(got), max_rel_err=max(errs.values()))


@pytest.mark.parametrize("name", MUTANTS)
def test_mutants_miss(full_sd, sessions, whole, parity_log, name):
    got = run_pool(full_sd, sessions, sc.ScaleMutant(**{name: True}))
    errs = {s: rel_err(y, whole[s]) for s, y in got.items()}
    record(parity_log, "decode_stream_scale_ref_mutant", mutant=name, factor=max(errs.values()) / ACT_TOL,
           sessions_moved=sum(e >= MISS for e in errs.values()))
    assert max(errs.values()) >= MISS, (name, errs)


# ---- encode: the pre-quantizer embedding ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clips():
    return sc.make_clips(M)


@pytest.fixture(scope="module")
def enc_whole(state_dict, clips):
    import encode_stream_ref as esr
    sd = esr.as_tensors(state_dict)
    return {name: mimi_ref.pre_quantizer(x, sd, CFG5) for name, x in clips.items()}


def run_enc_pool(state_dict, clips, mutant=None, pad=0.25, pool=None):
    pool = pool or sc.encode_pool(state_dict, M, CFG5, mutant)
    step = pool.embed_ragged if isinstance(pool, rag.EncRaggedPool) else pool.step_ragged
    return rag.play_encode(clips, step, pool.reset, lambda: pool.positions, schedule=sc.schedule(M), batch=M, pad=pad)


def test_encode_pool_equals_whole(state_dict, clips, enc_whole, parity_log):
    """The existing pool (``stream_ragged_ref.EncRaggedPool``) on this schedule, every item's padding NaN (it is never
    read); the pool the mutants live in is that pool bit for bit when no mutant is on."""
    import torch
    got = run_enc_pool(state_dict, clips, pad=float("nan"), pool=rag.EncRaggedPool(state_dict, M, CFG5))
    same = run_enc_pool(state_dict, clips, pad=float("nan"))
    assert all(torch.equal(got[name], same[name]) for name in got)
    errs = {}
    for name, y in got.items():
        assert y.shape == enc_whole[name].shape
        errs[name] = rel_err(y, enc_whole[name])
        assert errs[name] < ACT_TOL, (name, errs[name])
    record(parity_log, "encode_stream_scale_ref", m=M, sessions=len(got), max_rel_err=max(errs.values()))


@pytest.mark.parametrize("name", MUTANTS)
def test_encode_mutants_miss(state_dict, clips, enc_whole, parity_log, name):
    got = run_enc_pool(state_dict, clips, sc.ScaleMutant(**{name: True}))
    errs = {s: rel_err(y, enc_whole[s]) for s, y in got.items()}
    record(parity_log, "encode_stream_scale_ref_mutant", mutant=name, factor=max(errs.values()) / ACT_TOL,
           sessions_moved=sum(e >= MISS for e in errs.values()))
    assert max(errs.values()) >= MISS, (name, errs)
