"""Decode-stream slots without a GPU: the pool of slots (tests/decode_stream_slots_ref.py) on the schedule the GPU test
runs, the mistakes that schedule must catch, and the C entry points' declarations.

* POOL = WHOLE.  Every session of the schedule (four sessions that start and end at different times on four slots,
  ``sliding_window`` = 5, K = 8) comes out of the pool within ``ACT_TOL`` = 1e-4 (the project's ``rel_err``) of
  ``decode_ref.decode`` of that session's whole sequence.
* MUTANTS.  Each mistake the slot plumbing invites -- RoPE rows of the first listed slot for everybody, rings or
  carries addressed by the item's place in the step, a reset that keeps the carries -- moves at least one session beyond
  10 x ``ACT_TOL``.  This is a condition on the schedule: were a mutant below it, the GPU test could not tell that
  mistake from a right kernel.
* The three new entry points are exported, declared, and refuse NULL like their siblings.
"""
import json
import os
import re

import pytest
import torch

import decode_ref
import decode_stream_slots_ref as slots_ref
from decode_stage_ref import rel_err
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

ACT_TOL = 1e-4
MISS = 10 * ACT_TOL
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mimi_hip.h")
NEW = ("mimi_decode_stream_step_slots", "mimi_decode_stream_reset_slot", "mimi_decode_stream_slot_position")
CFG5 = RefConfig(sliding_window=slots_ref.WINDOW)
MUTANTS = ("rope_from_first", "ring_by_item", "carry_by_item", "reset_keeps_carry")


@pytest.fixture(scope="module")
def full_sd(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return decode_ref.as_tensors(sd)


@pytest.fixture(scope="module")
def sessions():
    return slots_ref.make_sessions()


@pytest.fixture(scope="module")
def whole(full_sd, sessions):
    """name -> decode_ref.decode of the session's whole sequence; computed once, never written."""
    return {name: decode_ref.decode(codes, full_sd, CFG5) for name, codes in sessions.items()}


def run_pool(full_sd, sessions, mutant=None):
    pool = slots_ref.SlotPool(full_sd, slots_ref.BATCH, CFG5, mutant)
    return slots_ref.play(sessions, pool.step, pool.reset, lambda: pool.positions)


def record(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


def test_schedule_is_what_the_gpu_test_needs(sessions):
    steps = [op for op in slots_ref.SCHEDULE if op[0] == "step"]
    assert {len(op[1]) for op in steps} == {1, 2, 3}
    assert {op[2] for op in steps} == {1, 2, 3, 7} and max(op[2] for op in steps) == slots_ref.MAX_STEP_FRAMES
    listed = [[s for s, _ in op[1]] for op in steps]
    assert any(l != sorted(l) for l in listed) and any(len(l) > 1 and l == sorted(l) for l in listed)
    assert 2 not in {s for l in listed for s in l}  # a slot that is never used
    lengths = [c.shape[2] for c in sessions.values()]
    assert len(set(lengths)) == 4 and min(lengths) >= 9 and max(lengths) <= 13
    assert {n: sum(v) for n, v in slots_ref.splits().items()} == slots_ref.SESSION_FRAMES


def test_pool_equals_whole(full_sd, sessions, whole, parity_log):
    got = run_pool(full_sd, sessions)
    for name, y in got.items():
        assert y.shape == whole[name].shape
        err = rel_err(y, whole[name])
        record(parity_log, "decode_stream_slots_ref", session=name, rel_err=err)
        assert err < ACT_TOL, (name, err)


@pytest.mark.parametrize("name", MUTANTS)
def test_mutants_miss(full_sd, sessions, whole, parity_log, name):
    got = run_pool(full_sd, sessions, slots_ref.SlotMutant(**{name: True}))
    errs = {s: rel_err(y, whole[s]) for s, y in got.items()}
    record(parity_log, "decode_stream_slots_ref_mutant", mutant=name, rel_err=errs)
    assert max(errs.values()) >= MISS, (name, errs)


def test_reset_slot_is_a_fresh_stream(full_sd, sessions, whole):
    """The pool's own statement of reset(slot): D, decoded on the slot A left, is D decoded alone."""
    got = run_pool(full_sd, sessions)
    pool = slots_ref.SlotPool(full_sd, 1, CFG5)
    at, parts = 0, []
    for n in slots_ref.splits()["D"]:
        parts.append(pool.step([0], sessions["D"][:, :, at:at + n]))
        at += n
    assert torch.equal(torch.cat(parts, dim=-1), got["D"])


def test_symbols_exported_and_declared():
    with open(HEADER) as f:
        text = f.read()
    lib = _lib.load()
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"^\w[\w\s\*]*\b%s\(" % sym, text, re.M), sym  # a declaration, not a mention in a comment
        assert getattr(lib, sym).argtypes is not None


def test_null_calls_fail_without_gpu_work():
    lib = _lib.load()
    assert lib.mimi_decode_stream_step_slots(None, None, 1, None, 1, None, None) == 1
    assert b"null stream" in lib.mimi_last_error()
    assert lib.mimi_decode_stream_reset_slot(None, 0) == 1
    assert b"null stream" in lib.mimi_last_error()
    assert lib.mimi_decode_stream_slot_position(None, 0) == -1
