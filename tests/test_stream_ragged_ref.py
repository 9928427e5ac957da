"""A ragged stream step without a GPU, decode and encode: the pool of ``batch = 1`` streams
(tests/stream_ragged_ref.py) on the schedule the GPU tests run, the mistakes that schedule must catch, and the C entry
points' declarations.  (Encode: the same schedule on the encode stream's clips, the pre-quantizer embedding held to
``mimi_ref.pre_quantizer`` of the whole clip, one more mutant -- a replicate fill that is not per item.)

* POOL = WHOLE.  Every session of the schedule (the sessions of the slot tests, ``sliding_window`` = 5, K = 8, cut into
  calls whose items bring 1, 2, 3 or 7 frames) comes out of the pool within ``ACT_TOL`` = 1e-4 (the project's
  ``rel_err``) of ``decode_ref.decode`` of that session's whole sequence.
* MUTANTS.  Each mistake a packed layout invites -- an item that consumes its padding, a position that advances by the
  longest item's count, a carry-out taken at the longest item's end, item bases at the uniform stride -- moves at least
  one session beyond 100 x ``ACT_TOL`` (the factors measured: DESIGN 3.7.1).  This is a condition on the schedule.
* The new entry points are exported, declared, and refuse NULL like their siblings.
"""
import json
import os
import re

import pytest
import torch

import decode_ref
import stream_ragged_ref as rag
from decode_stage_ref import rel_err
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

ACT_TOL = 1e-4
MISS = 100 * ACT_TOL
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mimi_hip.h")
NEW = ("mimi_decode_stream_step_ragged", "mimi_stream_step_layout", "mimi_encode_stream_step_ragged")
CFG5 = RefConfig(sliding_window=rag.WINDOW)
MUTANTS = ("reads_padding", "advance_by_nmax", "carry_at_longest", "uniform_base")


@pytest.fixture(scope="module")
def full_sd(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return decode_ref.as_tensors(sd)


@pytest.fixture(scope="module")
def sessions():
    return rag.make_sessions()


@pytest.fixture(scope="module")
def whole(full_sd, sessions):
    """name -> decode_ref.decode of the session's whole sequence; computed once, never written."""
    return {name: decode_ref.decode(codes, full_sd, CFG5) for name, codes in sessions.items()}


def run_pool(full_sd, sessions, mutant=None):
    pool = rag.RaggedPool(full_sd, rag.BATCH, CFG5, mutant)
    return rag.play(sessions, pool.step_ragged, pool.reset, lambda: pool.positions)


def record(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


def test_schedule_is_what_the_gpu_test_needs(sessions):
    steps = [op for op in rag.SCHEDULE if op[0] == "step"]
    counts = [[f for _, _, f in op[1]] for op in steps]
    assert {f for c in counts for f in c} == {1, 2, 3, 7}
    assert any(len(set(c)) > 1 for c in counts)                           # calls that mix counts
    assert any(len(c) > 1 and len(set(c)) == 1 and c[0] == op[2] for c, op in zip(counts, steps))  # one with equal counts
    assert any(max(c) < op[2] for c, op in zip(counts, steps))            # padding beyond the longest item
    assert any(op[0] == "reset" for op in rag.SCHEDULE[1:-1])             # a reset mid-way
    # a fresh slot with 1 frame beside a mid-way slot with 7
    pos, seen = {}, False
    for op in rag.SCHEDULE:
        if op[0] == "reset":
            pos[op[1]] = 0
            continue
        here = [(pos.get(s, 0), f) for s, _, f in op[1]]
        seen = seen or ((0, 1) in here and any(p > 0 and f == 7 for p, f in here))
        for s, _, f in op[1]:
            pos[s] = pos.get(s, 0) + f
    assert seen
    assert 2 not in {s for op in steps for s, _, _ in op[1]}              # a slot that is never used
    assert {n: sum(v) for n, v in rag.splits().items()} == rag.SESSION_FRAMES  # every session's total unchanged
    assert 2 * 1 < RefConfig().kernel_size - 1                            # a 1-frame chunk is shorter than the 6-row carry


def test_pool_equals_whole(full_sd, sessions, whole, parity_log):
    got = run_pool(full_sd, sessions)
    for name, y in got.items():
        assert y.shape == whole[name].shape
        err = rel_err(y, whole[name])
        record(parity_log, "decode_stream_ragged_ref", session=name, rel_err=err)
        assert err < ACT_TOL, (name, err)


@pytest.mark.parametrize("name", MUTANTS)
def test_mutants_miss(full_sd, sessions, whole, parity_log, name):
    got = run_pool(full_sd, sessions, rag.RaggedMutant(**{name: True}))
    errs = {s: rel_err(y, whole[s]) for s, y in got.items()}
    record(parity_log, "decode_stream_ragged_ref_mutant", mutant=name, rel_err=errs,
           factor=max(errs.values()) / ACT_TOL)
    assert max(errs.values()) >= MISS, (name, errs)


# ---- the encode direction: the same schedule on the encode stream's clips, the embedding held to the whole-clip one --
ENC_MUTANTS = ("reads_padding", "advance_by_nmax", "carry_at_longest", "uniform_base", "fill_from_first_item")


@pytest.fixture(scope="module")
def enc_sessions():
    import encode_stream_ref as esr
    return {name: esr.clip(name) for name in rag.SESSION_FRAMES}


@pytest.fixture(scope="module")
def enc_whole(state_dict, enc_sessions):
    import encode_stream_ref as esr
    from oracle import mimi_ref
    sd = esr.as_tensors(state_dict)
    return {name: mimi_ref.pre_quantizer(x, sd, CFG5) for name, x in enc_sessions.items()}


def run_enc_pool(state_dict, sessions, mutant=None, pad=0.25):
    pool = rag.EncRaggedPool(state_dict, rag.BATCH, CFG5, mutant)
    return rag.play_encode(sessions, pool.embed_ragged, pool.reset, lambda: pool.positions, pad=pad)


def test_encode_pool_equals_whole(state_dict, enc_sessions, enc_whole, parity_log):
    got = run_enc_pool(state_dict, enc_sessions, pad=float("nan"))  # the padding is never read
    for name, y in got.items():
        assert y.shape == enc_whole[name].shape
        err = rel_err(y, enc_whole[name])
        record(parity_log, "encode_stream_ragged_ref", session=name, rel_err=err)
        assert err < ACT_TOL, (name, err)


@pytest.mark.parametrize("name", ENC_MUTANTS)
def test_encode_mutants_miss(state_dict, enc_sessions, enc_whole, parity_log, name):
    got = run_enc_pool(state_dict, enc_sessions, rag.EncRaggedMutant(**{name: True}))
    errs = {s: rel_err(y, enc_whole[s]) for s, y in got.items()}
    record(parity_log, "encode_stream_ragged_ref_mutant", mutant=name, rel_err=errs,
           factor=max(errs.values()) / ACT_TOL)
    assert max(errs.values()) >= MISS, (name, errs)


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
    assert lib.mimi_decode_stream_step_ragged(None, None, None, 1, 1, None, None, None) == 1
    assert b"null stream" in lib.mimi_last_error()
    assert lib.mimi_encode_stream_step_ragged(None, None, None, 1, 1, None, None, None) == 1
    assert b"null stream" in lib.mimi_last_error()
