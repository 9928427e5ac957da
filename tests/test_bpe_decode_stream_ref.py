"""The id stream without a GPU: the contract class of tests/bpe_decode_stream_ref.py against ``Encoder.decode_ids``
and the per-character loop, the mistakes the schedule must catch, the schedule's coverage, and the C entry points'
declarations.

* CONTRACT = BATCH FORM.  On every prefix of every ``bpe_decode.npz`` entry the frames the class has emitted equal
  ``decode_ids`` of that prefix; on hand-built models of K = 1, 2, 8, 16 they equal ``bpe_decode_cases.decode_loop``
  under 1-id steps, one step and a random split.
* MUTANTS.  Each likely mistake changes at least one session of the schedule.
* COVERAGE.  The schedule holds the situations the GPU test relies on; they are checked here from the reference alone.
"""
import os
import re

import numpy as np
import pytest

import bpe_decode_cases as cases
import bpe_decode_stream_ref as ref
from mimi_hip import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mimi_hip.h")
NEW = ("mimi_bpe_decode_stream_create", "mimi_bpe_decode_stream_max_frames", "mimi_bpe_decode_stream_step",
       "mimi_bpe_decode_stream_reset", "mimi_bpe_decode_stream_reset_slot", "mimi_bpe_decode_stream_slot_pending",
       "mimi_bpe_decode_stream_destroy")


@pytest.fixture(scope="module")
def enc():
    return ref.schedule_encoder()


@pytest.fixture(scope="module")
def sessions(enc):
    return ref.make_sessions(enc)


@pytest.fixture(scope="module")
def played(enc, sessions):
    pool = ref.PoolRef(enc, ref.SCHED_SLOTS)
    return ref.play(sessions, pool.step, pool.reset)


@pytest.mark.parametrize("case", cases.CASES)
def test_every_prefix_equals_decode_ids(case):
    e = cases.trained_encoder(case)
    for name, ids, codes in cases.entries(case):
        slot = ref.SlotRef(e)
        got = np.zeros((e.num_codebooks, 0), np.int64)
        for p in range(len(ids)):
            got = np.concatenate([got, slot.feed(ids[p:p + 1])], axis=1)
            want = e.decode_ids([ids[:p + 1]])[0]
            assert np.array_equal(got, want), (case, name, p)
        assert np.array_equal(got, codes), (case, name)


@pytest.mark.parametrize("K", (1, 2, 8, 16))
def test_hand_models_equal_the_loop_under_every_split(K):
    e = cases.hand_encoder(K, seed=K, chain=2)
    rng = np.random.default_rng(K)
    for trial in range(6):
        ids = cases.random_ids(e, rng, 90, special=0.1)
        if trial % 2:  # a stream that mostly cycles, from a codebook that need not be 0
            cb = int(rng.integers(K))
            ids = np.array([e.n_special + ((cb + i) % K) * e.codebook_size + int(rng.integers(e.codebook_size))
                            for i in range(90)], np.int32)
            ids[rng.integers(0, 90, size=4)] = cases.random_ids(e, rng, 4)
        want = cases.decode_loop(e, ids)
        for name, cuts in ref.splits(len(ids), seed=trial).items():
            assert np.array_equal(ref.feed_split(ref.SlotRef(e), ids, cuts), want), (K, trial, name)


def test_schedule_sessions_equal_decode_ids(enc, sessions, played):
    _, whole = played
    for name in sessions:
        assert np.array_equal(whole[name], enc.decode_ids([ref.session_ids(sessions, name)])[0]), name


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_mutants_differ(enc, sessions, played, mutant):
    pool = ref.PoolRef(enc, ref.SCHED_SLOTS, mutant)
    _, got = ref.play(sessions, pool.step, pool.reset)
    assert any(not np.array_equal(got[n], played[1][n]) for n in sessions), mutant


def test_schedule_coverage(enc, sessions, played):
    log, _ = played
    K = enc.num_codebooks
    per_slot = {s: [] for s in range(ref.SCHED_SLOTS)}
    for slots, _, _, frames in log:
        for s, f in zip(slots, frames):
            per_slot[s].append(f.shape[1])
    for s, counts in per_slot.items():  # every slot: a step of 0 frames and one of at least 2
        assert 0 in counts and max(counts) >= 2, (s, counts)
    assert any(slots != sorted(slots) for slots, _, _, _ in log)          # item order is not slot order
    first_use = {s: min(i for i, (slots, _, _, _) in enumerate(log) if s in slots) for s in per_slot}
    assert max(first_use.values()) >= 3                                   # a slot that starts late
    assert any(op[0] == "reset" for op in ref.SCHEDULE[1:-1])             # a reset mid-way, steps after it
    assert any(len(c) == 0 for _, _, chunks, _ in log for c in chunks)    # a count of 0
    assert any(len(c) > 0 and (c < enc.n_special).all() for _, _, chunks, _ in log for c in chunks)  # only specials
    # replay each session alone: a begin drop that starts on a codebook != 0 and ends in a later step, a codebook
    # awaited across 3 steps that all bring characters, pending codes left behind at the reset
    late_drop = waits = False
    for name, chunks in sessions.items():
        slot, run = ref.SlotRef(enc), 0
        for i, c in enumerate(chunks):
            before = (slot.expected, slot.owed, len(slot.pend))
            slot.feed(c)
            if i == 0 and slot.cb0 != 0 and slot.owed > 0:
                late_drop = True
            brought = len(slot.characters(c)) > 0
            run = run + 1 if brought and before[0] is not None and (slot.expected, slot.owed, len(slot.pend)) == before \
                else 0
            waits = waits or run >= 3
        if name == ref.SLOT_SESSIONS[0][0]:
            assert len(slot.pend) > 0  # the reset discards something
    assert late_drop and waits
    # pending codes in front of a step that completes at least 2 frames (their column matters)
    pool, seen = ref.PoolRef(enc, ref.SCHED_SLOTS), []
    ref.play(sessions, lambda s, c: (seen.append(list(pool.pending)), pool.step(s, c))[1], pool.reset)
    assert any(before[s] > 0 and f.shape[1] >= 2
               for before, (slots, _, _, frames) in zip(seen, log) for s, f in zip(slots, frames))
    assert K == ref.SCHED_K


def test_symbols_exported_and_declared():
    with open(HEADER) as f:
        text = f.read()
    lib = _lib.load()
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"^\w[\w\s\*]*\b%s\(" % sym, text, re.M), sym  # a declaration, not a mention in a comment
        assert getattr(lib, sym).argtypes is not None


def test_null_calls_fail_without_gpu_work():
    import ctypes
    lib = _lib.load()
    assert lib.mimi_bpe_decode_stream_create(None, 1, 1, None) == 1
    assert b"out is NULL" in lib.mimi_last_error()
    h = ctypes.c_void_p()
    assert lib.mimi_bpe_decode_stream_create(None, 1, 1, ctypes.byref(h)) == 1
    assert b"null model" in lib.mimi_last_error() and not h
    assert lib.mimi_bpe_decode_stream_step(None, None, None, 1, None, 0, None, 0, None, None) == 1
    assert b"null stream" in lib.mimi_last_error()
    assert lib.mimi_bpe_decode_stream_reset(None) == 1
    assert lib.mimi_bpe_decode_stream_reset_slot(None, 0) == 1
    assert lib.mimi_bpe_decode_stream_max_frames(None, 1) == -1
    assert lib.mimi_bpe_decode_stream_slot_pending(None, 0) == -2
    lib.mimi_bpe_decode_stream_destroy(None)
