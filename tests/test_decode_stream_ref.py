"""Streaming decode without a GPU: the streamed reference (tests/decode_stream_ref.py) against ``decode_ref.decode`` of
the whole sequence, the mistakes it must catch, and the C entry points' declarations.

* STREAMED = WHOLE.  For every split the GPU tests use, the streamed reference's concatenated steps are within
  ``ACT_TOL`` = 1e-4 (the project's ``rel_err``) of the one-shot decode; the measured values (1e-6-ish: another
  summation split of the same sums) go to ``parity_log``.
* MUTANTS.  Each likely mistake, switched on in the reference, misses ``ACT_TOL`` by >= 10 x on these same inputs: were
  one of them below that, the GPU tests' inputs could not tell a wrong kernel from a right one.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import decode_ref
import decode_stream_ref as dstr
from decode_stage_ref import rel_err
from mimi_hip import _lib, synthetic
from oracle.mimi_ref import RefConfig

ACT_TOL = 1e-4
MISS = 10 * ACT_TOL
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mimi_hip.h")
NEW = ("mimi_decode_stream_create", "mimi_decode_stream_step", "mimi_decode_stream_reset",
       "mimi_decode_stream_position", "mimi_decode_stream_state_bytes", "mimi_decode_stream_destroy")
SPLITS_13 = ([13], [1] * 13, [2, 3, 1, 7], [12, 1])
SPLITS_9 = ([1] * 9, [4, 4, 1])
CFG5 = RefConfig(sliding_window=5)


def rand_codes(seed, B, K, T):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, (B, K, T)))


@pytest.fixture(scope="module")
def full_sd(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return decode_ref.as_tensors(sd)


@pytest.fixture(scope="module")
def case13(full_sd):
    codes = rand_codes(13, 1, 8, 13)
    return codes, decode_ref.decode(codes, full_sd)


@pytest.fixture(scope="module")
def case9(full_sd):
    codes = rand_codes(9, 1, 8, 9)
    return codes, decode_ref.decode(codes, full_sd, CFG5)


def record(parity_log, test, **kw):
    rec = dict(test=test, **kw)
    parity_log.append(rec)
    print(json.dumps(rec))


@pytest.mark.parametrize("split", SPLITS_13, ids=lambda s: "x".join(map(str, s)) if len(s) < 5 else f"{s[0]}x{len(s)}")
def test_streamed_equals_whole_T13(full_sd, case13, parity_log, split):
    codes, want = case13
    got = dstr.decode_stream(codes, full_sd, split)
    assert got.shape == want.shape == (1, 1, 1920 * 13)
    err = rel_err(got, want)
    record(parity_log, "decode_stream_ref_T13", split=list(split), rel_err=err)
    assert err < ACT_TOL, err


@pytest.mark.parametrize("split", SPLITS_9, ids=lambda s: "x".join(map(str, s)) if len(s) < 5 else f"{s[0]}x{len(s)}")
def test_streamed_equals_whole_T9_window5(full_sd, case9, parity_log, split):
    codes, want = case9
    err = rel_err(dstr.decode_stream(codes, full_sd, split, CFG5), want)
    record(parity_log, "decode_stream_ref_T9_w5", split=list(split), rel_err=err)
    assert err < ACT_TOL, err


def test_window_matters_at_T9(full_sd, case9):
    """The reference itself moves by far more than the tolerance when the window does: these inputs see the window."""
    codes, want = case9
    for w in (4, 6):
        assert rel_err(decode_ref.decode(codes, full_sd, RefConfig(sliding_window=w)), want) > MISS


MUTANTS_13 = [
    ("rope_restart", dstr.Mutant(rope_restart=True), [2, 3, 1, 7]),
    ("rope_restart", dstr.Mutant(rope_restart=True), [12, 1]),
    ("conv0_short", dstr.Mutant(conv0_short=True), [1] * 13),
    ("conv0_short", dstr.Mutant(conv0_short=True), [2, 3, 1, 7]),
    ("no_shift", dstr.Mutant(no_shift=True), [1] * 13),
    ("no_shift", dstr.Mutant(no_shift=True), [2, 3, 1, 7]),
    ("drop_upsample", dstr.Mutant(drop_upsample=True), [1] * 13),
    ("drop_upsample", dstr.Mutant(drop_upsample=True), [12, 1]),
]


@pytest.mark.parametrize("name,mutant,split", MUTANTS_13, ids=[f"{m[0]}-{len(m[2])}steps" for m in MUTANTS_13])
def test_mutants_miss_at_T13(full_sd, case13, parity_log, name, mutant, split):
    codes, want = case13
    err = rel_err(dstr.decode_stream(codes, full_sd, split, mutant=mutant), want)
    record(parity_log, "decode_stream_ref_mutant", mutant=name, split=list(split), rel_err=err)
    assert err >= MISS, (name, split, err)


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("split", SPLITS_9, ids=["1x9", "4x4x1"])
def test_window_mutants_miss_at_T9(full_sd, case9, parity_log, split, delta):
    codes, want = case9
    err = rel_err(dstr.decode_stream(codes, full_sd, split, CFG5, dstr.Mutant(window_delta=delta)), want)
    record(parity_log, "decode_stream_ref_mutant", mutant=f"window{delta:+d}", split=list(split), rel_err=err)
    assert err >= MISS, (delta, split, err)


def test_real_window_T130(full_sd, parity_log):
    """T = 130 (260 rows, 10 past the window of 250): streamed in steps of 7 equals the whole, and a window of 249 or
    251 misses.  The GPU tests' window case."""
    codes = rand_codes(130, 1, 8, 130)
    want = decode_ref.decode(codes, full_sd)
    split = [7] * 18 + [4]
    err = rel_err(dstr.decode_stream(codes, full_sd, split), want)
    record(parity_log, "decode_stream_ref_T130", split="7x18+4", rel_err=err)
    assert err < ACT_TOL, err
    for delta in (-1, 1):
        bad = rel_err(dstr.decode_stream(codes, full_sd, split, mutant=dstr.Mutant(window_delta=delta)), want)
        record(parity_log, "decode_stream_ref_mutant", mutant=f"window{delta:+d}", split="7x18+4", rel_err=bad)
        assert bad >= MISS, (delta, bad)


def test_state_is_bounded(full_sd):
    """The cache never holds more than W - 1 rows and the carries keep their sizes, however far the stream runs."""
    st = dstr.StreamState(full_sd, 1, CFG5)
    codes = rand_codes(3, 1, 8, 12)
    sizes = None
    for t in range(12):
        st.step(codes[:, :, t:t + 1])
        now = {k: tuple(v.shape) for k, v in st.carry.items()}
        assert sizes is None or now == sizes
        sizes = now
        assert all(k.shape[2] == min(2 * (t + 1), 4) for k in st.k)
    assert st.position == 12
    assert [(n, h) for n, h, _ in dstr.carry_plan(RefConfig())] == [
        ("upsample", 1), ("conv0", 6), ("up0", 1), ("res0", 2), ("up1", 1), ("res1", 2), ("up2", 1), ("res2", 2),
        ("up3", 1), ("res3", 2), ("last", 2)]


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
    assert lib.mimi_decode_stream_create(None, 1, 8, 1, None) == 1
    assert lib.mimi_decode_stream_step(None, None, 1, None, None) == 1
    assert b"null stream" in lib.mimi_last_error()
    assert lib.mimi_decode_stream_reset(None) == 1
    assert lib.mimi_decode_stream_position(None) == -1
    assert lib.mimi_decode_stream_state_bytes(None) == -1
    lib.mimi_decode_stream_destroy(None)
