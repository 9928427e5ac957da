"""Ragged decode without a GPU: the two C entry points are exported, declared and fail cleanly on a NULL engine, and
``strs_to_audio`` batches its strings as documented (checked over a stub model that records its calls)."""
import os
import re

import numpy as np
import pytest
import torch

from mimi_hip import _lib
from mimi_hip.codes import CODEBOOK_SIZE, NUM_CODEBOOKS, chars_to_codes, codes_to_chars

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mimi_hip.h")
NEW = ("mimi_decode_ragged", "mimi_decode_ragged_workspace_bytes")


def test_symbols_exported_and_declared():
    with open(HEADER) as f:
        text = f.read()
    lib = _lib.load()
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"^\w[\w\s\*]*\b%s\(" % sym, text, re.M), sym  # a declaration, not a mention in a comment
        assert getattr(lib, sym).argtypes is not None


def test_null_engine_calls_fail_without_gpu_work():
    lib = _lib.load()
    lens = np.array([1], dtype=np.int64)
    assert lib.mimi_decode_ragged(None, None, lens.ctypes.data, 1, 1, 1, None, None) == 1
    assert b"null engine" in lib.mimi_last_error()
    assert lib.mimi_decode_ragged_workspace_bytes(None, lens.ctypes.data, 1) == -1


class StubModel:
    """decode_ragged / decode that record their arguments and return recognisable samples: item b of a call gets the
    value of its first code in every sample."""

    def __init__(self):
        self.ragged_calls = []
        self.decode_calls = 0

    def decode_ragged(self, audio_codes, lengths, out=None):
        self.ragged_calls.append((audio_codes.clone(), list(lengths)))
        return [torch.full((1, 1920 * int(n)), float(audio_codes[b, 0, 0])) for b, n in enumerate(lengths)]

    def decode(self, codes):
        self.decode_calls += 1
        raise AssertionError("strs_to_audio goes through decode_ragged")


def make_strs(lengths, seed=0):
    rng = np.random.default_rng(seed)
    codes = [rng.integers(0, CODEBOOK_SIZE, (NUM_CODEBOOKS, T)) for T in lengths]
    return [codes_to_chars(c, codebook_size=CODEBOOK_SIZE) for c in codes], codes


def check_calls(model, codes, groups):
    """The recorded calls are exactly `groups` (lists of item indices), padded codes and lengths as chars_to_codes
    gives them."""
    assert [len(c[1]) for c in model.ragged_calls] == [len(g) for g in groups]
    for (got, lens), g in zip(model.ragged_calls, groups):
        assert lens == [codes[i].shape[1] for i in g]
        assert got.shape == (len(g), NUM_CODEBOOKS, max(lens)) and got.dtype == torch.int64
        for j, i in enumerate(g):
            assert np.array_equal(got[j, :, : lens[j]].numpy(), codes[i])


def test_strs_to_audio_order_and_empty_strings():
    from mimi_hip import strs_to_audio
    strs, codes = make_strs([5, 0, 13, 2, 13])
    assert strs[1] == ""
    for s, c in zip(strs, codes):
        assert np.array_equal(np.asarray(chars_to_codes(s, NUM_CODEBOOKS, CODEBOOK_SIZE)).reshape(NUM_CODEBOOKS, -1), c)
    m = StubModel()
    out = strs_to_audio(strs, m, "cpu")
    assert isinstance(out, list) and len(out) == 5
    for o, c in zip(out, codes):
        assert isinstance(o, np.ndarray) and o.dtype == np.float32 and o.shape == (1, 1920 * c.shape[1])
        if c.shape[1]:
            assert (o == np.float32(c[0, 0])).all()  # each string got ITS item back: input order kept
    check_calls(m, codes, [[0, 2, 3, 4]])  # one batch, the empty string not in it
    assert m.decode_calls == 0


def test_strs_to_audio_all_empty_makes_no_call():
    from mimi_hip import strs_to_audio
    m = StubModel()
    out = strs_to_audio(["", ""], m, "cpu")
    assert [o.shape for o in out] == [(1, 0), (1, 0)] and not m.ragged_calls
    assert strs_to_audio([], m, "cpu") == []


def test_strs_to_audio_split_by_budget():
    from mimi_hip import strs_to_audio
    lengths = [5, 0, 13, 2, 13, 40, 1, 1]
    strs, codes = make_strs(lengths, seed=1)
    m = StubModel()
    out = strs_to_audio(strs, m, "cpu", max_batch_frames=18)
    # consecutive batches with sum <= 18: [5, 13] | [2, 13] | [40] (over budget: alone) | [1, 1]
    check_calls(m, codes, [[0, 2], [3, 4], [5], [6, 7]])
    for o, c in zip(out, codes):
        assert o.shape == (1, 1920 * c.shape[1])
        if c.shape[1]:
            assert (o == np.float32(c[0, 0])).all()
    m2 = StubModel()
    strs_to_audio(strs, m2, "cpu", max_batch_frames=1)  # every item alone
    check_calls(m2, codes, [[i] for i, T in enumerate(lengths) if T])
    with pytest.raises(ValueError):
        strs_to_audio(strs, m2, "cpu", max_batch_frames=0)
