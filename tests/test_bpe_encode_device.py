"""Device-to-device codec-BPE encoding (``bpe_words.hip``: ``mimi_bpe_model_set_alphabet``,
``mimi_bpe_encode_codes``; ``bpe.Encoder.encode_device``): what can be checked without a GPU -- the exports, the
null-model returns, every argument error of ``encode_device`` (raised before any device call), and that the host word
model, which the GPU tests use as one of their references, equals ``tokenizers`` on the mark-run alphabet."""
import os
import re

import numpy as np
import pytest
import torch

import bpe_encode_ref as ref
from mimi_hip import _lib, bpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the mark-run alphabet: 27 starters U+02E5-02FF, 64 marks U+0300-033F (ccc 1, 202, 216, 220, 230, 232)
MARK_OFFSET, MARK_N, MARK_STARTERS = 0x2E5, 91, 27


def test_library_exports_the_two_entries_and_the_header_constants_agree():
    lib = _lib.load()
    for sym in ("mimi_bpe_model_set_alphabet", "mimi_bpe_encode_codes"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        text = f.read()
    cap = int(re.search(r"#define MIMI_BPE_WORDS_MAX_RUN (\d+)", text).group(1))
    assert cap == _lib.BPE_WORDS_MAX_RUN == bpe.Encoder.WORDS_MAX_RUN and cap >= 64
    assert int(re.search(r"#define MIMI_BPE_WORDS_SCAN_TILE (\d+)", text).group(1)) == _lib.BPE_WORDS_SCAN_TILE


def test_null_model_is_an_argument_error_without_a_device():
    lib = _lib.load()
    cls = np.zeros(4, np.uint8)
    assert lib.mimi_bpe_model_set_alphabet(None, 0, 1, 4, cls.ctypes.data, cls.ctypes.data) == 1
    assert b"null model" in lib.mimi_last_error()
    lens = np.array([3], np.int64)
    offs = np.zeros(2, np.int64)
    assert lib.mimi_bpe_encode_codes(None, None, 1, 0, 0, lens.ctypes.data, 0, None, 0, offs.ctypes.data, 1, None) == 1
    assert b"null model" in lib.mimi_last_error()


def test_encode_device_argument_errors_come_before_any_device_call():
    enc = bpe.Encoder(2, 2048, [], 1 + 4096, 1)
    good = torch.zeros(2, 5, dtype=torch.int32)
    cases = [
        ((np.zeros((2, 5), np.int32),), "CUDA torch.Tensor"),          # not a tensor
        ((torch.zeros(2, 5),), "int32 or int64"),                        # float
        ((torch.zeros(2, 5, dtype=torch.int16),), "int32 or int64"),
        ((torch.zeros(5, dtype=torch.int32),), r"\[B, K', T\]"),         # one dimension
        ((torch.zeros(1, 1, 2, 5, dtype=torch.int32),), r"\[B, K', T\]"),
        ((torch.zeros(1, 5, dtype=torch.int64),), "codebook rows"),      # K' < num_codebooks
        ((torch.zeros(3, 1, 5, dtype=torch.int64),), "codebook rows"),
        ((good, [6]), r"lengths must be in \[0, 5\]"),
        ((good, [-1]), r"lengths must be in \[0, 5\]"),
        ((good, [5, 5]), "2 lengths for 1 items"),
        ((good, None, -1), "chunk_frames"),
        ((good,), "CUDA torch.Tensor"),                                  # a CPU tensor, everything else right
        ((good[None], [5], 3), "CUDA torch.Tensor"),
    ]
    for args, match in cases:
        with pytest.raises(ValueError, match=match):
            enc.encode_device(*args)
    assert not enc._h  # no device model was made


def mark_encoder(merges=()):
    tri = np.asarray(merges, np.int32).reshape(-1, 3)
    return bpe.Encoder(1, MARK_N, tri, 1 + MARK_N + len(tri), 1, unicode_offset=MARK_OFFSET)


def mark_run_string(rng, runs, R, lead=True, tail=True):
    """`runs` runs of R random marks, 1-3 random starters before, between and after them (alphabet indices)."""
    out = []
    for r in range(runs):
        if r or lead:
            out += rng.integers(0, MARK_STARTERS, size=int(rng.integers(1, 4))).tolist()
        out += rng.integers(MARK_STARTERS, MARK_N, size=R).tolist()
    if tail:
        out += rng.integers(0, MARK_STARTERS, size=int(rng.integers(1, 4))).tolist()
    return np.array(out, np.int64)


def host_symbols(enc, idx):
    """The host word model's symbols of one sequence (its words joined: this alphabet has no split character)."""
    words = enc._chars.words(idx + MARK_OFFSET)
    return np.concatenate(words) + enc.n_special


def test_host_word_model_equals_tokenizers_on_the_mark_run_alphabet():
    """Runs of 1, 2, 5, 63, 64, 65 and 300 marks between starters and runs of up to 700 in an all-marks string:
    ``CharModel.words`` (the GPU tests' reference beside live ``tokenizers``) orders the marks as NFKC does."""
    enc = mark_encoder()
    assert set(enc._chars.ccc[MARK_STARTERS:].tolist()) == {1, 202, 216, 220, 230, 232}
    assert (enc._chars.cls[:MARK_STARTERS] == bpe.KEEP_STARTER).all()
    assert (enc._chars.cls[MARK_STARTERS:] == bpe.KEEP_MARK).all()
    spell = ref.spellings([], ["<pad>"], MARK_N, MARK_OFFSET, 1 + MARK_N)
    tok = ref.hf_tokenizer(spell, [], ["<pad>"])
    rng = np.random.default_rng(5)
    seqs = [mark_run_string(rng, 3, R) for R in (1, 2, 5, 63, 64, 65, 300)]
    seqs += [rng.integers(MARK_STARTERS, MARK_N, size=n).astype(np.int64) for n in (1, 2, 64, 65, 700)]
    for idx in seqs:
        want = ref.hf_ids(tok, "".join(chr(MARK_OFFSET + int(i)) for i in idx))
        assert host_symbols(enc, idx).tolist() == want
