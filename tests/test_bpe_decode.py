"""Codec-BPE decoding, ids back to codes (``bpe_decode.hip``: ``mimi_bpe_model_set_spellings``,
``mimi_bpe_decode_plan``, ``mimi_bpe_decode_write``; ``bpe.Encoder.decode_ids`` / ``decode_device``;
``codes.ids_to_audio``): what can be checked without a GPU.  ``decode_ids``, the host statement of the contract that
the GPU tests compare the kernels with, is pinned here to the committed fixture (``tokenizers`` ``decode`` followed by
the reference converter's ``chars_to_codes``) and to a plain per-character loop.  Every comparison is exact integer
equality."""
import os
import re

import numpy as np
import pytest
import torch

import bpe_decode_cases as cases
import bpe_encode_cases as enc_cases
import bpe_encode_ref as ref
from mimi_hip import _lib, bpe, codes as codes_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET, CBS = cases.OFFSET, cases.CBS


def test_library_exports_the_three_entries_and_the_header_constant_agrees():
    lib = _lib.load()
    for sym in ("mimi_bpe_model_set_spellings", "mimi_bpe_decode_plan", "mimi_bpe_decode_write"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        text = f.read()
    tile = int(re.search(r"#define MIMI_BPE_DECODE_SCAN_TILE (\d+)", text).group(1))
    assert tile == _lib.BPE_DECODE_SCAN_TILE and tile % 256 == 0


def test_null_model_is_an_argument_error_without_a_device():
    lib = _lib.load()
    offs = np.zeros(2, np.int64)
    assert lib.mimi_bpe_model_set_spellings(None, offs.ctypes.data, None) == 1
    assert b"null model" in lib.mimi_last_error()
    assert lib.mimi_bpe_decode_plan(None, None, offs.ctypes.data, 1, offs.ctypes.data, None) == 1
    assert b"null model" in lib.mimi_last_error()
    assert lib.mimi_bpe_decode_write(None, None, 0, 0, 0, None) == 1
    assert b"null model" in lib.mimi_last_error()


@pytest.mark.parametrize("case", cases.CASES)
def test_decode_ids_equals_every_fixture_entry(case):
    enc = cases.trained_encoder(case)
    names = [name for name, _, _ in cases.entries(case)]
    for required in ("ids3", "del10", "del40", "shuffled", "special_start", "special_middle", "special_end",
                     "all_special", "single_alphabet", "single_learned", "below_k"):
        assert required in names
    assert sum(n.startswith("phase") for n in names) == enc.num_codebooks
    got = enc.decode_ids([ids for _, ids, _ in cases.entries(case)])
    for (name, ids, want), g in zip(cases.entries(case), got):
        assert g.dtype == np.int64 and g.shape == want.shape and np.array_equal(g, want), (case, name)
        assert np.array_equal(cases.decode_loop(enc, ids), want), (case, name)


def test_the_fixture_exercises_both_branches_of_the_filter():
    """Over the deleted and shuffled sequences together the reference keeps between 20 % and 80 % of the characters."""
    meta, _ = cases.fixture()
    assert meta["mixed"] == ["del10", "del40", "shuffled"]
    chars = kept = 0
    for case in cases.CASES:
        enc = cases.trained_encoder(case)
        for name, ids, want in cases.entries(case):
            if name in meta["mixed"]:
                n = cases.spelled_length(enc, ids)
                assert n == meta["cases"][case]["entries"][name]["chars"]
                chars += n
                kept += want.size
    assert 0.2 <= kept / chars <= 0.8, kept / chars
    # and some sequence is dropped to nothing while still spelling characters
    assert all(meta["cases"][c]["entries"]["below_k"]["frames"] == 0 for c in cases.CASES)


@pytest.mark.parametrize("K", [1, 2, 3, 8, 16, 17])
def test_decode_ids_equals_the_loop_on_random_streams(K):
    enc = cases.hand_encoder(K, seed=K)
    rng = np.random.default_rng(100 + K)
    seqs = [cases.random_ids(enc, rng, int(rng.integers(0, 300))) for _ in range(40)]
    # consistent streams with deletions and a random start phase
    for _ in range(20):
        n = int(rng.integers(1, 400))
        cb = (int(rng.integers(K)) + np.arange(n)) % K
        ids = enc.n_special + cb * enc.codebook_size + rng.integers(0, enc.codebook_size, size=n)
        seqs.append(ids[rng.random(n) >= rng.choice([0.0, 0.1, 0.4])].astype(np.int32))
    got = enc.decode_ids(seqs)
    for ids, g in zip(seqs, got):
        assert np.array_equal(g, cases.decode_loop(enc, ids)), (K, ids.tolist()[:30])
    assert any(g.shape[1] > 0 for g in got)


def host_encode(enc, codes):
    """``encode_codes`` without the GPU: the host word model, then the host restatement of the merge rule."""
    cps = codes_mod.codes_to_codepoints(codes[:enc.num_codebooks], enc.codebook_size, unicode_offset=enc.unicode_offset)
    table = ref.merge_table(enc.merges.tolist())
    out = []
    for w in enc._chars.words(cps):
        out += ref.encode_word((w + enc.n_special).tolist(), table)
    return np.array(out, np.int32)


@pytest.mark.parametrize("case", cases.CASES)
def test_round_trip_of_nfkc_stable_codes(case):
    """decode_ids(encode(c)) == c for codes made only of characters NFKC keeps (the merge step on the host here,
    ``bpe_encode_ref.encode_word``; through ``encode_codes`` / ``encode_device`` in the GPU file)."""
    enc = cases.trained_encoder(case)
    K = enc.num_codebooks
    _, arrays = enc_cases.fixture()
    codes = arrays[f"{case}_cps3"].astype(np.int64).reshape(-1, K).T - OFFSET - CBS * np.arange(K)[:, None]
    # frames of kept starters only: NFKC neither rewrites nor reorders them
    plain = enc._chars.cls.reshape(K, CBS) == bpe.KEEP_STARTER
    frames = codes[:, plain[np.arange(K)[:, None], codes].all(axis=0)]
    assert frames.shape[1] >= 20
    ids = host_encode(enc, frames)
    assert ids.size < frames.size  # merges applied
    assert np.array_equal(enc.decode_ids([ids])[0], frames)


@pytest.mark.parametrize("case", ["k8_recipe", "k2_unlimited"])
def test_spellings_from_raw_merges_equal_those_from_the_tokenizer(case):
    meta, arrays = enc_cases.fixture()
    c = meta["trained"][case]
    K, tri = c["num_codebooks"], arrays[f"{case}_merges"]
    tok = ref.hf_tokenizer(ref.spellings(tri, enc_cases.SPECIALS, K * CBS, OFFSET, c["n_tokens"]), tri,
                           enc_cases.SPECIALS)
    from_tok = bpe.Encoder.from_tokenizer(tok, K, CBS, unicode_offset=OFFSET)
    raw = cases.trained_encoder(case)
    assert from_tok.n_tokens == raw.n_tokens and from_tok.n_special == raw.n_special
    (o1, i1), (o2, i2) = from_tok.spellings(), raw.spellings()
    assert np.array_equal(o1, o2) and np.array_equal(i1, i2)
    assert o1[1] == 0 and o1[2] == 1 and o1[-1] > raw.n_tokens  # <pad> empty, a character itself, learned longer


def test_from_trainer_spellings_equal_those_from_its_merges():
    class T:
        special_tokens = ["<pad>"]
        num_codebooks, codebook_size, unicode_offset, device, unk_token = 2, 4, OFFSET, 0, None
        last_tokens = [(0, 4), (0, 4, 1), (1, 5)]
        last_merges = [(1, 5), (9, 2), (2, 6)]
    enc = bpe.Encoder.from_trainer(T)
    raw = bpe.Encoder(2, 4, enc.merges, enc.n_tokens, 1, unicode_offset=OFFSET)
    assert all(np.array_equal(a, b) for a, b in zip(enc.spellings(), raw.spellings()))
    assert enc.decode_ids([[10, 7, 0, 11]])[0].tolist() == [[0, 1, 1], [0, 2, 1]]


def test_a_vocabulary_entry_that_is_not_code_characters_is_refused():
    spell = ["<pad>"] + [chr(OFFSET + i) for i in range(8)] + ["x" + chr(OFFSET)]
    tok = ref.hf_tokenizer(spell, [], ["<pad>"])
    with pytest.raises(NotImplementedError, match="not a string of code characters"):
        bpe.Encoder.from_tokenizer(tok, 2, 4, unicode_offset=OFFSET)


def test_argument_errors_come_before_any_device_call():
    enc = bpe.Encoder(2, 4, [(1, 5, 9)], 10, 1, unicode_offset=OFFSET)
    with pytest.raises(ValueError, match="outside"):
        enc.decode_ids([[1, 10]])
    with pytest.raises(ValueError, match="outside"):
        enc.decode_ids([[-1]])
    with pytest.raises(ValueError, match="spellings for"):
        bpe.Encoder(2, 4, [], 9, 1, unicode_offset=OFFSET, spellings=[()] * 8)
    with pytest.raises(ValueError, match="outside the code alphabet"):
        bpe.Encoder(2, 4, [], 9, 1, unicode_offset=OFFSET, spellings=[()] * 8 + [(8,)])
    good = torch.zeros(5, dtype=torch.int32)
    bad = [
        ((np.zeros(5, np.int32),), {}, "CUDA torch.Tensor"),
        ((torch.zeros(5),), {}, "int32 or int64"),
        ((torch.zeros(5, dtype=torch.int16),), {}, "int32 or int64"),
        ((torch.zeros(1, 2, 5, dtype=torch.int32),), {}, r"\[n\] or \[B, L\]"),
        ((good, [1, 3]), {}, "seq_offsets must"),
        ((good, [0, 3, 2]), {}, "seq_offsets must"),
        ((good, [0, 6]), {}, "seq_offsets must"),
        ((good, []), {}, "seq_offsets must"),
        ((good,), {"lengths": [5]}, "lengths go with 2-D"),
        ((good[None], [0, 5]), {}, "seq_offsets go with 1-D"),
        ((good[None],), {"lengths": [6]}, r"lengths must be in \[0, 5\]"),
        ((good[None],), {"lengths": [-1]}, r"lengths must be in \[0, 5\]"),
        ((good[None],), {"lengths": [1, 2]}, "2 lengths for 1 rows"),
        ((good, [0, 5]), {}, "CUDA torch.Tensor"),  # a CPU tensor, everything else right
        ((good[None],), {"lengths": [3]}, "CUDA torch.Tensor"),
    ]
    for args, kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            enc.decode_device(*args, **kwargs)
    assert not enc._h  # no device model was made
    with pytest.raises(ValueError, match="max_batch_frames"):
        codes_mod.ids_to_audio(good, [0, 5], enc, None, max_batch_frames=0)
    with pytest.raises(ValueError, match="8 codebooks"):
        codes_mod.ids_to_audio(good, [0, 5], enc, None)


def test_filter_scan_order_matters():
    """The composition does not commute: on random streams the commuted scan gives another keep mask."""
    rng = np.random.default_rng(3)
    differ = 0
    for _ in range(50):
        cb = rng.integers(0, 4, size=200)
        differ += not np.array_equal(bpe.filter_keep(cb, 4), bpe.filter_keep(cb, 4, commuted=True))
    assert differ >= 25
