"""Test infrastructure: the hand-built codec-BPE models and words shared by ``tests/golden/make_bpe_encode_golden.py``
(which records what ``tokenizers`` 0.22.2 gives for them), ``tests/test_bpe_encode.py`` (CPU) and
``tests/test_bpe_encode_gpu.py``.

Small vocabularies over a 6-letter alphabet ``a..f`` = alphabet indices 0..5 = symbol ids 1..6 (id 0 is ``<pad>``).
A model is its merges in rank order, written as pairs of spellings; a merged spelling that already is a token
reuses that token's id (the trainer's convention), and merges may name tokens that a later merge forms (a hand-built
rank order no training would give, to put a formed pair above its round).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

N_SPECIAL = 1
SPECIALS = ["<pad>"]
LETTERS = "abcdef"
OFFSET = 0xE000

HAND_MODELS: Dict[str, List[Tuple[str, str]]] = {
    # merging all local rank minima at once is wrong: a b c d -> abc d, not ab cd
    "local_min": [("a", "b"), ("ab", "c"), ("c", "d")],
    "runs_aa": [("a", "a")],
    "runs_aa_then_aa_a": [("a", "a"), ("aa", "a")],
    "runs_aa_then_a_aa": [("a", "a"), ("a", "aa")],
    "runs_aa_a_first": [("aa", "a"), ("a", "a")],
    "runs_a_aa_first": [("a", "aa"), ("a", "a")],
    "runs_mixed": [("a", "a"), ("aa", "aa"), ("aa", "a"), ("b", "a")],
    # abc is formed by two merges (the second reuses its id); (abc, ab) out-ranks every merge that forms abc or ab
    "reuse_outrank_1": [("abc", "ab"), ("a", "b"), ("ab", "c"), ("b", "c"), ("a", "bc")],
    "reuse_outrank_2": [("abc", "ab"), ("b", "c"), ("a", "bc"), ("a", "b"), ("ab", "c")],
    "no_match": [("e", "f")],
    "empty": [],
}
# models in which a round can form a pair that out-ranks it (the model flag of the GPU encoder)
OUTRANKS = {"runs_aa_a_first", "runs_a_aa_first", "reuse_outrank_1", "reuse_outrank_2"}


def model_triples(pairs: List[Tuple[str, str]]) -> Tuple[np.ndarray, int, List[str]]:
    """(merges as (left id, right id, new id) int32 [n, 3], n_tokens, spellings in id order)."""
    ids = {c: N_SPECIAL + i for i, c in enumerate(LETTERS)}
    for left, right in pairs:
        ids.setdefault(left + right, N_SPECIAL + len(ids))
    spell = SPECIALS + sorted(ids, key=ids.get)
    tri = np.array([(ids[a], ids[b], ids[a + b]) for a, b in pairs], np.int32).reshape(-1, 3)
    return tri, len(spell), spell


def word(s: str) -> np.ndarray:
    return np.array([N_SPECIAL + LETTERS.index(c) for c in s], np.int32)


def hand_words(name: str) -> List[np.ndarray]:
    if name.startswith("runs"):
        out = [word("a" * n) for n in range(1, 10)]
        out += [word("b" + "a" * n) for n in range(1, 10)]
        out += [word("a" * n + "b" + "a" * m) for n, m in ((2, 3), (3, 2), (5, 4), (4, 5), (7, 7))]
        return out
    if name == "local_min":
        return [word(s) for s in ("abcd", "abcdabcd", "cdab", "abccd", "", "a", "ab", "cd", "dc")]
    if name.startswith("reuse_outrank"):
        return [word(s) for s in ("abc", "abcab", "abcabc", "abcabcabc", "bcabc", "cabcab", "abcabcab", "ababc",
                                  "bcab", "", "c", "bc")]
    return [word(s) for s in ("abcd", "ef", "fe", "", "e", "eff", "abcdef")]


def random_model_and_words(seed: int = 7):
    """A model trained (CPU oracle of the trainer) on random 6-letter words, and 300 words of lengths 0..40."""
    from oracle.bpe_ref import train_bpe
    rng = np.random.default_rng(seed)
    train = [rng.integers(0, 4 + i % 3, size=int(rng.integers(2, 40))).astype(np.int32) + N_SPECIAL
             for i in range(60)]
    tokens, merges = train_bpe(train, [1] * len(train), len(LETTERS), N_SPECIAL, N_SPECIAL + len(LETTERS) + 30, 2,
                               None)
    first = {}
    for i, t in enumerate(tokens):
        if i >= N_SPECIAL:
            first.setdefault(t, i)
    tri = np.array([(a, b, first[tokens[a] + tokens[b]]) for a, b in merges], np.int32).reshape(-1, 3)
    spell = SPECIALS + ["".join(LETTERS[i] for i in t) for t in tokens[N_SPECIAL:]]
    words = [rng.integers(0, 4 + i % 3, size=int(rng.integers(0, 41))).astype(np.int32) + N_SPECIAL
             for i in range(300)]
    return tri, len(tokens), spell, words


def to_str(w) -> str:
    return "".join(chr(OFFSET + int(x) - N_SPECIAL) for x in w)


_fixture = None


def fixture():
    """(meta, arrays) of tests/golden/bpe_encode.npz (+ the K = 8 merges of bpe.npz it refers to), loaded once."""
    global _fixture
    if _fixture is None:
        import json
        import os
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(here, "bpe_encode_meta.json")) as f:
            meta = json.load(f)
        with np.load(os.path.join(here, "bpe_encode.npz"), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        with np.load(os.path.join(here, "bpe.npz"), allow_pickle=False) as z:
            for name in ("recipe", "unlimited"):
                arrays[f"k8_{name}_merges"] = z[f"{name}_merges"]
        for a in arrays.values():
            a.setflags(write=False)
        _fixture = (meta, arrays)
    return _fixture


def split(flat: np.ndarray, lens: np.ndarray) -> List[np.ndarray]:
    ends = np.cumsum(lens)
    return [flat[e - n:e] for e, n in zip(ends, lens)]
