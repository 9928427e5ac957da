"""Test infrastructure shared by ``tests/test_bpe_decode.py`` (CPU) and ``tests/test_bpe_decode_gpu.py``: the
``bpe_decode.npz`` fixture (``tests/golden/make_bpe_decode_golden.py``), hand-built models over small alphabets, and
the decode contract restated as a plain per-character loop -- the slow, obvious form that the vectorised
``Encoder.decode_ids`` is pinned to beside the fixture."""
from __future__ import annotations

import json
import os
from typing import List

import numpy as np

import bpe_encode_cases as enc_cases

OFFSET, CBS = enc_cases.OFFSET, 2048
CASES = ("k8_recipe", "k8_unlimited", "k2_ngram2", "k2_unlimited")

_fixture = None


def fixture():
    """(meta, arrays) of tests/golden/bpe_decode.npz, loaded once, read-only."""
    global _fixture
    if _fixture is None:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(here, "bpe_decode_meta.json")) as f:
            meta = json.load(f)
        with np.load(os.path.join(here, "bpe_decode.npz"), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        for a in arrays.values():
            a.setflags(write=False)
        _fixture = (meta, arrays)
    return _fixture


def entries(case):
    """[(name, ids int32, codes int64 [K, T])] of one trained case."""
    meta, arrays = fixture()
    return [(name, arrays[f"{case}_{name}_ids"], arrays[f"{case}_{name}_codes"].astype(np.int64))
            for name in meta["cases"][case]["entries"]]


_encoders = {}


def trained_encoder(case):
    """The encoder of a trained case, built from its raw merges (so its spellings come from the merges)."""
    from mimi_hip import bpe
    if case not in _encoders:
        meta, arrays = enc_cases.fixture()
        c = meta["trained"][case]
        _encoders[case] = bpe.Encoder(c["num_codebooks"], CBS, arrays[f"{case}_merges"], c["n_tokens"], 1,
                                      unicode_offset=OFFSET)
    return _encoders[case]


def hand_encoder(K, cbs=4, n_special=2, n_merges=24, max_len=40, seed=0, chain=0):
    """A model of K codebooks of `cbs` codes in the private-use area: `n_merges` random merges of earlier tokens
    (spellings up to `max_len` characters), then `chain` merges that double one token (2^chain times its length)."""
    from mimi_hip import bpe
    rng = np.random.default_rng(seed)
    n_base = K * cbs
    lens = [0] * n_special + [1] * n_base
    tri = []
    while len(tri) < n_merges:
        a, b = (int(x) for x in rng.integers(n_special, len(lens), size=2))
        if lens[a] + lens[b] > max_len:
            continue
        tri.append((a, b, len(lens)))
        lens.append(lens[a] + lens[b])
    last = n_special  # the first alphabet id
    for _ in range(chain):
        tri.append((last, last, len(lens)))
        lens.append(2 * lens[last])
        last = len(lens) - 1
    return bpe.Encoder(K, cbs, tri, len(lens), n_special, unicode_offset=OFFSET)


def decode_loop(enc, ids, commuted=None) -> np.ndarray:
    """The contract, one character at a time: expand, drop inconsistent, drop hanging, frames."""
    K, cbs = enc.num_codebooks, enc.codebook_size
    off, idx = enc.spellings()
    chars: List[int] = []
    for i in ids:
        i = int(i)
        if not 0 <= i < enc.n_tokens:
            raise ValueError("id")
        chars += idx[off[i]:off[i + 1]].tolist()
    if not chars:
        return np.zeros((K, 0), np.int64)
    cb0 = chars[0] // cbs
    expected, kept = cb0, []
    for c in chars:
        if c // cbs == expected:
            kept.append(c)
            expected = (expected + 1) % K
    kept = kept[min((K - cb0) % K, len(kept)):]
    kept = kept[:len(kept) - len(kept) % K]
    frames = np.array(kept, np.int64).reshape(-1, K)
    return np.ascontiguousarray((frames - np.arange(K) * cbs).T)


def random_ids(enc, rng, n, special=0.05):
    """n random ids of the whole vocabulary, a share of them special."""
    ids = rng.integers(enc.n_special, enc.n_tokens, size=n)
    if enc.n_special:
        where = rng.random(n) < special
        ids[where] = rng.integers(0, enc.n_special, size=int(where.sum()))
    return ids.astype(np.int32)


def spelled_length(enc, ids) -> int:
    off, _ = enc.spellings()
    ids = np.asarray(ids, np.int64)
    return int((off[ids + 1] - off[ids]).sum())
