"""Test infrastructure: a plain-Python restatement of how HF ``tokenizers``' BPE model encodes one word
(``Word::merge_all``, no dropout, ``ignore_merges`` off), pinned against ``tokenizers`` 0.22.2 itself in
``tests/test_bpe_encode.py``.

The rule: among all adjacent pairs that have a merge take the lowest rank; on equal rank the leftmost; merge that
one occurrence; repeat until no adjacent pair has a merge.  Two shortcuts are NOT equivalent: merging all local
rank minima at once (merges 1:(w,x)->p, 2:(p,a)->z, 3:(a,b)->n turn ``w x a b`` into ``z b``, not ``p n``), and a
sweep over the merges in rank order (the trainer reuses the id of an existing token with the same spelling, so a
pair formed by a merge can have a lower rank than the merge that formed it).
"""
from __future__ import annotations

import heapq
from typing import Dict, List, Sequence, Tuple


def merge_table(merges: Sequence[Sequence[int]]) -> Dict[Tuple[int, int], Tuple[int, int]]:
    """(left, right) -> (rank, new id) from (left, right, new id) triples in rank order; a repeated pair keeps
    its last rank, as tokenizers' merge map (a HashMap collected in order) does."""
    return {(int(a), int(b)): (r, int(c)) for r, (a, b, c) in enumerate(merges)}


def encode_word_naive(word: Sequence[int], table: Dict[Tuple[int, int], Tuple[int, int]]) -> List[int]:
    """The rule as stated, one full scan per round (quadratic: for short words)."""
    w = [int(x) for x in word]
    while True:
        best = None
        for i in range(len(w) - 1):
            m = table.get((w[i], w[i + 1]))
            if m is not None and (best is None or m[0] < best[0]):
                best = (m[0], i, m[1])
        if best is None:
            return w
        _, i, new = best
        w[i:i + 2] = [new]


def encode_word(word: Sequence[int], table: Dict[Tuple[int, int], Tuple[int, int]]) -> List[int]:
    """The same rule with a priority queue keyed (rank, position) over a linked word: positions never move, so
    the position order is the left-to-right order; an entry is stale when its pair no longer stands there."""
    sym = [int(x) for x in word]
    n = len(sym)
    nxt = list(range(1, n)) + [-1] if n else []
    prv = [-1] + list(range(n - 1)) if n else []
    heap = []
    for p in range(n - 1):
        m = table.get((sym[p], sym[p + 1]))
        if m is not None:
            heap.append((m[0], p))
    heapq.heapify(heap)
    while heap:
        rank, p = heapq.heappop(heap)
        if sym[p] < 0 or nxt[p] < 0:
            continue
        q = nxt[p]
        m = table.get((sym[p], sym[q]))
        if m is None or m[0] != rank:
            continue
        sym[p] = m[1]
        sym[q] = -1
        r = nxt[q]
        nxt[p] = r
        if r >= 0:
            prv[r] = p
            m2 = table.get((sym[p], sym[r]))
            if m2 is not None:
                heapq.heappush(heap, (m2[0], p))
        left = prv[p]
        if left >= 0:
            m2 = table.get((sym[left], sym[p]))
            if m2 is not None:
                heapq.heappush(heap, (m2[0], left))
    return [s for s in sym if s >= 0]


def formed_pair_outranks(merges: Sequence[Sequence[int]]) -> bool:
    """Some merge has on either side an id that a merge of higher rank produces: a round can then form a pair
    that out-ranks it, and merging every occurrence of a round's pair at once would be wrong."""
    formed: Dict[int, int] = {}
    for r, (_, _, c) in enumerate(merges):
        formed[int(c)] = r
    return any(formed.get(int(a), -1) > r or formed.get(int(b), -1) > r for r, (a, b, _) in enumerate(merges))


def spellings(merges: Sequence[Sequence[int]], specials: Sequence[str], n_base: int, unicode_offset: int,
              n_tokens: int) -> List[str]:
    """Token strings in id order: special tokens, the code characters, then the learned tokens."""
    spell: List = list(specials) + [chr(unicode_offset + i) for i in range(n_base)]
    spell += [None] * (n_tokens - len(spell))
    for a, b, c in merges:
        s = spell[int(a)] + spell[int(b)]
        assert spell[int(c)] in (None, s)
        spell[int(c)] = s
    return spell


def hf_tokenizer(spell: Sequence[str], merges: Sequence[Sequence[int]], specials: Sequence[str]):
    """The ``tokenizers`` object ``mimi_hip.bpe.Trainer`` assembles (BPE with ``unk_token=None``, NFKC, Metaspace
    without prefix) for a vocabulary given as spellings in id order and merges as id triples."""
    from tokenizers import Tokenizer, decoders, pre_tokenizers
    from tokenizers.models import BPE
    from tokenizers.normalizers import NFKC
    vocab = {}
    for i, s in enumerate(spell):
        vocab.setdefault(s, i)
    tok = Tokenizer(BPE(vocab, [(spell[int(a)], spell[int(b)]) for a, b, _ in merges], unk_token=None))
    if specials:
        tok.add_special_tokens(list(specials))
    tok.normalizer = NFKC()
    tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="never")
    tok.decoder = decoders.Metaspace(replacement="▁", prepend_scheme="never")
    return tok


def hf_ids(tok, text: str) -> List[int]:
    return list(getattr(tok, "backend_tokenizer", tok).encode(text, add_special_tokens=False).ids)
