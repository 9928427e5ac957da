"""TEST INFRASTRUCTURE -- never shipped.  Two plain-Python models of the codec-BPE trainer (``csrc/bpe.hip``) and
the corpora that audit it after every merge (``tests/test_bpe_train_ref.py`` on the CPU,
``tests/test_bpe_train_kernels.py`` on the GPU).

* ``Reference``: the rules and nothing else.  Words are lists; a merge rewrites every word left to right
  (``apply_merge``); the pair counts are recounted from scratch after every merge (``recount``) under the
  eligibility rule; ``best`` takes the highest count, ties to the smallest (left, right).  It shares no data
  structure with the kernels: no links, no table, no deltas.  ``merge`` accepts any pair and any id.
* ``Emulation``: ``bpe.hip`` restated step by step -- flat ``sym`` / ``nxt`` / ``prv`` / ``wc`` / ``flag`` arrays,
  starts marked from the pre-merge state (parity rule for ``a == b``), the deltas of ``delta_kernel`` per start
  (``flag[R]``, ``lpartner``, absent keys skipped on decrement), relink, zeroing of the merged pair -- and the
  table's bookkeeping (keys inserted since the last rebuild, the rebuild keeping positive counts only, the doubling
  rule of ``mimi_bpe_best``, the post-count size), so it predicts ``table_slots`` and ``growth_rehashes`` for any
  ``min_table_slots``.  ``FAULTS`` names single faults it can carry, each standing for one line of ``bpe.hip``.

Both offer ``best() / merge(a, b, nid, nlen) / words() / pairs()``, as does the GPU handle wrapper of the GPU test;
``drive`` runs any of them through a training ("best pair each step") or a forced schedule.
"""
from __future__ import annotations

import heapq
import random
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

K_MAX_ID = (1 << 17) - 1  # bpe.hip kMaxId: ids up to 131070, vocab_size <= 131071
DEFAULT_ROOM = 1 << 20    # the default min_table_slots
DEFAULT_GRID = 256 * 8    # CUs x 8 on an MI355X (only fault 13 and the info figure depend on it)


def pow2_at_least(x: int, floor: int = 1024) -> int:
    c = floor
    while c < x:
        c <<= 1
    return c


def small_table(vocab_size: int) -> int:
    """The smallest min_table_slots mimi_bpe_create_opts accepts: pow2(8 x vocab_size)."""
    return pow2_at_least(8 * vocab_size, 1)


def eligible(lx: int, ly: int, maxlen: int) -> bool:
    return maxlen <= 0 or (lx == 1 and ly == 1) or lx + ly < maxlen


# ---- the reference ---------------------------------------------------------------------------------------------
def apply_merge(word: Sequence[int], a: int, b: int, nid: int) -> List[int]:
    """The sequential left-to-right rewrite of one word."""
    out, i, n = [], 0, len(word)
    while i < n:
        if i + 1 < n and word[i] == a and word[i + 1] == b:
            out.append(nid)
            i += 2
        else:
            out.append(word[i])
            i += 1
    return out


def recount(words, counts, lens: Dict[int, int], maxlen: int) -> Dict[Tuple[int, int], int]:
    """Positive pair counts of the current words, weighted by word count, under eligible()."""
    pc: Dict[Tuple[int, int], int] = {}
    for w, c in zip(words, counts):
        if c <= 0:
            continue
        for x, y in zip(w, w[1:]):
            pc[(x, y)] = pc.get((x, y), 0) + c
    if maxlen > 0:
        pc = {p: c for p, c in pc.items() if eligible(lens.get(p[0], 1), lens.get(p[1], 1), maxlen)}
    return pc


def best(pairs: Dict[Tuple[int, int], int]) -> Tuple[int, int, int]:
    """(left, right, count) of the max count, ties to the smallest (left, right); (-1, -1, 0) when none."""
    if not pairs:
        return (-1, -1, 0)
    c = max(pairs.values())
    a, b = min(p for p, v in pairs.items() if v == c)
    return (a, b, c)


class Reference:
    def __init__(self, words, counts, maxlen: int = 0):
        self.w = [list(w) for w in words]
        self.counts = [int(c) for c in counts]
        self.maxlen = int(maxlen or 0)
        self.lens: Dict[int, int] = {}  # learned tokens; every other id has length 1
        self._pairs = recount(self.w, self.counts, self.lens, self.maxlen)

    def best(self):
        return best(self._pairs)

    def merge(self, a, b, nid, nlen):
        self.lens[nid] = nlen
        self.w = [apply_merge(w, a, b, nid) if a in w else w for w in self.w]
        self._pairs = recount(self.w, self.counts, self.lens, self.maxlen)

    def words(self):
        return [list(w) for w in self.w]

    def pairs(self):
        return dict(self._pairs)


# ---- the emulation ---------------------------------------------------------------------------------------------
# name -> the line of bpe.hip it stands for (numbered as in the audit's table)
FAULTS = {
    "parity_dropped": (1, "mark_kernel: `if (k & 1) continue;` removed"),
    "parity_from_right": (2, "mark_kernel: the a == b walk follows nxt from the partner instead of prv from p"),
    "flagR_dropped": (3, "delta_kernel: `R >= 0 && !flag[R]` -> `R >= 0`"),
    "lpartner_ignored": (4, "delta_kernel: `ls = lpartner ? m.nid : sym[L]` -> `ls = sym[L]`"),
    "le_maxlen": (5, "eligible: `lx + ly < m.maxlen` -> `<=`"),
    "no_11_exemption": (6, "eligible: `(lx == 1 && ly == 1) ||` removed"),
    "pair_not_zeroed": (7, "mimi_bpe_merge: zero_pair_kernel not launched"),
    "ties_largest": (8, "best_kernel<true>: `kMaxId - a`, `kMaxId - b` -> `a`, `b`"),
    "ties_left_only": (9, "best_kernel<true>: the right field always kMaxId (ties of one left id: largest right)"),
    "id16": (10, "kIdBits = 16, kMaxId = 65535"),
    "rebuild_gt1": (11, "rehash_kernel: `v > 0` -> `v > 1`"),
    "rebuild_keeps_nkeys": (12, "rehash: the new table's nkeys starts at the old table's"),
    "single_pass": (13, "count_pairs_kernel / mark_kernel: `for (p = tid; p < n; p += stride)` -> `if (p < n)`"),
    "prv_not_relinked": (14, "relink_kernel: `if (R >= 0) prv[R] = p;` removed"),
    "len_not_written": (15, "relink_kernel: `len[nid] = nlen` removed"),
}


class StateError(Exception):
    """What mimi_bpe_read_words reports as MIMI_ERR_STATE."""


class Emulation:
    def __init__(self, words, counts, maxlen: int = 0, min_table_slots: Optional[int] = None,
                 grid_blocks: Optional[int] = None, faults: Iterable[str] = ()):
        self.F = frozenset(faults)
        assert self.F <= set(FAULTS), self.F - set(FAULTS)
        self.maxlen = int(maxlen or 0)
        self.grid = grid_blocks or DEFAULT_GRID
        self.floor = min_table_slots or 1024
        self.room = min_table_slots or DEFAULT_ROOM
        sym, nxt, prv, wc, first = [], [], [], [], []
        for w, c in zip(words, counts):
            p0 = len(sym)
            first.append((p0, len(w)))
            for i, x in enumerate(w):
                sym.append(int(x))
                prv.append(p0 + i - 1 if i else -1)
                nxt.append(p0 + i + 1 if i + 1 < len(w) else -1)
                wc.append(int(c))
        self.sym, self.nxt, self.prv, self.wc, self.first = sym, nxt, prv, wc, first
        self.n = len(sym)
        self.symv = np.array(sym, dtype=np.int64)  # a mirror of sym: the mark scan's `sym[p] == a` in one numpy pass
        self.heap: list = []  # (-count, tie key, pair) of every count ever set: best() without a table sweep
        self.flag = [0] * self.n
        self.len: Dict[int, int] = {}  # the device array starts at 1 everywhere
        self.table: Dict[Tuple[int, int], int] = {}
        self.nkeys = 0
        self.slots = pow2_at_least(2 * max(self.n, 1) + 1024, self.floor)
        self.rehashes = 0  # growth rehashes (mimi_bpe_best)
        # count_pairs_kernel, then the post-count rebuild
        for p in range(self._visited()):
            q = nxt[p]
            if sym[p] >= 0 and q >= 0:
                self._add((sym[p], sym[q]), wc[p], True)
        self._rehash(pow2_at_least(4 * self.nkeys + self.room, self.floor))

    def _visited(self) -> int:
        return min(self.n, self.grid * 256) if "single_pass" in self.F else self.n

    def _add(self, key, delta, insert):
        t = self.table
        if key in t:
            t[key] += delta
        elif insert:
            t[key] = delta
            self.nkeys += 1
        else:
            return
        if t[key] > 0:
            heapq.heappush(self.heap, (-t[key], self._tie_key(key), key))

    def _tie_key(self, p):
        """Smaller wins among equal counts: what the second sweep's packed maximum decides."""
        if "ties_largest" in self.F:
            return (-p[0], -p[1])
        if "ties_left_only" in self.F:
            return (p[0], -p[1])
        if "id16" in self.F:  # 32-bit unsigned 65535 - id, shifted by 16 into a 64-bit word
            return -(((((65535 - p[0]) & 0xFFFFFFFF) << 16) | ((65535 - p[1]) & 0xFFFFFFFF)) & ((1 << 64) - 1))
        return p

    def _rehash(self, cap):
        keep = 1 if "rebuild_gt1" in self.F else 0
        old = self.nkeys
        self.table = {k: v for k, v in self.table.items() if v > keep}
        self.nkeys = len(self.table) + (old if "rebuild_keeps_nkeys" in self.F else 0)
        self.slots = cap

    def _tok_len(self, x, nid, nlen):
        return nlen if x == nid else self.len.get(x, 1)

    def _elig(self, x, y, nid, nlen):
        lx, ly = self._tok_len(x, nid, nlen), self._tok_len(y, nid, nlen)
        if self.maxlen <= 0:
            return True
        if "no_11_exemption" not in self.F and lx == 1 and ly == 1:
            return True
        return lx + ly <= self.maxlen if "le_maxlen" in self.F else lx + ly < self.maxlen

    def best(self):
        h, t = self.heap, self.table
        while h and t.get(h[0][2]) != -h[0][0]:  # counts that have changed since, or were dropped by a rebuild
            heapq.heappop(h)
        if not h:
            res = (-1, -1, 0)
        elif "id16" in self.F:  # the ids as decoded from the 16-bit fields
            m = -h[0][1]
            res = (65535 - ((m >> 16) & 65535), 65535 - (m & 65535), -h[0][0])
        else:
            res = (h[0][2][0], h[0][2][1], -h[0][0])
        if 2 * self.nkeys > self.slots:  # the doubling rule
            self._rehash(self.slots * 2)
            self.rehashes += 1
        return res

    def merge(self, a, b, nid, nlen):
        F, sym, nxt, prv, wc, flag = self.F, self.sym, self.nxt, self.prv, self.wc, self.flag
        # mark_kernel (the parity walk of every p at once: links only run forward, so prv[p] < p < nxt[p])
        cand = [p for p in np.flatnonzero(self.symv == a).tolist() if nxt[p] >= 0 and sym[nxt[p]] == b]
        k = None
        if a == b and "parity_dropped" not in F:
            # the walk's count for every candidate at once (the kernel walks per thread: quadratic in the run).  p's
            # neighbour in the run is a candidate itself, and comes earlier in the order taken here.
            k = {}
            if "parity_from_right" in F:  # the a's after p's partner
                for p in reversed(cand):
                    k[p] = k.get(nxt[p], -1) + 1
            else:  # the a's before p
                for p in cand:
                    r = prv[p]
                    k[p] = k[r] + 1 if r >= 0 and sym[r] == a else 0
        starts = []
        visited = self._visited()
        for p in cand:
            if p >= visited or (k is not None and k[p] & 1):
                continue
            flag[p] = 1
            starts.append(p)
        # delta_kernel
        for p in starts:
            q = nxt[p]
            L, R, c = prv[p], nxt[q], wc[p]
            if L >= 0:
                self._add((sym[L], a), -c, False)
                lpartner = prv[L] >= 0 and flag[prv[L]] and "lpartner_ignored" not in F
                ls = nid if lpartner else sym[L]
                if self._elig(ls, nid, nid, nlen):
                    self._add((ls, nid), c, True)
            if R >= 0 and (not flag[R] or "flagR_dropped" in F):
                self._add((b, sym[R]), -c, False)
                if self._elig(nid, sym[R], nid, nlen):
                    self._add((nid, sym[R]), c, True)
        # relink_kernel (every start reads its links before any write here; on the device the starts never overlap)
        if "len_not_written" not in F:
            self.len[nid] = nlen
        for p, q, R in [(p, nxt[p], nxt[nxt[p]]) for p in starts]:
            sym[p] = self.symv[p] = nid
            nxt[p] = R
            if R >= 0 and "prv_not_relinked" not in F:
                prv[R] = p
            sym[q] = nxt[q] = prv[q] = self.symv[q] = -1
            flag[p] = 0
        # zero_pair_kernel
        if "pair_not_zeroed" not in F and (a, b) in self.table:
            self.table[(a, b)] = 0

    def words(self):
        """As mimi_bpe_read_words: StateError where it returns MIMI_ERR_STATE."""
        sym, nxt, prv = self.sym, self.nxt, self.prv
        live = 0
        for p in range(self.n):
            if sym[p] >= 0:
                live += 1
            elif nxt[p] != -1 or prv[p] != -1:
                raise StateError(f"dead symbol {p} is linked")
        out, seen = [], 0
        for p0, n in self.first:
            w = []
            p = p0 if n else -1
            if n and prv[p0] != -1:
                raise StateError(f"first symbol {p0} has a predecessor")
            while p >= 0:
                if not p0 <= p < p0 + n or sym[p] < 0 or seen >= live:
                    raise StateError(f"bad link to {p}")
                q = nxt[p]
                if q >= 0 and (q >= self.n or prv[q] != p):
                    raise StateError(f"prv[nxt[{p}]] != {p}")
                w.append(sym[p])
                seen += 1
                p = q
            out.append(w)
        if seen != live:
            raise StateError(f"{live - seen} live symbols unreachable")
        return out

    def pairs(self):
        return {p: v for p, v in self.table.items() if v > 0}


# ---- driving a model -------------------------------------------------------------------------------------------
def drive(model, corpus, forced: Sequence[Tuple[int, int, int, int]] = (), max_merges: Optional[int] = None):
    """Generator over one run of ``model``: first the ``forced`` merges (a, b, nid, nlen) as given, then training,
    best pair each step, until the vocabulary is full or the best count is below min_frequency.  Yields
    ("merge", (a, b, nid, nlen)) after every merge and ("best", (a, b, count)) after every best, the one that ends
    training included; the consumer reads the model's state in between.  Ids are assigned as
    ``mimi_hip.bpe.train_words_gpu`` does: a spelling that exists reuses its id."""
    n0, vocab, mf = corpus["n_initial"], corpus["vocab_size"], corpus["min_frequency"]
    learned: Dict[int, Tuple[int, ...]] = {}
    tok_id: Dict[Tuple[int, ...], int] = {}
    spell = lambda x: learned[x] if x in learned else (x,)  # noqa: E731
    next_id = n0
    for a, b, nid, nlen in forced:
        model.merge(a, b, nid, nlen)
        if nid not in learned and nid >= n0:
            learned[nid] = spell(a) + spell(b)
            tok_id.setdefault(learned[nid], nid)
        next_id = max(next_id, nid + 1)
        yield "merge", (a, b, nid, nlen)
    done = 0
    while True:
        a, b, c = model.best()
        yield "best", (a, b, c)
        if next_id >= vocab or c < 1 or c < mf or (max_merges is not None and done >= max_merges):
            return
        new = spell(a) + spell(b)
        nid = tok_id.get(new)
        if nid is None:
            nid = next_id
            next_id += 1
            learned[nid] = new
            tok_id[new] = nid
        model.merge(a, b, nid, len(new))
        done += 1
        yield "merge", (a, b, nid, len(new))


def snapshot(model):
    """(words, positive pairs) of a model, or ("invalid", message) where the links are inconsistent."""
    try:
        w = model.words()
    except StateError as e:
        return ("invalid", str(e))
    return (w, model.pairs())


def trajectory(model, corpus, forced=(), max_merges=None):
    """Every event of a run with the state after it: [(kind, payload, snapshot)], the creation state first."""
    out = [("create", None, snapshot(model))]
    for kind, payload in drive(model, corpus, forced, max_merges):
        out.append((kind, payload, snapshot(model) if kind == "merge" else None))
    return out


def merges_of(traj):
    return [p[:2] for k, p, _ in traj if k == "merge"]


def first_difference(ref_traj, traj):
    """(first state step, first merge-list step) at which ``traj`` leaves ``ref_traj``; None = never.  Step s is the
    state after s merges: its words, its positive pairs and the winner taken from it.  The merge-list step is the
    index of the first merge whose pair differs (or that one run has and the other has not)."""
    def by_step(t):
        steps, s = {}, 0
        for kind, payload, snap in t:
            if kind == "merge":
                s += 1
            d = steps.setdefault(s, {})
            if kind == "best":
                d["best"] = payload
            else:
                d["state"] = snap
        return steps
    A, B = by_step(ref_traj), by_step(traj)
    state = next((s for s in range(max(len(A), len(B))) if A.get(s) != B.get(s)), None)
    ma, mb = merges_of(ref_traj), merges_of(traj)
    merge = next((i for i in range(max(len(ma), len(mb))) if i >= len(ma) or i >= len(mb) or ma[i] != mb[i]), None)
    return state, merge


# ---- corpora ---------------------------------------------------------------------------------------------------
# Ids: 0 is the one special token, the alphabet follows; words hold ids, not alphabet indices.
def _corpus(name, words, counts, n_initial, n_merges, min_frequency=1, maxlen=0):
    return {"name": name, "words": [list(map(int, w)) for w in words], "counts": [int(c) for c in counts],
            "n_initial": n_initial, "vocab_size": n_initial + n_merges, "min_frequency": min_frequency,
            "maxlen": maxlen}


RUN_LENGTHS = list(range(1, 10)) + [63, 64, 65, 255, 256, 257, 4096, 4097]


def runs():
    """Runs of one symbol, bare and bracketed by another symbol: the a == b parity walk at every length class."""
    rng = random.Random(101)
    a, b = 1, 2
    words = [[a] * n for n in RUN_LENGTHS] + [[b] + [a] * n + [b] for n in RUN_LENGTHS]
    return _corpus("runs", words, [rng.randint(1, 3) for _ in words], 3, 40)


def overlap():
    """Adjacent occurrences: flag[R] and lpartner, both in one word where three occurrences touch."""
    rng = random.Random(102)
    a, b, c = 1, 2, 3
    ab = lambda n: [a if i % 2 == 0 else b for i in range(n)]  # noqa: E731
    words = [ab(n) for n in (2, 3, 4, 5, 6, 7, 8, 9, 12, 31, 32)]
    words += [[a, b, a], [b, a, b], [a, b, b, a], [a, a, b, b], [a, b, a, a, b], [b] + ab(6), [c] + ab(6) + [c],
              [c] + ab(7) + [c], [a, b, c, a, b, a, b, c, a, b]]
    return _corpus("overlap", words, [rng.randint(1, 3) for _ in words], 4, 30)


def ties():
    """Every pair count equal at creation; groups that differ only in the right id, or only in the left id."""
    words = [[x, y] for x in range(1, 7) for y in range(1, 7)]
    words += [[7, 8, 9, 10], [11, 12, 7, 9], [10, 12, 8, 11], [9, 7, 10, 8]]
    return _corpus("ties", words, [2] * len(words), 13, 30)


HIGH_N_INITIAL = 131000


def highid():
    """Ids on both sides of 65535 | 65536 and at the top: the (kMaxId - a) << 17 | (kMaxId - b) packing, with ties,
    and new ids up to 131070 = the last one vocab_size 131071 allows."""
    rng = random.Random(103)
    ids = list(range(65516, 65556)) + list(range(HIGH_N_INITIAL - 10, HIGH_N_INITIAL))
    words = [[rng.choice(ids) for _ in range(rng.randint(2, 30))] for _ in range(150)]
    counts = [rng.randint(1, 3) for _ in words]
    tie = [[65535, 65536], [65536, 65535], [65535, 65535], [65536, 65536], [65534, 65537], [65537, 65534],
           [HIGH_N_INITIAL - 1, HIGH_N_INITIAL - 1], [HIGH_N_INITIAL - 1, 65536], [65535, HIGH_N_INITIAL - 1],
           [65536, HIGH_N_INITIAL - 2]]
    words += tie
    counts += [200] * len(tie)
    # one word of 63 symbols, all its pairs distinct (and none a tie pair), count 100: once the ten tie pairs are
    # merged every further winner lies in it, so it ends as two symbols, one of them the last id 131070
    z, seen = [rng.choice(ids)], {tuple(t) for t in tie}
    while len(z) < 63:
        x = rng.choice(ids)
        if (z[-1], x) not in seen:
            seen.add((z[-1], x))
            z.append(x)
    words.append(z)
    counts.append(100)
    return _corpus("highid", words, counts, HIGH_N_INITIAL, K_MAX_ID - HIGH_N_INITIAL)


def growth():
    """200 words of 2-200 symbols over 8 letters, 119 merges: the pair set outgrows a table floored at 8 x vocab."""
    rng = random.Random(104)
    words = [[rng.randint(1, 8) for _ in range(rng.randint(2, 200))] for _ in range(200)]
    return _corpus("growth", words, [1] * len(words), 9, 119)


def strided():
    """6-8 k symbols: with grid_blocks 1 or 3 every grid-stride loop goes round many times."""
    rng = random.Random(105)
    words = [[rng.randint(1, 12) for _ in range(rng.randint(50, 200))] for _ in range(56)]
    return _corpus("strided", words, [rng.randint(1, 3) for _ in words], 13, 40)


def zerocount():
    """Words with count 0: their pairs enter the table at 0 and must never win or be read back.  Letters 6 and 7
    occur in such words only."""
    rng = random.Random(106)
    words, counts = [], []
    for i in range(40):
        zero = i % 3 == 0
        words.append([rng.randint(1, 7 if zero else 5) for _ in range(rng.randint(0, 30))])
        counts.append(0 if zero else rng.randint(1, 3))
    return _corpus("zerocount", words, counts, 8, 30)


def lengths(maxlen):
    """max_token_length 2, 3, 4, 5, 9 over three letters: pairs form with lx + ly on both sides of the limit."""
    rng = random.Random(107 + maxlen)
    words = [[rng.randint(1, 3) for _ in range(rng.randint(0, 40))] for _ in range(30)]
    return _corpus(f"lengths{maxlen}", words, [rng.randint(1, 3) for _ in words], 4, 40, maxlen=maxlen)


def degenerate():
    return [_corpus("empty", [], [], 4, 5), _corpus("short", [[], [1], [2], [], [3]], [1, 2, 3, 4, 5], 4, 5),
            _corpus("one_pair", [[1, 2]], [1], 4, 5)]


def all_corpora():
    return ([runs(), overlap(), ties(), highid(), growth(), strided(), zerocount()]
            + [lengths(m) for m in (2, 3, 4, 5, 9)] + degenerate())


def forced_corpus():
    rng = random.Random(108)
    words = [[1, 2, 1, 2, 3, 4], [3, 3, 3, 3, 1, 2, 3, 3], [3, 4, 3, 4, 3], [1, 2, 3, 3, 3, 1, 2], [2, 1, 1, 2],
             [3, 3, 3, 3, 3, 3, 3], [4, 1, 2, 3, 4, 1, 2, 4], [1, 2, 3, 3, 1, 2, 3, 3, 3, 3, 1, 2]]
    for _ in range(20):  # (4, 4) never occurs: the "no_occurrence" schedule merges it
        w = []
        for _ in range(rng.randint(2, 25)):
            w.append(rng.randint(1, 3 if w and w[-1] == 4 else 4))
        words.append(w)
    return _corpus("forced", words, [rng.randint(1, 3) for _ in words], 5, 14, maxlen=6)


def forced_schedules():
    """name -> the merges made before training resumes (ids 1..4 the alphabet, 5.. new)."""
    c = forced_corpus()
    pc = recount(c["words"], c["counts"], {}, c["maxlen"])
    worst = min(pc, key=lambda p: (pc[p], p))
    assert worst != best(pc)[:2]
    return {
        # a pair that is not the best (the one of smallest count), as a new token
        "not_best": [worst + (5, 2)],
        # a pair with no occurrence: only len[5] changes
        "no_occurrence": [(4, 4, 5, 2), (1, 2, 6, 2)],
        # (3, 4) into id 5, which exists and occurs in the corpus: the pairs it forms add to those 5 already has
        "existing_id": [(1, 2, 5, 2), (3, 4, 5, 2)],
        # (3, 3) into the existing id 5, next to 5s that are already there: runs, lpartner with ls = an existing id
        "aa_existing_id": [(1, 2, 5, 2), (3, 3, 5, 2)],
    }
