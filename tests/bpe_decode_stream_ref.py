"""The id stream's contract without a GPU (``mimi_bpe_decode_stream_*``, ``bpe.IdStream``), shared by
``tests/test_bpe_decode_stream_ref.py`` (CPU) and ``tests/test_bpe_decode_stream_gpu.py``: the per-slot state machine
as a plain class, a pool of slots, a fixed-seed schedule of sessions on three slots, and the mistakes that schedule
must catch.

Per slot, with ``K = num_codebooks`` and ``cbs = codebook_size``::

    fresh:  expected = None, owed = 0, pend = []
    for each character (alphabet index idx, cb = idx // cbs) spelled by the slot's new ids, in order:
        if expected is None: expected = cb; owed = (K - cb) % K
        if cb != expected: continue
        expected = (expected + 1) % K
        if owed: owed -= 1; continue
        pend.append(idx - len(pend) * cbs)
        if len(pend) == K: emit pend as one frame; pend = []
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import bpe_decode_cases as cases

MUTANTS = ("drops_pending", "first_every_step", "owed_reapplied", "owed_forgotten", "state_by_item",
           "special_is_character", "pending_in_last_column", "commuted_carry", "reset_keeps_pending")


class SlotRef:
    """One slot: ``feed(ids)`` returns the frames those ids complete, int64 ``[K, T]``.  ``mutant`` names one mistake."""

    def __init__(self, enc, mutant: Optional[str] = None):
        self.enc, self.mutant = enc, mutant
        self.K, self.cbs = enc.num_codebooks, enc.codebook_size
        self.off, self.idx = enc.spellings()
        self.pend: List[int] = []
        self.reset()

    def reset(self):
        self.expected: Optional[int] = None
        self.owed = 0
        self.cb0 = 0
        if self.mutant != "reset_keeps_pending":
            self.pend = []

    @property
    def pending(self) -> int:
        return -1 if self.expected is None else len(self.pend)

    def characters(self, ids) -> List[int]:
        chars: List[int] = []
        for i in np.asarray(ids).reshape(-1).tolist():
            if not 0 <= i < self.enc.n_tokens:
                raise ValueError(f"a token id is outside [0, {self.enc.n_tokens})")
            if self.mutant == "special_is_character" and i < self.enc.n_special:
                chars.append(0)
            chars += self.idx[self.off[i]:self.off[i + 1]].tolist()
        return chars

    def feed(self, ids) -> np.ndarray:
        K, cbs, mutant = self.K, self.cbs, self.mutant
        chars = self.characters(ids)
        frames: List[List[int]] = []
        npend0 = len(self.pend)
        fresh = self.expected is None
        refirst = mutant == "first_every_step" and not fresh
        if mutant == "owed_reapplied" and not fresh:
            self.owed = (K - self.cb0) % K
        at_entry = self.expected  # what a carry composed the wrong way round judges every character of the step by
        for idx in chars:
            cb = idx // cbs
            if self.expected is None:
                self.expected, self.cb0 = cb, cb
                self.owed = (K - cb) % K
            elif refirst:
                self.expected = cb
            refirst = False
            if mutant == "commuted_carry" and not fresh:
                if cb != at_entry:
                    continue
            else:
                if cb != self.expected:
                    continue
                self.expected = (self.expected + 1) % K
            if self.owed:
                self.owed -= 1
                continue
            self.pend.append(idx - len(self.pend) * cbs)
            if len(self.pend) == K:
                frames.append(self.pend)
                self.pend = []
        if mutant == "pending_in_last_column" and frames and npend0:
            first, last = list(frames[0]), list(frames[-1])
            frames[0] = last[:npend0] + first[npend0:]
            frames[-1] = first[:npend0] + last[npend0:]
        if mutant == "drops_pending":
            self.pend = []
        if mutant == "owed_forgotten":
            self.owed = 0
        return np.ascontiguousarray(np.array(frames, np.int64).reshape(-1, K).T)


class PoolRef:
    """``slots`` independent ``SlotRef``: ``step(slots, chunks)`` -> the frames of each item, ``reset(slot)``."""

    def __init__(self, enc, slots: int, mutant: Optional[str] = None):
        self.by_item = mutant == "state_by_item"
        self.slots = [SlotRef(enc, None if self.by_item else mutant) for _ in range(slots)]

    def step(self, slots: Sequence[int], chunks: Sequence[np.ndarray]) -> List[np.ndarray]:
        return [self.slots[i if self.by_item else s].feed(c) for i, (s, c) in enumerate(zip(slots, chunks))]

    def reset(self, slot: int):
        self.slots[slot].reset()

    @property
    def pending(self) -> List[int]:
        return [s.pending for s in self.slots]


def feed_split(slot, ids: np.ndarray, cuts: Sequence[int]) -> np.ndarray:
    """``ids`` fed to ``slot.feed`` in pieces that end at ``cuts`` (and at the end): the frames, end to end."""
    out, a = [], 0
    for b in list(cuts) + [len(ids)]:
        out.append(slot.feed(ids[a:b]))
        a = b
    return np.concatenate(out, axis=1)


def splits(n: int, seed: int = 0) -> Dict[str, List[int]]:
    """The cut points of the three splits every sequence is fed under: 1-id steps, one step, random."""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, max(2, n // 3)))
    return {"one_id": list(range(1, n)), "whole": [],
            "random": sorted(set(rng.integers(0, n + 1, size=k).tolist()) - {n})}


# ---- the schedule --------------------------------------------------------------------------------------------------
SCHED_K, SCHED_CBS, SCHED_SPECIAL, SCHED_SLOTS = 8, 4, 2, 3


def schedule_encoder():
    return cases.hand_encoder(SCHED_K, cbs=SCHED_CBS, n_special=SCHED_SPECIAL, n_merges=24, max_len=40, seed=3, chain=3)


class _Session:
    """Builds one session's chunks; the contract itself tracks which codebook the session expects next."""

    def __init__(self, enc, rng):
        self.enc, self.rng, self.ref = enc, rng, SlotRef(enc)
        self.chunks: List[np.ndarray] = []

    def _add(self, ids):
        ids = np.asarray(ids, np.int32).reshape(-1)
        self.ref.feed(ids)
        self.chunks.append(ids)
        return self

    def _char(self, cb):
        return SCHED_SPECIAL + cb * SCHED_CBS + int(self.rng.integers(SCHED_CBS))

    def clean(self, n, cb=None):  # n characters that cycle from the expected codebook (a fresh session: from cb)
        cb = self.ref.expected if cb is None else cb
        return self._add([self._char((cb + i) % SCHED_K) for i in range(n)])

    def junk(self, n):  # n characters of other codebooks than the expected one: all dropped
        e = self.ref.expected
        return self._add([self._char((e + 1 + int(self.rng.integers(SCHED_K - 1))) % SCHED_K) for _ in range(n)])

    def special(self, n):
        return self._add(self.rng.integers(0, SCHED_SPECIAL, size=n))

    def empty(self):
        return self._add([])

    def merged(self, n):  # n learned ids: spellings of several characters, most of them dropped
        return self._add(self.rng.integers(SCHED_SPECIAL + SCHED_K * SCHED_CBS, self.enc.n_tokens, size=n))


def make_sessions(enc) -> Dict[str, List[np.ndarray]]:
    """name -> the session's chunks of ids, one per step that lists its slot."""
    rng = np.random.default_rng(20260)
    s = {n: _Session(enc, rng) for n in "abcd"}
    # a: first character of codebook 5, so 3 characters are owed and the last of them arrives two steps later; a step
    # of only special ids, an empty one, three steps that wait for one codebook
    s["a"].clean(1, cb=5).clean(1).clean(1 + 16 + 3).special(3).empty().junk(4).junk(3).junk(5).clean(8 + 5) \
          .merged(6).clean(3)
    # b: whole frames from the start, special ids while codebook 0 is expected
    s["b"].clean(24, cb=0).special(2).clean(2).merged(5).clean(6).empty().clean(16).clean(3)
    # c: starts late; its begin drop ends inside its second step; pending codes in front of a step of 3 frames
    s["c"].clean(3, cb=2).clean(3 + 4).clean(4 + 16).junk(2).merged(3).clean(20)
    # d: takes a's slot after the reset
    s["d"].clean(1 + 8 + 8 + 2, cb=7).merged(4).clean(9).special(1)
    return {n: v.chunks for n, v in s.items()}


SLOT_SESSIONS = {0: ["a", "d"], 1: ["c"], 2: ["b"]}  # the sessions of each slot, in order; a reset starts the next
SCHEDULE: Tuple = (
    ("step", (2, 0)), ("step", (0, 2)), ("step", (0,)), ("step", (1, 2, 0)), ("step", (2, 1, 0)), ("step", (0, 1)),
    ("step", (1, 0, 2)), ("step", (0,)), ("step", (0, 2)), ("step", (0, 1)), ("step", (2, 0)),
    ("reset", 0),
    ("step", (1, 0, 2)), ("step", (0,)), ("step", (0,)), ("step", (0,)),
)


def play(sessions: Dict[str, List[np.ndarray]], step: Callable, reset: Callable, each: Optional[Callable] = None):
    """Runs SCHEDULE: ``step(slots, chunks)`` -> one ``[K, T]`` array per item, ``reset(slot)``.  Returns (log, whole):
    log[i] = (slots, sessions, chunks, frames) of step i, whole[name] = the session's frames end to end.  ``each(i,
    slots, frames)`` is called after every step."""
    current = {slot: 0 for slot in SLOT_SESSIONS}
    used = {name: 0 for name in sessions}
    log, parts = [], {name: [] for name in sessions}
    for op in SCHEDULE:
        if op[0] == "reset":
            reset(op[1])
            current[op[1]] += 1
            continue
        slots = list(op[1])
        names = [SLOT_SESSIONS[s][current[s]] for s in slots]
        chunks = [sessions[n][used[n]] for n in names]
        frames = [np.asarray(f, np.int64) for f in step(slots, chunks)]
        for n, f in zip(names, frames):
            used[n] += 1
            parts[n].append(f)
        log.append((slots, names, chunks, frames))
        if each is not None:
            each(len(log) - 1, slots, frames)
    assert all(used[n] == len(sessions[n]) for n in sessions), used  # the schedule feeds every chunk
    return log, {n: np.concatenate(p, axis=1) for n, p in parts.items()}


def session_ids(sessions, name) -> np.ndarray:
    return np.concatenate(sessions[name]).astype(np.int32)


def pad_ids(chunks: Sequence[np.ndarray], fill: int = 0, width: Optional[int] = None) -> Tuple[np.ndarray, List[int]]:
    """Chunks -> (int32 ``[m, L]`` padded with ``fill``, counts)."""
    counts = [int(len(c)) for c in chunks]
    L = max(counts + [1]) if width is None else width
    ids = np.full((len(chunks), L), fill, np.int32)
    for i, c in enumerate(chunks):
        ids[i, :len(c)] = c
    return ids, counts


def frame_chain_encoder(K: int = 8, cbs: int = 4, n_special: int = 2, doublings: int = 3):
    """A model with one id that spells whole frames: merges join the characters (0, 0), (1, 0) .. (K - 1, 0) (K a power
    of two) into one token, then ``doublings`` merges double it.  Returns (encoder, that id): it spells ``K *
    2^doublings`` characters that cycle through the codebooks from 0."""
    from mimi_hip import bpe
    level = [n_special + k * cbs for k in range(K)]
    nxt, tri = n_special + K * cbs, []
    while len(level) > 1:
        pairs = []
        for a, b in zip(level[0::2], level[1::2]):
            tri.append((a, b, nxt))
            pairs.append(nxt)
            nxt += 1
        level = pairs
    last = level[0]
    for _ in range(doublings):
        tri.append((last, last, nxt))
        last, nxt = nxt, nxt + 1
    return bpe.Encoder(K, cbs, tri, nxt, n_special, unicode_offset=cases.OFFSET), last


def cycling_ids(enc, rng, chars, phase):
    """Ids that spell exactly `chars` characters cycling through the codebooks from `phase` (all of them kept): learned
    ids whose spelling cycles where one fits (two times in three), alphabet ids otherwise."""
    K, cbs = enc.num_codebooks, enc.codebook_size
    off, idx = enc.spellings()
    by_start = {k: [] for k in range(K)}
    for i in range(enc.n_special + K * cbs, enc.n_tokens):
        cb = idx[off[i]:off[i + 1]] // cbs
        if cb.size > 1 and np.array_equal(cb, (cb[0] + np.arange(cb.size)) % K):
            by_start[int(cb[0])].append((i, int(cb.size)))
    ids, e, left = [], phase, chars
    while left:
        fits = [t for t in by_start[e] if t[1] <= left]
        i, n = fits[int(rng.integers(len(fits)))] if fits and rng.random() < 2 / 3 else (enc.n_special + e * cbs + int(rng.integers(cbs)), 1)
        ids.append(i)
        e, left = (e + n) % K, left - n
    return np.array(ids, np.int32)
