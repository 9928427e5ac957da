"""Test infrastructure only (CPU): ONE schedule of stream steps at serving scale -- ``m`` sessions on ``m`` slots, 128 and
129 of them on the GPU -- shared by both directions, by the CPU test (tests/test_stream_scale_ref.py, at ``m`` = 17) and by
the GPU tests (tests/test_decode_stream_scale_gpu.py, tests/test_encode_stream_scale_gpu.py).

The schedule is a pure function of ``m``, in the form ``stream_ragged_ref.play`` / ``play_encode`` run
(``("step", [(slot, session, frames), ...], nmax)`` / ``("reset", slot)``):

* session ``i`` (``0 <= i < m``) lives in slot ``(37 i) mod m``.  37 is coprime to 17, 128 and 129, so this is a
  permutation; it still has fixed points beyond 0 (``36 i = 0 mod m``: i = 32, 64, 96 at 128, i = 43, 86 at 129), which
  is why the steps list their items in an order of their own: what must differ is an item's PLACE in the step and its
  slot, and ``check`` asserts that it does for every item of the big step but at most one.
* warm-up: two ragged steps bring slot ``s`` to position ``(3 s) mod 11`` frames (0 .. 10: fresh, mid-ring and -- against
  the ring's ``cap = 4 + 2 * 7 = 18`` rows at ``sliding_window`` = 5 -- wrapped), the first with ``min(position, 7)``
  frames, the second with the rest (1 .. 3);
* the big step: every slot, session ``i`` with ``1 + (5 i mod 7)`` frames, item ``j`` being session ``(13 j + 16) mod m``:
  511 frames = 1022 flat rows at ``m`` = 128, 515 frames = 1030 rows at ``m`` = 129 -- the two sides of the fp32 GEMM's
  tile boundary (``M > 1024``).  No two neighbouring items stand at the same position;
* the slots of the big step's first, middle and last item are reset and three new sessions (``m``, ``m + 1``,
  ``m + 2``) start there;
* the final step: every slot again, in descending slot order.

``ScalePool`` is the pool the mutants live in; without a mutant it is ``stream_ragged_ref.RaggedPool`` /
``EncRaggedPool`` bit for bit, which tests/test_stream_scale_ref.py asserts and which are the pools held to the whole
sequence there.  ``ScaleMutant`` switches on, one at a time, the mistakes a table indexed by the wrong thing makes at
item 8 or 100 and not at item 2; tests/test_stream_scale_ref.py shows that the schedule tells each of them from the
right answer.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

import decode_stream_ref as dstr
from oracle.mimi_ref import RefConfig

FRAME = 1920
K, WINDOW, MAX_STEP_FRAMES = 8, 5, 7
SLOT_MUL, ORDER_MUL, ORDER_ADD = 37, 13, 16
M_CPU, M_GPU = 17, (128, 129)
MIN_FRAMES, MAX_FRAMES = 4, 18
CODE_SEED, AUDIO_SEED = 900, 31


def slot_of(i: int, m: int) -> int:
    return (SLOT_MUL * i) % m


def warm_position(slot: int) -> int:
    return (3 * slot) % 11


def big_count(i: int) -> int:
    return 1 + (5 * i) % 7


def big_order(m: int) -> List[int]:
    """The sessions of the big step in the order it lists them."""
    return [(ORDER_MUL * j + ORDER_ADD) % m for j in range(m)]


def reset_sessions(m: int) -> List[int]:
    """The sessions that end with the big step: its first, middle and last item."""
    order = big_order(m)
    return [order[0], order[m // 2], order[m - 1]]


def final_count(i: int, m: int) -> int:
    """What session ``i`` brings to the final step: 1 + (3 i mod 7), moved so that the session has 4 .. 18 frames."""
    if i >= m:  # a session opened on a reset slot: the final step is all of it
        return MIN_FRAMES + (i - m)
    if i in reset_sessions(m):
        return 0
    before = warm_position(slot_of(i, m)) + big_count(i)
    return min(max(1 + (3 * i) % 7, MIN_FRAMES - before), MAX_FRAMES - before)


def session_frames(m: int) -> Dict[int, int]:
    out = {i: warm_position(slot_of(i, m)) + big_count(i) + final_count(i, m) for i in range(m)}
    out.update({m + k: final_count(m + k, m) for k in range(3)})
    return out


def schedule(m: int):
    ops = []
    warm = {i: warm_position(slot_of(i, m)) for i in range(m)}
    first = [(slot_of(i, m), i, min(w, MAX_STEP_FRAMES)) for i, w in warm.items() if w > 0]
    ops.append(("step", first, MAX_STEP_FRAMES))
    rest = [(slot_of(i, m), i, w - MAX_STEP_FRAMES) for i, w in reversed(list(warm.items())) if w > MAX_STEP_FRAMES]
    ops.append(("step", rest, max(f for _, _, f in rest)))
    ops.append(("step", [(slot_of(i, m), i, big_count(i)) for i in big_order(m)], MAX_STEP_FRAMES))
    owner = {slot_of(i, m): i for i in range(m)}
    for k, i in enumerate(reset_sessions(m)):
        ops.append(("reset", slot_of(i, m)))
        owner[slot_of(i, m)] = m + k
    last = [(s, owner[s], final_count(owner[s], m)) for s in sorted(owner, reverse=True)]
    ops.append(("step", last, max(f for _, _, f in last)))
    return ops


BIG = 2  # the big step's index in schedule(m)


def splits(m: int) -> Dict[int, List[int]]:
    """session -> the steps the schedule cuts it into."""
    out: Dict[int, List[int]] = {}
    for op in schedule(m):
        if op[0] == "step":
            for _, name, f in op[1]:
                out.setdefault(name, []).append(f)
    return out


def flat_rows(m: int):
    """[(first flat row, rows)] of the big step's items: 2 rows per frame, packed in the order listed."""
    out, at = [], 0
    for _, _, f in schedule(m)[BIG][1]:
        out.append((at, 2 * f))
        at += 2 * f
    return out


def items_at_row(m: int, row: int) -> List[int]:
    """The items of the big step that hold flat rows ``row - 1`` and ``row`` (one item, or the two that meet there); the
    last two items if the step ends before ``row``."""
    rows = flat_rows(m)
    hit = [j for j, (lo, n) in enumerate(rows) if lo <= row - 1 < lo + n or lo <= row < lo + n]
    return hit if hit else [m - 2, m - 1]


def tap_items(m: int) -> List[int]:
    """The four items whose packed taps the GPU tests compare at m = 129: the first, the last, and the two that meet at
    flat row 1024."""
    around = items_at_row(m, 1024)
    assert len(around) == 2 and around[1] < m - 1, around
    return [0, *around, m - 1]


def value_sample(m: int) -> List[int]:
    """The 8 sessions held to the CPU reference: those of the big step's first and last item, of the items at flat rows
    63 / 64 and 1023 / 1024 (the last two items where the step is shorter), of the middle item (it ends there and its
    slot is reset) and the new session on the first item's slot; filled up from the step's items 8, 9, ... ."""
    sched = schedule(m)
    items = [name for _, name, _ in sched[BIG][1]]
    want = [items[0], items[m - 1]] + [items[j] for j in items_at_row(m, 64) + items_at_row(m, 1024)]
    want += [items[m // 2], m]
    out = list(dict.fromkeys(want))
    for j in range(8, m):
        if len(out) >= 8:
            break
        if items[j] not in out:
            out.append(items[j])
    return out[:8]


def make_sessions(m: int) -> Dict[int, torch.Tensor]:
    """session -> codes [1, K, T]."""
    return {i: torch.from_numpy(np.random.default_rng(CODE_SEED + i).integers(0, 2048, (1, K, T)))
            for i, T in session_frames(m).items()}


def make_clips(m: int) -> Dict[int, torch.Tensor]:
    """session -> audio [1, 1, 1920 T], each cut from its own speech-like clip."""
    from mimi_hip import synthetic
    return {i: torch.from_numpy(synthetic.speech_like(FRAME * T, AUDIO_SEED, i))[None, None]
            for i, T in session_frames(m).items()}


def check(m: int):
    """What the schedule promises, asserted; returns (frames of the big step, its items that sit on their own index)."""
    sched = schedule(m)
    assert [op[0] for op in sched] == ["step", "step", "step", "reset", "reset", "reset", "step"]
    assert sorted(slot_of(i, m) for i in range(m)) == list(range(m))
    pos = [0] * m
    for op in sched[:BIG]:
        items = op[1]
        assert len({f for _, _, f in items}) > 1 and all(1 <= f <= op[2] <= MAX_STEP_FRAMES for _, _, f in items)
        for s, _, f in items:
            pos[s] += f
    assert pos == [warm_position(s) for s in range(m)]
    cap = WINDOW - 1 + 2 * MAX_STEP_FRAMES
    assert any(p == 0 for p in pos) and any(0 < 2 * p < cap for p in pos) and any(2 * p > cap for p in pos)
    big = sched[BIG][1]
    slots, names, counts = [s for s, _, _ in big], [n for _, n, _ in big], [f for _, _, f in big]
    assert sorted(slots) == list(range(m)) and slots != sorted(slots) and names != sorted(names)
    assert counts == [big_count(i) for i in names] and set(counts) == set(range(1, 8))
    own = [j for j, s in enumerate(slots) if s == j]
    assert len(own) <= 1, own  # an item's place in the step is not its slot (none at 128 and 129, item 5 at 17)
    assert all(pos[a] != pos[b] for a, b in zip(slots, slots[1:]))  # no two neighbours at the same position
    frames = session_frames(m)
    assert all(MIN_FRAMES <= T <= MAX_FRAMES for T in frames.values()), frames
    assert {n: sum(v) for n, v in splits(m).items()} == frames
    last = sched[-1][1]
    assert sorted(s for s, _, _ in last) == list(range(m)) and len({f for _, _, f in last}) > 1
    assert {sched[3][1], sched[4][1], sched[5][1]} == {slots[0], slots[m // 2], slots[m - 1]}
    return sum(counts), own


# ---- the pool and the mistakes it must tell apart --------------------------------------------------------------------
@dataclass(frozen=True)
class ScaleMutant:
    state_by_item: bool = False        # item i works on slot i's rings and carries, not on slots[i]'s
    position_from_8_back: bool = False  # the position of item i >= 8 is read from item i - 8's slot (a table of 8)
    rope_of_previous_item: bool = False  # item i >= 1 is rotated with the RoPE rows of the item listed before it
    reset_keeps_position: bool = False  # reset(slot) zeroes the slot's carries but not its position: the position is what
    #                                     says how much of the ring is valid, so the old session's keys stay in view
    #                                     (RoPE is relative: on an empty cache a kept position alone changes nothing)


class ScalePool:
    """``m`` ``batch = 1`` reference streams (``decode_stream_ref.StreamState`` or ``encode_stream_ref.StreamState``) as
    the slots of one stream: a ragged step feeds slot ``slots[i]`` the first ``frames[i]`` frames of item ``i``.  The
    statement of the contract, with the mutants above; not a second implementation."""

    def __init__(self, states, run: Callable, in_unit: int, mutant: Optional[ScaleMutant] = None):
        self.states, self.run, self.in_unit = states, run, in_unit
        self.mut = mutant or ScaleMutant()
        self.told = [0] * len(states)  # what the pool reports: a mutant's states may stand elsewhere

    @property
    def positions(self) -> List[int]:
        return list(self.told)

    def reset(self, slot: int):
        st = self.states[slot]
        keep = (st.position, st.k, st.v)
        st.reset()
        if self.mut.reset_keeps_position:
            st.position, st.k, st.v = keep
        self.told[slot] = 0

    def step_ragged(self, slots: Sequence[int], x, frames: Sequence[int]) -> torch.Tensor:
        """x [m, ., unit nmax] padded -> [m, ., out_unit nmax], zero past item i's frames[i]."""
        slots, frames = list(slots), [int(f) for f in frames]
        x = torch.as_tensor(x)
        m, nmax = x.shape[0], x.shape[-1] // self.in_unit
        assert len(slots) == len(frames) == m and len(set(slots)) == m and all(1 <= f <= nmax for f in frames)
        before = [self.states[s].position for s in slots]
        out = None
        for i, (s, f) in enumerate(zip(slots, frames)):
            st = self.states[s]
            src = self.states[i] if self.mut.state_by_item else st
            own = (st.k, st.v, st.carry)
            st.k, st.v, st.carry = src.k, src.v, src.carry
            # (the mask and the cache see differences of positions only: moving `position` moves the rotation alone)
            if self.mut.position_from_8_back and i >= 8:
                st.position = before[i - 8]
            if self.mut.rope_of_previous_item and i >= 1:
                st.position = before[i - 1]
            y = self.run(st, x[i:i + 1, ..., :self.in_unit * f])
            worked = (st.k, st.v, st.carry)
            st.k, st.v, st.carry = own
            src.k, src.v, src.carry = worked
            st.position = before[i] + f
            self.told[s] += f
            unit = y.shape[-1] // f
            if out is None:
                out = torch.zeros(m, y.shape[1], unit * nmax, dtype=y.dtype)
            out[i, :, :unit * f] = y[0]
        return out


def decode_pool(sd, m: int, cfg: RefConfig, mutant: Optional[ScaleMutant] = None) -> ScalePool:
    return ScalePool([dstr.StreamState(sd, 1, cfg) for _ in range(m)], lambda st, c: st.step(c), 1, mutant)


def encode_pool(sd, m: int, cfg: RefConfig, mutant: Optional[ScaleMutant] = None) -> ScalePool:
    """The pre-quantizer embedding [m, 512, nmax] (the codes quantise it and can hide a small error)."""
    import encode_stream_ref as esr
    sdt = esr.as_tensors(sd)
    return ScalePool([esr.StreamState(sdt, 1, cfg) for _ in range(m)], lambda st, a: st.embed(a), FRAME, mutant)
