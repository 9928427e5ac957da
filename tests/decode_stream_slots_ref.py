"""Test infrastructure only (CPU): a decode stream as a pool of SLOTS, stated on ``decode_stream_ref.StreamState``.

The contract of ``mimi_decode_stream_step_slots`` / ``DecodeStream.step(codes, slots=...)`` in one sentence: slot ``s``
IS a ``batch = 1`` stream, and a step that lists it feeds that stream its item -- whatever the other slots are, where
they stand, in which order the step lists them.  ``SlotPool`` says exactly that: one ``StreamState(batch=1)`` per slot,
``step(slots, codes)`` steps the listed ones, ``reset(slot)`` makes one fresh.  It is not a second implementation.

``SlotMutant`` switches on, one at a time, the mistakes the engine's plumbing invites (a table indexed by the wrong
thing); tests/test_decode_stream_slots_ref.py shows that the schedule the GPU test runs tells each of them from the
right answer by >= 10 x the tolerance.

``SCHEDULE`` / ``play`` are that schedule and the loop that runs it, shared by the CPU and the GPU test: four sessions
of different lengths that start and end at different times on a pool of four slots, one of which is never used.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

import decode_stream_ref as dstr
from oracle.mimi_ref import RefConfig


@dataclass(frozen=True)
class SlotMutant:
    rope_from_first: bool = False    # every listed item is rotated with the first listed slot's position
    ring_by_item: bool = False       # the k / v cache is addressed by the item's place in the step, not by its slot
    carry_by_item: bool = False      # the same for the carries
    reset_keeps_carry: bool = False  # reset(slot) zeroes the position (and so empties the cache) but not the carries


class SlotPool:
    def __init__(self, sd, batch: int, cfg: Optional[RefConfig] = None, mutant: Optional[SlotMutant] = None):
        self.batch = batch
        self.mut = mutant or SlotMutant()
        self.states = [dstr.StreamState(sd, 1, cfg) for _ in range(batch)]

    @property
    def positions(self) -> List[int]:
        return [st.position for st in self.states]

    def reset(self, slot: int):
        assert 0 <= slot < self.batch
        st = self.states[slot]
        if self.mut.reset_keeps_carry:
            st.position = 0
            st.k = [None] * len(st.k)
            st.v = [None] * len(st.v)
        else:
            st.reset()

    def step(self, slots: Sequence[int], codes) -> torch.Tensor:
        """codes [m, K, n], item i the next n frames of slot slots[i] -> [m, 1, 1920 n]."""
        slots = list(slots)
        codes = torch.as_tensor(codes)
        assert 1 <= len(slots) <= self.batch and len(set(slots)) == len(slots), slots
        assert all(0 <= s < self.batch for s in slots) and codes.shape[0] == len(slots), (slots, tuple(codes.shape))
        n = codes.shape[2]
        first = self.states[slots[0]].position
        out = []
        for i, s in enumerate(slots):
            st = self.states[s]
            # the mutants: whose cache / carries item i works on, and the position its rows are rotated with (the
            # mask and the cache only see differences of positions, so moving `position` moves the rotation alone)
            ring = self.states[i] if self.mut.ring_by_item else st
            car = self.states[i] if self.mut.carry_by_item else st
            own = (st.k, st.v, st.carry, st.position)
            st.k, st.v, st.carry = ring.k, ring.v, car.carry
            if self.mut.rope_from_first:
                st.position = first
            out.append(st.step(codes[i:i + 1]))
            worked = (st.k, st.v, st.carry)
            st.k, st.v, st.carry = own[:3]
            ring.k, ring.v = worked[:2]
            car.carry = worked[2]
            st.position = own[3] + n
        return torch.cat(out, dim=0)


# ---- the schedule ----------------------------------------------------------------------------------------------------
BATCH, MAX_STEP_FRAMES, K, WINDOW = 4, 7, 8, 5
SESSION_FRAMES = {"A": 9, "B": 13, "C": 11, "D": 10}
# ("step", [(slot, session), ...], n) in the order the call lists them, or ("reset", slot).  A starts alone; B joins at
# call 2; C joins at call 3 on slot 3 (slot 2 is never used); A ends after call 4, its slot is reset and D starts on it
# while B and C are mid-way.  1 to 3 slots per call, ascending and permuted; n over 1, 2, 3, 7; from call 2 on every
# call with more than one slot mixes positions.
SCHEDULE = [
    ("step", [(0, "A")], 2),
    ("step", [(0, "A")], 1),
    ("step", [(1, "B"), (0, "A")], 3),
    ("step", [(3, "C"), (0, "A"), (1, "B")], 1),
    ("step", [(0, "A"), (3, "C")], 2),
    ("reset", 0),
    ("step", [(0, "D"), (1, "B"), (3, "C")], 1),
    ("step", [(3, "C"), (0, "D")], 2),
    ("step", [(1, "B"), (0, "D")], 7),
    ("step", [(3, "C"), (1, "B")], 1),
    ("step", [(3, "C")], 3),
    ("step", [(3, "C")], 1),
]


def make_sessions(seed: int = 400) -> Dict[str, torch.Tensor]:
    """name -> codes [1, K, T]: different random codes, different lengths."""
    return {name: torch.from_numpy(np.random.default_rng(seed + i).integers(0, 2048, (1, K, T)))
            for i, (name, T) in enumerate(SESSION_FRAMES.items())}


def splits(schedule=SCHEDULE) -> Dict[str, List[int]]:
    """name -> the steps the schedule cuts that session into."""
    out: Dict[str, List[int]] = {}
    for op in schedule:
        if op[0] == "step":
            for _, name in op[1]:
                out.setdefault(name, []).append(op[2])
    return out


def play(sessions: Dict[str, torch.Tensor], step: Callable, reset: Callable, positions: Callable,
         schedule=SCHEDULE, batch: int = BATCH) -> Dict[str, torch.Tensor]:
    """Run the schedule through ``step(slots, codes[m, K, n]) -> [m, 1, 1920 n]``, ``reset(slot)`` and
    ``positions() -> [batch]``; the positions are checked after every call.  name -> that session's samples."""
    at = {name: 0 for name in sessions}
    want_pos = [0] * batch
    parts: Dict[str, List[torch.Tensor]] = {name: [] for name in sessions}
    for op in schedule:
        if op[0] == "reset":
            reset(op[1])
            want_pos[op[1]] = 0
        else:
            _, items, n = op
            codes = torch.cat([sessions[name][:, :, at[name]:at[name] + n] for _, name in items])
            assert codes.shape[2] == n, (op, tuple(codes.shape))
            y = step([s for s, _ in items], codes)
            assert tuple(y.shape) == (len(items), 1, 1920 * n), (op, tuple(y.shape))
            for i, (s, name) in enumerate(items):
                parts[name].append(y[i:i + 1].cpu())
                at[name] += n
                want_pos[s] += n
        assert list(positions()) == want_pos, (op, list(positions()), want_pos)
    assert all(at[name] == sessions[name].shape[2] for name in sessions), at
    return {name: torch.cat(v, dim=-1) for name, v in parts.items()}
