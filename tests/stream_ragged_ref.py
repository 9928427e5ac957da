"""Test infrastructure only (CPU): a ragged step of a decode stream -- every listed slot advances by its own number of
frames -- stated on ``decode_stream_ref.StreamState`` (and, at the end of the file, of an encode stream, on
``encode_stream_ref.StreamState``).

The contract of ``mimi_decode_stream_step_ragged`` / ``DecodeStream.step(codes, slots=..., frames=...)`` in one
sentence: slot ``s`` IS a ``batch = 1`` stream, and a step that lists it with ``frames[i]`` feeds that stream the first
``frames[i]`` columns of its padded item -- whatever the other slots bring.  ``RaggedPool`` says exactly that on
``decode_stream_slots_ref.SlotPool``'s states.  It is not a second implementation.

``RaggedMutant`` switches on, one at a time, the mistakes a packed layout invites; tests/test_stream_ragged_ref.py
shows that the schedule the GPU test runs tells each of them from the right answer by a wide factor.

``SCHEDULE`` / ``play`` are that schedule and the loop that runs it, shared by the CPU and the GPU test: the sessions of
tests/decode_stream_slots_ref.py (same codes, same totals) cut into calls that mix counts over 1, 2, 3 and 7.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

import decode_stream_slots_ref as slots_ref
from oracle.mimi_ref import RefConfig

FRAME = 1920


@dataclass(frozen=True)
class RaggedMutant:
    reads_padding: bool = False     # every item consumes nmax frames: its padding goes through the state
    advance_by_nmax: bool = False   # position (RoPE, mask) and with it the cache advance by nmax, not by frames[i]
    carry_at_longest: bool = False  # carry-out is taken where the longest item ends: a shorter item's own last rows
    #                                 never reach its state (modelled: its carries keep the rows from before the step)
    uniform_base: bool = False      # item i's chunk is read at the uniform stride i * nmax of the packed frames


class RaggedPool(slots_ref.SlotPool):
    def __init__(self, sd, batch: int, cfg: Optional[RefConfig] = None, mutant: Optional[RaggedMutant] = None):
        super().__init__(sd, batch, cfg)
        self.rmut = mutant or RaggedMutant()
        self.told = [0] * batch  # what the pool reports: a mutant's states may stand elsewhere

    @property
    def positions(self) -> List[int]:
        return list(self.told)

    def reset(self, slot: int):
        super().reset(slot)
        self.told[slot] = 0

    def step_ragged(self, slots: Sequence[int], codes, frames: Sequence[int]) -> torch.Tensor:
        """codes [m, K, nmax] padded, item i the next frames[i] frames of slot slots[i] -> [m, 1, 1920 nmax], zero past
        1920 frames[i]."""
        slots, frames = list(slots), [int(f) for f in frames]
        codes = torch.as_tensor(codes)
        m, nmax = codes.shape[0], codes.shape[2]
        assert len(slots) == len(frames) == m and len(set(slots)) == m and all(1 <= f <= nmax for f in frames)
        packed = torch.cat([codes[i, :, :f] for i, f in enumerate(frames)], dim=-1)  # [K, sum]
        packed = torch.cat([packed, torch.zeros(codes.shape[1], m * nmax, dtype=packed.dtype)], dim=-1)
        out = torch.zeros(m, 1, FRAME * nmax)
        for i, (s, f) in enumerate(zip(slots, frames)):
            st = self.states[s]
            own = st.position
            item = codes[i:i + 1, :, :f]
            if self.rmut.uniform_base:
                item = packed[None, :, i * nmax:i * nmax + f]
            if self.rmut.reads_padding:
                item = codes[i:i + 1]
            before = {k: v.clone() for k, v in st.carry.items()}
            y = st.step(item)
            if self.rmut.carry_at_longest and f < nmax:
                st.carry = before
            st.position = own + (nmax if self.rmut.advance_by_nmax else f)
            self.told[s] += f
            out[i, :, :FRAME * f] = y[0, :, :FRAME * f]
        return out


# ---- the schedule ----------------------------------------------------------------------------------------------------
BATCH, MAX_STEP_FRAMES, K, WINDOW = slots_ref.BATCH, slots_ref.MAX_STEP_FRAMES, slots_ref.K, slots_ref.WINDOW
SESSION_FRAMES = slots_ref.SESSION_FRAMES
# ("step", [(slot, session, frames), ...], nmax) in the order the call lists them, or ("reset", slot).  Counts mix over
# 1, 2, 3 and 7; call 2 pads beyond its longest item; call 3 puts a fresh slot with 1 frame (a 2-row chunk, shorter than
# decoder.layers.0's 6-row carry) beside a mid-way slot with 7; call 4 has equal counts (the slot step itself); A ends,
# its slot is reset and D starts on it while C is mid-way.  Slot 2 is never used.
SCHEDULE = [
    ("step", [(0, "A", 2)], 2),
    ("step", [(1, "B", 3), (0, "A", 1)], 4),
    ("step", [(3, "C", 1), (1, "B", 7)], 7),
    ("step", [(0, "A", 2), (3, "C", 2), (1, "B", 2)], 2),
    ("step", [(3, "C", 7), (0, "A", 3), (1, "B", 1)], 7),
    ("step", [(0, "A", 1)], 1),
    ("reset", 0),
    ("step", [(3, "C", 1), (0, "D", 2)], 2),
    ("step", [(0, "D", 7)], 7),
    ("step", [(0, "D", 1)], 1),
]


def make_sessions():
    return slots_ref.make_sessions()


def splits(schedule=SCHEDULE) -> Dict[str, List[int]]:
    """name -> the steps the schedule cuts that session into."""
    out: Dict[str, List[int]] = {}
    for op in schedule:
        if op[0] == "step":
            for _, name, f in op[1]:
                out.setdefault(name, []).append(f)
    return out


def play(sessions: Dict[str, torch.Tensor], step: Callable, reset: Callable, positions: Callable, schedule=SCHEDULE,
         batch: int = BATCH, pad_seed: int = 77) -> Dict[str, torch.Tensor]:
    """Run the schedule through ``step(slots, codes[m, K, nmax], frames) -> [m, 1, 1920 nmax]``, ``reset(slot)`` and
    ``positions() -> [batch]``.  The padding of every item holds random valid codes that belong to nobody; the
    positions are checked after every call.  name -> that session's samples."""
    rng = np.random.default_rng(pad_seed)
    at = {name: 0 for name in sessions}
    want_pos = [0] * batch
    parts: Dict[str, List[torch.Tensor]] = {name: [] for name in sessions}
    for op in schedule:
        if op[0] == "reset":
            reset(op[1])
            want_pos[op[1]] = 0
        else:
            _, items, nmax = op
            codes = torch.from_numpy(rng.integers(0, 2048, (len(items), K, nmax)))
            for i, (_, name, f) in enumerate(items):
                codes[i, :, :f] = sessions[name][0, :, at[name]:at[name] + f]
            y = step([s for s, _, _ in items], codes, [f for _, _, f in items])
            assert tuple(y.shape) == (len(items), 1, FRAME * nmax), (op, tuple(y.shape))
            for i, (s, name, f) in enumerate(items):
                parts[name].append(y[i:i + 1, :, :FRAME * f].cpu())
                at[name] += f
                want_pos[s] += f
        assert list(positions()) == want_pos, (op, list(positions()), want_pos)
    assert all(at[name] == sessions[name].shape[2] for name in sessions), at
    return {name: torch.cat(v, dim=-1) for name, v in parts.items()}


# ---- the encode direction ---------------------------------------------------------------------------------------------
# The same sentence for ``mimi_encode_stream_step_ragged`` / ``EncodeStream.step(audio, slots=..., frames=...)`` on
# ``encode_stream_ref.SlotPool``'s ``batch = 1`` states: slot s is fed the first ``1920 frames[i]`` samples of its padded
# item.  The schedule is SCHEDULE on the clips of tests/encode_stream_ref.py (same names, same totals).
@dataclass(frozen=True)
class EncRaggedMutant:
    reads_padding: bool = False      # every item consumes nmax frames: its padding goes through the state
    advance_by_nmax: bool = False    # position (RoPE, mask, cache) advances by nmax, not by frames[i]
    carry_at_longest: bool = False   # a shorter item's own last rows never reach its state (its carries keep the old rows)
    uniform_base: bool = False       # item i's chunk is read at the uniform stride i * nmax of the packed frames
    fill_from_first_item: bool = False  # a fresh slot that is not the step's first item gets no replicate fill of its
    #                                     own: its downsample carry is the first item's rows


class EncRaggedPool:
    def __init__(self, sd, batch: int, cfg: Optional[RefConfig] = None, mutant: Optional[EncRaggedMutant] = None):
        import encode_stream_ref as esr
        self.pool = esr.SlotPool(sd, batch, cfg)
        self.states, self.batch = self.pool.states, batch
        self.rmut = mutant or EncRaggedMutant()
        self.told = [0] * batch

    @property
    def positions(self) -> List[int]:
        return list(self.told)

    def reset(self, slot: int):
        self.pool.reset(slot)
        self.told[slot] = 0

    def embed_ragged(self, slots: Sequence[int], audio, frames: Sequence[int]) -> torch.Tensor:
        """audio [m, 1, 1920 nmax] padded -> the pre-quantizer embedding [m, 512, nmax], zero past frames[i]."""
        slots, frames = list(slots), [int(f) for f in frames]
        audio = torch.as_tensor(audio)
        m, nmax = audio.shape[0], audio.shape[-1] // FRAME
        assert len(slots) == len(frames) == m and len(set(slots)) == m and all(1 <= f <= nmax for f in frames)
        packed = torch.cat([audio[i, :, :FRAME * f] for i, f in enumerate(frames)], dim=-1)
        packed = torch.cat([packed, torch.zeros(1, FRAME * m * nmax)], dim=-1)
        out = None
        for i, (s, f) in enumerate(zip(slots, frames)):
            st = self.states[s]
            own = st.position
            item = audio[i:i + 1, :, :FRAME * f]
            if self.rmut.uniform_base:
                item = packed[None, :, FRAME * i * nmax:FRAME * (i * nmax + f)]
            if self.rmut.reads_padding:
                item = audio[i:i + 1]
            before = {k: v.clone() for k, v in st.carry.items()}
            if self.rmut.fill_from_first_item and i > 0 and own == 0:
                st.carry["ds"] = self.states[slots[0]].carry["ds"].clone()
                st.ds_stale = True
            e = st.embed(item)
            if self.rmut.carry_at_longest and f < nmax:
                st.carry = before
            st.position = own + (nmax if self.rmut.advance_by_nmax else f)
            self.told[s] += f
            if out is None:
                out = torch.zeros(m, e.shape[1], nmax)
            out[i, :, :f] = e[0, :, :f]
        return out


def play_encode(sessions: Dict[str, torch.Tensor], step: Callable, reset: Callable, positions: Callable,
                schedule=SCHEDULE, batch: int = BATCH, pad=float("nan")) -> Dict[str, torch.Tensor]:
    """Run the schedule through ``step(slots, audio[m, 1, 1920 nmax], frames) -> [m, X, nmax]``; sessions: name -> audio
    [1, 1, 1920 T].  Every item's padding holds ``pad``.  name -> that session's concatenated output [1, X, T]."""
    at = {name: 0 for name in sessions}
    want_pos = [0] * batch
    parts: Dict[str, List[torch.Tensor]] = {name: [] for name in sessions}
    for op in schedule:
        if op[0] == "reset":
            reset(op[1])
            want_pos[op[1]] = 0
        else:
            _, items, nmax = op
            audio = torch.full((len(items), 1, FRAME * nmax), pad, dtype=torch.float32)
            for i, (_, name, f) in enumerate(items):
                audio[i, :, :FRAME * f] = sessions[name][0, :, FRAME * at[name]:FRAME * (at[name] + f)]
            y = step([s for s, _, _ in items], audio, [f for _, _, f in items])
            assert y.shape[0] == len(items) and y.shape[-1] == nmax, (op, tuple(y.shape))
            for i, (s, name, f) in enumerate(items):
                parts[name].append(y[i:i + 1, :, :f].cpu())
                at[name] += f
                want_pos[s] += f
        assert list(positions()) == want_pos, (op, list(positions()), want_pos)
    assert all(FRAME * at[name] == sessions[name].shape[-1] for name in sessions), at
    return {name: torch.cat(v, dim=-1) for name, v in parts.items()}
