"""Test infrastructure only (CPU): the DECODER transformer one stage at a time in float64, on the stage table of
tests/encode_stage_ref.py (imported, not copied: ``transformer_stages``, its values and derived condition sums).

Decode differs from encode in three things, and only those are stated here:
  * the weights: ``decoder_transformer.*``, read through ``encode_stage_ref.decoder_view`` (the renaming view of
    ``decode_ref.decoder_transformer``);
  * layer 0 reads the ``upsample`` tap;
  * the sliding window is the engine's configuration (the tests build engines at window 70 so that a window's edge, the
    stream ring's wrap and eviction fall inside a 40-frame sequence), passed in as an argument.
The arithmetic is fp32 throughout (``Arith("f32")``, c = 0); the two conditions are decode's
(``decode_stage_ref.failures``): HARD q <= n, WORKING q <= 16 max(q_ref, 1), q_ref torch-CPU fp32 on the same input.

HOW EACH DECODE FORM MAPS ONTO THE WHOLE-SEQUENCE STAGES
  whole    the taps are [B][rows][C]: checked as they are.
  ragged   the taps are [1][packed rows][C]: item b's rows (``unpack``) are checked as a B = 1 sequence.
  stream   the per-step taps [B][R][C] concatenated in time are the sequence's taps: a row's index in the
           concatenation is its absolute position, so the RoPE and the mask of the whole-sequence stage apply as they
           are (``Concat``).
  slots    a step's taps are indexed by the step's item; ``Concat.add(taps, slots)`` files item i under slot
           slots[i], and a ``reset(slot)`` starts that slot's concatenation anew (``Concat.cut``).

FAULTS (``att_fault``, ``chain``): value-only mistakes the whole-decode checks do not see, for the CPU test
tests/test_decode_xfmr_ref.py to show that the per-stage conditions do.
"""
from __future__ import annotations

import functools
import math
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch

import decode_ref
import encode_stage_ref as esr

CFG = esr.CFG
LAYERS = CFG.num_hidden_layers
KINDS = esr.XFMR_STAGES
FIRST = "upsample"
AR = esr.Arith("f32")


@functools.lru_cache(maxsize=None)
def stages(window: Optional[int] = None) -> Dict[str, esr.Stage]:
    """The 8 x 5 stages of the decoder transformer at sliding window ``window`` (None: the reference's 250)."""
    return esr.transformer_stages(FIRST, window)


def names(layers: Iterable[int] = range(LAYERS), kinds: Sequence[str] = KINDS) -> List[str]:
    return [f"{k}{l}" for l in layers for k in kinds]


def view(sd) -> Dict[str, torch.Tensor]:
    """The decoder transformer's weights of a (merged) state dict, as tensors under the names the stages read."""
    return decode_ref.as_tensors(esr.decoder_view(sd))


def upsample_tap(codes, sd, dtype=torch.float32) -> torch.Tensor:
    """The transformer's input [B, 2 T, C] of ``decode_ref``: quantizer.decode + upsample at ``dtype``."""
    sdt = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in decode_ref.as_tensors(sd).items()
           if k.startswith(("quantizer.", "upsample."))}
    with torch.no_grad():
        q = decode_ref.quantizer_decode(torch.as_tensor(codes).long(), sdt, CFG)
        return decode_ref.upsample(q, sdt).transpose(1, 2).contiguous()


def chain(x, dsd, window=None, dtype=torch.float32, fault: Optional[Dict[str, Callable]] = None,
          last: int = LAYERS - 1) -> Dict[str, torch.Tensor]:
    """Every stage of layers 0 .. last at ``dtype``, each on the ``dtype`` value of its inputs: {tap: tensor}, with
    "upsample".  ``fault``: {stage: value(xs, sd, dtype)} evaluated in place of that stage's own value."""
    taps = {FIRST: torch.as_tensor(x).to(dtype)}
    with torch.no_grad():
        for name in names(range(last + 1)):
            st = stages(window)[name]
            f = (fault or {}).get(name, st.value)
            taps[name] = f([taps[s] for s in st.source], dsd, dtype)
    return taps


def measure(name: str, taps, dsd, window=None, got=None, f32=None) -> dict:
    """One stage on the taps it reads: n, q_ref, and q_engine / worst when ``got`` is given."""
    tab = stages(window)
    return esr.measure(name, [taps[s] for s in tab[name].source], dsd, AR, got=got, f32=f32, stages=tab)


def failures(rec: dict, key: str = "q_engine") -> list:
    return esr.conditions(rec, key)


# ---- the forms ------------------------------------------------------------------------------------------------------
def unpack(tap, lengths: Sequence[int]) -> List[torch.Tensor]:
    """A ragged pass's tap [1][packed rows][C] -> one [1][2 lengths[b]][C] per item (rows are packed in item order)."""
    tap = torch.as_tensor(tap)
    assert tap.shape[0] == 1 and tap.shape[1] == 2 * sum(lengths), (tuple(tap.shape), list(lengths))
    out, at = [], 0
    for n in lengths:
        out.append(tap[:, at:at + 2 * n])
        at += 2 * n
    return out


class Concat:
    """Per-step taps [items][R][C] concatenated in time per lane (a lock-step stream's item, or a slot).  A lane's
    finished concatenations are its sequences: ``cut(lane)`` (a reset) closes the current one."""

    def __init__(self, tap_names: Iterable[str]):
        self.names = list(tap_names)
        self.parts: Dict[int, Dict[str, list]] = {}
        self.done: Dict[int, List[Dict[str, torch.Tensor]]] = {}

    def add(self, taps: Dict[str, torch.Tensor], lanes: Optional[Sequence[int]] = None):
        """``taps[name]`` [m][R][C] of one step; item i belongs to lane ``lanes[i]`` (default: lane i)."""
        m = next(iter(taps.values())).shape[0]
        lanes = list(range(m)) if lanes is None else list(lanes)
        assert len(lanes) == m, (lanes, m)
        for i, lane in enumerate(lanes):
            p = self.parts.setdefault(lane, {n: [] for n in self.names})
            for n in self.names:
                assert taps[n].shape[0] == m, (n, tuple(taps[n].shape), m)
                p[n].append(torch.as_tensor(taps[n])[i:i + 1].clone())

    def cut(self, lane: int):
        p = self.parts.pop(lane, None)
        if p is not None and p[self.names[0]]:
            self.done.setdefault(lane, []).append({n: torch.cat(v, dim=1) for n, v in p.items()})

    def sequences(self) -> Dict[int, List[Dict[str, torch.Tensor]]]:
        """lane -> its sequences' taps ([1][rows][C] each), in the order they were played."""
        for lane in list(self.parts):
            self.cut(lane)
        return self.done

    def batch(self) -> Dict[str, torch.Tensor]:
        """A lock-step stream: the lanes' single sequences stacked as [B][rows][C]."""
        seqs = self.sequences()
        assert all(len(v) == 1 for v in seqs.values()), {k: len(v) for k, v in seqs.items()}
        return {n: torch.cat([seqs[lane][0][n] for lane in sorted(seqs)], dim=0) for n in self.names}


class StepXfmr:
    """One lane of a stream on the CPU, stage by stage in float64: ``step(x [1, R, C])`` -> the step's taps
    {"upsample", qkv0, ..., xfmr7}, each [1, R, .].  Per layer it keeps the last window - 1 rows of the qkv tap (the
    rotated keys and the values a ring holds); the step's rows are rotated at their absolute positions and attend
    [kept rows | own rows] under the whole-sequence mask, which only sees differences of positions."""

    def __init__(self, dsd, window: int):
        self.dsd, self.window = dsd, int(window)
        self.reset()

    def reset(self):
        self.rows = 0
        self.kept: List[Optional[torch.Tensor]] = [None] * LAYERS

    def step(self, x) -> Dict[str, torch.Tensor]:
        tab, P, R = stages(self.window), self.rows, x.shape[1]
        taps = {FIRST: x.double()}
        with torch.no_grad():
            for l in range(LAYERS):
                for kind in KINDS:
                    st = tab[f"{kind}{l}"]
                    xs = [taps[s] for s in st.source]
                    if kind == "qkv":   # row m of the step is row P + m of the sequence: P rows of padding in front
                        pad = torch.zeros(1, P, xs[0].shape[2], dtype=torch.float64)
                        y = st.value([torch.cat([pad, xs[0]], dim=1)], self.dsd, torch.float64)[:, P:]
                    elif kind == "att":
                        hist = xs[0] if self.kept[l] is None else torch.cat([self.kept[l], xs[0]], dim=1)
                        y = st.value([hist], self.dsd, torch.float64)[:, hist.shape[1] - R:]
                        self.kept[l] = hist[:, max(hist.shape[1] - (self.window - 1), 0):].clone()
                    else:
                        y = st.value(xs, self.dsd, torch.float64)
                    taps[st.name] = y
        self.rows += R
        return taps


# ---- the slot schedule shared by the CPU and the GPU test -------------------------------------------------------------
SLOTS, SLOT_MAX_STEP, SLOT_K = 3, 3, 8
SLOT_SESSIONS = {"A": (0, 40), "B": (1, 33), "C": (2, 12), "D": (2, 26)}   # name -> (slot, frames); D follows C
SLOT_START = {"A": 0, "C": 1, "B": 3}                                      # the tick a session joins at


def slot_sessions(seed: int = 700) -> Dict[str, torch.Tensor]:
    import numpy as np
    return {name: torch.from_numpy(np.random.default_rng(seed + i).integers(0, 2048, (1, SLOT_K, T)))
            for i, (name, (_, T)) in enumerate(SLOT_SESSIONS.items())}


def slot_schedule() -> list:
    """[("step", [(slot, session), ...], n) | ("reset", slot)]: three slots at staggered starts, steps of 1 .. 3
    frames over all or some of the running slots in changing order; slot 2 plays C, is reset, then plays D while A
    and B are mid-way.  With window 70 and ``max_step_frames`` = 3 the ring has 75 rows: A (80 rows) wraps it."""
    left = {name: T for name, (_, T) in SLOT_SESSIONS.items()}
    running, ops, tick = [], [], 0
    ns = (1, 3, 2, 3, 3, 1, 2, 3)
    while any(left.values()):
        for name, t0 in SLOT_START.items():
            if t0 == tick:
                running.append(name)
        n = ns[tick % len(ns)]
        items = [(SLOT_SESSIONS[name][0], name) for name in running if left[name] >= n]
        if tick % 4 == 3 and len(items) > 1:   # a subset: one running slot sits this step out
            items.pop(tick // 4 % len(items))
        if tick % 2:
            items.reverse()
        if items:
            ops.append(("step", items, n))
            for _, name in items:
                left[name] -= n
        for name in list(running):   # a tail shorter than the tick's n: a step of its own
            if 0 < left[name] < n and (SLOT_SESSIONS[name][0], name) not in items:
                ops.append(("step", [(SLOT_SESSIONS[name][0], name)], left[name]))
                left[name] = 0
        for name in list(running):
            if left[name] == 0:
                running.remove(name)
                if name == "C":
                    ops.append(("reset", 2))
                    running.append("D")
        tick += 1
        assert tick < 1000
    return ops


# ---- faults ---------------------------------------------------------------------------------------------------------
LATE = 64   # attention_stream_kernel: key t of a row (counted from the oldest key in its window) belongs to lane
            # t % 64, so t >= 64 is a lane's second and later keys


def att_fault(kind: str, window=None) -> Callable:
    """The attention stage with a fault on the keys t >= 64 of every row, t counted from the oldest key in the row's
    window: ``weights`` (their softmax weights x 1.0001), ``fp16`` / ``bf16`` (their scores rounded to that format)."""
    assert kind in ("weights", "fp16", "bf16"), kind
    W = esr._window_cfg(window).sliding_window

    def value(xs, sd, dtype):
        q, k, v = esr.heads(xs[0].to(dtype))
        B, H, T, D = q.shape
        mask = esr.att_mask(T, W)
        i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
        late = mask & (j - (i - W + 1).clamp(min=0) >= LATE)
        s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
        if kind != "weights":
            s = torch.where(late, s.to(torch.float16 if kind == "fp16" else torch.bfloat16).to(dtype), s)
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
        if kind == "weights":
            p = torch.where(late, p * 1.0001, p)
        return (p @ v).transpose(1, 2).contiguous().reshape(B, T, H * D)
    return value


def qkv_rope_restart(l: int, boundary: int, window=None) -> Callable:
    """qkv{l} with the RoPE position restarted at row ``boundary`` (a stream step that rotates with the row's place in
    the step, not in the sequence)."""
    st = stages(window)[f"qkv{l}"]

    def value(xs, sd, dtype):
        x = xs[0]
        return torch.cat([st.value([x[:, :boundary]], sd, dtype), st.value([x[:, boundary:]], sd, dtype)], dim=1)
    return value


def oproj_next_scale(l: int) -> Callable:
    """oproj{l} with layer l + 1's layer scale."""
    def value(xs, sd, dtype):
        ls = esr._w(sd, esr._lp(l + 1) + "self_attn_layer_scale.scale", dtype)
        w = esr._w(sd, esr._lp(l) + "self_attn.o_proj.weight", dtype)
        return xs[1].to(dtype) + ls * torch.nn.functional.linear(xs[0].to(dtype), w)
    return value


def ff_one_pass_variance(l: int) -> Callable:
    """ff{l} in fp32 with LayerNorm's variance as E[x^2] - mean^2 in one fp32 pass (cancels on offset rows)."""
    p = esr._lp(l)

    def value(xs, sd, dtype):
        x = xs[0].float()
        mean = x.mean(-1, keepdim=True)
        var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp(min=0.0)
        h = (x - mean) * (var + CFG.norm_eps).rsqrt() * esr._w(sd, p + "post_attention_layernorm.weight", torch.float32) \
            + esr._w(sd, p + "post_attention_layernorm.bias", torch.float32)
        return torch.nn.functional.gelu(torch.nn.functional.linear(h, esr._w(sd, p + "mlp.fc1.weight", torch.float32)))
    return value


def xfmr_dropped_column(l: int, column: int = 100) -> Callable:
    """xfmr{l} with column ``column`` of fc2 (one of its 2048 terms) dropped."""
    def value(xs, sd, dtype):
        w = esr._w(sd, esr._lp(l) + "mlp.fc2.weight", dtype).clone()
        w[:, column] = 0
        return xs[1].to(dtype) + esr._w(sd, esr._lp(l) + "mlp_layer_scale.scale", dtype) * \
            torch.nn.functional.linear(xs[0].to(dtype), w)
    return value
