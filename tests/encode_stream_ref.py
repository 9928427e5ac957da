"""Test infrastructure only (CPU): the STREAMED encoder, stated with torch-CPU ops on ``oracle/mimi_ref.py`` functions --
``StreamState`` holds what an encode stream carries from step to step, ``step`` encodes the next ``n`` whole frames
(``FRAME`` = 1920 samples each).

Every stage of the encoder is causal, and fed whole frames every strided length divides exactly
(``1920 n -> 480 n -> 96 n -> 16 n -> 2 n -> 2 n -> n``), so the reference's right-hand "extra padding" is 0 at every
conv and a stage needs from the past only the rows its kernel reaches back to (tensors channel-first ``[B, C, T]``;
``C_s`` = 64, 128, 256, 512 and ``r_s`` = 4, 5, 6, 8):

    stage                           reads from the past       carry
    conv 0 (k 7)                    6 samples                 6 floats of audio
    residual block s (k 3, k 1)     2 rows                    2 rows [C_s]   of the block's raw input
    down conv s (k 2 r_s, str r_s)  r_s rows                  r_s rows [C_s] of the block's ELU'd output
    final conv (k 3)                2 rows                    2 rows [1024]  of the ELU'd down conv 3 output
    attention, 8 layers             k / v of rows (P - W, P)  W - 1 rows per layer of the ROTATED k and of v
    downsample (k 4, stride 2)      2 rows                    2 rows [512]   of the transformer output

A fresh state is all zeros with an empty cache at position 0 -- zero is what causal padding is and ELU(0) = 0 -- with
ONE exception: the reference pads the downsample with copies of the sequence's first row (``F.pad(mode="replicate")``
in one shot, ``MimiConv1dPaddingCache`` when streaming), so the step that finds the state at position 0 fills the
downsample's carry from row 0 of its own transformer output.  The statement is exact: the codes of frames [p, p + n)
are those of ``mimi_ref.encode`` of any sequence that contains those frames whole (to the rounding of another
summation split).

``SlotPool`` is the contract of the slot form, not a second implementation: slot ``s`` IS a ``batch = 1`` stream.

``Mutant`` switches on, one at a time, the mistakes an implementation is likely to make;
tests/test_encode_stream_ref.py shows that each moves the embedding far beyond the tolerance on the inputs the GPU
tests use.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

FRAME = 1920


@dataclass(frozen=True)
class Mutant:
    window_delta: int = 0             # the attention window off by this many rows (mask and cache)
    rope_restart: bool = False        # RoPE positions restart at 0 in every step
    down_short: bool = False          # a down conv carries r_s - 1 rows: the oldest one reads as zero
    final_short: bool = False         # the final conv's carry a row short
    ds_zero_fresh: bool = False       # the downsample's carry stays zero on a fresh state (zero instead of replicate)
    ds_replicate_every: bool = False  # ... is filled from the step's first row on EVERY step
    drop_conv0: bool = False          # conv 0's 6 carried samples stay zero
    # the two mistakes of the slot plumbing (SlotPool):
    reset_keeps_ds: bool = False      # reset(slot) keeps the previous session's downsample carry and uses it
    carry_by_item: bool = False       # the carries are addressed by the item's place in the step, not by its slot


def as_tensors(sd) -> Dict[str, torch.Tensor]:
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).float() for k, v in sd.items()}


def ratios(cfg: RefConfig) -> List[int]:
    return list(reversed(cfg.upsampling_ratios))


def carry_plan(cfg: RefConfig):
    """[(name, rows, channels)] in stage order: the table above (the rings apart).  (The engine keeps conv 0's 6 samples
    as the last 8, for 16-byte copies: inside its 256-byte rounding.)"""
    plan = [("conv0", cfg.kernel_size - 1, 1)]
    C = cfg.num_filters
    for s, r in enumerate(ratios(cfg)):
        plan.append((f"res{s}", cfg.residual_kernel_size - 1, C))
        plan.append((f"down{s}", r, C))
        C *= 2
    plan.append(("final", cfg.last_kernel_size - 1, C))
    plan.append(("ds", 2, cfg.hidden_size))
    return plan


def state_floats(cfg: RefConfig, batch: int, max_step_frames: int) -> int:
    """Floats of a stream's state as the engine lays it out: the carries, a k and a v ring of
    ``W - 1 + 2 max_step_frames`` rows per layer, and the RoPE rows of a step of every slot (before the engine's
    256-byte rounding of each section)."""
    carries = sum(batch * h * c for _, h, c in carry_plan(cfg))
    ring = cfg.sliding_window - 1 + 2 * max_step_frames
    kv = 2 * cfg.num_hidden_layers * batch * cfg.num_attention_heads * ring * cfg.head_dim
    rope = 2 * batch * 2 * max_step_frames * (cfg.head_dim // 2)
    return carries + kv + rope


def state_sections(cfg: RefConfig) -> int:
    """How many separately rounded sections the state has: the carries, two rings, two RoPE tables."""
    return len(carry_plan(cfg)) + 4


class StreamState:
    def __init__(self, sd, batch: int = 1, cfg: Optional[RefConfig] = None, mutant: Optional[Mutant] = None):
        self.sd = as_tensors(sd)
        self.cfg = cfg or RefConfig()
        self.mut = mutant or Mutant()
        self.batch = batch
        self.reset()

    def reset(self):
        self.position = 0  # frames encoded so far
        self.carry = {name: torch.zeros(self.batch, c, h) for name, h, c in carry_plan(self.cfg)}
        self.ds_stale = False  # (Mutant.reset_keeps_ds) the downsample carry is a previous session's and is used
        self.k: List[Optional[torch.Tensor]] = [None] * self.cfg.num_hidden_layers  # [B, H, rows <= W - 1, D]
        self.v: List[Optional[torch.Tensor]] = [None] * self.cfg.num_hidden_layers

    # ---- carries -------------------------------------------------------------------------------
    def _extend(self, name: str, x: torch.Tensor, short: bool = False) -> torch.Tensor:
        """[carry | chunk], and the carry advanced to its last rows.  short: the oldest carried row reads as zero."""
        old = self.carry[name]
        h = old.shape[-1]
        ext = torch.cat([old, x], dim=-1)
        self.carry[name] = ext[..., -h:].clone()
        if short:
            ext = torch.cat([torch.zeros_like(ext[..., :1]), ext[..., 1:]], dim=-1)
        return ext

    # ---- the transformer on a KV cache ---------------------------------------------------------
    def _transformer(self, x: torch.Tensor, taps: Optional[dict]) -> torch.Tensor:
        """x: [B, R, C], the rows at absolute positions P .. P + R - 1."""
        cfg, sd = self.cfg, self.sd
        B, R, C = x.shape
        H, D = cfg.num_attention_heads, cfg.head_dim
        W = cfg.sliding_window + self.mut.window_delta
        P = 2 * self.position
        cos, sin = mimi_ref.rope_cos_sin(P + R, cfg)
        lo = 0 if self.mut.rope_restart else P
        cos, sin = cos[:, None, lo:lo + R], sin[:, None, lo:lo + R]
        scale = 1.0 / math.sqrt(D)
        for l in range(cfg.num_hidden_layers):
            p = f"encoder_transformer.layers.{l}."
            res = x
            h = F.layer_norm(x, (C,), sd[p + "input_layernorm.weight"], sd[p + "input_layernorm.bias"], cfg.norm_eps)
            q = F.linear(h, sd[p + "self_attn.q_proj.weight"]).view(B, R, H, D).transpose(1, 2)
            k = F.linear(h, sd[p + "self_attn.k_proj.weight"]).view(B, R, H, D).transpose(1, 2)
            v = F.linear(h, sd[p + "self_attn.v_proj.weight"]).view(B, R, H, D).transpose(1, 2)
            q = (q * cos) + (mimi_ref.rotate_half(q) * sin)
            k = (k * cos) + (mimi_ref.rotate_half(k) * sin)
            if self.k[l] is not None:
                k = torch.cat([self.k[l], k], dim=2)
                v = torch.cat([self.v[l], v], dim=2)
            n_keys = k.shape[2]
            j = (P + R - n_keys) + torch.arange(n_keys)[None, :]  # the keys' absolute positions
            i = P + torch.arange(R)[:, None]
            mask = (j <= i) & (j > i - W)
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask[None, None], dropout_p=0.0, scale=scale)
            keep = max(W - 1, 0)
            self.k[l] = k[:, :, n_keys - min(keep, n_keys):].clone()
            self.v[l] = v[:, :, n_keys - min(keep, n_keys):].clone()
            a = F.linear(a.transpose(1, 2).contiguous().reshape(B, R, C), sd[p + "self_attn.o_proj.weight"])
            x = res + sd[p + "self_attn_layer_scale.scale"] * a
            res = x
            h = F.layer_norm(x, (C,), sd[p + "post_attention_layernorm.weight"],
                             sd[p + "post_attention_layernorm.bias"], cfg.norm_eps)
            h = F.linear(F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"])), sd[p + "mlp.fc2.weight"])
            x = res + sd[p + "mlp_layer_scale.scale"] * h
            if taps is not None:
                taps[f"xfmr{l}"] = x.transpose(1, 2)
        return x

    # ---- one step ------------------------------------------------------------------------------
    def embed(self, audio, taps: Optional[dict] = None) -> torch.Tensor:
        """audio [B, 1, 1920 n] -> the pre-quantizer embedding [B, 512, n] of frames [position, position + n)."""
        cfg, sd, mut = self.cfg, self.sd, self.mut
        x = torch.as_tensor(audio).float()
        assert x.dim() == 3 and x.shape[0] == self.batch and x.shape[1] == 1, tuple(x.shape)
        assert x.shape[2] >= FRAME and x.shape[2] % FRAME == 0, tuple(x.shape)
        n = x.shape[2] // FRAME
        with torch.no_grad():
            ext = self._extend("conv0", x)
            if mut.drop_conv0:
                ext = torch.cat([torch.zeros_like(ext[..., :cfg.kernel_size - 1]), x], dim=-1)
            x = F.conv1d(ext, sd["encoder.layers.0.conv.weight"], sd["encoder.layers.0.conv.bias"])
            if taps is not None:
                taps["conv0"] = x
            idx = 1
            for s, r in enumerate(ratios(cfg)):
                p = f"encoder.layers.{idx}.block."
                ext = self._extend(f"res{s}", x)
                h = F.conv1d(F.elu(ext), sd[p + "1.conv.weight"], sd[p + "1.conv.bias"])
                h = F.conv1d(F.elu(h), sd[p + "3.conv.weight"], sd[p + "3.conv.bias"])
                x = x + h
                if taps is not None:
                    taps[f"res{s}"] = x
                idx += 2
                p = f"encoder.layers.{idx}.conv."
                ext = self._extend(f"down{s}", F.elu(x), short=mut.down_short)
                x = F.conv1d(ext, sd[p + "weight"], sd[p + "bias"], stride=r)
                if taps is not None:
                    taps[f"down{s}"] = x
                idx += 1
            idx += 1
            p = f"encoder.layers.{idx}.conv."
            ext = self._extend("final", F.elu(x), short=mut.final_short)
            x = F.conv1d(ext, sd[p + "weight"], sd[p + "bias"])
            assert x.shape[2] == 2 * n, (tuple(x.shape), n)
            if taps is not None:
                taps["encoder"] = x
            x = self._transformer(x.transpose(1, 2), taps).transpose(1, 2)
            # the downsample's replicate padding: a property of a state at position 0
            fresh = self.position == 0 and not self.ds_stale
            if (fresh and not mut.ds_zero_fresh) or mut.ds_replicate_every:
                self.carry["ds"] = x[..., :1].repeat(1, 1, 2).clone()
            ext = self._extend("ds", x)
            e = F.conv1d(ext, sd["downsample.conv.weight"], None, stride=2)
            assert e.shape[2] == n
            if taps is not None:
                taps["downsample"] = e
        self.position += n
        self.ds_stale = False
        return e

    def step(self, audio, num_quantizers: int = 8, taps: Optional[dict] = None) -> torch.Tensor:
        """audio [B, 1, 1920 n] -> int64 codes [B, K, n] of frames [position, position + n)."""
        e = self.embed(audio, taps)
        with torch.no_grad():
            return mimi_ref.split_rvq_encode(e, self.sd, num_quantizers, self.cfg).transpose(0, 1)


def chunks(audio: torch.Tensor, split: Sequence[int]):
    assert sum(split) * FRAME == audio.shape[-1], (split, tuple(audio.shape))
    at = 0
    for n in split:
        yield audio[..., at * FRAME:(at + n) * FRAME]
        at += n


def embed_stream(audio, sd, split, cfg: Optional[RefConfig] = None, mutant: Optional[Mutant] = None) -> torch.Tensor:
    """``audio [B, 1, 1920 T]`` in steps of ``split`` frames: the concatenated pre-quantizer embedding ``[B, 512, T]``."""
    audio = torch.as_tensor(audio)
    st = StreamState(sd, audio.shape[0], cfg, mutant)
    out = [st.embed(a) for a in chunks(audio, split)]
    assert st.position == sum(split)
    return torch.cat(out, dim=-1)


def encode_stream(audio, sd, split, K: int = 8, cfg: Optional[RefConfig] = None,
                  mutant: Optional[Mutant] = None) -> torch.Tensor:
    """The concatenated codes ``[B, K, T]`` of the same."""
    e = embed_stream(audio, sd, split, cfg, mutant)
    with torch.no_grad():
        return mimi_ref.split_rvq_encode(e, as_tensors(sd), K, cfg or RefConfig()).transpose(0, 1)


class SlotPool:
    """One ``StreamState(batch=1)`` per slot; ``embed(slots, audio)`` steps the listed ones, ``reset(slot)`` makes one
    fresh.  The two plumbing mutants live here."""

    def __init__(self, sd, batch: int, cfg: Optional[RefConfig] = None, mutant: Optional[Mutant] = None):
        self.batch = batch
        self.mut = mutant or Mutant()
        sdt = as_tensors(sd)
        self.states = [StreamState(sdt, 1, cfg) for _ in range(batch)]

    @property
    def positions(self) -> List[int]:
        return [st.position for st in self.states]

    def reset(self, slot: int):
        assert 0 <= slot < self.batch
        st = self.states[slot]
        old = st.carry["ds"]
        used = st.position > 0
        st.reset()
        if self.mut.reset_keeps_ds and used:
            st.carry["ds"] = old
            st.ds_stale = True

    def embed(self, slots: Sequence[int], audio) -> torch.Tensor:
        """audio [m, 1, 1920 n], item i the next n frames of slot slots[i] -> [m, 512, n]."""
        slots = list(slots)
        audio = torch.as_tensor(audio)
        assert 1 <= len(slots) <= self.batch and len(set(slots)) == len(slots), slots
        assert all(0 <= s < self.batch for s in slots) and audio.shape[0] == len(slots), (slots, tuple(audio.shape))
        out = []
        for i, s in enumerate(slots):
            st = self.states[s]
            car = self.states[i] if self.mut.carry_by_item else st
            own = st.carry
            st.carry = car.carry
            out.append(st.embed(audio[i:i + 1]))
            car.carry = st.carry
            if car is not st:
                st.carry = own
        return torch.cat(out, dim=0)

    def step(self, slots: Sequence[int], audio, num_quantizers: int = 8) -> torch.Tensor:
        e = self.embed(slots, audio)
        with torch.no_grad():
            return mimi_ref.split_rvq_encode(e, self.states[0].sd, num_quantizers, self.states[0].cfg).transpose(0, 1)


# ---- the slot schedule (the decode slots schedule's shape) ----------------------------------------------------------
BATCH, MAX_STEP_FRAMES, K, WINDOW = 4, 7, 8, 5
SESSION_FRAMES = {"A": 9, "B": 13, "C": 11, "D": 10}
# ("step", [(slot, session), ...], n) in the order the call lists them, or ("reset", slot).  A starts alone; B joins at
# call 2; C joins at call 3 on slot 3 (slot 2 is never used); A ends after call 4, its slot is reset and D starts on it
# while B and C are mid-way.  1 to 3 slots per call, ascending and permuted; n over 1, 2, 3, 7.
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


def splits(schedule=SCHEDULE) -> Dict[str, List[int]]:
    """name -> the steps the schedule cuts that session into."""
    out: Dict[str, List[int]] = {}
    for op in schedule:
        if op[0] == "step":
            for _, name in op[1]:
                out.setdefault(name, []).append(op[2])
    return out


def play(sessions: Dict[str, torch.Tensor], step, reset, positions, schedule=SCHEDULE, batch: int = BATCH):
    """Run the schedule through ``step(slots, audio[m, 1, 1920 n]) -> [m, X, n]``, ``reset(slot)`` and
    ``positions() -> [batch]``; the positions are checked after every call.  name -> that session's concatenated
    output.  sessions: name -> audio [1, 1, 1920 T]."""
    at = {name: 0 for name in sessions}
    want_pos = [0] * batch
    parts: Dict[str, List[torch.Tensor]] = {name: [] for name in sessions}
    for op in schedule:
        if op[0] == "reset":
            reset(op[1])
            want_pos[op[1]] = 0
        else:
            _, items, n = op
            audio = torch.cat([sessions[name][..., at[name] * FRAME:(at[name] + n) * FRAME] for _, name in items])
            assert audio.shape[-1] == n * FRAME, (op, tuple(audio.shape))
            y = step([s for s, _ in items], audio)
            assert y.shape[0] == len(items) and y.shape[-1] == n, (op, tuple(y.shape))
            for i, (s, name) in enumerate(items):
                parts[name].append(y[i:i + 1].cpu())
                at[name] += n
                want_pos[s] += n
        assert list(positions()) == want_pos, (op, list(positions()), want_pos)
    assert all(at[name] * FRAME == sessions[name].shape[-1] for name in sessions), at
    return {name: torch.cat(v, dim=-1) for name, v in parts.items()}


# ---- the clips the tests use -----------------------------------------------------------------------------------------
# name -> (frames, audio seed, clip index, sliding_window).  Chosen on the CPU (tests/test_encode_stream_ref.py
# test_clips_have_no_flip, which prints each clip's smallest top-2 relative margin at K = 8) so that the streamed
# reference's codes equal ``mimi_ref.encode``'s at every level with no flip.
# "t130", the real-window clip, is that speech-like clip moved by a few per cent of full scale so that the rows which
# leave / enter the 250-row window hold enough of the last queries' attention for a window off by one to show
# (tests/golden/encode_stream_window_clip.npz, made by tests/golden/make_window_clip.py: on natural input one key in
# 250 moves the embedding by 3e-4 .. 8e-4 only).
CLIPS = {
    "t13": (13, 7, 0, 250), "t13b": (13, 7, 1, 250), "t13c": (13, 7, 2, 250), "t13d": (13, 8, 0, 250),
    "t130": (130, 24, 0, 250), "t133": (133, 19, 3, 250), "t9w5": (9, 10, 0, 5),
    "A": (9, 11, 0, 5), "B": (13, 11, 1, 5), "C": (11, 11, 2, 5), "D": (10, 11, 3, 5),
}
WINDOW_CLIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_stream_window_clip.npz")


def clip(name: str) -> torch.Tensor:
    """The clip as audio [1, 1, 1920 T]."""
    from mimi_hip import synthetic
    frames, seed, index, _ = CLIPS[name]
    if name == "t130":
        with np.load(WINDOW_CLIP, allow_pickle=False) as z:
            assert int(z["frames"]) == frames and int(z["seed"]) == seed
            x = torch.from_numpy(z["audio"].astype(np.float32))[None, None]
        assert x.shape[-1] == FRAME * frames
        return x
    return torch.from_numpy(synthetic.speech_like(FRAME * frames, seed, index))[None, None]


def clip_cfg(name: str) -> RefConfig:
    return RefConfig(sliding_window=CLIPS[name][3])
