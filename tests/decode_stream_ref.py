"""Test infrastructure only (CPU): the STREAMED decoder, stated with torch-CPU ops on ``oracle/mimi_ref.py`` and
``tests/decode_ref.py`` functions -- ``StreamState`` holds what a decode stream carries from step to step, ``step``
decodes the next ``n`` frames.

Every stage of the decoder is causal, so a stage needs from the past only the rows its kernel reaches back to (all
tensors channel-first ``[B, C, T]`` as in ``decode_ref``):

    stage                       reads from the past       carry
    upsample (k 4, stride 2)    x[t - 1]                  1 row  [512]      of the output_proj embedding
    attention, 8 layers         k / v of rows (P - W, P)  W - 1 rows per layer of the ROTATED k and of v
    decoder.layers.0 (k 7)      6 rows                    6 rows [512]      of the transformer output
    up conv s (k 2r, stride r)  1 row                     1 row  [C_s]      of the ELU'd tensor it reads
    residual block s (k 3, 1)   2 rows                    2 rows [C_s / 2]  of the up conv's raw output
    last conv (k 3)             2 rows                    2 rows [64]       of the last block's ELU'd output

A fresh state is all zeros with an empty cache at position 0: zero is what causal padding is and ELU(0) = 0, so the
first step is no special case.  The statement a streamed decode makes is exact: the samples of frames [p, p + n) are
those ``decode_ref.decode`` of the whole sequence gives (to the rounding of another summation split).

``Mutant`` switches on, one at a time, the mistakes an implementation is likely to make;
tests/test_decode_stream_ref.py shows that each moves the output far beyond the tolerance on the inputs the GPU tests
use.  This file pins the carry sizes and the position bookkeeping; it is not a second implementation to be tuned.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn.functional as F

import decode_ref
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig


@dataclass(frozen=True)
class Mutant:
    window_delta: int = 0         # the attention window off by this many rows (mask and cache)
    rope_restart: bool = False    # RoPE positions restart at 0 in every step
    conv0_short: bool = False     # decoder.layers.0 sees 5 carried rows, the oldest one zero
    no_shift: bool = False        # a chunk with fewer rows than a carry overwrites its tail without shifting it
    drop_upsample: bool = False   # the upsample's x[t - 1] carry stays zero


def carry_plan(cfg: RefConfig):
    """[(name, rows, channels)] in stage order: the table above."""
    plan = [("upsample", 1, cfg.hidden_size), ("conv0", cfg.kernel_size - 1, cfg.hidden_size)]
    C = cfg.num_filters << len(cfg.upsampling_ratios)
    for s in range(len(cfg.upsampling_ratios)):
        plan.append((f"up{s}", 1, C))
        C //= 2
        plan.append((f"res{s}", cfg.residual_kernel_size - 1, C))
    plan.append(("last", cfg.last_kernel_size - 1, C))
    return plan


def state_floats(cfg: RefConfig, batch: int, max_step_frames: int) -> int:
    """Floats of a stream's state as the engine lays it out: the carries, a k and a v ring of
    ``W - 1 + 2 max_step_frames`` rows per layer, and the step's RoPE rows (before the engine's 256-byte rounding)."""
    carries = sum(batch * h * c for _, h, c in carry_plan(cfg))
    ring = cfg.sliding_window - 1 + 2 * max_step_frames
    kv = 2 * cfg.num_hidden_layers * batch * cfg.num_attention_heads * ring * cfg.head_dim
    rope = 2 * 2 * max_step_frames * (cfg.head_dim // 2)
    return carries + kv + rope


class StreamState:
    def __init__(self, sd, batch: int = 1, cfg: Optional[RefConfig] = None, mutant: Optional[Mutant] = None):
        self.sd = decode_ref.as_tensors(sd)
        self.cfg = cfg or RefConfig()
        self.mut = mutant or Mutant()
        self.batch = batch
        self.reset()

    def reset(self):
        self.position = 0  # frames decoded so far
        self.carry = {name: torch.zeros(self.batch, c, h) for name, h, c in carry_plan(self.cfg)}
        self.k: List[Optional[torch.Tensor]] = [None] * self.cfg.num_hidden_layers  # [B, H, rows <= W - 1, D]
        self.v: List[Optional[torch.Tensor]] = [None] * self.cfg.num_hidden_layers

    # ---- carries -------------------------------------------------------------------------------
    def _extend(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """[carry | chunk], and the carry advanced to its last rows."""
        old = self.carry[name]
        h = old.shape[-1]
        ext = torch.cat([old, x], dim=-1)
        if self.mut.no_shift and x.shape[-1] < h:
            new = old.clone()
            new[..., h - x.shape[-1]:] = x
        else:
            new = ext[..., -h:]
        self.carry[name] = new.clone()
        return ext

    # ---- the transformer on a KV cache ---------------------------------------------------------
    def _transformer(self, x: torch.Tensor) -> torch.Tensor:
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
            p = f"decoder_transformer.layers.{l}."
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
        return x

    # ---- one step ------------------------------------------------------------------------------
    def step(self, codes, taps: Optional[dict] = None) -> torch.Tensor:
        """codes [B, K, n] -> float32 [B, 1, 1920 n], the samples of frames [position, position + n)."""
        cfg, sd = self.cfg, self.sd
        codes = torch.as_tensor(codes).long()
        assert codes.dim() == 3 and codes.shape[0] == self.batch and codes.shape[2] >= 1, tuple(codes.shape)
        with torch.no_grad():
            q = decode_ref.quantizer_decode(codes, sd, cfg)
            if taps is not None:
                taps["quantized"] = q
            ext = self._extend("upsample", q)
            if self.mut.drop_upsample:
                ext = torch.cat([torch.zeros_like(ext[..., :1]), ext[..., 1:]], dim=-1)
            x = decode_ref.upsample(ext, sd)[..., 2:]  # the 2 rows of the carried frame are the last step's
            if taps is not None:
                taps["upsample"] = x
            x = self._transformer(x.transpose(1, 2)).transpose(1, 2)
            if taps is not None:
                taps[f"xfmr{cfg.num_hidden_layers - 1}"] = x
            ext = self._extend("conv0", x)
            if self.mut.conv0_short:
                ext = torch.cat([torch.zeros_like(ext[..., :1]), ext[..., 1:]], dim=-1)
            x = F.conv1d(ext, sd["decoder.layers.0.conv.weight"], sd["decoder.layers.0.conv.bias"])
            if taps is not None:
                taps["dconv0"] = x
            idx = 1
            for s, ratio in enumerate(cfg.upsampling_ratios):
                idx += 1
                p = f"decoder.layers.{idx}.conv."
                ext = self._extend(f"up{s}", F.elu(x))
                x = decode_ref.conv_transpose1d_causal(ext, sd[p + "weight"], sd[p + "bias"], stride=ratio)[..., ratio:]
                if taps is not None:
                    taps[f"up{s}"] = x
                idx += 1
                p = f"decoder.layers.{idx}.block."
                ext = self._extend(f"res{s}", x)
                h = F.conv1d(F.elu(ext), sd[p + "1.conv.weight"], sd[p + "1.conv.bias"])
                h = F.conv1d(F.elu(h), sd[p + "3.conv.weight"], sd[p + "3.conv.bias"])
                x = x + h
                if taps is not None:
                    taps[f"dres{s}"] = x
                idx += 1
            idx += 1
            p = f"decoder.layers.{idx}.conv."
            ext = self._extend("last", F.elu(x))
            y = F.conv1d(ext, sd[p + "weight"], sd[p + "bias"])
            if taps is not None:
                taps["audio"] = y
        self.position += codes.shape[2]
        return y


def decode_stream(codes, sd, split, cfg: Optional[RefConfig] = None, mutant: Optional[Mutant] = None) -> torch.Tensor:
    """``codes [B, K, T]`` decoded in steps of ``split`` frames (summing to T), concatenated."""
    codes = torch.as_tensor(codes)
    assert sum(split) == codes.shape[2], (split, tuple(codes.shape))
    st = StreamState(sd, codes.shape[0], cfg, mutant)
    out, at = [], 0
    for n in split:
        out.append(st.step(codes[:, :, at:at + n]))
        at += n
    assert st.position == codes.shape[2]
    return torch.cat(out, dim=-1)
