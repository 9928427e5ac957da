"""Test infrastructure only (CPU): adversarial checkpoints and degenerate audio for the ENCODE path, and the measures
that say which regime of the transformer kernels a case reaches.

Every GPU encode test before these fed speech-like clips through the seeded synthetic checkpoint, where attention
scores span 3.6, the median largest softmax weight is 0.26 and LayerNorm rows have |mean| / std <= 0.08: a benign
corner of the attention and LayerNorm kernels' domain.  Trained transformers have peaky attention and "massive"
residual channels; real corpora have digital silence, DC, clipped stretches and the odd non-finite sample.

CHECKPOINTS: pure functions of ``synthetic.make_state_dict(seed=0, num_quantizers=8)`` (``CHECKPOINTS[name](base)``;
only the final conv and the transformer change, so every case shares the SEANet taps of the base checkpoint).
AUDIO: functions of (length, seed) (``AUDIO[name](L, seed)``); ``FINITE_AUDIO`` lists the ones without Inf / NaN.
MEASURES: ``attention_regime`` (of a qkv tap), ``layernorm_regime`` (of a LayerNorm input), in float64.
``speech_scales`` gives the f16x3 plane scales the calibration rule sets on full-level speech: the engine's scales are
fixed at load time, so a quiet clip meets scales that were set by loud audio, not by itself.

The GPU tests are tests/test_encode_adversarial.py; tests/test_encode_adversarial_ref.py proves on the CPU that each
case reaches its regime, that the references stay inside the hard condition there, and which injected faults the cases
catch that speech on the base checkpoint does not.
"""
from __future__ import annotations

import math
from typing import Callable, Dict

import numpy as np
import torch

import encode_stage_ref as esr
from mimi_hip import synthetic

LAYERS = esr.CFG.num_hidden_layers
CHUNK = 32   # keys per online-softmax step of the f16x3 attention kernels (attn_h16.h attn_chunk_h16)
OFFSET_GAIN = 5000.0   # 200 gave |mean| / std up to 137, 2000 gave 530 .. 1670 over the rows; 5000: every row >= 1e3


def base_state_dict() -> Dict[str, np.ndarray]:
    return synthetic.make_state_dict(seed=0, num_quantizers=8)


def _copy(sd):
    return {k: np.array(v, copy=True) for k, v in sd.items()}


def _scale_qk(sd, gq, gk):
    out = _copy(sd)
    for l in range(LAYERS):
        p = esr._lp(l) + "self_attn."
        out[p + "q_proj.weight"] = out[p + "q_proj.weight"] * np.float32(gq)
        out[p + "k_proj.weight"] = out[p + "k_proj.weight"] * np.float32(gk)
    return out


def peaky3(sd):
    """q_proj and k_proj of all 8 layers x 3 (scores x 9).  Aims at the online-softmax rescale across 32-key chunks
    (attn_h16.h: corr = exp(m - mnew)) at a moderate range: weights still spread over several keys, so the p planes
    hold both large and small weights."""
    return _scale_qk(sd, 3.0, 3.0)


def peaky8(sd):
    """q_proj and k_proj x 8 (scores x 64): score ranges of hundreds, the largest weight 1.0000, almost every other
    weight underflows, and the running maximum jumps by tens between chunks.  Aims at corr = exp(m - mnew) far from 1,
    at exp underflow, and at the p-plane split at 2^14 flushing small weights."""
    return _scale_qk(sd, 8.0, 8.0)


def flat(sd):
    """q_proj x 0: every score is 0, the output a uniform average over up to 250 keys.  Aims at the normaliser and the
    P V sum at their longest with no weight dominating, and at p = 1 / 250 on the p planes (a systematic hi-plane
    rounding is not averaged out)."""
    return _scale_qk(sd, 0.0, 1.0)


def offset(sd):
    """Final conv bias + OFFSET_GAIN (max|bias| + 1) on every channel: the residual stream keeps a common offset, so
    every LayerNorm row has |mean| / std >= 1e3.  Aims at LayerNorm's x rstd + (-mean rstd) under cancellation
    (kernels.h ln_affine) and at the two-pass variance."""
    out = _copy(sd)
    b = out[esr.PF + "bias"]
    out[esr.PF + "bias"] = (b + np.float32(OFFSET_GAIN * (float(np.abs(b).max()) + 1.0))).astype(np.float32)
    return out


def massive(sd):
    """Final conv bias + 3000 on channel 5 and - 2000 on channel 300: two "massive" residual channels.  One tensor
    maximum of 3e3 sets each fixed plane scale while a typical value is near 1: the other 510 channels sit at the
    fp16-plane floors, and the residual epilogues x + ls (W a) add updates far below |x| on the massive channels."""
    out = _copy(sd)
    b = np.array(out[esr.PF + "bias"], copy=True)
    b[5] += np.float32(3000.0)
    b[300] -= np.float32(2000.0)
    out[esr.PF + "bias"] = b
    return out


def onehot(sd):
    """Final conv weight rows zeroed except output channel 7, bias 0: layer 0's LayerNorm rows are one-hot, the rows
    that reach |g| sqrt(D - 1) -- the bound the engine uses to skip that output's range check (engine.cpp
    DevXfmr::ln1_bound)."""
    out = _copy(sd)
    w = np.zeros_like(out[esr.PF + "weight"])
    w[7] = out[esr.PF + "weight"][7]
    out[esr.PF + "weight"] = w
    out[esr.PF + "bias"] = np.zeros_like(out[esr.PF + "bias"])
    return out


CHECKPOINTS: Dict[str, Callable] = {"peaky3": peaky3, "peaky8": peaky8, "flat": flat, "offset": offset,
                                    "massive": massive, "onehot": onehot}
ATTENTION_CASES = ("peaky3", "peaky8", "flat")
LAYERNORM_CASES = ("offset", "massive", "onehot")


def torch_sd(sd):
    return {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}


# ---- degenerate audio -------------------------------------------------------------------------------------------------
def _speech(L, seed):
    return synthetic.speech_like(L, seed, 0)


def _const(v):
    return lambda L, seed: np.full(L, v, dtype=np.float32)


def square(L, seed):
    """+-1.0 at 100 Hz (120 samples high, 120 low at 24 kHz)."""
    return np.where((np.arange(L) // 120) % 2 == 0, 1.0, -1.0).astype(np.float32)


def impulse(L, seed):
    x = np.zeros(L, dtype=np.float32)
    x[5000] = 1.0
    return x


def tiny_noise(L, seed):
    return (synthetic.noise_clip(L, seed, 0, std=1.0 / math.sqrt(3.0)).astype(np.float64) * 1e-20).astype(np.float32)


def subnormal_noise(L, seed):
    """Uniform noise at 1e-40: every sample an fp32 subnormal (the smallest normal is 1.18e-38)."""
    return (synthetic.noise_clip(L, seed, 0, std=1.0 / math.sqrt(3.0)).astype(np.float64) * 1e-40).astype(np.float32)


def half_silence(L, seed):
    x = _speech(L, seed).copy()
    x[:L // 2] = 0.0
    return x


def _with(value):
    def f(L, seed):
        x = _speech(L, seed).copy()
        x[7000:7004] = value
        return x
    return f


AUDIO: Dict[str, Callable] = {
    "zeros": _const(0.0), "neg_zeros": _const(-0.0), "dc_half": _const(0.5), "dc_one": _const(1.0), "square": square,
    "impulse": impulse, "noise_1e-20": tiny_noise, "subnormal_1e-40": subnormal_noise, "half_silence": half_silence,
    "inf": _with(np.inf), "nan": _with(np.nan),
}
FINITE_AUDIO = [n for n in AUDIO if n not in ("inf", "nan")]


def audio_batch(name, L, seed):
    """[2, L]: item 0 the case, item 1 speech."""
    return torch.from_numpy(np.stack([AUDIO[name](L, seed), synthetic.speech_like(L, seed, 1)]))


def speech_batch(B, L, seed):
    return torch.from_numpy(np.stack([synthetic.speech_like(L, seed, i) for i in range(B)]))


# ---- measures ---------------------------------------------------------------------------------------------------------
def attention_regime(qkv_tap, window=None) -> dict:
    """Of a qkv tap [B, T, 3 H D] at sliding window ``window`` (None: the reference's), over every (item, head, row), in float64: the largest score range of a row (over
    its unmasked keys), the median and the smallest largest-softmax-weight, the largest |score|, and how often the
    running maximum of a row changes in a chunk after its first (the kernels walk the keys in 32-key chunks from key 0
    of the item; every such change is a corr = exp(m - mnew) < 1)."""
    q, k, v = esr.heads(torch.as_tensor(qkv_tap).double())
    T = q.shape[2]
    mask = esr.att_mask(T, window)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    lo = s.masked_fill(~mask, float("inf")).amin(-1)
    hi = s.masked_fill(~mask, float("-inf")).amax(-1)
    top = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1).amax(-1)
    changes = torch.zeros_like(hi)
    m = torch.full_like(hi, float("-inf"))
    for c0 in range(0, T, CHUNK):
        cm = s[..., c0:c0 + CHUNK].masked_fill(~mask[:, c0:c0 + CHUNK], float("-inf")).amax(-1)
        changes += ((cm > m) & torch.isfinite(m)).double()
        m = torch.maximum(m, cm)
    return {"score_range": float((hi - lo).max()), "median_top_weight": float(top.median()),
            "min_top_weight": float(top.min()), "max_abs_score": float(s.masked_fill(~mask, 0.0).abs().max()),
            "max_later_chunk_changes": int(changes.max()), "rows_with_2_changes": int((changes >= 2).sum())}


def layernorm_regime(x) -> dict:
    """Of a LayerNorm input [B, T, C] in float64: the extremes of |mean| / std over rows, the largest normalised
    value (against sqrt(C - 1)), and the ratio of the tensor's maximum to its median magnitude."""
    x = torch.as_tensor(x).double()
    mean = x.mean(-1, keepdim=True)
    std = x.var(-1, unbiased=False, keepdim=True).sqrt()
    ratio = (mean.abs() / std.clamp(min=1e-300)).flatten()
    z = (x - mean) * (x.var(-1, unbiased=False, keepdim=True) + esr.CFG.norm_eps).rsqrt()
    return {"min_mean_over_std": float(ratio.min()), "max_mean_over_std": float(ratio.max()),
            "max_normalised": float(z.abs().max()), "sqrt_C_minus_1": math.sqrt(x.shape[-1] - 1),
            "max_over_median": float(x.abs().max() / x.abs().median().clamp(min=1e-300))}


class CalibratingArith(esr.Arith):
    """f16x3 arithmetic that keeps the scale the calibration rule gives each plane tensor the first time it sees it."""

    def __init__(self):
        super().__init__("f16x3")

    def scale(self, slot, t):
        if slot not in self.scales:
            self.scales[slot] = esr.pow2_floor_scale(float(torch.as_tensor(t).abs().max()), 7)
        return float(self.scales[slot])


def speech_scales(sd, taps) -> Dict[str, float]:
    """{slot: scale} of the calibration rule on ``taps`` (the chained stages on full-level speech)."""
    ar = CalibratingArith()
    for name, st in esr.STAGES.items():
        esr.measure(name, [taps[s] for s in st.source], sd, ar, f32=taps[name])
    return dict(ar.scales)
