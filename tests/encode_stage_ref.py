"""Test infrastructure only (CPU): float64 references of the ENCODE path one stage at a time, each evaluated on the
tap(s) the engine itself read (engine.cpp encode_pass, save_tap / save_tap_planes), next to its condition sum.  The
metric, its two conditions and their helpers are decode's (tests/decode_stage_ref.py: ``q_metric``, ``worst_element``,
``rel_err``, ``working_bound``, ``failures``, ``U``, ``WORKING_FACTOR``), imported, not copied:

    q = max over elements of |got - ref64| / (2^-24 * mag64)

The stages are built from oracle/mimi_ref.py (``causal_conv1d``, ``rope_cos_sin``, ``rotate_half``, ``attention``) and the
layer text of its ``transformer`` (F.layer_norm, F.linear, F.gelu in the same order); tests/test_encode_stage_ref.py
chains them and compares the end with ``mimi_ref.encode``.  All tensors are channel-last ``[B, T, C]`` as the engine's
taps are (audio: ``[B, L]``); a stage's input is a tuple of taps (``Stage.source``).

Stages (output tap <- inputs: operation; n = accumulated terms + epilogue operations, the hard bound of f32 mode)
    conv0          <- audio: conv k = 7 (a kernel of its own that only taps run, fp32 in every mode)      n = 7 + 2
    res{s}_elu     <- down{s-1} (s = 0: AUDIO -- the stage-0 block recomputes conv 0 from the audio in every mode,
                      it never reads the conv0 tap; its float64 stage is conv 0 followed by the block):
                      ELU(x + b1 + W1 . ELU(b3 + W3 (*) ELU(x)))         n = [9 +] (3C + 2) + (C/2 + 2) + 3 x 3 + 1
    h{s}, s >= 2   <- down{s-1}: ELU(b3 + W3 (*) ELU(x)), the first GEMM of an unfused block (plane modes only: the
                      engine taps h between the two GEMMs of stages 2 and 3)                  n = (3C + 2) + 2 x 3
    res{s}_k1      <- h{s}, down{s-1}: ELU(x + b1 + W1 . h), the second GEMM; its output is the res{s}_elu tap
                                                                                          n = (C/2 + 2) + 1 + 3
    down{s}, s < 3 <- res{s}_elu: strided conv on an input that already is ELU'd                         n = K + 2
    down3_elu      <- res3_elu: the same + ELU                                                           n = K + 2 + 3
    encoder        <- down3_elu: conv k = 3                                                              n = K + 2
    qkv{l}         <- encoder / xfmr{l-1}: LayerNorm, q/k/v, RoPE on q and k           n = (C + 4) + (C + 2) + 3
    att{l}         <- qkv{l}: causal window-250 attention, scale 1/8                   n = (64 + 2) + 2 x 250 + 6
    oproj{l}       <- att{l}, encoder / xfmr{l-1}: x + ls1 (Wo a)                                        n = K + 2
    ff{l}          <- oproj{l}: GELU(W1 LayerNorm(x))                                  n = (C + 4) + (C + 2) + 17
    xfmr{l}        <- ff{l}, oproj{l}: x + ls2 (W2 h)                                                    n = K + 2
    ds_gemm        <- xfmr7: k = 4, s = 2 conv zero-padded; only its interior rows are compared
                      (``Stage.interior``, ``ds_interior``: the rows that read no padding)      n = K + 2
    downsample     <- xfmr7: the same conv replicate-padded at each item's ends                          n = K + 2
    proj           <- downsample: [W_sem | W_ac] input projections                                       n = K + 2
(K = taps x input channels.)  RVQ is not here: proj -> codes is audited in float64 by tests/rvq_ref.py and
tests/test_rvq_kernels.py (adversarial residuals and codebooks on every kernel form), beside the bit-exact quantizer
tests on natural embeddings (tests/test_gpu_parity.py).

CONDITION SUMS (derived, not fitted).  A stage's mag64 bounds, element by element, the first-order error of ANY
evaluation of it in units of u = 2^-24: every partial result's rounding error is at most its own n_i u times a
magnitude that mag64 dominates, so the total is at most (sum n_i) u mag64 = n u mag64.
  * sum of products + bias: sum |a||w| + |b|  (as decode's).
  * ELU.  elu_fast (kernels.h) is exp(z) - 1 for z < 0 in every mode, and the f16x3 block kernels form ELU(z) s as
    exp(z) s - s: the evaluation error is relative to exp(z) + 1, not to |ELU(z)|.  Three units:
    the argument product z log2(e) moves exp(z) by u |z| e^z <= 0.37 u, v_exp_f32 is within 1 ulp = 2 u e^z, the
    subtraction rounds once (u |e^z - 1| <= u): <= 3 u (e^z + 1).  An ELU of an exact tap therefore enters the next
    sum with the condition  z (z >= 0),  e^z + 1 (z < 0);  an ELU of a computed z whose own condition sum is m_z
    enters with  m_z + [z < 0] (e^z + 1):  ELU is 1-Lipschitz (its derivative is 1 or e^z <= 1), so z's error
    passes at most unchanged.
  * LayerNorm.  The kernel evaluates (v rstd - rstd mean) g + b (kernels.h ln_affine): per element
    (|v| + |mean|) rstd |g| + |b|, composed through the following GEMM's |W|.  n = C + 4: the C-term reductions
    behind mean and rstd and the four operations of ln_affine.
  * RoPE: q cos + rot(q) sin -> m_q |cos| + swap(m_q) |sin|, 3 operations.
  * residual / layer-scale epilogue: |x| + |ls| sum |a||w|.
  * GELU.  1.129-Lipschitz (sup of Phi(x) + x phi(x), attained at x = sqrt 2: 0.92135 + 1.41421 x 0.14676), so
    GELU(z) has the condition 1.129 m_z + |z|; the second term carries the evaluation, 17 units of it: the bounds
    tests/test_gelu.py asserts for gelu_fast (1e-6 relative for |x| < 2, 3e-7 for x >= 2, 1e-7 absolute for x <= -2)
    are at most 1e-6 |x| = 16.8 u |x|.
  * attention, per (row i, head, dim d).  Scores s_ij = q_i . k_j / 8 have the condition S_ij = sum_d |q||k| / 8 and
    n_s = 64 + 2.  A score error e_j moves the softmax weight p_j by p_j (e_j - sum_m p_m e_m), so the output moves by
    at most sum_j p_j (S_ij + Sbar_i) |v_jd| units of n_s, Sbar_i = sum_m p_m S_im.  The exponentials, the
    normaliser (<= 250 terms) and the P V sum (<= 250 terms) add 2 x 250 + 6 units of sum_j p_j |v_jd| (the
    argument's rounding u |s_j - max| p_j <= u / e is inside the 6).  mag = sum_j p_j (1 + S_ij + Sbar_i) |v_jd|.

HARD condition  q <= n + c,  c by precision mode (``Arith``):
  * f32: c = 0.
  * f16x3 (engine.cpp "Activation scales", kernels.h split2_f16s): each operand is hi + lo in fp16 at a per-tensor
    power-of-two scale s, relative error <= 2^-22 down to 2^-3 / s and absolute error <= 2^-25 / s below, so the
    condition sum is taken on max(|a|, 2^-3 / s) (``Arith.fa``; s from ``MimiHipModel.act_scales()``, or the
    calibration rule max|a| s in [2^7, 2^8) where no engine is at hand) and on max(|w|, 2^-3 / s_w) with s_w the
    upload's max|w| s_w in [2^13, 2^14) (``Arith.fw``).  The lo x lo product is dropped: <= 2^-22 |a||w|.  Together
    3 x 2^-22 = 12 units per term, i.e. c = 12 per sum-of-products layer of the stage (``Stage.gemms``: 1 for a conv
    or linear, 2 for a residual block, 3 for the stage-0 block with its conv 0; attention's two products each act on
    their own part of mag, so 12 once), + 4 where the output tap is itself a planes tensor (its own split, 2^-22
    relative: ``Stage.planes_out``).  The attention kernels split q, k, v and p at scales of their own (attn_h16.h
    pow2_scale: the maximum at [2^13, 2^14); p at 2^14): the same 12, floors 2^-17 of the head's maximum.
  * bf16x6: three bf16 planes leave <= 2^-27 |a| per operand (2^-9 per plane), the three dropped products of nine
    <= 2 x 2^-27 + 2^-36: under one unit in all, c = 1 per layer, + 1 for a planes output.
WORKING condition  q <= 16 max(q_ref, 1)  (decode's factor): q_ref is torch-CPU's fp32 evaluation of the stage on the
same input; in f16x3 mode the larger of that and ``q_emul``, a CPU emulation of the stage's f16x3 arithmetic for the
sum-of-products stages (the halves of the unfused blocks, down convs, final conv, o_proj, fc2, downsample, input
projections): both operands split as
above at the engine's scales, three products summed exactly, the epilogue in float64.  Attention, the LayerNorm
prologues and the residual blocks are not emulated: q_ref alone.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from decode_stage_ref import U, WORKING_FACTOR, failures, q_metric, rel_err, working_bound, worst_element  # noqa: F401
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

CFG = RefConfig()
GELU_LIP = 1.129
N_ELU, N_GELU, N_ROPE = 3, 17, 3
MODES = ("f32", "bf16x6", "f16x3")


def pow2_floor_scale(mx: float, top: int) -> float:
    """The power of two s with mx s in [2^top, 2^(top + 1)) (1 for mx = 0)."""
    return 2.0 ** (top - math.floor(math.log2(mx))) if mx > 0 and math.isfinite(mx) else 1.0


class Arith:
    """The arithmetic of one precision mode: c per layer / planes output, the operand floors, the scales."""

    def __init__(self, mode: str = "f32", scales: Optional[Dict[str, float]] = None):
        assert mode in MODES, mode
        self.mode = mode
        self.scales = dict(scales or {})
        self.c_term = {"f32": 0, "bf16x6": 1, "f16x3": 12}[mode]
        self.c_out = {"f32": 0, "bf16x6": 1, "f16x3": 4}[mode]

    @property
    def h16(self):
        return self.mode == "f16x3"

    def scale(self, slot: str, t) -> float:
        """The fixed scale of plane tensor ``slot`` (the engine's), else the calibration rule on t itself."""
        if slot in self.scales:
            return float(self.scales[slot])
        return pow2_floor_scale(float(t.abs().max()), 7)

    @staticmethod
    def wscale(w) -> float:
        return pow2_floor_scale(float(w.abs().max()), 13)  # engine.cpp f16_weight_scale

    def fa(self, slot: str, a_abs, t=None):
        """|a| floored at 2^-3 / s in f16x3 mode (t: the tensor whose planes the kernel forms, default a itself)."""
        if not self.h16:
            return a_abs
        return a_abs.clamp(min=2.0 ** -3 / self.scale(slot, a_abs if t is None else t))

    def fw(self, w_abs):
        return w_abs.clamp(min=2.0 ** -3 / self.wscale(w_abs)) if self.h16 else w_abs


def split_f16(v, s: float):
    """kernels.h split2_f16s in exact arithmetic: hi = RN16(v s), lo = RN16(v s - hi); returned as float64."""
    t = (v.double() * s).float()
    hi = t.half()
    lo = (t.double() - hi.double()).float().half()
    return hi.double(), lo.double()


def f16x3_product(op: Callable, a, w, sa: float, sw: float, hook: Optional[Callable] = None):
    """op(a, w) (bilinear, no bias) in the engine's f16x3 arithmetic: hi hi + hi lo + lo hi, summed in float64.
    ``hook(a_hi, a_lo, w_hi, w_lo)`` (tests) returns the four planes to use instead: w_lo only meets a_hi, so a zeroed
    part of w_lo is the w_lo a_hi cross product dropped there."""
    ah, al = split_f16(a, sa)
    wh, wl = split_f16(w, sw)
    if hook is not None:
        ah, al, wh, wl = hook(ah, al, wh, wl)
    return (op(ah, wh) + op(ah, wl) + op(al, wh)) / (sa * sw)


def _w(sd, key, dtype=torch.float64):
    return torch.as_tensor(sd[key]).to(dtype)


def _cf(x):
    return x.transpose(1, 2)


def elu_cond(z, mz=None):
    """The condition of ELU(z) as an operand: of an exact z, or of a computed z with condition sum mz."""
    ev = torch.where(z < 0, z.exp() + 1.0, torch.zeros_like(z))
    return torch.where(z < 0, ev, z) if mz is None else mz + ev


def _conv(x_cf, w, b, stride=1, pad_mode="constant"):
    return mimi_ref.causal_conv1d(x_cf, w, b, stride=stride, pad_mode=pad_mode)


# ---- SEANet ---------------------------------------------------------------------------------------------------------
P0 = "encoder.layers.0.conv."


def _res_keys(s):
    p = f"encoder.layers.{1 + 3 * s}.block."
    return p + "1.conv.", p + "3.conv."


def _down_key(s):
    return f"encoder.layers.{3 + 3 * s}.conv."


PF = f"encoder.layers.{3 * len(CFG.upsampling_ratios) + 2}.conv."
RATIOS = list(reversed(CFG.upsampling_ratios))
UNFUSED_FROM = 2   # engine.cpp kUnfuseFrom: from this stage on the plane modes run a block as two GEMMs
HALVES = [n for s in range(UNFUSED_FROM, len(RATIOS)) for n in (f"h{s}", f"res{s}_k1")]  # plane modes only


def conv0_value(xs, sd, dtype):
    return _cf(_conv(xs[0].to(dtype)[:, None], _w(sd, P0 + "weight", dtype), _w(sd, P0 + "bias", dtype)))


def conv0_cond(xs, sd, ar, slot=None):
    a = xs[0].double().abs()[:, None]
    wa = _w(sd, P0 + "weight").abs()
    if slot:
        a, wa = ar.fa(slot, a), ar.fw(wa)
    return _cf(_conv(a, wa, _w(sd, P0 + "bias").abs()))


def res_value(s):
    k3, k1 = _res_keys(s)

    def f(xs, sd, dtype):
        x = _cf(conv0_value(xs, sd, dtype)) if s == 0 else _cf(xs[0].to(dtype))
        h = _conv(F.elu(x), _w(sd, k3 + "weight", dtype), _w(sd, k3 + "bias", dtype))
        h = _conv(F.elu(h), _w(sd, k1 + "weight", dtype), _w(sd, k1 + "bias", dtype))
        return _cf(F.elu(x + h))
    return f


def res_cond(s):
    k3, k1 = _res_keys(s)
    xslot, hslot = {0: ("s0.x", "s0.h"), 1: ("s1.x", "s1.h")}.get(s, (f"xe{s}", f"h{s}"))

    def f(xs, sd, ar):
        if s == 0:
            x = _cf(conv0_value(xs, sd, torch.float64))
            mx = _cf(conv0_cond(xs, sd, ar, "s0.audio"))
            ax = elu_cond(x, mx)
        else:
            x = _cf(xs[0].double())
            mx = x.abs()
            ax = elu_cond(x)
        ax = ar.fa(xslot, ax, F.elu(x))
        w3, b3, w1, b1 = (_w(sd, k3 + "weight"), _w(sd, k3 + "bias"), _w(sd, k1 + "weight"), _w(sd, k1 + "bias"))
        h = _conv(F.elu(x), w3, b3)
        mh = _conv(ax, ar.fw(w3.abs()), b3.abs())
        ah = ar.fa(hslot, elu_cond(h, mh), F.elu(h))
        z = x + _conv(F.elu(h), w1, b1)
        mz = mx + _conv(ah, ar.fw(w1.abs()), b1.abs())
        return _cf(elu_cond(z, mz))
    return f


def res_n(s):
    k3, k1 = _res_keys(s)

    def f(sd):
        w3, w1 = sd[k3 + "weight"], sd[k1 + "weight"]
        n = (int(w3.shape[1] * w3.shape[2]) + 2) + (int(w1.shape[1] * w1.shape[2]) + 2) + 3 * N_ELU + 1
        return n + (CFG.kernel_size + 2 if s == 0 else 0)
    return f


def res_halves(s):
    """The two GEMMs of an unfused block (stages 2 and 3 in the plane modes), each on its own input tap:
    h = ELU(b3 + W3 (*) ELU(x)) from x, and y = ELU(x + b1 + W1 . h) from (h, x).  As one stage the block hides its k3
    conv: a fault there reaches y through W1 with random signs (~ sqrt(C / 2) of its C / 2 terms) while the condition sum
    composes all C / 2, beside the skip -- 10 x or more of dilution.  -> ((value, cond, n, emul), (value, cond, n, emul))"""
    k3, k1 = _res_keys(s)

    def h_value(xs, sd, dtype):
        x = _cf(xs[0].to(dtype))
        return _cf(F.elu(_conv(F.elu(x), _w(sd, k3 + "weight", dtype), _w(sd, k3 + "bias", dtype))))

    def h_cond(xs, sd, ar):
        x = _cf(xs[0].double())
        w3, b3 = _w(sd, k3 + "weight"), _w(sd, k3 + "bias")
        mh = _conv(ar.fa(f"xe{s}", elu_cond(x), F.elu(x)), ar.fw(w3.abs()), b3.abs())
        return _cf(elu_cond(_conv(F.elu(x), w3, b3), mh))

    def h_n(sd):
        w3 = sd[k3 + "weight"]
        return int(w3.shape[1] * w3.shape[2]) + 2 + 2 * N_ELU

    def h_emul(xs, sd, ar, hook=None):
        a, w3 = F.elu(_cf(xs[0].double())), _w(sd, k3 + "weight")
        y = f16x3_product(lambda a_, w_: _conv(a_, w_, None), a, w3, ar.scale(f"xe{s}", a), ar.wscale(w3), hook)
        return _cf(F.elu(y + _w(sd, k3 + "bias")[None, :, None]))

    def y_value(xs, sd, dtype):
        h, x = _cf(xs[0].to(dtype)), _cf(xs[1].to(dtype))
        return _cf(F.elu(x + _conv(h, _w(sd, k1 + "weight", dtype), _w(sd, k1 + "bias", dtype))))

    def y_cond(xs, sd, ar):
        h, x = _cf(xs[0].double()), _cf(xs[1].double())
        w1, b1 = _w(sd, k1 + "weight"), _w(sd, k1 + "bias")
        mz = x.abs() + _conv(ar.fa(f"h{s}", h.abs()), ar.fw(w1.abs()), b1.abs())
        return _cf(elu_cond(x + _conv(h, w1, b1), mz))

    def y_n(sd):
        w1 = sd[k1 + "weight"]
        return int(w1.shape[1] * w1.shape[2]) + 2 + 1 + N_ELU

    def y_emul(xs, sd, ar, hook=None):
        h, x, w1 = _cf(xs[0].double()), _cf(xs[1].double()), _w(sd, k1 + "weight")
        y = f16x3_product(lambda a_, w_: _conv(a_, w_, None), h, w1, ar.scale(f"h{s}", h), ar.wscale(w1), hook)
        return _cf(F.elu(x + y + _w(sd, k1 + "bias")[None, :, None]))
    return (h_value, h_cond, h_n, h_emul), (y_value, y_cond, y_n, y_emul)


def conv_stage(key, slot, stride=1, elu_out=False, pad_mode="constant", bias=True):
    """A conv on an input that already is ELU'd: (value, cond, n, emul)."""
    def wb(sd, dtype):
        return _w(sd, key + "weight", dtype), (_w(sd, key + "bias", dtype) if bias else None)

    def value(xs, sd, dtype):
        w, b = wb(sd, dtype)
        y = _conv(_cf(xs[0].to(dtype)), w, b, stride, pad_mode)
        return _cf(F.elu(y) if elu_out else y)

    def cond(xs, sd, ar):
        w, b = wb(sd, torch.float64)
        x = _cf(xs[0].double())
        m = _conv(ar.fa(slot, x.abs()), ar.fw(w.abs()), None if b is None else b.abs(), stride, pad_mode)
        return _cf(elu_cond(_conv(x, w, b, stride, pad_mode), m) if elu_out else m)

    def n(sd):
        w = sd[key + "weight"]
        return int(w.shape[1] * w.shape[2]) + 2 + (N_ELU if elu_out else 0)

    def emul(xs, sd, ar, hook=None):
        w, b = wb(sd, torch.float64)
        x = _cf(xs[0].double())
        y = f16x3_product(lambda a_, w_: _conv(a_, w_, None, stride, pad_mode), x, w, ar.scale(slot, x), ar.wscale(w), hook)
        if b is not None:
            y = y + b[None, :, None]
        return _cf(F.elu(y) if elu_out else y)
    return value, cond, n, emul


# ---- transformer ----------------------------------------------------------------------------------------------------
def _lp(l):
    return f"encoder_transformer.layers.{l}."


def ln_value(x, sd, pre, dtype):
    return F.layer_norm(x.to(dtype), (x.shape[-1],), _w(sd, pre + "weight", dtype), _w(sd, pre + "bias", dtype), CFG.norm_eps)


def ln_cond(x, sd, pre):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + CFG.norm_eps).rsqrt()
    return (x.abs() + mean.abs()) * rstd * _w(sd, pre + "weight").abs() + _w(sd, pre + "bias").abs()


def _rope_tables(pos, dtype):
    """cos / sin [T, D] of the reference (its fp32 tables are part of the model) at positions ``pos``."""
    cos, sin = mimi_ref.rope_cos_sin(int(pos.max()) + 1, CFG)
    return cos[0, pos].to(dtype)[None, :, None, :], sin[0, pos].to(dtype)[None, :, None, :]


def _swap_halves(x):
    h = x.shape[-1] // 2
    return torch.cat((x[..., h:], x[..., :h]), dim=-1)


def qkv_value(l):
    p = _lp(l)

    def f(xs, sd, dtype):
        x = xs[0]
        B, T, C = x.shape
        H, D = CFG.num_attention_heads, CFG.head_dim
        cos, sin = _rope_tables(torch.arange(T), dtype)
        h = ln_value(x, sd, p + "input_layernorm.", dtype)
        out = []
        for name in ("q", "k", "v"):
            t = F.linear(h, _w(sd, p + f"self_attn.{name}_proj.weight", dtype)).view(B, T, H, D)
            if name != "v":
                t = (t * cos) + (mimi_ref.rotate_half(t) * sin)
            out.append(t.reshape(B, T, H * D))
        return torch.cat(out, dim=-1)
    return f


def qkv_cond(l):
    p = _lp(l)

    def f(xs, sd, ar):
        x = xs[0].double()
        B, T, C = x.shape
        H, D = CFG.num_attention_heads, CFG.head_dim
        cos, sin = _rope_tables(torch.arange(T), torch.float64)
        mh = ar.fa(f"xf{l}.ln1", ln_cond(x, sd, p + "input_layernorm."), ln_value(x, sd, p + "input_layernorm.", torch.float64))
        wall = torch.cat([_w(sd, p + f"self_attn.{n}_proj.weight") for n in ("q", "k", "v")]).abs()
        wall = ar.fw(wall)
        out = []
        for i, name in enumerate(("q", "k", "v")):
            m = F.linear(mh, wall[i * H * D:(i + 1) * H * D]).view(B, T, H, D)
            if name != "v":  # |cos|, |sin| do not depend on the sign of the position; their size does on its value
                m = m * cos.abs() + _swap_halves(m) * sin.abs()
            out.append(m.reshape(B, T, H * D))
        return torch.cat(out, dim=-1)
    return f


def heads(x):
    """qkv tap [B, T, 3 H D] -> q, k, v [B, H, T, D]"""
    B, T, _ = x.shape
    H, D = CFG.num_attention_heads, CFG.head_dim
    t = x.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _window_cfg(window=None):
    return CFG if window is None else dataclasses.replace(CFG, sliding_window=int(window))


def att_value(xs, sd, dtype, window=None):
    """``window``: the sliding window (None: the module's ``CFG``, what the encode stages use)."""
    q, k, v = heads(xs[0].to(dtype))
    B, H, T, D = q.shape
    return mimi_ref.attention(q, k, v, _window_cfg(window)).transpose(1, 2).contiguous().reshape(B, T, H * D)


def att_mask(T, window=None):
    window = CFG.sliding_window if window is None else window
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return (j <= i) & (j > i - window)


def att_cond(xs, sd, ar, window=None):
    q, k, v = heads(xs[0].double())
    B, H, T, D = q.shape
    scale = 1.0 / math.sqrt(D)
    mask = att_mask(T, window)
    aq, ak, av = q.abs(), k.abs(), v.abs()
    pfloor = 0.0
    if ar.h16:  # the kernels' own plane scales: the maximum at [2^13, 2^14) -> floors 2^-17 of each head's maximum
        aq, ak, av = (t.clamp(min=t.amax(dim=(-1, -2), keepdim=True) * 2.0 ** -16) for t in (aq, ak, av))
        pfloor = 2.0 ** -17
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
    S = (aq @ ak.transpose(-1, -2)) * scale
    sbar = (p * S).sum(-1, keepdim=True)
    pf = p.clamp(min=pfloor).masked_fill(~mask, 0.0)
    m = (pf * (1.0 + S + sbar)) @ av
    return m.transpose(1, 2).contiguous().reshape(B, T, H * D)


def att_n(window=None) -> int:
    """The attention stage's hard bound: the score's 64 + 2, two sums of at most ``window`` terms, 6 operations."""
    return (CFG.head_dim + 2) + 2 * _window_cfg(window).sliding_window + 6


def att_stage(window=None):
    """(value, cond, n) of the attention stage at a sliding window of its own (None: ``CFG``'s)."""
    if window is None:
        return att_value, att_cond, lambda sd: att_n()
    return (lambda xs, sd, dtype: att_value(xs, sd, dtype, window), lambda xs, sd, ar: att_cond(xs, sd, ar, window),
            lambda sd: att_n(window))


DECODER_PREFIX, ENCODER_PREFIX = "decoder_transformer.", "encoder_transformer."


def decoder_view(sd):
    """The decoder transformer's weights under the encoder transformer's names, which every transformer stage here
    reads: the renaming view of ``decode_ref.decoder_transformer`` (the tensors are shared, not copied)."""
    return {ENCODER_PREFIX + k[len(DECODER_PREFIX):]: v for k, v in sd.items() if k.startswith(DECODER_PREFIX)}


def linear_res_stage(l, wkey, lskey, slot):
    """x + ls (W a): inputs (a, x)."""
    p = _lp(l)

    def value(xs, sd, dtype):
        return xs[1].to(dtype) + _w(sd, p + lskey, dtype) * F.linear(xs[0].to(dtype), _w(sd, p + wkey, dtype))

    def cond(xs, sd, ar):
        w = _w(sd, p + wkey)
        return xs[1].double().abs() + _w(sd, p + lskey).abs() * F.linear(ar.fa(slot, xs[0].double().abs()), ar.fw(w.abs()))

    def n(sd):
        return int(sd[p + wkey].shape[1]) + 2

    def emul(xs, sd, ar, hook=None):
        a, w = xs[0].double(), _w(sd, p + wkey)
        y = f16x3_product(F.linear, a, w, ar.scale(slot, a), ar.wscale(w), hook)
        return xs[1].double() + _w(sd, p + lskey) * y
    return value, cond, n, emul


def ff_value(l, gelu=F.gelu):
    p = _lp(l)

    def f(xs, sd, dtype):
        return gelu(F.linear(ln_value(xs[0], sd, p + "post_attention_layernorm.", dtype), _w(sd, p + "mlp.fc1.weight", dtype)))
    return f


def ff_cond(l):
    p = _lp(l)

    def f(xs, sd, ar):
        x = xs[0].double()
        h = ln_value(x, sd, p + "post_attention_layernorm.", torch.float64)
        w = _w(sd, p + "mlp.fc1.weight")
        mz = F.linear(ar.fa(f"xf{l}.ln2", ln_cond(x, sd, p + "post_attention_layernorm."), h), ar.fw(w.abs()))
        return GELU_LIP * mz + F.linear(h, w).abs()
    return f


def proj_weight(sd, dtype=torch.float64):
    return torch.cat([_w(sd, f"quantizer.{h}_residual_vector_quantizer.input_proj.weight", dtype)
                      for h in ("semantic", "acoustic")])


def proj_stage():
    def value(xs, sd, dtype):
        return F.linear(xs[0].to(dtype), proj_weight(sd, dtype)[..., 0])

    def cond(xs, sd, ar):
        return F.linear(ar.fa("ds.out", xs[0].double().abs()), ar.fw(proj_weight(sd)[..., 0].abs()))

    def n(sd):
        return int(proj_weight(sd).shape[1]) + 2

    def emul(xs, sd, ar, hook=None):
        a, w = xs[0].double(), proj_weight(sd)[..., 0]
        return f16x3_product(F.linear, a, w, ar.scale("ds.out", a), ar.wscale(w), hook)
    return value, cond, n, emul


def ds_interior(T_in: int, T_out: int) -> slice:
    """The output rows of the k = 4, s = 2 downsample that read no padding: not row 0 (two rows of left padding), and
    not the last one when the input length is odd (one row of right padding)."""
    extra = mimi_ref.extra_padding(T_in, 4, 2)
    return slice(1, T_out - (1 if extra > 0 else 0))


# ---- the table ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Stage:
    name: str
    source: Tuple[str, ...]      # the input taps ("audio": the samples)
    value: Callable              # value(xs, sd, dtype) -> [B, T, C]
    cond: Callable               # cond(xs, sd, ar) -> mag64
    n: Callable                  # n(sd) -> the f32 hard bound
    gemms: int = 1               # sum-of-products layers an f16x3 / bf16x6 mode runs on planes
    planes_out: bool = False     # the output tap is a planes tensor in the plane modes
    emul: Optional[Callable] = None   # emul(xs, sd, ar) -> the f16x3 arithmetic's float64 result
    interior: bool = False       # only ds_interior rows are defined
    tap: str = ""                # the output tap where it is not ``name`` (res{s}_k1 writes res{s}_elu)

    @property
    def out(self) -> str:
        return self.tap or self.name

    def ref(self, xs, sd, ar):
        """(ref64, mag64)"""
        with torch.no_grad():
            return self.value(xs, sd, torch.float64), self.cond(xs, sd, ar)

    def f32(self, xs, sd):
        with torch.no_grad():
            return self.value(xs, sd, torch.float32)

    def c(self, ar: Arith) -> int:
        return ar.c_term * self.gemms + (ar.c_out if self.planes_out else 0)


XFMR_STAGES = ("qkv", "att", "oproj", "ff", "xfmr")   # the five stages of a transformer layer, in order


def transformer_stages(first: str, window=None) -> Dict[str, Stage]:
    """The 5 stages of each of the 8 layers; layer 0 reads the tap ``first``, attention has the sliding window
    ``window`` (None: ``CFG``'s).  The weights are read under the encoder transformer's names (``decoder_view``)."""
    st: Dict[str, Stage] = {}
    av, ac, an = att_stage(window)
    for l in range(CFG.num_hidden_layers):
        x = first if l == 0 else f"xfmr{l - 1}"
        C = CFG.hidden_size
        st[f"qkv{l}"] = Stage(f"qkv{l}", (x,), qkv_value(l), qkv_cond(l), lambda sd, C=C: (C + 4) + (C + 2) + N_ROPE)
        st[f"att{l}"] = Stage(f"att{l}", (f"qkv{l}",), av, ac, an, planes_out=True)
        v, c, n, e = linear_res_stage(l, "self_attn.o_proj.weight", "self_attn_layer_scale.scale", f"xf{l}.att")
        st[f"oproj{l}"] = Stage(f"oproj{l}", (f"att{l}", x), v, c, n, emul=e)
        st[f"ff{l}"] = Stage(f"ff{l}", (f"oproj{l}",), ff_value(l), ff_cond(l),
                             lambda sd, C=C: (C + 4) + (C + 2) + N_GELU, planes_out=True)
        v, c, n, e = linear_res_stage(l, "mlp.fc2.weight", "mlp_layer_scale.scale", f"xf{l}.ff")
        st[f"xfmr{l}"] = Stage(f"xfmr{l}", (f"ff{l}", f"oproj{l}"), v, c, n, emul=e)
    return st


def _stages() -> Dict[str, Stage]:
    st: Dict[str, Stage] = {}
    st["conv0"] = Stage("conv0", ("audio",), conv0_value, conv0_cond, lambda sd: CFG.kernel_size + 2, gemms=0)
    for s, r in enumerate(RATIOS):
        st[f"res{s}_elu"] = Stage(f"res{s}_elu", ("audio",) if s == 0 else (f"down{s - 1}",), res_value(s), res_cond(s),
                                  res_n(s), gemms=3 if s == 0 else 2, planes_out=True)
        if s >= UNFUSED_FROM:  # the plane modes run these blocks as two GEMMs and tap h between them
            (hv, hc, hn, he), (yv, yc, yn, ye) = res_halves(s)
            st[f"h{s}"] = Stage(f"h{s}", (f"down{s - 1}",), hv, hc, hn, planes_out=True, emul=he)
            st[f"res{s}_k1"] = Stage(f"res{s}_k1", (f"h{s}", f"down{s - 1}"), yv, yc, yn, planes_out=True, emul=ye,
                                     tap=f"res{s}_elu")
        last = s == len(RATIOS) - 1
        v, c, n, e = conv_stage(_down_key(s), f"y{s}", stride=r, elu_out=last)
        name = f"down{s}_elu" if last else f"down{s}"
        st[name] = Stage(name, (f"res{s}_elu",), v, c, n, planes_out=last, emul=e)
    v, c, n, e = conv_stage(PF, "x_last")
    st["encoder"] = Stage("encoder", (f"down{len(RATIOS) - 1}_elu",), v, c, n, emul=e)
    st.update(transformer_stages("encoder"))
    last = f"xfmr{CFG.num_hidden_layers - 1}"
    v, c, n, e = conv_stage("downsample.conv.", "ds.in", stride=2, bias=False)
    st["ds_gemm"] = Stage("ds_gemm", (last,), v, c, n, emul=e, interior=True)
    v, c, n, e = conv_stage("downsample.conv.", "ds.in", stride=2, bias=False, pad_mode="replicate")
    st["downsample"] = Stage("downsample", (last,), v, c, n, emul=e)
    v, c, n, e = proj_stage()
    st["proj"] = Stage("proj", ("downsample",), v, c, n, emul=e)
    return st


STAGES = _stages()


def chain_f32(audio, sd, names=None) -> Dict[str, torch.Tensor]:
    """Every stage's fp32 value from the audio on, each on the fp32 value of its inputs: {tap: tensor} (with "audio")."""
    taps = {"audio": torch.as_tensor(audio).float()}
    with torch.no_grad():
        for name, st in STAGES.items():
            if names is not None and name not in names:
                continue
            taps[name] = st.f32([taps[s] for s in st.source], sd)
    return taps


def measure(name: str, xs, sd, ar: Arith, got=None, f32=None, stages=None) -> dict:
    """One stage on inputs xs: n, c, q_ref (torch-CPU fp32, or the given ``f32`` evaluation), q_emul (f16x3 mode, the
    emulated stages), and q_engine / worst when ``got`` is given.  ``stages``: another table than ``STAGES``."""
    st = (STAGES if stages is None else stages)[name]
    xs = [torch.as_tensor(x) for x in xs]
    ref64, mag64 = st.ref(xs, sd, ar)
    rows = slice(None)
    if st.interior:
        rows = ds_interior(xs[0].shape[1], ref64.shape[1])
        ref64, mag64 = ref64[:, rows], mag64[:, rows]
    f32 = st.f32(xs, sd) if f32 is None else f32
    rec = {"stage": name, "mode": ar.mode, "n": int(st.n(sd)), "c": int(st.c(ar)),
           "q_ref": q_metric(f32[:, rows], ref64, mag64), "q_emul": None}
    if ar.h16 and st.emul is not None:
        with torch.no_grad():
            rec["q_emul"] = q_metric(st.emul(xs, sd, ar)[:, rows], ref64, mag64)
    if got is not None:
        got = torch.as_tensor(got)[:, rows]
        rec["q_engine"] = q_metric(got, ref64, mag64)
        rec["worst"] = list(worst_element(got, ref64, mag64))
    return rec


def conditions(rec: dict, key: str = "q_engine") -> list:
    """The conditions that rec[key] misses (empty: both hold): decode's ``failures`` on n + c and on the larger of
    q_ref and q_emul."""
    return failures({"stage": f"{rec['stage']} [{rec['mode']}]", "n": rec["n"] + rec["c"],
                     "q_ref": max(rec["q_ref"], rec["q_emul"] or 0.0), key: rec[key]}, key=key)
