"""Test infrastructure only (CPU): float64 references of the decode path ONE STAGE AT A TIME, and the metric that
compares a stage's output with them element by element.

``tests/decode_ref.py`` restates the whole decode; a stage tap compared with it carries the error of every stage before
it, and the project metric (``max|err| / max|ref|``) hides a wrong element under the tensor's largest one.  Here each
stage is evaluated on the tensor the implementation under test itself read (the previous tap), in float64, next to its
CONDITION SUM

    mag64 = sum |a| |w| + |b|      (the same stage on |input|, |weights|, |bias|, ELU replaced by the identity, which
                                    is exact on these non-negative values)

and the metric is

    q = max over elements of |got - ref64| / (2^-24 * mag64)

the error in units of one fp32 rounding of the element's own condition sum.  Two conditions on q:

* HARD   ``q <= n``: n = accumulated terms + epilogue operations.  The textbook worst case of fp32 summation,
  |fl(sum) - sum| <= n u sum|a||w| to first order in u = 2^-24, holds for every summation order, with or without FMA,
  so no correct fp32 kernel exceeds it.  n per stage (``Stage.n``):
      conv, K = taps x input channels, bias: K + 2                    (K - 1 adds + bias + store, rounded up)
      decoder conv 0 with its ELU epilogue (``dconv0_elu``): K + 3    (ELU is 1-Lipschitz; + its own evaluation)
      residual block: (3C + 2) + (C/2 + 2) + 4                        (its two convs; ELU is 1-Lipschitz, so the first
                      conv's error passes through |W1| at most unchanged, which is what mag64 composes; + the three
                      ELU evaluations and the residual add)
      depthwise upsample: 2 + 2                                       (two products, one add, no bias)
      quantizer: 2 Dq + K + 2                                         (K - 2 gather adds in all, through a 2 Dq-term
                      projection whose condition sum is composed the same way)
* WORKING  ``q <= 16 * max(q_ref, 1)``: q_ref is the same metric of torch-CPU's fp32 evaluation of the same stage on
  the same input, measured in the same test.  16 = headroom of one sequential accumulation chain (an MFMA K loop)
  over a CPU library's blocked sums; one dropped up-conv weight gives q = 4e3 .. 7e5, 74 x the bound at the least
  (tests/test_decode_stage_ref.py injects the faults and asserts the margins).

All tensors are channel-first ``[B, C, T]`` as in ``decode_ref`` (an engine tap ``[B][T][C]`` is transposed by the
caller).  Here the decoder transformer is checked as a whole with the project metric against ``mimi_ref.transformer``
in float64; its 8 x 5 stages, with condition sums derived for LayerNorm, softmax and GELU, are in
tests/decode_xfmr_ref.py (on the table of tests/encode_stage_ref.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict

import torch
import torch.nn.functional as F

import decode_ref
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

U = 2.0 ** -24
WORKING_FACTOR = 16.0
CFG = RefConfig()


def _t(sd, key, dtype, mag):
    w = sd[key].to(dtype)
    return w.abs() if mag else w


def _in(x, dtype, mag):
    x = x.to(dtype)
    return x.abs() if mag else x


def _act(mag):
    return (lambda v: v) if mag else F.elu


# ---- the stages, each at a dtype, on the true values or (mag) on the absolute ones ---------------------------------
def _quantizer(codes, sd, dtype, mag, cfg=CFG):
    """codes [B, K, T] -> [B, 512, T]: gather-sum per half in level order, then the [W_sem | W_ac] projection (K = 2 Dq).
    The codebook rows are the reference's fp32 ``embed_sum / clamp(cluster_usage)``: they are the stage's weights."""
    codes = codes.long()
    ns = cfg.num_semantic_quantizers
    halves, ws = [], []
    for which, lo, hi in (("semantic", 0, min(ns, codes.shape[1])), ("acoustic", ns, codes.shape[1])):
        pre = f"quantizer.{which}_residual_vector_quantizer."
        s = torch.zeros(codes.shape[0], codes.shape[2], sd[pre + "output_proj.weight"].shape[1], dtype=dtype)
        for lv in range(lo, hi):
            e = mimi_ref.codebook_embed(sd, pre + f"layers.{lv - lo}.codebook.", cfg).to(dtype)
            s = s + F.embedding(codes[:, lv], e.abs() if mag else e)
        halves.append(s.permute(0, 2, 1))
        ws.append(_t(sd, pre + "output_proj.weight", dtype, mag))
    return F.conv1d(torch.cat(halves, 1), torch.cat(ws, 1))


def _upsample(x, sd, dtype, mag):
    w = _t(sd, "upsample.conv.weight", dtype, mag)
    return decode_ref.conv_transpose1d_causal(_in(x, dtype, mag), w, None, stride=2, groups=w.shape[0])


def _conv(prefix, elu_out=False):
    def f(x, sd, dtype, mag):
        y = mimi_ref.causal_conv1d(_in(x, dtype, mag), _t(sd, prefix + "weight", dtype, mag),
                                   _t(sd, prefix + "bias", dtype, mag))
        return _act(mag)(y) if elu_out else y
    return f


def _upconv(s, cfg=CFG):
    p = f"decoder.layers.{2 + 3 * s}.conv."

    def f(x, sd, dtype, mag):
        return decode_ref.conv_transpose1d_causal(_in(x, dtype, mag), _t(sd, p + "weight", dtype, mag),
                                                  _t(sd, p + "bias", dtype, mag), stride=cfg.upsampling_ratios[s])
    return f


def _resblock(s):
    p = f"decoder.layers.{3 + 3 * s}.block."

    def f(x, sd, dtype, mag):
        act = _act(mag)
        x = _in(x, dtype, mag)
        h = mimi_ref.causal_conv1d(act(x), _t(sd, p + "1.conv.weight", dtype, mag), _t(sd, p + "1.conv.bias", dtype, mag))
        h = mimi_ref.causal_conv1d(act(h), _t(sd, p + "3.conv.weight", dtype, mag), _t(sd, p + "3.conv.bias", dtype, mag))
        return act(x + h)
    return f


@dataclass(frozen=True)
class Stage:
    name: str        # the output tap
    source: str      # the input tap ("codes" for the quantizer)
    fn: Callable     # fn(x, sd, dtype, mag) -> tensor
    n: Callable      # n(x, sd) -> the hard bound

    def ref(self, x, sd):
        """(ref64, mag64)"""
        with torch.no_grad():
            return self.fn(x, sd, torch.float64, False), self.fn(x, sd, torch.float64, True)

    def f32(self, x, sd):
        """torch-CPU's fp32 evaluation of the same stage on the same input."""
        with torch.no_grad():
            return self.fn(x, sd, torch.float32, False)


def _stages(cfg=CFG) -> Dict[str, Stage]:
    st = {}
    st["quantized"] = Stage("quantized", "codes", _quantizer,
                            lambda x, sd: 2 * int(sd["quantizer.semantic_residual_vector_quantizer.output_proj.weight"].shape[1])
                            + int(x.shape[1]) + 2)
    st["upsample"] = Stage("upsample", "quantized", _upsample, lambda x, sd: 4)
    p0 = "decoder.layers.0.conv."
    st["dconv0"] = Stage("dconv0", "xfmr7", _conv(p0),
                         lambda x, sd: int(sd[p0 + "weight"].shape[1] * sd[p0 + "weight"].shape[2]) + 2)
    # the tensor the pass itself computes (bias + ELU epilogue) and up conv 0 reads: + 1 for the ELU evaluation
    st["dconv0_elu"] = Stage("dconv0_elu", "xfmr7", _conv(p0, elu_out=True),
                             lambda x, sd: int(sd[p0 + "weight"].shape[1] * sd[p0 + "weight"].shape[2]) + 3)
    for s, r in enumerate(cfg.upsampling_ratios):
        pu = f"decoder.layers.{2 + 3 * s}.conv.weight"   # [Cin, Cout, 2 r]: an output sees 2 taps of every input channel
        st[f"up{s}"] = Stage(f"up{s}", "dconv0_elu" if s == 0 else f"dres{s - 1}_elu", _upconv(s),
                             lambda x, sd, pu=pu: 2 * int(sd[pu].shape[0]) + 2)
        pb = f"decoder.layers.{3 + 3 * s}.block."

        def n_res(x, sd, pb=pb):
            w3, w1 = sd[pb + "1.conv.weight"], sd[pb + "3.conv.weight"]
            return (int(w3.shape[1] * w3.shape[2]) + 2) + (int(w1.shape[1] * w1.shape[2]) + 2) + 4
        st[f"dres{s}_elu"] = Stage(f"dres{s}_elu", f"up{s}", _resblock(s), n_res)
    pl = f"decoder.layers.{2 + 3 * len(cfg.upsampling_ratios)}.conv."
    st["audio"] = Stage("audio", f"dres{len(cfg.upsampling_ratios) - 1}_elu", _conv(pl),
                        lambda x, sd: int(sd[pl + "weight"].shape[1] * sd[pl + "weight"].shape[2]) + 2)
    return st


STAGES = _stages()


# ---- the functions of the table: input tensor + state dict -> (ref64, mag64) ----------------------------------------
def quantizer(codes, sd):
    return STAGES["quantized"].ref(codes, sd)


def upsample(x, sd):
    return STAGES["upsample"].ref(x, sd)


def conv0(x, sd):
    return STAGES["dconv0"].ref(x, sd)


def upconv(x, sd, s):
    return STAGES[f"up{s}"].ref(x, sd)


def resblock(x, sd, s):
    return STAGES[f"dres{s}_elu"].ref(x, sd)


def last_conv(x, sd):
    return STAGES["audio"].ref(x, sd)


def transformer(x, sd, dtype=torch.float64, cfg=CFG):
    """The decoder transformer as a whole: x [B, 512, T] -> [B, 512, T] at ``dtype`` (``mimi_ref.transformer`` on the
    ``decoder_transformer.*`` weights; its RoPE tables stay the reference's fp32 values, which are part of the model)."""
    pre = "decoder_transformer."
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(pre)}
    with torch.no_grad():
        return decode_ref.decoder_transformer(x.to(dtype).transpose(1, 2), sdd, cfg).transpose(1, 2)


# ---- the metric -----------------------------------------------------------------------------------------------------
def q_metric(got, ref64, mag64) -> float:
    """max |got - ref64| / (2^-24 mag64).  An element whose condition sum is 0 is exactly 0 in any implementation
    (every product is 0): a non-zero there is an infinite q, not a division by zero."""
    got = torch.as_tensor(got)
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(mag64.shape), (got.shape, ref64.shape, mag64.shape)
    err = (got.double() - ref64).abs()
    den = U * mag64
    q = torch.where(den > 0, err / den.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                      torch.zeros_like(err)))
    return float(q.max())


def worst_element(got, ref64, mag64):
    """Index (tuple) of the element that sets q: where to look when a condition fails."""
    q = (torch.as_tensor(got).double() - ref64).abs() / (U * mag64).clamp(min=1e-300)
    flat = int(q.argmax())
    return tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), q.shape))


def rel_err(a, b) -> float:
    """The project metric (tests/test_gpu_parity.py): max-abs error over max-abs value."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def measure(name: str, x, sd, got=None) -> dict:
    """One stage on input x: q_ref always (torch-CPU fp32 against float64), q_engine when ``got`` is given."""
    st = STAGES[name]
    ref64, mag64 = st.ref(x, sd)
    rec = {"stage": name, "n": int(st.n(x, sd)), "q_ref": q_metric(st.f32(x, sd), ref64, mag64)}
    if got is not None:
        rec["q_engine"] = q_metric(got, ref64, mag64)
        rec["worst"] = list(worst_element(got, ref64, mag64))
    return rec


def working_bound(q_ref: float) -> float:
    return WORKING_FACTOR * max(q_ref, 1.0)


def failures(rec: dict, key: str = "q_engine") -> list:
    """The conditions that ``rec[key]`` misses (empty: both hold)."""
    out = []
    if not rec[key] <= rec["n"]:
        out.append(f"{rec['stage']}: hard condition q = {rec[key]:.3g} > n = {rec['n']}")
    if not rec[key] <= working_bound(rec["q_ref"]):
        out.append(f"{rec['stage']}: working condition q = {rec[key]:.3g} > 16 max(q_ref = {rec['q_ref']:.3g}, 1)")
    return out
