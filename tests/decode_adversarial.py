"""Test infrastructure only (CPU): adversarial checkpoints and codes for the DECODE path's transformer, the mirror
of tests/encode_adversarial.py (whose measures ``attention_regime`` and ``layernorm_regime`` are reused here, with
the window passed in).

Every decode test before these ran random codes through the seeded checkpoint: at 80 rows attention there has a score
range of 5.8 and a median largest weight of 0.09, and LayerNorm rows have |mean| / std <= 0.07.

CHECKPOINTS: pure functions of the merged seeded state dict (``synthetic.make_state_dict(seed=0)`` +
``synthetic.make_decoder_state_dict(seed=0)``), ``CHECKPOINTS[name](sd)``; the SEANet decoder is never changed.
  peaky3, peaky8, flat   decoder q_proj / k_proj x (3, 3), (8, 8), (0, 1)
  massive                rows 5 and 300 of both quantizer output_proj weights x 1000 and x -700.  The projections and
                         the upsample have no bias and the upsample is depthwise, so exactly these two channels of the
                         transformer's input are massive, and the residual stream keeps them through all 8 layers.
  offset                 every LayerNorm input row of every layer gets a common offset far above its spread:
                           * every entry of semantic level 0 gets + d (d = OFFSET_D in every coordinate),
                           * W_sem += G 1 d^T / |d|^2, so W_sem (e + d) gains G (1 + d.e / |d|^2) on EVERY channel,
                           * upsample.conv.weight = 0.5 + eps base: a row sums two taps, so the offset passes at about
                             G (G / 2 on row 0) with a spread of eps G |base| over the channels.
                         OFFSET_G = 5000, OFFSET_EPS = 1e-5 (G = 1000, eps = 0.01 gave |mean| / std of 70 .. 100: the
                         ratio is about 1 / eps while G / 2 is far above the layers' O(1) updates).  Measured in
                         float64 on B = 2 x T = 40, window 70, the smallest ratio over the rows of the 16 LayerNorm
                         inputs falls from 1.1e4 at layer 0 to 4.6e3 at layer 7 (T = 13, window 250: 1.1e4 to 4.2e3).
                         tests/test_decode_xfmr_ref.py asserts >= 1e3 on every row of every layer.
  zero                   entry 0 of every level's codebook is the zero vector: with all-zero codes the transformer's
                         input is exactly 0, LayerNorm has variance 0, the residual stream holds the updates alone.
CODES: ``random``, ``constant`` (one frame repeated: the keys tie exactly within a row parity), ``zeros``.
"""
from __future__ import annotations

from typing import Callable, Dict

import numpy as np
import torch

import decode_xfmr_ref as dxr
import encode_adversarial as eadv
import encode_stage_ref as esr
from mimi_hip import synthetic

LAYERS = esr.CFG.num_hidden_layers
DP = esr.DECODER_PREFIX
SEM = "quantizer.semantic_residual_vector_quantizer."
AC = "quantizer.acoustic_residual_vector_quantizer."
OFFSET_G, OFFSET_EPS, OFFSET_D = 5000.0, 1.0e-5, 1.0


def base_state_dict() -> Dict[str, np.ndarray]:
    sd = dict(synthetic.make_state_dict(seed=0))
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return sd


def _copy(sd, keys):
    """A shallow copy with fresh arrays under ``keys`` (the only ones a checkpoint function writes)."""
    out = dict(sd)
    for k in keys:
        out[k] = np.array(sd[k], copy=True)
    return out


def _scale_qk(sd, gq, gk):
    keys = [f"{DP}layers.{l}.self_attn.{n}_proj.weight" for l in range(LAYERS) for n in "qk"]
    out = _copy(sd, keys)
    for k in keys:
        out[k] = out[k] * np.float32(gq if ".q_proj." in k else gk)
    return out


def peaky3(sd):
    return _scale_qk(sd, 3.0, 3.0)


def peaky8(sd):
    return _scale_qk(sd, 8.0, 8.0)


def flat(sd):
    return _scale_qk(sd, 0.0, 1.0)


def massive(sd):
    keys = [SEM + "output_proj.weight", AC + "output_proj.weight"]
    out = _copy(sd, keys)
    for k in keys:
        out[k][5] *= np.float32(1000.0)
        out[k][300] *= np.float32(-700.0)
    return out


def offset(sd):
    cb = SEM + "layers.0.codebook."
    out = _copy(sd, [cb + "embed_sum", SEM + "output_proj.weight", "upsample.conv.weight"])
    usage = np.maximum(out[cb + "cluster_usage"], np.float32(esr.CFG.codebook_eps))   # the reference's clamp
    dq = out[cb + "embed_sum"].shape[1]
    out[cb + "embed_sum"] = (out[cb + "embed_sum"] + usage[:, None] * np.float32(OFFSET_D)).astype(np.float32)
    # G 1 d^T / |d|^2 with d = OFFSET_D in each of the dq coordinates
    out[SEM + "output_proj.weight"] = (out[SEM + "output_proj.weight"] +
                                       np.float32(OFFSET_G * OFFSET_D / (dq * OFFSET_D ** 2))).astype(np.float32)
    out["upsample.conv.weight"] = (np.float32(0.5) + np.float32(OFFSET_EPS) * out["upsample.conv.weight"]).astype(np.float32)
    return out


def zero(sd):
    keys = [k for k in sd if k.endswith("codebook.embed_sum")]
    out = _copy(sd, keys)
    for k in keys:
        out[k][0] = 0.0
    return out


CHECKPOINTS: Dict[str, Callable] = {"peaky3": peaky3, "peaky8": peaky8, "flat": flat, "massive": massive,
                                    "offset": offset, "zero": zero}
ADVERSARIAL = ("peaky3", "peaky8", "flat", "massive", "offset")   # the five that run on random codes


# ---- codes ----------------------------------------------------------------------------------------------------------
def random_codes(seed, B, K, T):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, (B, K, T)))


def constant_codes(seed, B, K, T):
    """One random frame per item, repeated T times."""
    return random_codes(seed, B, K, 1).expand(B, K, T).contiguous()


def zero_codes(seed, B, K, T):
    return torch.zeros(B, K, T, dtype=torch.int64)


CODES: Dict[str, Callable] = {"random": random_codes, "constant": constant_codes, "zeros": zero_codes}


# ---- measures (encode's, at the decoder's window) ---------------------------------------------------------------------
def attention_regime(qkv_tap, window=None) -> dict:
    return eadv.attention_regime(qkv_tap, window)


def layernorm_regime(x) -> dict:
    return eadv.layernorm_regime(x)


def regimes(taps, layers=(0, LAYERS - 1), window=None) -> dict:
    """{layer: {attention, ln1, ln2}} of a chain's taps (``decode_xfmr_ref.chain``)."""
    out = {}
    for l in layers:
        x = taps[dxr.FIRST] if l == 0 else taps[f"xfmr{l - 1}"]
        out[l] = {"attention": attention_regime(taps[f"qkv{l}"], window), "ln1": layernorm_regime(x),
                  "ln2": layernorm_regime(taps[f"oproj{l}"])}
    return out
