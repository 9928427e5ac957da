"""Test infrastructure only: a CPU restatement of the Mimi decode path of ``transformers`` 5.15.0
(``MimiModel.decode``; ``TF/`` = ``transformers/models/mimi/``), the mirror of ``oracle/mimi_ref.py``.

Written with torch-CPU functional ops in the reference's op order and layout (channel-first, fp32), so that on the
same CPU it reproduces ``MimiModel.decode`` bit for bit (pinned by ``tests/golden/make_decode_golden.py`` against
the real ``transformers`` model).  On the GPU box it is the parity checker and the CPU yardstick of
``tools/decode_bench.py``.

    quantizer.decode      TF/modeling_mimi.py:1128-1137 (split), :1070-1081 (one RVQ), :1004-1006 (codebook)
    upsample / up convs   TF/modeling_mimi.py:399-405 (MimiConvTranspose1d.forward: conv_transpose1d, trim right)
    decoder               TF/modeling_mimi.py:931-961
    model                 TF/modeling_mimi.py:1388-1406 (_decode_frame), :1408-1458 (decode)
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

FRAME = 1920  # samples per 12.5 Hz frame: 2 (upsample) x 8 x 6 x 5 x 4

TAP_NAMES = ("quantized", "upsample", "xfmr7", "dconv0", "up0", "up1", "up2", "up3", "dres0", "dres1", "dres2",
             "dres3", "audio")


def decoded_length(frames: int, cfg: Optional[RefConfig] = None) -> int:
    cfg = cfg or RefConfig()
    n = 2 * int(frames)
    for r in cfg.upsampling_ratios:
        n *= r
    return n


def conv_transpose1d_causal(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int,
                            groups: int = 1) -> torch.Tensor:
    """``MimiConvTranspose1d.forward`` (:399-405), causal, trim_right_ratio 1: all ``k - stride`` trimmed right."""
    y = F.conv_transpose1d(x, w, b, stride=stride, groups=groups)
    pad = w.shape[-1] - stride
    return y[..., : y.shape[-1] - pad]


def rvq_decode(codes: torch.Tensor, sd, which: str, first_level: int, cfg: RefConfig) -> torch.Tensor:
    """``MimiResidualVectorQuantizer.decode`` (:1070-1081).  codes [B, k, T] -> [B, 512, T]."""
    pre = f"quantizer.{which}_residual_vector_quantizer."
    out = torch.full((), 0.0)
    for i, idx in enumerate(codes.transpose(0, 1)):
        embed = mimi_ref.codebook_embed(sd, pre + f"layers.{i}.codebook.", cfg)
        out = out + F.embedding(idx, embed).permute(0, 2, 1)
    return F.conv1d(out, sd[pre + "output_proj.weight"])


def quantizer_decode(codes: torch.Tensor, sd, cfg: RefConfig) -> torch.Tensor:
    """``MimiSplitResidualVectorQuantizer.decode`` (:1128-1137)."""
    ns = cfg.num_semantic_quantizers
    q = rvq_decode(codes[:, :ns], sd, "semantic", 0, cfg)
    if codes.shape[1] > ns:
        q += rvq_decode(codes[:, ns:], sd, "acoustic", ns, cfg)
    return q


def upsample(x: torch.Tensor, sd) -> torch.Tensor:
    w = sd["upsample.conv.weight"]
    return conv_transpose1d_causal(x, w, None, stride=2, groups=w.shape[0])


def decoder_transformer(x: torch.Tensor, sd, cfg: RefConfig, taps: Optional[dict] = None) -> torch.Tensor:
    """``MimiTransformerModel.forward`` on the ``decoder_transformer.*`` weights.  x: [B, T, C]."""
    pre = "decoder_transformer."
    rk = {"encoder_transformer." + k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    return mimi_ref.transformer(x, rk, cfg, taps)


def seanet_decoder(x: torch.Tensor, sd, cfg: RefConfig, taps: Optional[dict] = None) -> torch.Tensor:
    """``MimiDecoder.forward`` (:931-961).  x: [B, 512, T25] -> [B, 1, 960 T25]."""
    x = mimi_ref.causal_conv1d(x, sd["decoder.layers.0.conv.weight"], sd["decoder.layers.0.conv.bias"])
    if taps is not None:
        taps["dconv0"] = x
    idx = 1
    for si, ratio in enumerate(cfg.upsampling_ratios):
        idx += 1  # ELU
        p = f"decoder.layers.{idx}.conv."
        x = conv_transpose1d_causal(F.elu(x), sd[p + "weight"], sd[p + "bias"], stride=ratio)
        if taps is not None:
            taps[f"up{si}"] = x
        idx += 1
        p = f"decoder.layers.{idx}.block."
        h = mimi_ref.causal_conv1d(F.elu(x), sd[p + "1.conv.weight"], sd[p + "1.conv.bias"])
        h = mimi_ref.causal_conv1d(F.elu(h), sd[p + "3.conv.weight"], sd[p + "3.conv.bias"])
        x = x + h
        if taps is not None:
            taps[f"dres{si}"] = x
        idx += 1
    idx += 1  # ELU
    p = f"decoder.layers.{idx}.conv."
    return mimi_ref.causal_conv1d(F.elu(x), sd[p + "weight"], sd[p + "bias"])


def as_tensors(sd) -> Dict[str, torch.Tensor]:
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}


def decode(audio_codes, sd, cfg: Optional[RefConfig] = None, taps: Optional[dict] = None,
           padding_mask=None) -> torch.Tensor:
    """``MimiModel.decode`` (:1408-1458) -> float32 waveform [B, 1, 1920 T].  ``sd`` holds the encode-path state dict
    (for the codebooks) and the decode-only one (``synthetic.make_decoder_state_dict``) merged."""
    cfg = cfg or RefConfig()
    codes = torch.as_tensor(np.asarray(audio_codes) if not torch.is_tensor(audio_codes) else audio_codes).long()
    if codes.dim() != 3:
        raise ValueError("audio_codes must be [batch, num_quantizers, frames]")
    if codes.shape[1] > cfg.num_quantizers or codes.shape[1] < 1:
        raise ValueError("num_quantizers out of range")
    sdt = as_tensors(sd)
    with torch.no_grad():
        q = quantizer_decode(codes, sdt, cfg)
        if taps is not None:
            taps["quantized"] = q
        u = upsample(q, sdt)
        if taps is not None:
            taps["upsample"] = u
        xt = {}
        t = decoder_transformer(u.transpose(1, 2), sdt, cfg, xt).transpose(1, 2)
        if taps is not None:
            taps[f"xfmr{cfg.num_hidden_layers - 1}"] = t
        y = seanet_decoder(t, sdt, cfg, taps)
        if taps is not None:
            taps["audio"] = y
    if padding_mask is not None and padding_mask.shape[-1] < y.shape[-1]:
        y = y[..., : padding_mask.shape[-1]]
    return y
