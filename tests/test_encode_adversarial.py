"""GPU: the encode kernels in float64 on adversarial checkpoints and degenerate audio (tests/encode_adversarial.py).

The harness is tests/test_encode_kernels.py's, imported: one profiled, taps-on encode per case (``run_case``), each
stage's output tap against the float64 evaluation of that stage on the engine's own input taps (``check_stages``: hard
condition q <= n + c, working condition q <= 16 max(q_ref, q_emul, 1)), the kernel family per stage pinned from the
launch sequence (``assert_kernels``).  No tolerance is new.  What is new is the input: every earlier case measured the
kernels on speech through the seeded checkpoint, where attention is flat (score range 3.6) and LayerNorm rows are
centred (|mean| / std <= 0.08).  tests/test_encode_adversarial_ref.py shows on the CPU that each case reaches its
regime and which faults only these cases catch.

  checkpoints (one engine each)   ALL at B = 2 x 13 frames; layers 0 and 7 + the tail at B = 2 x 250 frames (eight
                                  32-key chunks in the T <= 256 attention); att0 / att7 at B = 1 x 257 frames in both
                                  banded decompositions; the fused q/k/v + attention at 2 x 250 frames; q/k/v and fc1
                                  with and without their LayerNorm prologue at 2 x 13 frames
  degenerate audio (base)         ALL at B = 2 x 13 frames, item 0 the case and item 1 speech; the pre-quantizer tap
                                  against the oracle (1e-4), the quantizer on the oracle's embedding, no fallback
  overflow boundary               one clip at gains 2^0 .. 2^15: the first gain k* that takes the fallback, monotone
                                  from there; the stages one step below it; bf16x6 codes at it
  batch-mates                     [speech, silence, square, 1e-20 noise, speech x 2^k*, a 2^k* click, Inf clip, NaN clip]:
                                  every finite item bitwise its own B = 1 encode, uniform and ragged
  LayerNorm bound                 ``onehot``: layer 0's LayerNorm rows reach |g| sqrt(D - 1) on the device, on the path
                                  that skips that tensor's range check (the device side of tests/test_ln_bound.py)

Every stage record goes to ``parity_log`` as test "encode_adversarial" (the baseline copy is
profiles/encode_adversarial_parity.json), k* beside them.

The two non-finite items have no reference (the oracle spreads one NaN to every frame through P @ V): only that the
call returns, that the codes are codebook indices and that two runs agree.  Before they were run on a GPU, every place
that forms a code or an index from a comparison was read: none can leave its table on NaN.
"""
import numpy as np
import pytest
import torch

import encode_adversarial as adv
import encode_stage_ref as esr
from mimi_hip import synthetic
from mimi_hip.config import encoded_length
from oracle import mimi_ref
from test_encode_kernels import ALL, LNA, SMALL_F16, TAIL, assert_kernels, check_stages, layer, make_engine, pk, run_case

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
LAYERS = adv.LAYERS
ENDS = layer(0) + layer(LAYERS - 1)
ATT = ["att0", f"att{LAYERS - 1}"]
L13, L250, L257 = 960 * 13, 960 * 250, 960 * 257
B2_F250 = dict(SMALL_F16, down_s1=pk(256, 128, 12), res3_s2=pk(256, 128), res3_s3=pk(64, 64), fc1=pk(64, 64, LNA),
               fc2=pk(32, 32))   # (tests/test_encode_kernels.py test_b2_f250_kernels)


def checked(parity_log, case, stages, taps, sd, ar, kern, items=None):
    """``check_stages`` with its records filed under this test."""
    n0 = len(parity_log)
    try:
        check_stages(parity_log, case, stages, taps, sd, ar, kern, items=items)
    finally:
        for rec in parity_log[n0:]:
            rec["test"] = "encode_adversarial"


# ---- crafted checkpoints: one engine each -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_np():
    return adv.base_state_dict()


@pytest.fixture(scope="module", params=list(adv.CHECKPOINTS))
def ckpt(request, base_np):
    sd_np = adv.CHECKPOINTS[request.param](base_np)
    m = make_engine(sd_np)
    yield request.param, m, adv.torch_sd(sd_np)
    m.close()


def test_checkpoint_every_stage(ckpt, parity_log):
    name, m, sd = ckpt
    taps, kern, ar = run_case(m, adv.speech_batch(2, L13, 41), ALL)
    assert_kernels(kern, SMALL_F16)
    checked(parity_log, f"{name}_B2_F13", ALL, taps, sd, ar, kern)
    if name == "onehot":
        # the device side of tests/test_ln_bound.py: the rows above reach the bound (CPU: test_case_reaches_its_regime)
        # and qkv0 was just checked on them; the range check of that LayerNorm output was skipped while they ran
        reg = adv.layernorm_regime(taps["encoder"])
        assert abs(reg["max_normalised"] / reg["sqrt_C_minus_1"] - 1.0) < 0.01, reg
        scale, last_max, _ = m.act_scales()["xf0.ln1"]
        assert scale > 0 and last_max == -1.0, (scale, last_max)


def test_checkpoint_250_frames(ckpt, parity_log):
    """Layers 0 and 7 and the tail at B = 2 x 250 frames: the T <= 256 attention walks eight 32-key chunks."""
    name, m, sd = ckpt
    stages = ENDS + TAIL
    taps, kern, ar = run_case(m, adv.speech_batch(2, L250, 42), stages)
    assert_kernels(kern, B2_F250)
    if name == "peaky8":
        reg = adv.attention_regime(taps["qkv0"])
        assert reg["score_range"] >= 60 and reg["max_later_chunk_changes"] >= 2, reg
    checked(parity_log, f"{name}_B2_F250", stages, taps, sd, ar, kern)


@pytest.mark.parametrize("split,symbol", [(1, "mimi::attention_band_h16_kernel<"), (0, "mimi::attention_band_h16_kernel<false>"),
                                          (2, "mimi::attention_band_h16_kernel<true>")])
def test_checkpoint_banded_attention(ckpt, parity_log, split, symbol):
    """B = 1 x 257 frames: rows 250 .. 256 have a full window; as the engine picks the decomposition (1) and each forced."""
    name, m, sd = ckpt
    m.set_option("attn_band_split", split)
    try:
        taps, kern, ar = run_case(m, adv.speech_batch(1, L257, 43), ATT)
    finally:
        m.set_option("attn_band_split", 1)
    assert_kernels(kern, {"attention": symbol, "qkv_attention": None})
    checked(parity_log, f"{name}_band_split_{split}_B1_F257", ATT, taps, sd, ar, kern)


def test_checkpoint_fused_qkv_attention(ckpt, parity_log):
    name, m, sd = ckpt
    stages = [s for l in range(LAYERS) for s in (f"qkv{l}", f"att{l}")]
    taps, kern, ar = run_case(m, adv.speech_batch(2, L250, 44), stages, opts={"qkv_attn": 2})
    assert_kernels(kern, {"qkv_attention": "mimi::qkv_attention_h16_kernel<512>", "qkv": None, "attention": None})
    checked(parity_log, f"{name}_qkv_attn_2_B2_F250", stages, taps, sd, ar, kern)


@pytest.mark.parametrize("value,qkv,fc1", [(0, pk(16, 64, 0), pk(16, 64, 0)), (2, pk(16, 64, LNA), pk(16, 64, LNA))])
def test_checkpoint_layernorm_forms(ckpt, parity_log, value, qkv, fc1):
    """ln_fused = 0: the LayerNorm kernel in front of q/k/v and fc1; 2: both GEMMs compute their rows' LayerNorm."""
    name, m, sd = ckpt
    stages = [s for l in range(LAYERS) for s in (f"qkv{l}", f"ff{l}")]
    taps, kern, ar = run_case(m, adv.speech_batch(2, L13, 45), stages, opts={"ln_fused": value})
    assert_kernels(kern, {"qkv": qkv, "fc1": fc1})
    if value == 2:
        assert_kernels(kern, {"layernorm": None})
    else:
        assert_kernels(kern, {"layernorm": "mimi::layernorm_kernel<512,"})
    checked(parity_log, f"{name}_ln_fused_{value}_B2_F13", stages, taps, sd, ar, kern)


# ---- degenerate audio on the base checkpoint ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd(state_dict):
    return adv.torch_sd(state_dict)


@pytest.fixture(scope="module")
def engine(state_dict):
    m = make_engine(state_dict)
    yield m
    m.close()


@pytest.mark.parametrize("name", adv.FINITE_AUDIO)
def test_degenerate_audio_every_stage(engine, state_dict, sd, parity_log, name):
    x = adv.audio_batch(name, L13, 46)
    reruns = engine.f16_reruns
    taps, kern, ar = run_case(engine, x, ALL)
    assert_kernels(kern, SMALL_F16)
    assert engine.f16_reruns == reruns, name
    ref = {}
    ref_codes = mimi_ref.encode(x[:, None], state_dict, 8, taps=ref)
    want = ref["pre_quantizer"].permute(0, 2, 1)
    got = taps["downsample"]
    print({"audio": name, "pre_quantizer rel_err": esr.rel_err(got, want),
           "per item": [esr.rel_err(got[i], want[i]) for i in range(2)]})
    assert esr.rel_err(got, want) < ACT_TOL, name
    for i in range(2):  # (the quiet item is not hidden under the speech beside it)
        assert esr.rel_err(got[i], want[i]) < ACT_TOL, (name, i)
    assert torch.equal(engine.quantize(ref["pre_quantizer"].cuda(), 8).cpu(), ref_codes), name
    assert engine.f16_reruns == reruns, name
    checked(parity_log, f"audio_{name}_B2_F13", ALL, taps, sd, ar, kern)


# ---- the overflow boundary ------------------------------------------------------------------------------------------------
def loud_clip(k):
    return torch.from_numpy(synthetic.speech_like(L13, 47, 0) * np.float32(2.0 ** k))[None]


@pytest.fixture(scope="module")
def sweep(engine):
    """One clip at gains 2^k, k = 0 .. 15, each encoded once at B = 1: ({k: took the fallback}, {k: codes},
    {k: act_scales() after it}, k* = the first k that took it)."""
    over, codes, scales = {}, {}, {}
    for k in range(16):
        before = engine.f16_reruns
        codes[k] = engine.encode_int32(loud_clip(k).cuda(), 8).cpu()
        over[k] = engine.f16_reruns > before
        scales[k] = engine.act_scales()
    hits = [k for k in range(16) if over[k]]
    assert hits, "no gain up to 2^15 overflows a fixed scale"
    return over, codes, scales, hits[0]


def test_overflow_boundary(engine, sd, sweep, parity_log):
    over, codes, scales, ks = sweep
    parity_log.append({"test": "encode_adversarial", "case": "overflow_boundary", "k_star": ks,
                       "fallback": [bool(over[k]) for k in range(16)]})
    print({"k*": ks, "fallback": [bool(over[k]) for k in range(16)]})
    assert ks >= 1, "full-level speech overflows"
    assert all(over[k] for k in range(ks, 16)), over   # monotone from k* on
    # one step below: some tensor within a factor 2 of its limit, and every stage inside its conditions there
    near = {n: mx * s for n, (s, mx, _) in scales[ks - 1].items() if 2.0 ** 14 <= mx * s < 2.0 ** 15}
    print({"k* - 1": ks - 1, "within a factor 2 of the limit": near})
    assert near, {n: mx * s for n, (s, mx, _) in scales[ks - 1].items()}
    reruns = engine.f16_reruns
    taps, kern, ar = run_case(engine, loud_clip(ks - 1), ALL)
    assert engine.f16_reruns == reruns
    checked(parity_log, f"gain_2^{ks - 1}_B1_F13", ALL, taps, sd, ar, kern)
    # at k*: the item overflows alone, so its codes are the scale-free arithmetic's
    engine.set_precision("bf16x6")
    try:
        want = engine.encode_int32(loud_clip(ks).cuda(), 8).cpu()
    finally:
        engine.set_precision("f16x3")
    assert torch.equal(codes[ks], want), int((codes[ks] != want).sum())


# ---- batch-mates ------------------------------------------------------------------------------------------------------------
# "click": one sample of 2^k* among zeros.  It overflows the audio planes alone ("s0.audio", 2^(k* + 7) >= 2^15) and no
# other tensor, and the Inf clip's only non-finite maximum is that same tensor's (further on its Inf has become NaN,
# which no maximum records): the one batch-mate whose overflow the Inf hid entirely.  "loud" overflows seven tensors,
# six of which the Inf clip leaves finite, so its fallback was taken before the fix too.
MATES = ["speech", "zeros", "square", "noise_1e-20", "loud", "click", "inf", "nan"]
FINITE = [i for i, n in enumerate(MATES) if n not in ("inf", "nan")]


def mates(ks, L=L13):
    rows = []
    for n in MATES:
        if n == "speech":
            rows.append(synthetic.speech_like(L, 48, 0))
        elif n == "loud":
            rows.append(synthetic.speech_like(L, 48, 1) * np.float32(2.0 ** ks))
        elif n == "click":
            rows.append(adv.impulse(L, 48) * np.float32(2.0 ** ks))
        else:
            rows.append(adv.AUDIO[n](L, 48))
    return torch.from_numpy(np.stack(rows))


def test_batch_mates_uniform(engine, sweep):
    """An item's codes do not depend on its batch-mates (README): not on a silent one, not on one that overflows, and
    not on one that carries an Inf -- whose +inf tensor maxima used to hide the loud item's overflow from the check."""
    ks = sweep[3]
    x = mates(ks).cuda()
    before = engine.f16_reruns
    got = engine.encode_int32(x, 32).cpu()
    assert engine.f16_reruns > before  # the loud item sends the batch to the per-item fallback
    again = engine.encode_int32(x, 32).cpu()
    bad = []
    for i in FINITE:
        before = engine.f16_reruns
        alone = engine.encode_int32(x[i:i + 1], 32).cpu()
        if MATES[i] in ("loud", "click"):
            assert engine.f16_reruns > before, MATES[i]
        if not torch.equal(got[i], alone[0]):
            bad.append((MATES[i], int((got[i] != alone[0]).sum())))
    assert not bad, bad
    assert torch.equal(got, again)   # the non-finite items too: the same codes twice
    assert int(got.min()) >= 0 and int(got.max()) < 2048


def test_batch_mates_ragged(engine, sweep):
    ks = sweep[3]
    lengths = [L13, 9001, 12001, 7777, 11520, 6001, 12480, 8000]
    x = mates(ks)
    for i, L in enumerate(lengths):
        x[i, L:] = 0.0
    xd = x.cuda()
    got = engine.encode_ragged(xd, lengths, 32).cpu()
    again = engine.encode_ragged(xd, lengths, 32).cpu()
    bad = []
    for i, L in enumerate(lengths):
        F = encoded_length(L)
        assert int(got[i, :, :F].min()) >= 0 and int(got[i, :, :F].max()) < 2048, MATES[i]
        assert torch.equal(got[i, :, :F], again[i, :, :F]), MATES[i]
        if i in FINITE:
            alone = engine.encode_int32(xd[i:i + 1, :L].contiguous(), 32).cpu()
            if not torch.equal(got[i, :, :F], alone[0]):
                bad.append((MATES[i], int((got[i, :, :F] != alone[0]).sum())))
    assert not bad, bad


@pytest.mark.parametrize("ragged", [False, True])
def test_inf_does_not_hide_a_batch_mates_overflow(engine, sweep, ragged):
    """[speech, click, Inf clip], without the loud speech whose other tensors would send the batch to the fallback
    anyway: the click's overflow shows in "s0.audio" alone, where the Inf clip's maximum is +inf, the per-tensor maximum
    of the batch.  The overflow check used to pass over a non-finite maximum, so the click's codes came from saturated
    audio planes; now a non-finite maximum in a batch sends every item to its own pass."""
    ks = sweep[3]
    keep = [MATES.index(n) for n in ("speech", "click", "inf")]
    x = mates(ks)[keep].cuda()
    lengths = [L13, 6001, 9001] if ragged else [L13] * 3
    before = engine.f16_reruns
    got = (engine.encode_ragged(x, lengths, 32) if ragged else engine.encode_int32(x, 32)).cpu()
    took_fallback = engine.f16_reruns > before
    bad = []
    for i in (0, 1):
        F = encoded_length(lengths[i])
        alone = engine.encode_int32(x[i:i + 1, :lengths[i]].contiguous(), 32).cpu()
        if not torch.equal(got[i, :, :F], alone[0]):
            bad.append((("speech", "click")[i], int((got[i, :, :F] != alone[0]).sum()), alone[0].numel()))
    assert not bad, bad
    assert took_fallback
