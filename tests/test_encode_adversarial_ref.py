"""CPU: the adversarial encode cases (tests/encode_adversarial.py) checked themselves, before the GPU runs them.

(1) each crafted checkpoint reaches the regime it claims, measured in the float64-checked fp32 chain (printed, and
    asserted where the case names a number);
(2) on every case torch-fp32 meets the hard condition q <= n and the f16x3 emulation q <= n + c, on every stage the
    case changes (checkpoints: from the final conv on; audio: every stage) -- so a miss on the GPU is the kernel's, not
    the reference's.  The audio cases take their plane scales from full-level speech (``speech_scales``): the engine's
    scales are fixed by calibration, a quiet clip does not get scales of its own;
(3) five faults of the transformer kernels, each a CPU variant of its stage, miss the working condition on their
    adversarial case.  Whether speech on the base checkpoint catches them too is printed beside it (nothing asserted):
    that column is the gap these cases close.  The table is kept in profiles/encode_adversarial_mutants.txt.
"""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import encode_adversarial as adv
import encode_stage_ref as esr

B, L13, L250 = 2, 12480, 240000
NAMES = list(esr.STAGES)
FRONT = NAMES[:NAMES.index("encoder")]          # SEANet up to the final conv's input: the same for every checkpoint
REST = NAMES[NAMES.index("encoder"):]
ENDS = [s for l in (0, adv.LAYERS - 1) for s in (f"qkv{l}", f"att{l}", f"oproj{l}", f"ff{l}", f"xfmr{l}")]
H, D = esr.CFG.num_attention_heads, esr.CFG.head_dim


@pytest.fixture(scope="module")
def base():
    return adv.base_state_dict()


@pytest.fixture(scope="module")
def sds(base):
    cache = {"base": adv.torch_sd(base)}

    def get(name):
        if name not in cache:
            cache[name] = adv.torch_sd(adv.CHECKPOINTS[name](base))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def chains(sds):
    """chain(name, L) -> the fp32 taps of checkpoint ``name`` on B = 2 speech clips of L samples; the SEANet taps are
    computed once per length."""
    fronts, cache = {}, {}

    def get(name, L):
        if L not in fronts:
            fronts[L] = esr.chain_f32(adv.speech_batch(B, L, 77), sds("base"), names=set(FRONT))
        if (name, L) not in cache:
            taps = dict(fronts[L])
            with torch.no_grad():
                for n in REST:
                    st = esr.STAGES[n]
                    taps[n] = st.f32([taps[s] for s in st.source], sds(name))
            cache[name, L] = taps
        return cache[name, L]
    return get


def ln_input(taps, l):
    return taps["encoder" if l == 0 else f"xfmr{l - 1}"]


# ---- (1) regimes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base"] + list(adv.CHECKPOINTS))
def test_case_reaches_its_regime(chains, name):
    reg = {}
    for frames, L in ((13, L13), (250, L250)):
        if frames == 250 and name not in ("base",) + adv.ATTENTION_CASES:
            continue
        taps = chains(name, L)
        for l in (0, adv.LAYERS - 1):
            reg[f"att{l}_F{frames}"] = adv.attention_regime(taps[f"qkv{l}"])
            reg[f"ln{l}_F{frames}"] = adv.layernorm_regime(ln_input(taps, l))
    print(json.dumps({"case": name, "regime": reg}))
    if name == "base":  # the benign corner every earlier test measured in
        assert reg["att0_F13"]["score_range"] < 10 and reg["ln0_F13"]["max_mean_over_std"] < 0.2
    if name == "peaky8":
        for k in ("att0_F13", "att7_F13", "att0_F250", "att7_F250"):
            assert reg[k]["score_range"] >= 60, (k, reg[k])
        assert reg["att0_F250"]["max_later_chunk_changes"] >= 2 and reg["att0_F250"]["rows_with_2_changes"] > 0
        assert reg["att7_F250"]["max_later_chunk_changes"] >= 2
    if name == "flat":
        assert all(reg[k]["max_abs_score"] == 0.0 for k in reg if k.startswith("att")), reg
        assert reg["att0_F250"]["min_top_weight"] == pytest.approx(1.0 / 250)
    if name == "offset":
        assert all(reg[k]["min_mean_over_std"] >= 1e3 for k in ("ln0_F13", "ln7_F13")), reg
    if name == "massive":
        assert all(reg[k]["max_over_median"] >= 1e3 for k in ("ln0_F13", "ln7_F13")), reg
    if name == "onehot":
        r = reg["ln0_F13"]
        assert abs(r["max_normalised"] / r["sqrt_C_minus_1"] - 1.0) < 0.01, r


# ---- (2) the references stay inside the hard condition ------------------------------------------------------------------
def assert_references(recs):
    for rec in recs:
        assert rec["q_ref"] <= rec["n"], rec
        assert not esr.conditions(rec, key="q_ref"), rec
        if rec["q_emul"] is not None:
            assert rec["q_emul"] <= rec["n"] + rec["c"], rec
            assert not esr.conditions(rec, key="q_emul"), rec


def summary(recs):
    out = {}
    for r in recs:
        out[f"{r['stage']}[{r['mode']}]"] = (round(r["q_ref"], 3), None if r["q_emul"] is None else round(r["q_emul"], 3),
                                             r["n"], r["c"])
    return out


@pytest.mark.parametrize("name", list(adv.CHECKPOINTS))
def test_references_on_checkpoint(chains, sds, name):
    recs = []
    for frames, L, stages in ((13, L13, REST), (250, L250, ENDS)):
        if frames == 250 and name not in adv.ATTENTION_CASES:
            continue
        taps = chains(name, L)
        for mode in ("f32", "f16x3"):
            ar = esr.Arith(mode)
            recs += [esr.measure(s, [taps[i] for i in esr.STAGES[s].source], sds(name), ar, f32=taps[s]) for s in stages]
    print(json.dumps({"case": name, "q_ref, q_emul, n, c": summary(recs),
                      "max q_ref / n": max(r["q_ref"] / r["n"] for r in recs)}))
    assert_references(recs)


@pytest.fixture(scope="module")
def scales(chains, sds):
    return adv.speech_scales(sds("base"), chains("base", L13))


@pytest.mark.parametrize("name", adv.FINITE_AUDIO)
def test_references_on_degenerate_audio(sds, scales, name):
    """Item 0 the case, item 1 speech; the plane scales those of full-level speech."""
    sd = sds("base")
    taps = esr.chain_f32(adv.audio_batch(name, L13, 78), sd)
    recs = []
    for ar in (esr.Arith("f32"), esr.Arith("f16x3", scales)):
        recs += [esr.measure(s, [taps[i] for i in esr.STAGES[s].source], sd, ar, f32=taps[s]) for s in NAMES]
    print(json.dumps({"audio": name, "q_ref, q_emul, n, c": summary(recs),
                      "max q_ref / n": max(r["q_ref"] / r["n"] for r in recs)}))
    assert all(bool(torch.isfinite(t).all()) for t in taps.values())
    assert_references(recs)


def test_nonfinite_clips_have_no_reference(sds):
    """The reference spreads one NaN to every frame of the item (P @ V sums 0 x NaN), and an Inf becomes NaN in the
    first conv (Inf x w - Inf x w'): nothing to hold the engine's codes of these items to."""
    sd = sds("base")
    for name in ("inf", "nan"):
        taps = esr.chain_f32(adv.audio_batch(name, L13, 78), sd, names=set(FRONT + REST[:REST.index("xfmr0") + 1]))
        assert bool(torch.isnan(taps["xfmr0"][0]).any(dim=-1).all()), name
        assert bool(torch.isfinite(taps["xfmr0"][1]).all()), name  # the batch-mate is untouched


# ---- (3) mutants --------------------------------------------------------------------------------------------------------
def attention_chunked(x, skip_corr_chunk=None, drop_p_lo=False, leak_key=False):
    """attn_h16.h attn_chunk_h16 in float64: 32-key chunks from key 0, online softmax (m, l, corr), the weights split
    into fp16 hi + lo planes at 2^14 before P V.  Faults: ``skip_corr_chunk`` -- the output accumulator is not rescaled
    by corr in that chunk; ``drop_p_lo`` -- only the hi plane of p meets V; ``leak_key`` -- the first key past the causal
    limit (j = i + 1) is weighted exp(s - m) instead of 0."""
    q, k, v = esr.heads(x.double())
    T = q.shape[2]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D)
    mask = esr.att_mask(T)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    wmask = mask | (j == i + 1) if leak_key else mask
    m = torch.full(s.shape[:-1], float("-inf"), dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for ci, c0 in enumerate(range(0, T, adv.CHUNK)):
        sc, mk, wk = s[..., c0:c0 + adv.CHUNK], mask[:, c0:c0 + adv.CHUNK], wmask[:, c0:c0 + adv.CHUNK]
        mnew = torch.maximum(m, sc.masked_fill(~mk, float("-inf")).amax(-1))
        corr = torch.where(torch.isinf(m), torch.zeros_like(m), (m - mnew).exp())
        pv = torch.where(wk & torch.isfinite(mnew)[..., None], (sc - mnew[..., None]).exp(), torch.zeros_like(sc))
        l = l * corr + pv.sum(-1)
        hi, lo = esr.split_f16(pv, 2.0 ** 14)
        p = (hi if drop_p_lo else hi + lo) / 2.0 ** 14
        oc = torch.ones_like(corr) if ci == skip_corr_chunk else corr
        o = o * oc[..., None] + p @ v[..., c0:c0 + adv.CHUNK, :]
        m = mnew
    out = o / l[..., None]
    return out.transpose(1, 2).reshape(x.shape[0], T, H * D)


def qkv_with_layernorm(l, ln):
    """esr.qkv_value in fp32 with the LayerNorm replaced by ``ln(x, gamma, beta)``."""
    p = esr._lp(l)

    def f(xs, sd):
        x = xs[0].float()
        Bq, T, _ = x.shape
        cos, sin = esr._rope_tables(torch.arange(T), torch.float32)
        h = ln(x, esr._w(sd, p + "input_layernorm.weight", torch.float32), esr._w(sd, p + "input_layernorm.bias", torch.float32))
        out = []
        for name in ("q", "k", "v"):
            t = F.linear(h, esr._w(sd, p + f"self_attn.{name}_proj.weight", torch.float32)).view(Bq, T, H, D)
            if name != "v":
                t = (t * cos) + (esr.mimi_ref.rotate_half(t) * sin)
            out.append(t.reshape(Bq, T, H * D))
        return torch.cat(out, dim=-1)
    return f


def ln_one_pass(x, g, b):
    """LayerNorm with the variance as E[x^2] - mean^2 in fp32 (clamped at 0)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp(min=0.0)
    return (x - mean) * (var + esr.CFG.norm_eps).rsqrt() * g + b


def ln_two_pass(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, esr.CFG.norm_eps)


def oproj_residual_in_one_plane(xs, sd):
    """o_proj of layer 0 with the residual x read from ONE fp16 plane at its tensor's fixed scale, not as fp32.  (Read
    from both planes, hi + lo, it would carry 2^-22 |x| = 4 units: the harness's own allowance for a planes tensor,
    ``Stage.planes_out``, and inside the working factor by construction -- measured here at q = 9.4 against a bound of
    21.8 on ``massive``; that is an arithmetic the conditions permit, not a fault they could name.)"""
    a, x = xs[0].float(), xs[1].float()
    p = esr._lp(0)
    s = esr.pow2_floor_scale(float(x.abs().max()), 7)
    hi, _ = esr.split_f16(x, s)
    return (hi / s).float() + esr._w(sd, p + "self_attn_layer_scale.scale", torch.float32) * F.linear(
        a, esr._w(sd, p + "self_attn.o_proj.weight", torch.float32))


# (label, stage, adversarial case, frames there, variant(xs, sd) -> the stage's output)
MUTANTS = [
    ("attention_corr_rescale_left_out_in_chunk_1", "att0", "peaky8", 250, lambda xs, sd: attention_chunked(xs[0], skip_corr_chunk=1)),
    ("attention_p_lo_plane_dropped", "att0", "peaky3", 13, lambda xs, sd: attention_chunked(xs[0], drop_p_lo=True)),
    ("attention_masked_key_weighted_exp", "att0", "peaky8", 13, lambda xs, sd: attention_chunked(xs[0], leak_key=True)),
    ("layernorm_variance_one_pass_fp32", "qkv0", "offset", 13, qkv_with_layernorm(0, ln_one_pass)),
    ("residual_added_in_plane_precision", "oproj0", "massive", 13, oproj_residual_in_one_plane),
]


def margin(chains, sds, case, frames, stage, variant):
    taps, sd = chains(case, L13 if frames == 13 else L250), sds(case)
    xs = [taps[s] for s in esr.STAGES[stage].source]
    ar = esr.Arith("f16x3")
    rec = esr.measure(stage, xs, sd, ar, f32=taps[stage])
    with torch.no_grad():
        got = variant(xs, sd)
    ref64, mag64 = esr.STAGES[stage].ref(xs, sd, ar)
    q = esr.q_metric(got, ref64, mag64)
    q = q if math.isfinite(q) else float("inf")  # (a NaN output is a miss, not a comparison that says nothing)
    bound = esr.working_bound(max(rec["q_ref"], rec["q_emul"] or 0.0))
    return q, bound, esr.rel_err(torch.nan_to_num(got.double(), nan=1e300, posinf=1e300, neginf=-1e300), ref64)


def test_unfaulted_variants_meet_the_working_condition(chains, sds):
    """The variants without their fault are the stage: the margins below are the faults', not the variants'."""
    for case, frames in (("peaky8", 250), ("flat", 250), ("peaky8", 13), ("base", 250)):
        q, bound, _ = margin(chains, sds, case, frames, "att0", lambda xs, sd: attention_chunked(xs[0]))
        assert q <= bound, (case, frames, q, bound)
    for case in ("offset", "base"):
        q, bound, _ = margin(chains, sds, case, 13, "qkv0", qkv_with_layernorm(0, ln_two_pass))
        assert q <= bound, (case, q, bound)


def test_mutants_miss_on_their_adversarial_case(chains, sds):
    rows = []
    for label, stage, case, frames, variant in MUTANTS:
        q, bound, old = margin(chains, sds, case, frames, stage, variant)
        qb, bb, oldb = margin(chains, sds, "base", frames, stage, variant)
        rows.append({"mutant": label, "stage": stage, "case": f"{case}_F{frames}", "q": q, "working_bound": bound,
                     "margin": q / bound, "whole_tensor_metric": old, "base_q": qb, "base_bound": bb,
                     "base_margin": qb / bb, "base_misses": qb > bb, "base_whole_tensor_metric": oldb})
        print(json.dumps(rows[-1]))
    for r in rows:
        assert r["margin"] > 1.0, r
