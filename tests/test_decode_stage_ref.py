"""CPU: the per-stage float64 checker of the decode path (tests/decode_stage_ref.py) checked itself.

(a) torch-CPU's fp32 evaluation of every stage meets the hard and the working condition against the float64 reference
    of the same stage on the same input (the taps of ``decode_ref.decode`` at B = 2, T = 13, K = 8);
(b) the same fp32 stage with one fault injected misses the working condition by at least 100 x: the proof that
    tests/test_decode_kernels.py would fail on a subtly wrong kernel.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_ref
import decode_stage_ref as dsr
from mimi_hip import synthetic

ACT_TOL = 1e-4
MARGIN = 100.0
B, T, K = 2, 13, 8


@pytest.fixture(scope="module")
def full_sd(state_dict):
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    return decode_ref.as_tensors(sd)


@pytest.fixture(scope="module")
def inputs(full_sd):
    """The input tensor of every stage: the taps of one fp32 reference decode."""
    codes = torch.from_numpy(np.random.default_rng(0).integers(0, 2048, (B, K, T)))
    taps = {}
    decode_ref.decode(codes, full_sd, taps=taps)
    x = {"codes": codes, "quantized": taps["quantized"], "upsample": taps["upsample"], "xfmr7": taps["xfmr7"],
         "dconv0_elu": F.elu(taps["dconv0"])}
    for s in range(4):
        x[f"up{s}"] = taps[f"up{s}"]
        x[f"dres{s}_elu"] = F.elu(taps[f"dres{s}"])
    return x


@pytest.fixture(scope="module")
def baseline(inputs, full_sd):
    """{stage: (ref64, mag64, q_ref, n)}, computed once."""
    out = {}
    for name, st in dsr.STAGES.items():
        x = inputs[st.source]
        ref64, mag64 = st.ref(x, full_sd)
        out[name] = (ref64, mag64, dsr.q_metric(st.f32(x, full_sd), ref64, mag64), int(st.n(x, full_sd)))
    return out


def test_stage_table_is_complete():
    assert list(dsr.STAGES) == ["quantized", "upsample", "dconv0", "dconv0_elu", "up0", "dres0_elu", "up1",
                                "dres1_elu", "up2", "dres2_elu", "up3", "dres3_elu", "audio"]


def test_stage_shapes_and_bounds(inputs, baseline):
    shapes = {"quantized": (512, T), "upsample": (512, 2 * T), "dconv0": (1024, 2 * T),
              "dconv0_elu": (1024, 2 * T), "up0": (512, 16 * T), "dres0_elu": (512, 16 * T), "up1": (256, 96 * T), "dres1_elu": (256, 96 * T), "up2": (128, 480 * T),
              "dres2_elu": (128, 480 * T), "up3": (64, 1920 * T), "dres3_elu": (64, 1920 * T), "audio": (1, 1920 * T)}
    ns = {"quantized": 512 + K + 2, "upsample": 4, "dconv0": 3586, "dconv0_elu": 3587, "up0": 2050, "up1": 1026,
          "up2": 514, "up3": 258,
          "dres0_elu": 1538 + 258 + 4, "dres1_elu": 770 + 130 + 4, "dres2_elu": 386 + 66 + 4,
          "dres3_elu": 194 + 34 + 4, "audio": 194}
    for name, (ref64, mag64, _, n) in baseline.items():
        assert tuple(ref64.shape) == (B,) + shapes[name] == tuple(mag64.shape), name
        assert ref64.dtype == mag64.dtype == torch.float64
        assert n == ns[name], (name, n)
        assert bool((mag64 >= ref64.abs() * (1 - 1e-12)).all()), name  # a condition sum bounds its own sum


def test_fp32_reference_meets_both_conditions(baseline):
    """(a) for every row of the table."""
    table = {}
    for name, (_, _, q_ref, n) in baseline.items():
        table[name] = round(q_ref, 3)
        rec = {"stage": name, "n": n, "q_ref": q_ref}
        assert not dsr.failures(rec, key="q_ref"), rec
    print(json.dumps({"q_ref": table}))


def test_float64_references_agree_with_decode_ref(inputs, baseline, full_sd):
    """The single-stage float64 evaluations restate decode_ref's stages: each equals the next fp32 tap within fp32
    rounding (which is (a) read the other way: q of the tap that decode_ref itself produced)."""
    taps = {}
    decode_ref.decode(inputs["codes"], full_sd, taps=taps)
    for name, (ref64, mag64, _, n) in baseline.items():
        got = F.elu(taps[name[:-4]]) if name.endswith("_elu") else taps[name]
        assert dsr.q_metric(got, ref64, mag64) <= n, name


def test_transformer_fp32_against_float64(inputs, full_sd):
    ref64 = dsr.transformer(inputs["upsample"], full_sd)
    assert ref64.dtype == torch.float64 and tuple(ref64.shape) == (B, 512, 2 * T)
    err = dsr.rel_err(inputs["xfmr7"], ref64)
    assert err < ACT_TOL, err
    assert err > 0.0  # (an fp32 evaluation is not the float64 one)


# ---- (b) injected faults --------------------------------------------------------------------------------------------
def _up_w(s):
    return f"decoder.layers.{2 + 3 * s}.conv.weight"


def fault_dropped_weight(x, sd, s, index=None):
    """One weight of up-conv s set to zero: the one of largest magnitude (a dropped weight near zero changes nothing
    and no test can see it; test_arbitrary_dropped_weight_misses_working_condition takes one without looking), or the
    given index."""
    sd = dict(sd)
    w = sd[_up_w(s)].clone()
    if index is None:
        index = tuple(int(i) for i in torch.unravel_index(w.abs().argmax(), w.shape))
    w[index] = 0.0
    sd[_up_w(s)] = w
    return dsr.STAGES[f"up{s}"].f32(x[dsr.STAGES[f"up{s}"].source], sd)


def fault_batch_leak(x, sd):
    """conv 0 on the items laid end to end with no zero rows between them."""
    xi = x["xfmr7"]
    flat = torch.cat(list(xi), dim=-1)[None]
    y = dsr.STAGES["dconv0"].f32(flat, sd)
    return torch.stack(y[0].split(xi.shape[-1], dim=-1))


def fault_phase_swap(x, sd, s=1):
    y = dsr.STAGES[f"up{s}"].f32(x[dsr.STAGES[f"up{s}"].source], sd)
    r = dsr.CFG.upsampling_ratios[s]
    v = y.view(y.shape[0], y.shape[1], -1, r).clone()
    v[..., [0, 1]] = v[..., [1, 0]]
    return v.view_as(y)


def fault_tap_swap(x, sd, s=2):
    """x[t] and x[t - 1] exchanged: the two halves of the transposed conv's kernel."""
    sd = dict(sd)
    r = dsr.CFG.upsampling_ratios[s]
    w = sd[_up_w(s)]
    sd[_up_w(s)] = torch.cat([w[..., r:], w[..., :r]], dim=-1)
    return dsr.STAGES[f"up{s}"].f32(x[dsr.STAGES[f"up{s}"].source], sd)


def fault_no_bias(x, sd):
    sd = dict(sd)
    sd["decoder.layers.14.conv.bias"] = torch.zeros_like(sd["decoder.layers.14.conv.bias"])
    return dsr.STAGES["audio"].f32(x["dres3_elu"], sd)


def fault_upsample_w12(x, sd):
    sd = dict(sd)
    w = sd["upsample.conv.weight"].clone()
    w[:, :, [1, 2]] = w[:, :, [2, 1]]
    sd["upsample.conv.weight"] = w
    return dsr.STAGES["upsample"].f32(x["quantized"], sd)


FAULTS = [
    ("up0_weight_zeroed", "up0", lambda x, sd: fault_dropped_weight(x, sd, 0)),
    ("up1_weight_zeroed", "up1", lambda x, sd: fault_dropped_weight(x, sd, 1)),
    ("up2_weight_zeroed", "up2", lambda x, sd: fault_dropped_weight(x, sd, 2)),
    ("up3_weight_zeroed", "up3", lambda x, sd: fault_dropped_weight(x, sd, 3)),
    ("conv0_item1_sees_item0", "dconv0", fault_batch_leak),
    ("up1_phases_swapped", "up1", fault_phase_swap),
    ("up2_taps_swapped", "up2", fault_tap_swap),
    ("last_conv_bias_omitted", "audio", fault_no_bias),
    ("upsample_w1_w2_exchanged", "upsample", fault_upsample_w12),
]


@pytest.mark.parametrize("label,stage,fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_injected_fault_misses_working_condition_by_100x(inputs, baseline, full_sd, label, stage, fault):
    ref64, mag64, q_ref, n = baseline[stage]
    q = dsr.q_metric(fault(inputs, full_sd), ref64, mag64)
    bound = dsr.working_bound(q_ref)
    print(json.dumps({"fault": label, "q": q, "q_ref": q_ref, "working_bound": bound}))
    assert q >= MARGIN * bound, (label, q, bound)


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_arbitrary_dropped_weight_misses_working_condition(inputs, baseline, full_sd, s):
    """A weight picked without looking (index [5, 7, 3]) is one term of K = 2 Cin <= 2048 in its output's condition
    sum: q ~ 2^24 / K >= 8192 against a working bound of at most 16 x 6.5 = 104.  Asserted at 10 x the bound, which
    leaves a term 8 x below the average one still caught (measured: 74 x for up-conv 0, 700 - 5000 x for the others)."""
    ref64, mag64, q_ref, _ = baseline[f"up{s}"]
    q = dsr.q_metric(fault_dropped_weight(inputs, full_sd, s, index=(5, 7, 3)), ref64, mag64)
    print(json.dumps({"fault": f"up{s}_w[5,7,3]_zeroed", "q": q, "working_bound": dsr.working_bound(q_ref)}))
    assert q >= 10.0 * dsr.working_bound(q_ref), (s, q, q_ref)


def test_project_metric_is_the_coarser_one(inputs, baseline, full_sd):
    """The dropped up-conv 0 weight stands further over the working bound (measured 852 x) than over the project
    metric's tolerance on the same tensor (198 x), and that before any later stage dilutes it: a tap compared end to
    end carries every earlier stage's error, this one only its own."""
    ref64, mag64, q_ref, _ = baseline["up0"]
    bad = fault_dropped_weight(inputs, full_sd, 0)
    over_q, over_rel = dsr.q_metric(bad, ref64, mag64) / dsr.working_bound(q_ref), dsr.rel_err(bad, ref64) / ACT_TOL
    print(json.dumps({"fault": "up0_weight_zeroed", "q_over_bound": over_q, "rel_err_over_tol": over_rel}))
    assert over_q > over_rel
