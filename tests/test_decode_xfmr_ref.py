"""CPU: the decoder transformer's per-stage float64 reference (tests/decode_xfmr_ref.py), the adversarial decode
checkpoints (tests/decode_adversarial.py), and what the per-stage conditions see that the whole-decode checks do not.

(a) every adversarial case reaches the regime it is named for, measured in float64;
(b) torch-CPU fp32 meets the hard and the working condition on all five stages of every case, so the conditions are
    sound where the GPU tests (tests/test_decode_xfmr_gpu.py) apply them;
(c) THE GAP: three value-only faults in the attention of decoder layer 3 at T = 130 (260 rows, window 250) -- keys
    counted from the oldest in the row's window, t >= 64 being a lane's second and later keys in
    attention_stream_kernel -- pass the checks applied at that shape before these tests (waveform rel_err < 1e-4; the
    fp16 fault even 16 x the fp32 reference's error on the whole transformer) and miss the attention stage's working
    condition;
(d) one fault per other stage misses that stage's working condition;
(e) the slot-wise concatenation of a staggered schedule's per-step taps equals the whole-sequence stages.

Shapes: window 70 at B = 2 x T = 40 (the window's edge inside the sequence), layers 0 and 7; the one T = 130 table.
Every figure is printed; none is copied from a text.
"""
import json

import pytest
import torch

import decode_adversarial as dadv
import decode_ref
import decode_stage_ref as dsr
import decode_xfmr_ref as dxr

W70, T40 = 70, 40
ENDS = (0, dxr.LAYERS - 1)
ACT_TOL = 1e-4   # the waveform bound of tests/test_decode_stream_gpu.py

# case -> (checkpoint, codes, K); every case at B = 2 x T = 40, window 70
CASES = {name: (name, "random", 8) for name in dadv.ADVERSARIAL}
CASES.update({"zero": ("zero", "zeros", 8), "constant": (None, "constant", 8), "base": (None, "random", 8),
              "K1": (None, "random", 1), "K32": (None, "random", 32)})


@pytest.fixture(scope="module")
def base():
    return dadv.base_state_dict()


@pytest.fixture(scope="module")
def chains(base):
    """case -> (decoder view, fp32 chain of all 40 stages on the case's own upsample tap)."""
    out = {}
    for case, (ckpt, codes, K) in CASES.items():
        sd = dadv.CHECKPOINTS[ckpt](base) if ckpt else base
        x = dxr.upsample_tap(dadv.CODES[codes](T40, 2, K, T40), sd)
        dsd = dxr.view(sd)
        out[case] = (dsd, dxr.chain(x, dsd, W70))
    return out


def ln_inputs(taps):
    for l in range(dxr.LAYERS):
        yield f"ln1.{l}", taps[dxr.FIRST] if l == 0 else taps[f"xfmr{l - 1}"]
        yield f"ln2.{l}", taps[f"oproj{l}"]


# ---- (a) regimes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(dadv.CHECKPOINTS) + ["constant"])
def test_case_reaches_its_regime(chains, case):
    dsd, taps = chains[case]
    reg = dadv.regimes(taps, ENDS, W70)
    print(json.dumps({"case": case, "regimes": reg}))
    for l in ENDS:
        att, ln = reg[l]["attention"], reg[l]["ln1"]
        if case == "peaky3":
            assert att["score_range"] >= 30 and 0.5 <= att["median_top_weight"] < 0.999, (l, att)
        elif case == "peaky8":
            assert att["median_top_weight"] >= 0.999 and att["score_range"] >= 100, (l, att)
        elif case == "flat":
            assert att["score_range"] == 0.0, (l, att)
        elif case == "massive":
            assert ln["max_over_median"] >= 1e3, (l, ln)
    if case == "offset":  # every row of every LayerNorm input of every layer
        ratios = {n: dadv.layernorm_regime(x)["min_mean_over_std"] for n, x in ln_inputs(taps)}
        print(json.dumps({"case": case, "min_mean_over_std": ratios}))
        assert min(ratios.values()) >= 1e3, ratios
    if case == "zero":
        assert float(taps[dxr.FIRST].abs().max()) == 0.0
        assert float(taps["xfmr0"].abs().max()) > 0.0   # the updates alone
    if case == "constant":  # the keys of one row parity tie exactly: at layer 0 every even row is the same row
        x = taps[dxr.FIRST]
        assert torch.equal(x[:, 2:-2:2], x[:, 4::2]) and torch.equal(x[:, 3:-2:2], x[:, 5::2])


# ---- (b) the reference inside the conditions ------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_reference_meets_both_conditions(chains, case):
    dsd, taps = chains[case]
    bad, worst = [], 0.0
    for name in dxr.names(ENDS):
        rec = dxr.measure(name, taps, dsd, W70)
        print(json.dumps({"case": case, **rec}))
        worst = max(worst, rec["q_ref"] / rec["n"])
        bad += dxr.failures(rec, key="q_ref")
    print(json.dumps({"case": case, "max_q_ref_over_n": worst}))
    assert not bad, bad


# ---- (c) the gap ----------------------------------------------------------------------------------------------------
FAULT_LAYER = 3


def seanet64(x_btc, sd64):
    return decode_ref.seanet_decoder(x_btc.transpose(1, 2), sd64, dxr.CFG)


def test_layer3_attention_faults_pass_the_whole_checks_and_miss_the_stage(base):
    sdt = decode_ref.as_tensors(base)
    dsd = dxr.view(base)
    sd64 = {k: v.double() for k, v in sdt.items() if k.startswith("decoder.")}
    x = dxr.upsample_tap(dadv.random_codes(130, 1, 8, 130), base)
    assert x.shape == (1, 260, 512)
    ref = dxr.chain(x, dsd, None, torch.float64)
    f32 = dxr.chain(x, dsd, None, torch.float32)
    last = f"xfmr{dxr.LAYERS - 1}"
    rel_ref = dsr.rel_err(f32[last], ref[last])
    whole_bound = dsr.WORKING_FACTOR * max(rel_ref, dsr.U)
    audio_ref = seanet64(ref[last], sd64)
    att = f"att{FAULT_LAYER}"
    clean = dxr.measure(att, ref, dsd)   # q_ref: torch-CPU fp32 on the float64 chain's own qkv3
    print(json.dumps({"T": 130, "rel_err_ref": rel_ref, "whole_bound": whole_bound, "att_q_ref": clean["q_ref"],
                      "att_working_bound": dsr.working_bound(clean["q_ref"]), "att_n": clean["n"]}))
    assert not dxr.failures(clean, key="q_ref"), clean
    rows = []
    for kind in ("weights", "fp16", "bf16"):
        fault = dxr.att_fault(kind)
        got = dxr.chain(x, dsd, None, torch.float64, fault={att: fault})
        rec = dxr.measure(att, ref, dsd, got=got[att])   # (the layers before the fault are exact: the same qkv3)
        row = {"fault": kind, "xfmr7_rel_err": dsr.rel_err(got[last], ref[last]),
               "audio_rel_err": dsr.rel_err(seanet64(got[last], sd64), audio_ref), "att_q": rec["q_engine"],
               "att_margin": rec["q_engine"] / dsr.working_bound(rec["q_ref"]), "worst": rec["worst"]}
        rows.append(row)
        print(json.dumps(row))
        # passes what was applied at this shape ...
        assert row["audio_rel_err"] < ACT_TOL, row
        if kind == "fp16":
            assert row["xfmr7_rel_err"] <= whole_bound, (row, whole_bound)
        # ... and misses the stage's working condition
        assert any("working condition" in f for f in dxr.failures(rec)), (row, rec)
        assert row["att_margin"] > 2.0, row
    # the first fault in all eight layers at once still passes the waveform check
    every = dxr.chain(x, dsd, None, torch.float64, fault={f"att{l}": dxr.att_fault("weights") for l in range(dxr.LAYERS)})
    all8 = dsr.rel_err(seanet64(every[last], sd64), audio_ref)
    print(json.dumps({"fault": "weights, all 8 layers", "audio_rel_err": all8}))
    assert all8 < ACT_TOL, all8


# ---- (d) one fault per other stage ------------------------------------------------------------------------------------
def test_per_stage_faults_miss_their_working_condition(chains):
    step_boundary = 14   # row 14 = the first row of a step that starts at frame 7
    table = [("base", "qkv7", dxr.qkv_rope_restart(7, step_boundary, W70), torch.float64),
             ("base", "oproj0", dxr.oproj_next_scale(0), torch.float64),
             ("offset", "ff7", dxr.ff_one_pass_variance(7), torch.float32),
             ("base", "xfmr7", dxr.xfmr_dropped_column(7), torch.float64)]
    for case, name, fault, dtype in table:
        dsd, taps = chains[case]
        st = dxr.stages(W70)[name]
        with torch.no_grad():
            got = fault([taps[s] for s in st.source], dsd, dtype)
        rec = dxr.measure(name, taps, dsd, W70, got=got)
        row = {"case": case, "stage": name, "q": rec["q_engine"], "bound": dsr.working_bound(rec["q_ref"]),
               "q_ref": rec["q_ref"], "whole_tensor": dsr.rel_err(got, st.ref([taps[s] for s in st.source], dsd, dxr.AR)[0])}
        print(json.dumps(row))
        assert not dxr.failures(rec, key="q_ref"), rec
        assert any("working condition" in f for f in dxr.failures(rec)), row
    # the one-pass variance is invisible on the base checkpoint: `offset` is what catches it
    dsd, taps = chains["base"]
    with torch.no_grad():
        got = dxr.ff_one_pass_variance(7)([taps["oproj7"]], dsd, torch.float32)
    rec = dxr.measure("ff7", taps, dsd, W70, got=got)
    print(json.dumps({"case": "base", "stage": "ff7", "q": rec["q_engine"], "bound": dsr.working_bound(rec["q_ref"])}))
    assert not dxr.failures(rec), rec


# ---- (e) slots --------------------------------------------------------------------------------------------------------
def play_slots(base, by_item=False):
    """The schedule of the GPU slot test on the CPU step reference: -> {session: taps of its concatenation}."""
    dsd = dxr.view(base)
    sessions = dxr.slot_sessions()
    xs = {name: dxr.upsample_tap(codes, base).double() for name, codes in sessions.items()}
    pool = [dxr.StepXfmr(dsd, W70) for _ in range(dxr.SLOTS)]
    cat = dxr.Concat([dxr.FIRST] + dxr.names())
    at = {name: 0 for name in sessions}
    order = {s: [] for s in range(dxr.SLOTS)}
    for op in dxr.slot_schedule():
        if op[0] == "reset":
            pool[op[1]].reset()
            cat.cut(op[1])
            continue
        _, items, n = op
        step = [pool[s].step(xs[name][:, 2 * at[name]:2 * (at[name] + n)]) for s, name in items]
        taps = {k: torch.cat([t[k] for t in step], dim=0) for k in cat.names}
        cat.add(taps, None if by_item else [s for s, _ in items])
        for s, name in items:
            at[name] += n
            if name not in order[s]:
                order[s].append(name)
    assert all(at[name] == sessions[name].shape[2] for name in sessions), at
    seqs = cat.sequences()
    return dsd, xs, {name: seqs[s][i] for s in order for i, name in enumerate(order[s]) if s in seqs and i < len(seqs[s])}


def test_slot_schedule_is_staggered():
    sched = dxr.slot_schedule()
    steps = [op for op in sched if op[0] == "step"]
    assert sum(op[0] == "reset" for op in sched) == 1
    assert {len(op[1]) for op in steps} == {1, 2, 3} and {op[2] for op in steps} == {1, 2, 3}
    assert any([s for s, _ in op[1]] != sorted(s for s, _ in op[1]) for op in steps)   # a permuted listing
    frames = {name: c.shape[2] for name, c in dxr.slot_sessions().items()}
    assert max(frames.values()) == T40 and 2 * T40 > W70 - 1 + 2 * dxr.SLOT_MAX_STEP   # the longest wraps its ring


def test_slotwise_concatenation_equals_the_whole_sequence(base):
    dsd, xs, got = play_slots(base)
    assert sorted(got) == sorted(xs)
    worst = 0.0
    for name, taps in got.items():
        assert torch.equal(taps[dxr.FIRST], xs[name])
        for stage in dxr.names():
            rec = dxr.measure(stage, taps, dsd, W70, got=taps[stage])
            worst = max(worst, rec["q_engine"])
            assert rec["q_engine"] < 1e-3, (name, rec)   # float64 against float64: 2^-29 units of its roundings
    print(json.dumps({"slots": "float64 concatenation vs whole sequence", "max_q": worst}))
    # filed by the item's place in the step instead of its slot, the concatenations are not the sequences
    _, _, wrong = play_slots(base, by_item=True)
    assert any(name not in wrong or wrong[name][dxr.FIRST].shape != xs[name].shape
               or not torch.equal(wrong[name][dxr.FIRST], xs[name]) for name in xs)
