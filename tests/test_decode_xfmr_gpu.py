"""GPU: the decoder transformer held to float64 STAGE BY STAGE, in every decode form and on adversarial checkpoints.

The engine taps ``qkv{l}``, ``att{l}``, ``oproj{l}``, ``ff{l}``, ``xfmr{l}`` of every decoder layer (engine.cpp
run_transformer_f32 and the stream step).  Each stage is evaluated in float64 on the tap(s) the engine itself read
(tests/decode_xfmr_ref.py, on the stage table of tests/encode_stage_ref.py) and held to the two derived conditions of
tests/decode_stage_ref.py: HARD q <= n, WORKING q <= 16 max(q_ref, 1), q_ref torch-CPU fp32 on the same input.
tests/test_decode_xfmr_ref.py shows on the CPU what these conditions catch that the whole-decode checks do not.

    form                      shape                                         attention launch
    whole                     B = 2 x T = 13, all 40 stages                 attention_t256_kernel
    whole, window 70          B = 2 x T = 40, all 40 stages                 attention_t256_kernel, window edge inside
    whole                     B = 1 x T = 129 (258 rows), layers 0 and 7    attention_kernel (banded)
    ragged                    (3, 13, 130) frames, layers 0 and 7           both ragged launches in one pass
    stream, window 70         B = 2 x T = 40, steps of 1 on the smallest    attention_stream_kernel: ring of 71 rows
                              ring, and steps [7, 7, 7, 7, 7, 5]; all       wrapped, eviction, 70 keys > 64 per row,
                              40 stages                                     every cnt % 4
    stream, window 250        B = 1 x T = 130, steps of 1; qkv and att      up to 250 keys, 4 per lane, ring of 251
                              of layers 0 and 7                             rows wrapped
    slots, window 70          3 slots, T <= 40, staggered, one reset;       attention_stream_slots_kernel,
                              all 40 stages per session                     attention_stream_append_slots_kernel
    adversarial checkpoints   peaky3, peaky8, flat, massive, offset: whole B = 2 x T = 13 and the window-70 stream in
                              steps of 1 (peaky8, flat: also B = 1 x T = 129 banded); zero and constant codes: whole
                              and stream; K = 1 and K = 32: the window-70 stream.  Layers 0 and 7.

Every case asserts the attention symbol(s) of its profiled launches, appends one ``decode_xfmr_stage`` record per stage
to the parity log, and collects all its failures before it asserts.
"""
import json

import pytest
import torch

import decode_adversarial as dadv
import decode_xfmr_ref as dxr

pytestmark = pytest.mark.gpu

W70 = 70
ENDS = (0, dxr.LAYERS - 1)
ATT256, ATTBAND = "mimi::attention_t256_kernel", "mimi::attention_kernel"
ATT256_R, ATTBAND_R = "mimi::attention_t256_ragged_kernel", "mimi::attention_ragged_kernel"
ATT_STREAM, ATT_SLOTS = "mimi::attention_stream_kernel", "mimi::attention_stream_slots_kernel"
LAUNCHES = {"qkv": ("dec_layernorm", "dec_qkv"), "att": ("dec_attention",), "oproj": ("dec_o_proj",),
            "ff": ("dec_layernorm", "dec_fc1"), "xfmr": ("dec_fc2",)}


@pytest.fixture(scope="module")
def base():
    return dadv.base_state_dict()


@pytest.fixture(scope="module")
def base_view(base):
    return dxr.view(base)


def make_engine(sd, window=None):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.config import MimiConfig
    from mimi_hip.model import MimiHipModel
    kw = {} if window is None else {"config": MimiConfig(sliding_window=window)}
    return MimiHipModel(sd, device="cuda:0", decode=True, **kw)


@pytest.fixture(scope="module")
def dec(base):
    m = make_engine(base)
    yield m
    m.close()


@pytest.fixture(scope="module")
def dec70(base):
    m = make_engine(base, W70)
    yield m
    m.close()


# ---- running a form with taps and profiling on -----------------------------------------------------------------------
def needed(stage_names, window=None):
    """The taps a check of ``stage_names`` reads: the stages' outputs and their inputs."""
    tab = dxr.stages(window)
    out = []
    for n in stage_names:
        for t in tab[n].source + (n,):
            if t not in out:
                out.append(t)
    return out


def read_taps(m, tap_names):
    return {n: torch.from_numpy(m.get_tap(n)).clone() for n in tap_names}


class Tapped:
    """Taps and profiling on for the block; ``kernels()`` folds the last pass's launches into {stage: {symbol}}."""

    def __init__(self, m):
        self.m, self.kern = m, {}

    def __enter__(self):
        self.m.set_taps(True)
        self.m.set_profiling(1)
        return self

    def __exit__(self, *exc):
        self.m.set_profiling(0)
        self.m.set_taps(False)

    def kernels(self):
        for stage, kernel in self.m.profile_sequence():
            self.kern.setdefault(stage, set()).add(kernel)
        return self.kern


def run_whole(m, codes, tap_names):
    with Tapped(m) as t:
        m.decode(codes)
        return read_taps(m, tap_names), t.kernels()


def run_ragged(m, codes, lens, tap_names):
    with Tapped(m) as t:
        m.decode_ragged(codes, lens)
        packed, kern = read_taps(m, tap_names), t.kernels()
    items = [{} for _ in lens]
    for n, p in packed.items():
        for b, rows in enumerate(dxr.unpack(p, lens)):
            items[b][n] = rows
    return items, kern


def run_stream(m, codes, split, tap_names, max_step_frames):
    B, K, T = codes.shape
    assert sum(split) == T
    cat = dxr.Concat(tap_names)
    with Tapped(m) as t:
        with m.decode_stream(batch=B, num_quantizers=K, max_step_frames=max_step_frames) as st:
            at = 0
            for n in split:
                st.step(codes[:, :, at:at + n])
                at += n
                t.kernels()
                taps = read_taps(m, tap_names)
                assert all(v.shape[:2] == (B, 2 * n) for v in taps.values()), {k: v.shape for k, v in taps.items()}
                cat.add(taps)
            assert st.position == T
        return cat.batch(), t.kern


def run_slots(m, tap_names):
    """tests/decode_xfmr_ref.py ``slot_schedule`` on one stream of 3 slots: -> ({session: taps}, kernels)."""
    sessions = dxr.slot_sessions()
    cat = dxr.Concat(tap_names)
    at = {name: 0 for name in sessions}
    order = {s: [] for s in range(dxr.SLOTS)}
    pos = [0] * dxr.SLOTS
    with Tapped(m) as t:
        with m.decode_stream(batch=dxr.SLOTS, num_quantizers=dxr.SLOT_K, max_step_frames=dxr.SLOT_MAX_STEP) as st:
            for op in dxr.slot_schedule():
                if op[0] == "reset":
                    st.reset(op[1])
                    cat.cut(op[1])
                    pos[op[1]] = 0
                else:
                    _, items, n = op
                    codes = torch.cat([sessions[name][:, :, at[name]:at[name] + n] for _, name in items])
                    slots = [s for s, _ in items]
                    st.step(codes, slots=slots)
                    t.kernels()
                    taps = read_taps(m, tap_names)   # indexed by the step's item, not by slot
                    assert all(v.shape[:2] == (len(items), 2 * n) for v in taps.values())
                    cat.add(taps, slots)
                    for s, name in items:
                        at[name] += n
                        pos[s] += n
                        if name not in order[s]:
                            order[s].append(name)
                assert st.positions == pos, (op, st.positions, pos)
    assert all(at[name] == sessions[name].shape[2] for name in sessions), at
    seqs = cat.sequences()
    assert all(len(seqs[s]) == len(order[s]) for s in order), ({s: len(v) for s, v in seqs.items()}, order)
    return {name: seqs[s][i] for s in order for i, name in enumerate(order[s])}, t.kern


# ---- checking ---------------------------------------------------------------------------------------------------------
def symbols(kern, kind):
    return " + ".join(sorted(k for s in LAUNCHES[kind] for k in kern.get(s, ())))


def check(parity_log, form, case, taps, dsd, window, stage_names, kern):
    """One record per stage; -> the failures of all of them."""
    bad = []
    for name in stage_names:
        rec = dxr.measure(name, taps, dsd, window, got=taps[name])
        rec.update(test="decode_xfmr_stage", form=form, case=case, kernel=symbols(kern, name.rstrip("0123456789")))
        parity_log.append(rec)
        print(json.dumps(rec))
        bad += [f"{form} / {case}: {f} (worst element {rec['worst']})" for f in dxr.failures(rec)]
    return bad


def assert_attention(kern, *want):
    assert sorted(kern.get("dec_attention", ())) == sorted(want), (sorted(kern.get("dec_attention", ())), want)


def assert_stream_kernels(kern, slots=False):
    assert_attention(kern, ATT_SLOTS if slots else ATT_STREAM)
    assert sorted(kern["dec_kv_append"]) == ["mimi::attention_stream_append_slots_kernel" if slots else
                                             "mimi::attention_stream_append_kernel"], kern["dec_kv_append"]


ALL, END_STAGES = dxr.names(), dxr.names(ENDS)
ONES40, SEVENS40 = [1] * 40, [7, 7, 7, 7, 7, 5]


# ---- the forms on the seeded checkpoint -------------------------------------------------------------------------------
def test_whole_T13_all_stages(dec, base_view, parity_log):
    codes = dadv.random_codes(13, 2, 8, 13)
    taps, kern = run_whole(dec, codes, needed(ALL))
    assert_attention(kern, ATT256)
    assert taps["qkv0"].shape == (2, 26, 1536) and taps["ff3"].shape == (2, 26, 2048) and taps["xfmr7"].shape == (2, 26, 512)
    bad = check(parity_log, "whole", "B2_T13", taps, base_view, None, ALL, kern)
    # item 1's row 0 has one key, its own: the output is that row's v, whatever item 0 holds
    for l in range(dxr.LAYERS):
        if not torch.equal(taps[f"att{l}"][1, 0], taps[f"qkv{l}"][1, 0, 1024:]):
            bad.append(f"att{l}: row 0 of item 1 is not its own value row")
    assert not bad, "\n".join(bad)


def test_whole_window70_T40(dec70, base_view, parity_log):
    codes = dadv.random_codes(40, 2, 8, 40)
    taps, kern = run_whole(dec70, codes, needed(ALL, W70))
    assert_attention(kern, ATT256)
    bad = check(parity_log, "whole_w70", "B2_T40", taps, base_view, W70, ALL, kern)
    assert not bad, "\n".join(bad)


def test_whole_T129_banded(dec, base_view, parity_log):
    codes = dadv.random_codes(129, 1, 8, 129)
    taps, kern = run_whole(dec, codes, needed(END_STAGES))
    assert_attention(kern, ATTBAND)
    bad = check(parity_log, "whole", "B1_T129", taps, base_view, None, END_STAGES, kern)
    assert not bad, "\n".join(bad)


def test_ragged_3_13_130(dec, base_view, parity_log):
    lens = [3, 13, 130]
    codes = dadv.random_codes(131, 3, 8, 130)
    items, kern = run_ragged(dec, codes, lens, needed(END_STAGES))
    assert_attention(kern, ATT256_R, ATTBAND_R)
    bad = []
    for b, T in enumerate(lens):
        assert items[b]["qkv0"].shape == (1, 2 * T, 1536)
        bad += check(parity_log, "ragged", f"item{b}_T{T}", items[b], base_view, None, END_STAGES, kern)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("split,msf", [(ONES40, 1), (SEVENS40, 7)], ids=["steps_of_1", "steps_of_7"])
def test_stream_window70(dec70, base_view, parity_log, split, msf):
    codes = dadv.random_codes(40, 2, 8, 40)
    taps, kern = run_stream(dec70, codes, split, needed(ALL, W70), msf)
    assert_stream_kernels(kern)
    assert taps["att0"].shape == (2, 80, 512)
    bad = check(parity_log, "stream_w70", f"B2_T40_msf{msf}", taps, base_view, W70, ALL, kern)
    assert not bad, "\n".join(bad)


def test_stream_T130_real_window(dec, base_view, parity_log):
    names = dxr.names(ENDS, ("qkv", "att"))
    codes = dadv.random_codes(130, 1, 8, 130)
    taps, kern = run_stream(dec, codes, [1] * 130, needed(names), 1)
    assert_stream_kernels(kern)
    assert taps["att7"].shape == (1, 260, 512)
    bad = check(parity_log, "stream", "B1_T130_msf1", taps, base_view, None, names, kern)
    assert not bad, "\n".join(bad)


def test_slots_window70(dec70, base_view, parity_log):
    got, kern = run_slots(dec70, needed(ALL, W70))
    assert_stream_kernels(kern, slots=True)
    sessions = dxr.slot_sessions()
    bad = []
    for name, taps in got.items():
        assert taps["att0"].shape == (1, 2 * sessions[name].shape[2], 512), (name, taps["att0"].shape)
        bad += check(parity_log, "slots_w70", f"session_{name}", taps, base_view, W70, ALL, kern)
    assert not bad, "\n".join(bad)


# ---- adversarial checkpoints and codes --------------------------------------------------------------------------------
def whole_and_stream(m, dsd, parity_log, case, codes13, codes40):
    """B = 2 x T = 13 whole and the window-70 stream in steps of 1 on the smallest ring, layers 0 and 7."""
    tn = needed(END_STAGES, W70)
    taps, kern = run_whole(m, codes13, tn)
    assert_attention(kern, ATT256)
    bad = check(parity_log, "whole_w70", f"{case}_B2_T13", taps, dsd, W70, END_STAGES, kern)
    taps, kern = run_stream(m, codes40, ONES40, tn, 1)
    assert_stream_kernels(kern)
    return bad + check(parity_log, "stream_w70", f"{case}_B2_T40_msf1", taps, dsd, W70, END_STAGES, kern)


@pytest.mark.parametrize("case", dadv.ADVERSARIAL)
def test_adversarial_checkpoint(base, parity_log, case):
    sd = dadv.CHECKPOINTS[case](base)
    dsd = dxr.view(sd)
    m = make_engine(sd, W70)
    try:
        bad = whole_and_stream(m, dsd, parity_log, case, dadv.random_codes(13, 2, 8, 13), dadv.random_codes(40, 2, 8, 40))
        if case in ("peaky8", "flat"):
            taps, kern = run_whole(m, dadv.random_codes(129, 1, 8, 129), needed(END_STAGES, W70))
            assert_attention(kern, ATTBAND)
            bad += check(parity_log, "whole_w70", f"{case}_B1_T129", taps, dsd, W70, END_STAGES, kern)
    finally:
        m.close()
    assert not bad, "\n".join(bad)


def test_zero_input(base, parity_log):
    sd = dadv.CHECKPOINTS["zero"](base)
    m = make_engine(sd, W70)
    try:
        with Tapped(m):
            m.decode(dadv.zero_codes(0, 2, 8, 13))
            assert float(torch.from_numpy(m.get_tap("upsample")).abs().max()) == 0.0
        bad = whole_and_stream(m, dxr.view(sd), parity_log, "zero", dadv.zero_codes(0, 2, 8, 13), dadv.zero_codes(0, 2, 8, 40))
    finally:
        m.close()
    assert not bad, "\n".join(bad)


def test_constant_codes(dec70, base_view, parity_log):
    bad = whole_and_stream(dec70, base_view, parity_log, "constant", dadv.constant_codes(13, 2, 8, 13),
                           dadv.constant_codes(40, 2, 8, 40))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("K", [1, 32])
def test_stream_window70_level_counts(dec70, base_view, parity_log, K):
    taps, kern = run_stream(dec70, dadv.random_codes(40 + K, 2, K, 40), ONES40, needed(END_STAGES, W70), 1)
    assert_stream_kernels(kern)
    bad = check(parity_log, "stream_w70", f"K{K}_B2_T40_msf1", taps, base_view, W70, END_STAGES, kern)
    assert not bad, "\n".join(bad)
