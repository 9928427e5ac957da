"""GPU: the encode path kernel by kernel, in float64, on both sides of each tile threshold of the f16x3 dispatch.

* STAGE CHECKS: each stage's output tap against the float64 evaluation of that one stage on the engine's own input
  tap(s) (tests/encode_stage_ref.py: q = max |got - ref64| / (2^-24 mag64); hard condition q <= n + c, working condition
  q <= 16 max(q_ref, q_emul, 1), q_ref torch-CPU's fp32 evaluation and q_emul the CPU emulation of the f16x3 arithmetic,
  both measured in the same test on the same input).  tests/test_encode_stage_ref.py shows on the CPU which faults miss
  the working condition and by how much.
* WHICH KERNEL RAN: every case reads the launch sequence of its profiled encode and pins the tile family per stage from
  the symbol's template arguments (``assert_kernels``).  A retune that moves a threshold fails there: move the shape
  with it, so that both sides of the threshold stay held to float64.
* Each stage check appends {test: "encode_stage", stage, case, mode, q_engine, q_ref, q_emul, n, c, kernel, worst} to
  ``parity_log`` (parity_report.json; the baseline copy is profiles/encode_stage_parity.json).

THRESHOLDS of the f16x3 dispatch and the case on each side.  t(bm, bn) = ceil(M / bm) ceil(N / bn) batch (gemm.hip
``tiles``); "small grid" = t(128, 128) < 128 (kSmallGrid), then ``run_small_h16`` takes its 64-row tile if that gives
>= 256 workgroups, else its 32-row tile if that does, else its 16-row tile.  Frames are 25 Hz frames (960 samples);
flat GEMMs (o_proj, fc1, fc2, input_proj) have M = B x frames, the per-item ones (convs, q/k/v, downsample) batch = B.

  role (symbol)                     rule                                       below -> above (case)
  final conv  <16,32|32,64|64,64>   small grid; t(32,64), t(64,64) >= 256      B2_F250 <16,32> | B4_F250 <32,64> | B8_F250 <64,64>
              <128,128>             t(128,128) >= 128                          B31_F125 (124) -> B32_F125 (128)
  q/k/v       <16,64|32,128>        small grid; t(32,128) >= 256               B2_F250 (192) <16,64> | B4_F250 (384) <32,128>
              <64,128>              never on a small grid (t(64,128) >= 256 needs t(128,128) >= 128)
              <128,128> persistent  t(128,128) >= 128 and not fused            B4_F250 (96) -> B4_F257 (144), B8_F250 (192)
              fused qkv_attention   B x 8 heads >= 256, frames <= 256          B8_F250 (64) -> B32_F125 (256); forced:
                                                                               qkv_attn = 2 at B2_F13, B2_F250
  q/k/v + LN  <16,64|32,64|16,128>  ln_fused = 2 | 3 | 4 (ln_tile)             ln_fused 2, 3, 4 at B2_F13
              <32,128>              t(32,128) >= 256                           ln_fused 2 at B2_F250 (192) -> B4_F250 (384)
  attention   t256_h16 | band_h16   frames <= 256                              B1_F256 -> B1_F257; B2_F257, B4_F257 (batch)
  o_proj      <16,32|32,64|64,64>   small grid; t(32,64), t(64,64) >= 256      B2_F250 (128) <16,32> | B4_F250 <32,64> | B8_F250 <64,64>
              <128,128>             t(128,128) >= 128                          B31_F125 (124: 3875 rows) -> B32_F125 (128: 4000 rows, 32-row tail)
  fc1 + LN    <16,64|32,64|64,64>   ln_fused >= 1, small grid (M <= 896);      B2_F13 <16,64> | B1_F256, B1_F257 <32,64> |
                                    t(32,64), t(64,64) >= 256                  B2_F250 (500 rows) <64,64>
  fc1         <16,64|32,64|64,64>   the same without the prologue              ln_fused = 0 at B2_F13 | B1_F256 | B2_F250
              <128,128>             t(128,128) >= 128 (M > 896)                B2_F250 (500) -> B4_F250 (1000)
              planes256             gemm256 & 1, t(256,256) >= 256 (M > 7936)  B32_F125 (128) -> B64_F253 (512: 16192 rows); forced:
                                                                               gemm256 = 7 at 256 | 258 rows (one tile | a 2-row tail)
  fc2         <16,32|32,32|64,32>   small grid; t(32,32), t(64,32) >= 256      B2_F13 | B2_F250 (500) <32,32> | B4_F250 (1000) <64,32>
              <128,128>             t(128,128) >= 128 (+ planes out, layer 7)  B31_F125 (124) -> B32_F125 (128)
  downsample  <16,32|32,64|64,64>   t(128,128) < 256; t(32,64), t(64,64) >= 256  B4_F250 <16,32> | B8_F250, B31_F125 <32,64> | B32_F125 <64,64>
  input_proj  <16,32|32,64|64,64>   the same, flat rows                        B4_F250 <16,32> | B8_F250, B31_F125 <32,64> | B32_F125 <64,64>
              <128,128> (both)      t(128,128) >= 256: 64 items / > 8064 rows  B32_F125 (128 / 64) -> B64_F253 (256 / 256: 8128 rows)
  res k3 conv <16,64|32,64|64,64>   small grid; t(32,64), t(64,64) >= 256      B2_F13 <16,64> | B1_F256 s3 <32,64> | B1_F256 s2, B2_F250 s3 <64,64>
              <256,128>             t(128,128) >= 128                          B2_F250 s2; B4_F250 s3
  res k1 conv res1_stream | <128,128>  stage 2 | stage 3 (res1_stream = 1)     every case; forced: res1_stream = 2 (stage 3 streams)
              (both convs of stages 2 and 3 are also checked each on its own input: stages h{s} and res{s}_k1)
  down 1, 2   <64,64> pair          t(256,128) < 128                           B2_F13; B2_F250 down 2 (64)
              <256,128> pair        t(256,128) >= 128                          B2_F250 down 1 (188); B4_F250 down 2 (128)
              planes256             gemm256 & 2, t(256,256) >= 256             B4_F250 (188 / 64) -> B8_F250 down 1 (376), B32_F125 (768 / 256); forced:
                                                                               gemm256 = 7 at 256 | 257 rows per item
  down 3      <32,32|64,64> pair KG2  t(256,128) < 128; t(64,64) >= 256        B2_F250 (128) <32,32> | B4_F250 (256) <64,64>
              <256,128> pair        t(256,128) >= 128                          B8_F250 (64) -> B31_F125 (248), B32_F125 (256)
  down 0      <64,64> | <256,128>   stage0_fused = 0 only; t(256,128) >= 128   stage0_fused = 0 at B2_F13 (26) | B2_F250 (470)
  stage 0     fused | block + conv  stage0_fused                               every case | stage0_fused = 0
  stage 1     resblock128<2> | <1>  res1_form                                  every case | res1_form = 0
  ragged      the FL_RAGGED forms   lengths                                    ragged (1, 5121, 61234): every item, from conv0 to proj
Blocks 0 and 1 are one kernel each, with no tensor between their two convs to tap: they are held by the whole-block stage
alone, which sees a fault of the k3 conv about 10 x fainter than a stage of its own would (tests/test_encode_stage_ref.py
test_block_as_one_stage_dilutes_its_k3_conv); blocks 2 and 3 are held half by half through the h{s} tap.
Row tails inside a tile: 13 and 26 rows everywhere at B2_F13; 500 rows on 64-row tiles (B2_F250), 250 per item on 32-,
64- and 128-row tiles, 4000 flat rows on 128-row tiles (B32_F125), 257 rows (the banded attention, the forced tiles).
"""
import json

import numpy as np
import pytest
import torch

import encode_stage_ref as esr
from mimi_hip import synthetic

pytestmark = pytest.mark.gpu

LAYERS = esr.CFG.num_hidden_layers
DEFAULTS = {"gemm256": 3, "qkv_attn": 1, "res1_stream": 1, "res1_form": 1, "stage0_fused": 1, "ln_fused": 1}
PL, P256 = "mimi::gemm_planes_kernel<", "mimi::gemm_planes256_kernel<"


def pk(bm, bn, fl=None):
    """A planes-GEMM tile family: (prefix, suffix) of the symbol; fl pins the FL template argument too."""
    return (f"{PL}{bm}, {bn},", None if fl is None else f" {fl}, true>")


LNA, RAGGED = 2048, 512
FRONT = ["conv0", "res0_elu", "down0", "res1_elu"]
BACK = ["down1", "h2", "res2_k1", "res2_elu", "down2", "h3", "res3_k1", "res3_elu", "down3_elu", "encoder"]
TAIL = ["ds_gemm", "downsample", "proj"]


def layer(l):
    return [f"qkv{l}", f"att{l}", f"oproj{l}", f"ff{l}", f"xfmr{l}"]


ALL = list(esr.STAGES)
ALL_F32 = [s for s in ALL if s not in esr.HALVES]   # f32 mode runs every block fused: no h tap
ENDS = layer(0) + layer(LAYERS - 1)   # layer 7's fc2 writes planes too

# the profiled launch(es) behind each output tap
LAUNCHES = {"conv0": (), "res0_elu": ("res_down_s0", "res_s0"), "down0": ("res_down_s0", "down_s0"), "res1_elu": ("res_s1",),
            "down1": ("down_s1",), "res2_elu": ("res3_s2", "res1_s2", "res_s2"), "down2": ("down_s2",),
            "res3_elu": ("res3_s3", "res1_s3", "res_s3"), "h2": ("res3_s2",), "res2_k1": ("res1_s2",), "h3": ("res3_s3",),
            "res3_k1": ("res1_s3",), "down3_elu": ("down_s3",), "encoder": ("final",),
            "ds_gemm": ("downsample",), "downsample": ("downsample",), "proj": ("input_proj",)}
for _l in range(LAYERS):
    LAUNCHES.update({f"qkv{_l}": ("layernorm", "qkv", "qkv_attention"), f"att{_l}": ("attention", "qkv_attention"),
                     f"oproj{_l}": ("o_proj",), f"ff{_l}": ("fc1",), f"xfmr{_l}": ("fc2",)})


@pytest.fixture(scope="module")
def sd(state_dict):
    return {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()}


def make_engine(state_dict):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(state_dict, device="cuda:0")


@pytest.fixture(scope="module")
def engine(state_dict):
    m = make_engine(state_dict)
    yield m
    m.close()


def batch(B, L, seed):
    return torch.from_numpy(np.stack([synthetic.speech_like(L, seed, i) for i in range(B)]))


def tap_names(stages):
    names = set()
    for s in stages:
        names.add(esr.STAGES[s].out)
        names.update(esr.STAGES[s].source)
    names.discard("audio")
    return sorted(names)


def run_case(m, x, stages, mode="f16x3", opts=None, lengths=None):
    """One profiled, taps-on encode: ({tap: tensor}, {stage: set of kernel symbols}, Arith of the mode with the
    engine's activation scales)."""
    opts = opts or {}
    saved = m.precision
    try:
        m.set_precision(mode)
        for k, v in opts.items():
            m.set_option(k, v)
        m.set_taps(True)
        m.set_profiling(1)
        xd = x.cuda()
        if lengths is None:
            m.encode_int32(xd, 8)
        else:
            m.encode_ragged(xd, lengths, 8)
        seq = m.profile_sequence()
        taps = {n: torch.from_numpy(m.get_tap(n).copy()) for n in tap_names(stages)}
        scales = {k: v[0] for k, v in m.act_scales().items()}
    finally:
        m.set_profiling(0)
        m.set_taps(False)
        for k in opts:
            m.set_option(k, DEFAULTS[k])
        m.set_precision(saved)
    taps["audio"] = x
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    assert "final" in kern and "rvq" in kern, sorted(kern)  # the sequence is this encode's
    return taps, kern, esr.Arith(mode, scales)


def assert_kernels(kern, want):
    """want: {profiled stage: symbol prefix | (prefix, suffix) | None (the stage must not have run)}; every symbol of
    the stage (fc2 runs two: layer 7 writes planes too) is of that family."""
    for stage, fam in want.items():
        if fam is None:
            assert stage not in kern, (stage, sorted(kern[stage]))
            continue
        prefix, suffix = (fam, None) if isinstance(fam, str) else fam
        assert stage in kern, (stage, sorted(kern))
        for sym in sorted(kern[stage]):
            assert sym.startswith(prefix) and (suffix is None or sym.endswith(suffix)), (stage, sym, fam)


def symbols(kern, name):
    return " + ".join(sorted(k for s in LAUNCHES[name] for k in kern.get(s, ()))) or "conv0 (taps only)"


def check_stage(parity_log, case, name, xs, got, sd, ar, kern, bad):
    st = esr.STAGES[name]
    if st.interior and esr.ds_interior(xs[0].shape[1], got.shape[1]).stop <= 1:
        return None  # (every output row reads padding: nothing of ds_gemm is defined)
    rec = esr.measure(name, xs, sd, ar, got)
    rec.update(test="encode_stage", case=case, kernel=symbols(kern, name))
    parity_log.append(rec)
    print(json.dumps(rec))
    bad.extend(f"{case}: {f} at {rec['worst']} ({rec['kernel']})" for f in esr.conditions(rec))
    return rec


def check_stages(parity_log, case, stages, taps, sd, ar, kern, items=None):
    """Every stage of ``stages`` on the engine's own taps (``items``: those batch items only); all conditions asserted
    at the end, so that the log holds every stage of a failing case."""
    bad = []
    for name in stages:
        xs = [taps[s] for s in esr.STAGES[name].source]
        got = taps[esr.STAGES[name].out]
        if items is None:
            check_stage(parity_log, case, name, xs, got, sd, ar, kern, bad)
        else:
            for i in items:
                check_stage(parity_log, f"{case}[{i}]", name, [x[i:i + 1] for x in xs], got[i:i + 1], sd, ar, kern, bad)
    assert not bad, "\n".join(bad)


SMALL_F16 = {"res_down_s0": "mimi::stage0_fused_h16_kernel", "res_s1": "mimi::resblock128_h16_kernel<2>",
             "down_s1": pk(64, 64, 4), "res3_s2": pk(16, 64), "res1_s2": "mimi::res1_stream_kernel<128,",
             "down_s2": pk(64, 64, 4), "res3_s3": pk(16, 64), "res1_s3": pk(128, 128), "down_s3": pk(32, 32, 20),
             "final": pk(16, 32), "layernorm": "mimi::layernorm_kernel<512,", "qkv": pk(16, 64, 0),
             "attention": "mimi::attention_t256_h16_kernel", "o_proj": pk(16, 32), "fc1": pk(16, 64, LNA),
             "fc2": pk(16, 32), "downsample": pk(16, 32), "input_proj": pk(16, 32), "qkv_attention": None}


# ---- a. B = 2 x 13 frames: every stage and layer in three precision modes; L = 12481 and L = 1 ------------------------
@pytest.mark.parametrize("mode", ["f16x3", "f32", "bf16x6"])
def test_small_batch_every_stage(engine, sd, parity_log, mode):
    """Smallest tiles everywhere, the LayerNorm prologue in fc1, the <= 256-frame attention; item 1's first rows must
    see zeros, not item 0 (tests/test_encode_stage_ref.py: that fault stands 1e5 x over the bound)."""
    stages = ALL_F32 if mode == "f32" else ALL
    taps, kern, ar = run_case(engine, batch(2, 12480, 21), stages, mode=mode)
    if mode == "f16x3":
        assert_kernels(kern, SMALL_F16)
    elif mode == "f32":
        assert_kernels(kern, {s: "mimi::gemm_f32_kernel<" for s in ("down_s0", "down_s1", "down_s2", "down_s3", "final",
                                                                    "qkv", "o_proj", "fc1", "fc2", "downsample", "input_proj")})
        assert_kernels(kern, {"res_s0": "mimi::resblock0_wave_kernel", "res_s1": "mimi::resblock_kernel<128,",
                              "res_s2": "mimi::resblock_kernel<256,", "res_s3": "mimi::resblock_kernel<512,",
                              "attention": "mimi::attention_t256_kernel"})
    else:
        assert_kernels(kern, {s: (PL, "false>") for s in ("down_s0", "down_s1", "res3_s2", "res1_s2", "down_s2", "res3_s3",
                                                          "res1_s3", "down_s3", "final", "qkv", "o_proj", "fc1", "fc2")})
        assert_kernels(kern, {"downsample": "mimi::gemm_bf16x_kernel<", "input_proj": "mimi::gemm_f32_kernel<",
                              "attention": "mimi::attention_t256_kernel"})
    check_stages(parity_log, f"B2_F13_{mode}", stages, taps, sd, ar, kern)


@pytest.mark.parametrize("L", [12481, 1])
def test_odd_lengths_every_stage(engine, sd, parity_log, L):
    """The fused stage 0 assumes T1 = ceil(T0 / 4) and walks 32-step blocks: one sample past a block, and one sample."""
    taps, kern, ar = run_case(engine, batch(2, L, 22), ALL)
    assert_kernels(kern, SMALL_F16)
    assert taps["down0"].shape[1] == -(-L // 4)
    check_stages(parity_log, f"B2_L{L}", ALL, taps, sd, ar, kern)


# ---- b. B = 2 x 250 frames: 500 flat rows ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def b2_f250(engine):
    return run_case(engine, batch(2, 240000, 23), BACK + ENDS + TAIL)


def test_b2_f250_kernels(b2_f250):
    _, kern, _ = b2_f250
    assert_kernels(kern, dict(SMALL_F16, down_s1=pk(256, 128, 12), res3_s2=pk(256, 128), res3_s3=pk(64, 64),
                              fc1=pk(64, 64, LNA), fc2=pk(32, 32)))


@pytest.mark.parametrize("group", ["back", "layers", "tail"])
def test_b2_f250_stages(b2_f250, sd, parity_log, group):
    taps, kern, ar = b2_f250
    check_stages(parity_log, "B2_F250", {"back": BACK, "layers": ENDS, "tail": TAIL}[group], taps, sd, ar, kern)


# ---- c. B = 4 x 10 s: the SEANet GEMMs leave the small grid; first and last item ---------------------------------------
@pytest.fixture(scope="module")
def b4_f250(engine):
    return run_case(engine, batch(4, 240000, 24), ALL)


def test_b4_f250_kernels(b4_f250):
    _, kern, _ = b4_f250
    assert_kernels(kern, dict(SMALL_F16, down_s1=pk(256, 128, 12), res3_s2=pk(256, 128), down_s2=pk(256, 128, 12),
                              res3_s3=pk(256, 128), down_s3=pk(64, 64, 20), final=pk(32, 64), qkv=pk(32, 128, 0),
                              o_proj=pk(32, 64), fc1=pk(128, 128), fc2=pk(64, 32)))


@pytest.mark.parametrize("group,items", [("front", (3,)), ("back", (0, 3)), ("layers", (0, 3)), ("tail", (0, 3))])
def test_b4_f250_stages(b4_f250, sd, parity_log, group, items):
    """(The front stages -- 240 000 steps -- on the last item only: their float64 takes 5 s an item.)"""
    taps, kern, ar = b4_f250
    stages = {"front": FRONT, "back": BACK, "layers": ENDS, "tail": TAIL}[group]
    if group == "layers":  # flat rows: the GEMMs are checked over all four items, attention per item
        check_stages(parity_log, "B4_F250", [s for s in stages if not s.startswith("att")], taps, sd, ar, kern)
        stages = [s for s in stages if s.startswith("att")]
    check_stages(parity_log, "B4_F250", stages, taps, sd, ar, kern, items=items)


# ---- d. B = 8 x 10 s: the 64-row small tiles of final conv and o_proj, the persistent q/k/v tile ----------------------
def test_b8_f250(engine, sd, parity_log):
    stages = ["down3_elu", "encoder"] + ENDS + TAIL
    taps, kern, ar = run_case(engine, batch(8, 240000, 25), stages)
    assert_kernels(kern, dict(SMALL_F16, down_s1=P256, res3_s2=pk(256, 128), down_s2=pk(256, 128, 12),
                              res3_s3=pk(256, 128), down_s3=pk(64, 64, 20), final=pk(64, 64), qkv=pk(128, 128),
                              o_proj=pk(64, 64), fc1=pk(128, 128), fc2=pk(64, 32), downsample=pk(32, 64),
                              input_proj=pk(32, 64)))
    check_stages(parity_log, "B8_F250", stages, taps, sd, ar, kern, items=(0, 7))


# ---- e. B = 32 x 125 frames: 4000 flat rows on the large tiles, the fused q/k/v + attention, the 256 x 256 tile --------
@pytest.fixture(scope="module")
def b32_f125(state_dict):
    """An engine of its own (its tap buffers hold several GB of device memory), closed afterwards."""
    stages = ["down1", "down2", "down3_elu", "encoder"] + ENDS + TAIL
    m = make_engine(state_dict)
    try:
        return run_case(m, batch(32, 120000, 26), stages) + (stages,)
    finally:
        m.close()


def test_b32_f125_kernels(b32_f125):
    _, kern, _, _ = b32_f125
    assert_kernels(kern, dict(SMALL_F16, down_s1=P256, res3_s2=pk(256, 128), down_s2=P256, res3_s3=pk(256, 128),
                              down_s3=pk(256, 128, 12), final=pk(128, 128), qkv=None, attention=None,
                              qkv_attention="mimi::qkv_attention_h16_kernel<512>", o_proj=pk(128, 128),
                              fc1=pk(128, 128), fc2=pk(128, 128), downsample=pk(64, 64), input_proj=pk(64, 64)))


@pytest.mark.parametrize("group", ["convs", "layers", "tail"])
def test_b32_f125_stages(b32_f125, sd, parity_log, group):
    taps, kern, ar, stages = b32_f125
    if group == "convs":
        check_stages(parity_log, "B32_F125", stages[:4], taps, sd, ar, kern, items=(0, 31))
    elif group == "layers":  # all 4000 flat rows
        check_stages(parity_log, "B32_F125", ENDS, taps, sd, ar, kern)
    else:
        check_stages(parity_log, "B32_F125", TAIL, taps, sd, ar, kern)


def test_b31_f125_last_small_grid(engine, sd, parity_log):
    """One item fewer: downsample and input_proj fall below 256 64-row tiles and take the 32-row one; final conv, o_proj
    and fc2 (3875 flat rows, t(128, 128) = 124) are the last small-grid shapes below B = 32."""
    stages = ["encoder", "oproj0", "xfmr0"] + TAIL
    taps, kern, ar = run_case(engine, batch(31, 120000, 27), stages)
    assert_kernels(kern, {"downsample": pk(32, 64), "input_proj": pk(32, 64), "final": pk(64, 64), "o_proj": pk(64, 64),
                          "fc2": pk(64, 32), "down_s3": pk(256, 128, 12), "qkv": pk(128, 128), "qkv_attention": None})
    check_stages(parity_log, "B31_F125", stages, taps, sd, ar, kern)


def test_b64_f253_largest_tiles(state_dict, sd, parity_log):
    """B = 64 x 253 frames (16 192 flat rows, 8128 quantizer rows): downsample and input_proj leave the small grid, fc1
    runs its 256 x 256 tile by default.  An engine of its own, closed afterwards; only fc1's, the downsample's and the
    input projections' taps are fetched."""
    stages = ["ff0", f"ff{LAYERS - 1}"] + TAIL
    m = make_engine(state_dict)
    try:
        taps, kern, ar = run_case(m, torch.from_numpy(synthetic.clip_batch(64, 960 * 253, seed=36)), stages)
    finally:
        m.close()
    assert_kernels(kern, {"downsample": pk(128, 128), "input_proj": pk(128, 128), "fc1": P256, "down_s1": P256,
                          "down_s2": P256, "qkv_attention": "mimi::qkv_attention_h16_kernel<512>"})
    assert taps["proj"].shape[:2] == (64, 127)
    check_stages(parity_log, "B64_F253", stages, taps, sd, ar, kern)


# ---- f. attention at 256 | 257 frames, and the banded form with a batch ------------------------------------------------
ATT = [f"att{l}" for l in (0, LAYERS - 1)]


@pytest.mark.parametrize("B,frames,att,qkv", [(1, 256, "mimi::attention_t256_h16_kernel", pk(16, 64, 0)),
                                               (1, 257, "mimi::attention_band_h16_kernel", pk(16, 64, 0)),
                                               (2, 257, "mimi::attention_band_h16_kernel", pk(16, 64, 0)),
                                               (4, 257, "mimi::attention_band_h16_kernel", pk(128, 128))])
def test_attention_forms(engine, sd, parity_log, B, frames, att, qkv):
    """257 frames: rows 250 .. 256 have a full window (tests/test_encode_stage_ref.py: a window of 249 or 251 stands
    3000 x over the bound there).  B = 4 x 257 also puts q/k/v on its persistent 128-row tile with a 1-row tail."""
    stages = ["h2", "res2_k1", "res2_elu", "h3", "res3_k1", "res3_elu"] + layer(0) + ATT[1:] if B == 1 else layer(0) + ATT[1:]
    taps, kern, ar = run_case(engine, batch(B, 960 * frames, 28), stages)
    assert_kernels(kern, {"attention": att, "qkv": qkv, "qkv_attention": None})
    if B == 1:
        assert_kernels(kern, {"res3_s2": pk(64, 64), "res3_s3": pk(32, 64), "fc1": pk(32, 64, LNA)})
    check_stages(parity_log, f"B{B}_F{frames}", stages, taps, sd, ar, kern)


# ---- g. forms that only large totals select by default, through their force options ------------------------------------
@pytest.mark.parametrize("L,rows", [(5120, 256), (5140, 257)])
def test_forced_gemm256_down_convs(engine, sd, parity_log, L, rows):
    taps, kern, ar = run_case(engine, batch(2, L, 29), ["down1", "down2"], opts={"gemm256": 7})
    assert taps["down1"].shape[1] == rows
    assert_kernels(kern, {"down_s1": P256, "down_s2": P256})
    check_stages(parity_log, f"gemm256_7_B2_L{L}", ["down1", "down2"], taps, sd, ar, kern)


@pytest.mark.parametrize("frames", [128, 129])
def test_forced_gemm256_fc1(engine, sd, parity_log, frames):
    stages = [f"ff{l}" for l in range(LAYERS)]
    taps, kern, ar = run_case(engine, batch(2, 960 * frames, 30), stages, opts={"gemm256": 7})
    assert_kernels(kern, {"fc1": P256, "layernorm": "mimi::layernorm_kernel<512,"})
    check_stages(parity_log, f"gemm256_7_B2_F{frames}", stages, taps, sd, ar, kern)


@pytest.mark.parametrize("frames", [13, 250])
def test_forced_qkv_attention(engine, sd, parity_log, frames):
    stages = [s for l in range(LAYERS) for s in (f"qkv{l}", f"att{l}")]
    taps, kern, ar = run_case(engine, batch(2, 960 * frames, 31), stages, opts={"qkv_attn": 2})
    assert_kernels(kern, {"qkv_attention": "mimi::qkv_attention_h16_kernel<512>", "qkv": None, "attention": None})
    check_stages(parity_log, f"qkv_attn_2_B2_F{frames}", stages, taps, sd, ar, kern)


@pytest.mark.parametrize("key,value,stage,want,stages", [
    ("res1_stream", 2, "res1_s3", "mimi::res1_stream_kernel<256,", ["h2", "res2_k1", "h3", "res3_k1", "res3_elu"]),
    ("res1_form", 0, "res_s1", "mimi::resblock128_h16_kernel<1>", ["res1_elu"]),
])
def test_forced_block_forms(engine, sd, parity_log, key, value, stage, want, stages):
    taps, kern, ar = run_case(engine, batch(2, 12480, 32), stages, opts={key: value})
    assert_kernels(kern, {stage: want})
    check_stages(parity_log, f"{key}_{value}_B2_F13", stages, taps, sd, ar, kern)


@pytest.mark.parametrize("frames,tile", [(13, pk(64, 64, 4)), (250, pk(256, 128))])
def test_unfused_stage0(engine, sd, parity_log, frames, tile):
    """stage0_fused = 0: the stage-0 block and down conv 0 as two kernels (250 frames: the last item only)."""
    taps, kern, ar = run_case(engine, batch(2, 960 * frames, 33), ["res0_elu", "down0"], opts={"stage0_fused": 0})
    assert_kernels(kern, {"res_s0": "mimi::resblock0_h16_kernel", "down_s0": tile, "res_down_s0": None})
    check_stages(parity_log, f"stage0_fused_0_B2_F{frames}", ["res0_elu", "down0"], taps, sd, ar, kern,
                 items=None if frames == 13 else (1,))


@pytest.mark.parametrize("value,B,frames,qkv,fc1", [
    (2, 2, 13, pk(16, 64, LNA), pk(16, 64, LNA)), (3, 2, 13, pk(32, 64, LNA), pk(16, 64, LNA)),
    (4, 2, 13, pk(16, 128, LNA), pk(16, 64, LNA)), (2, 2, 250, pk(16, 64, LNA), pk(64, 64, LNA)),
    (2, 4, 250, pk(32, 128, LNA), pk(128, 128)),
    (0, 2, 13, pk(16, 64, 0), pk(16, 64, 0)), (0, 1, 256, pk(16, 64, 0), pk(32, 64, 0)), (0, 2, 250, pk(16, 64, 0), pk(64, 64, 0)),
])
def test_forced_layernorm_prologue(engine, sd, parity_log, value, B, frames, qkv, fc1):
    """ln_fused = 2 with each ln_tile (q/k/v computes its rows' LayerNorm itself), and ln_fused = 0 (fc1 without it)."""
    stages = [s for l in range(LAYERS) for s in (f"qkv{l}", f"ff{l}")]
    taps, kern, ar = run_case(engine, batch(B, 960 * frames, 34), stages, opts={"ln_fused": value})
    assert_kernels(kern, {"qkv": qkv, "fc1": fc1})
    if value >= 2 and B * frames <= 896:
        assert_kernels(kern, {"layernorm": None})
    check_stages(parity_log, f"ln_fused_{value}_B{B}_F{frames}", stages, taps, sd, ar, kern)


# ---- h. one ragged batch: every item against its own float64 stages ----------------------------------------------------
def test_ragged_batch(engine, sd, parity_log):
    """Lengths 1, 5121, 61234.  The SEANet taps are [B][Tmax][C] (an item's rows past its own length are unspecified),
    the transformer section's are packed [1][R][C]: item b's frames from row toff[b] on -- RoPE positions come from rpos,
    attention and the downsample find the items through toff."""
    lengths = [1, 5121, 61234]
    x = torch.zeros(len(lengths), max(lengths))
    for i, L in enumerate(lengths):
        x[i, :L] = torch.from_numpy(synthetic.speech_like(L, 35, i))
    taps, kern, ar = run_case(engine, x, ALL, lengths=lengths)
    rg = lambda bm, bn, fl: pk(bm, bn, RAGGED | fl)  # noqa: E731
    assert_kernels(kern, dict(SMALL_F16, down_s1=rg(64, 64, 4), res3_s2=rg(64, 64, 0), down_s2=rg(64, 64, 4),
                              res3_s3=rg(16, 64, 0), res1_s3=rg(128, 128, 0), down_s3=rg(32, 32, 20), final=rg(16, 32, 0),
                              downsample=rg(16, 32, 0), input_proj=rg(16, 32, 0),
                              res1_s2="mimi::res1_stream_kernel<128, 2, 64, true>"))
    packed = {"encoder"} | {s for l in range(LAYERS) for s in layer(l)}
    toff, bad = 0, []
    for b, L in enumerate(lengths):
        T = [L]
        for r in esr.RATIOS:
            T.append(-(-T[-1] // r))
        F25, F12 = T[-1], -(-T[-1] // 2)
        rows = {"audio": L, "conv0": T[0], "encoder": F25, "ds_gemm": F12, "downsample": F12, "proj": F12}
        for s in range(4):
            rows[f"res{s}_elu"] = rows[f"h{s}"] = T[s]
            rows[f"down{s}" if s < 3 else "down3_elu"] = T[s + 1]

        def item(name):
            if name in packed:
                return taps[name][:, toff:toff + F25]
            return taps[name][b:b + 1, :rows[name]]
        for name in ALL:
            check_stage(parity_log, f"ragged[{b}]", name, [item(s) for s in esr.STAGES[name].source],
                        item(esr.STAGES[name].out), sd, ar, kern, bad)
        toff += F25
    assert taps["encoder"].shape[:2] == (1, toff)
    assert not bad, "\n".join(bad)
