"""GPU: streaming encode (``MimiHipModel.encode_stream``), audio to codes chunk by chunk on a KV cache.

What a stream promises, and what these tests hold it to:

1. CHUNKING DOES NOT MOVE A BIT: the codes of any split of a clip into steps are ``torch.equal`` to one another; the
   concatenated ``downsample`` taps are within ``ACT_TOL`` = 1e-4 (the project's ``rel_err``) of
   ``mimi_ref.pre_quantizer`` of the whole clip; against ``mimi_ref.encode`` every flip is explained by the measured
   embedding error (``audit.perturbation_near_tie`` + ``margin_audit``) and explained flips stay under 1 % of the
   frame-chains (the clips were chosen on the CPU so that the reference alone has none:
   tests/test_encode_stream_ref.py test_clips_have_no_flip);
2. the sliding window, eviction and the ring's wrap at the real window (T = 130: 260 rows against 250), with the
   smallest ring (``max_step_frames`` = 1), a mid-sized one and one chunk that holds the whole clip; the state's size;
3. the window comes from the config (``sliding_window`` = 5);
4. THE REPLICATE EDGE: the downsample's carry of a slot at position 0 is that step's first row -- on a first step of one
   frame, after ``reset`` with another clip, and on a slot reset while its neighbour is mid-session;
5. stage by stage in float64 on the per-step taps concatenated in time (tests/encode_stage_ref.py, f32 arithmetic, its
   hard and working conditions), the kernels a step runs and their number;
6. items of a batch and streams of an engine do not see one another, nor the encodes / decodes run between their steps;
7. (slots: tests/test_encode_stream_slots_gpu.py)
8. ordinary extreme inputs (silence of both signs, a full-scale square);
9. the ``out`` buffer and the arguments;
10. the round trip through ``decode_stream``.

tests/test_encode_stream_ref.py shows on the CPU that these inputs tell the likely mistakes apart.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import encode_stage_ref as stg
import encode_stream_ref as esr
from audit import first_flip_margins, margin_audit, perturbation_near_tie
from conftest import assert_codes_in_range
from mimi_hip import synthetic
from mimi_hip.config import encoded_length
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4
FRAME = esr.FRAME
G64, G128 = "mimi::gemm_f32_kernel<64, 128,", "mimi::gemm_f32_kernel<128, 128,"
SPLITS_13 = ([13], [1] * 13, [2, 3, 1, 7], [12, 1])
LAYERS = stg.CFG.num_hidden_layers


@pytest.fixture(scope="module")
def sd(state_dict):
    return esr.as_tensors(state_dict)


def make_engine(state_dict, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(state_dict, device="cuda:0", **kw)


@pytest.fixture(scope="module")
def enc(state_dict):
    """An encode-only model: the stream needs no decode weights."""
    m = make_engine(state_dict)
    yield m
    m.close()


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def emb_tap(m):
    """The step's pre-quantizer embedding [B, 512, n]."""
    return torch.from_numpy(m.get_tap("downsample").copy()).transpose(1, 2)


def run_stream(m, x, split, K=8, max_step_frames=None, emb=False):
    """One fresh stream over audio x [B, 1, 1920 T]: (codes [B, K, T] int32 on the host, the concatenated embedding)."""
    B = x.shape[0]
    codes, embs = [], []
    if emb:
        m.set_taps(True)
    try:
        with m.encode_stream(batch=B, num_quantizers=K, max_step_frames=max_step_frames or max(split)) as st:
            for a in esr.chunks(x, split):
                c = st.step(a)
                n = a.shape[-1] // FRAME
                assert c.shape == (B, K, n) and c.dtype == torch.int32 and c.is_cuda
                assert_codes_in_range(c)
                codes.append(c.cpu())
                if emb:
                    embs.append(emb_tap(m))
            assert st.position == sum(split)
    finally:
        if emb:
            m.set_taps(False)
    return torch.cat(codes, dim=-1), (torch.cat(embs, dim=-1) if emb else None)


def whole(name, sd, K=8):
    x, cfg = esr.clip(name), esr.clip_cfg(name)
    taps = {}
    codes = mimi_ref.encode(x, sd, K, cfg, taps=taps)
    return x, taps["pre_quantizer"], codes


def audit(parity_log, test, codes, emb, ref_codes, ref_emb, sd, cfg=None, **kw):
    """Every flip against the reference explained by the measured embedding error, and explained flips <= 1 % of the
    frame-chains."""
    K = ref_codes.shape[1]
    _, margins, sec = mimi_ref.rvq_from_embedding(ref_emb, sd, K, cfg, return_margins=True, return_second=True)
    thr = perturbation_near_tie(emb.numpy(), ref_emb.numpy(), sd, sec.numpy())
    flips, bad, chains = [], [], 0
    for b in range(ref_codes.shape[0]):
        _, unexplained = margin_audit(codes[b].numpy(), ref_codes[b].numpy(), margins[b].numpy(), thr[b])
        bad += unexplained
        flips += first_flip_margins(codes[b].numpy(), ref_codes[b].numpy(), margins[b].numpy())
        chains += ref_codes.shape[2] * (2 if K > 1 else 1)
    rec = dict(test=test, codes=int(ref_codes.numel()), exact=float((codes.long() == ref_codes).float().mean()),
               chain_flips=len(flips), frame_chains=chains, max_flip_margin=max(flips) if flips else None,
               max_audit_threshold=float(thr.max()), rel_err=rel_err(emb, ref_emb), **kw)
    parity_log.append(rec)
    print(json.dumps(rec))
    assert not bad, bad
    assert len(flips) <= 0.01 * chains, rec
    return rec


# ---- 1. chunking does not move a bit --------------------------------------------------------------------------------
def test_chunking_does_not_move_a_bit(enc, sd, parity_log):
    x, want_emb, want = whole("t13", sd)
    outs = [run_stream(enc, x, split, emb=True) for split in SPLITS_13]
    for split, (codes, emb) in zip(SPLITS_13, outs):
        err = rel_err(emb, want_emb)
        print(json.dumps(dict(test="encode_stream_T13_K8", split=list(split), rel_err=err)))
        assert err < ACT_TOL, (split, err)
        audit(parity_log, "encode_stream_T13_K8", codes, emb, want, want_emb, sd, split=list(split))
    for split, (codes, emb) in zip(SPLITS_13[1:], outs[1:]):
        assert torch.equal(codes, outs[0][0]), f"split {split} differs from one step of 13 frames"
        assert torch.equal(emb, outs[0][1]), f"split {split}: the embedding differs from one step of 13 frames"


@pytest.mark.parametrize("K,split", [(1, [2, 3, 1, 7]), (32, [12, 1])])
def test_chunking_other_level_counts(enc, sd, parity_log, K, split):
    x, want_emb, want = whole("t13", sd, K)
    codes, emb = run_stream(enc, x, split, K=K, emb=True)
    assert rel_err(emb, want_emb) < ACT_TOL
    audit(parity_log, f"encode_stream_T13_K{K}", codes, emb, want, want_emb, sd, split=list(split))
    assert torch.equal(codes, run_stream(enc, x, [13], K=K)[0])


# ---- 2. window, eviction and ring wrap at the real window -----------------------------------------------------------
@pytest.fixture(scope="module")
def t130(enc):
    """T = 130 three ways; the 1-frame stream's state size after its first and after its last step."""
    x = esr.clip("t130")
    enc.set_taps(True)
    try:
        with enc.encode_stream(batch=1, num_quantizers=8, max_step_frames=1) as st:
            cs, es, sizes = [], [], []
            for a in esr.chunks(x, [1] * 130):
                cs.append(st.step(a).cpu())
                es.append(emb_tap(enc))
                sizes.append(st.state_bytes)
            assert st.position == 130
    finally:
        enc.set_taps(False)
    ones = (torch.cat(cs, dim=-1), torch.cat(es, dim=-1))
    sevens = run_stream(enc, x, [7] * 18 + [4], max_step_frames=7, emb=True)
    one = run_stream(enc, x, [130], max_step_frames=130, emb=True)
    return x, ones, sevens, one, sizes


def test_window_eviction_and_ring_wrap(t130, sd, parity_log):
    x, ones, sevens, one, _ = t130
    taps = {}
    want = mimi_ref.encode(x, sd, 8, taps=taps)
    want_emb = taps["pre_quantizer"]
    for name, (codes, emb) in (("1x130", ones), ("7x18+4", sevens), ("130", one)):
        assert_codes_in_range(codes)
        err = rel_err(emb, want_emb)
        print(json.dumps(dict(test="encode_stream_T130", split=name, rel_err=err)))
        assert err < ACT_TOL, (name, err)
        audit(parity_log, "encode_stream_T130", codes, emb, want, want_emb, sd, split=name)
    assert torch.equal(ones[0], one[0]) and torch.equal(ones[1], one[1]), "130 steps of 1 frame differ from one of 130"
    assert torch.equal(sevens[0], one[0]) and torch.equal(sevens[1], one[1]), "steps of 7 frames differ from one of 130"


def test_state_bytes(t130):
    """Constant, and the reference's count: each of its sections rounded up to 256 bytes (conv 0's 6 samples kept as 8
    falls inside its section's rounding)."""
    sizes = t130[4]
    assert len(sizes) == 130 and len(set(sizes)) == 1
    cfg = RefConfig()
    want = 4 * esr.state_floats(cfg, 1, 1)
    assert want <= sizes[0] < want + 256 * esr.state_sections(cfg), (sizes[0], want)
    assert want <= sizes[129] < want + 256 * esr.state_sections(cfg), (sizes[129], want)


# ---- 3. the window comes from the config ----------------------------------------------------------------------------
def test_window_from_the_config(state_dict, sd, parity_log):
    from mimi_hip.config import MimiConfig
    x, want_emb, want = whole("t9w5", sd)
    cfg = esr.clip_cfg("t9w5")
    assert rel_err(mimi_ref.pre_quantizer(x, sd, RefConfig()), want_emb) > 10 * ACT_TOL  # the window shows in this clip
    m = make_engine(state_dict, config=MimiConfig(sliding_window=5))
    try:
        outs = {}
        for split in ([1] * 9, [4, 4, 1], [9]):
            codes, emb = run_stream(m, x, split, emb=True)
            err = rel_err(emb, want_emb)
            print(json.dumps(dict(test="encode_stream_T9_window5", split=list(split), rel_err=err)))
            assert err < ACT_TOL, (split, err)
            audit(parity_log, "encode_stream_T9_window5", codes, emb, want, want_emb, sd, cfg, split=list(split))
            outs[len(split)] = (codes, emb)
    finally:
        m.close()
    assert torch.equal(outs[9][0], outs[1][0]) and torch.equal(outs[3][0], outs[1][0])
    assert torch.equal(outs[9][1], outs[1][1]) and torch.equal(outs[3][1], outs[1][1])


# ---- 4. the replicate edge ------------------------------------------------------------------------------------------
def test_first_step_of_one_frame(enc, sd):
    """The carry is the chunk's own first row: frame 0 alone is the reference's frame 0."""
    x, want_emb, _ = whole("t13", sd)
    codes, emb = run_stream(enc, x, [1, 12], emb=True)
    assert rel_err(emb[..., :1], want_emb[..., :1]) < ACT_TOL
    assert rel_err(emb, want_emb) < ACT_TOL
    # and a one-frame clip is a sequence of its own
    x1 = x[..., :FRAME]
    _, e1 = run_stream(enc, x1, [1], emb=True)
    assert rel_err(e1, mimi_ref.pre_quantizer(x1, sd, RefConfig())) < ACT_TOL


def test_reset_then_another_clip_is_a_fresh_stream(enc, sd):
    xa, xb = esr.clip("t13"), esr.clip("t13d")
    fresh_b, fresh_emb = run_stream(enc, xb, [2, 3, 1, 7], emb=True)
    enc.set_taps(True)
    try:
        with enc.encode_stream(batch=1, num_quantizers=8, max_step_frames=7) as st:
            for a in esr.chunks(xa, [2, 3, 1, 7]):
                st.step(a)
            assert st.position == 13
            st.reset()
            assert st.position == 0
            cs, es = [], []
            for a in esr.chunks(xb, [2, 3, 1, 7]):
                cs.append(st.step(a).cpu())
                es.append(emb_tap(enc))
    finally:
        enc.set_taps(False)
    assert torch.equal(torch.cat(cs, dim=-1), fresh_b)
    assert torch.equal(torch.cat(es, dim=-1), fresh_emb)  # not the previous session's carry
    assert rel_err(fresh_emb, mimi_ref.pre_quantizer(xb, sd, RefConfig())) < ACT_TOL


def test_slot_reset_beside_a_running_neighbour(enc, sd):
    xa, xb, xc = esr.clip("t13"), esr.clip("t13d"), esr.clip("t13c")
    alone_b = run_stream(enc, xb, [2, 3, 1, 7])[0]
    alone_c = run_stream(enc, xc[..., :8 * FRAME], [1, 7])[0]
    both = torch.cat([xa, xb])
    with enc.encode_stream(batch=2, num_quantizers=8, max_step_frames=7) as st:
        got_b = [st.step(both[..., :2 * FRAME])[1:].cpu(), st.step(both[..., 2 * FRAME:5 * FRAME])[1:].cpu()]
        st.reset(0)
        assert st.positions == [0, 5]
        # slot 0 starts clip c at position 0 while slot 1 stands at frame 5: one call, mixed positions
        y = st.step(torch.cat([xc[..., :FRAME], xb[..., 5 * FRAME:6 * FRAME]])).cpu()
        got_c = [y[:1]]
        got_b.append(y[1:])
        y = st.step(torch.cat([xc[..., FRAME:8 * FRAME], xb[..., 6 * FRAME:]])).cpu()
        got_c.append(y[:1])
        got_b.append(y[1:])
        assert st.positions == [8, 13]
    assert torch.equal(torch.cat(got_b, dim=-1), alone_b)
    assert torch.equal(torch.cat(got_c, dim=-1), alone_c)


# ---- 5. stage by stage, in float64 ----------------------------------------------------------------------------------
FRONT = ["conv0", "res0_elu", "down0", "res1_elu", "down1", "res2_elu", "down2", "res3_elu", "down3_elu", "encoder"]
TAIL = ["downsample", "proj"]


def layer(l):
    return [f"qkv{l}", f"att{l}", f"oproj{l}", f"ff{l}", f"xfmr{l}"]


STAGE_NAMES = FRONT + [n for l in range(LAYERS) for n in layer(l)] + TAIL
LAUNCHES = {"conv0": ("encs_conv0",), "encoder": ("encs_final",), "downsample": ("encs_ds_rows", "encs_downsample"),
            "proj": ("encs_input_proj",), "down3_elu": ("encs_down_s3",)}
for _s in range(4):
    LAUNCHES[f"res{_s}_elu"] = (f"encs_res_s{_s}",)
    LAUNCHES[f"down{_s}"] = (f"encs_down_s{_s}",)
for _l in range(LAYERS):
    LAUNCHES.update({f"qkv{_l}": ("encs_layernorm", "encs_qkv"), f"att{_l}": ("encs_attention",),
                     f"oproj{_l}": ("encs_o_proj",), f"ff{_l}": ("encs_layernorm", "encs_fc1"), f"xfmr{_l}": ("encs_fc2",)})


def res0_view(sd):
    """The stage-0 block's weights under the stage-1 block's names.  The stream's stage-0 block reads the conv0 tap (a
    one-shot encode recomputes conv 0 from the audio, and so does ``STAGES['res0_elu']``); ``STAGES['res1_elu']`` is
    the block-from-its-input-tap stage -- value, condition sum and n from the weights' shapes -- so it is evaluated
    on a view that hands it stage 0's weights, as ``encode_stage_ref.decoder_view`` does for the decoder's layers."""
    (k3, k1), (v3, v1) = stg._res_keys(0), stg._res_keys(1)
    view = dict(sd)
    for a, b in ((k3, v3), (k1, v1)):
        for t in ("weight", "bias"):
            view[b + t] = sd[a + t]
    return view


def profiled_step(m, st, a):
    m.set_profiling(1)
    try:
        c = st.step(a)
        seq = m.profile_sequence()
    finally:
        m.set_profiling(0)
    return c, seq


@pytest.fixture(scope="module")
def staged(enc):
    """B = 2 x T = 13 in steps [1, 1, 1, 1, 1, 3, 5] with taps on: every tap concatenated in time, and the launch
    sequence of the last step."""
    x = torch.cat([esr.clip("t13"), esr.clip("t13d")])
    split = [1, 1, 1, 1, 1, 3, 5]
    names = sorted(set(STAGE_NAMES))
    parts = {n: [] for n in names}
    enc.set_taps(True)
    try:
        with enc.encode_stream(batch=2, num_quantizers=8, max_step_frames=5) as st:
            cs = []
            for i, a in enumerate(esr.chunks(x, split)):
                if i == len(split) - 1:
                    c, seq = profiled_step(enc, st, a)
                else:
                    c = st.step(a)
                cs.append(c.cpu())
                for n in names:
                    t = torch.from_numpy(enc.get_tap(n).copy())
                    assert t.shape[0] == 2 and t.shape[1] % (a.shape[-1] // FRAME) == 0, (n, tuple(t.shape))
                    parts[n].append(t)
    finally:
        enc.set_taps(False)
    taps = {n: torch.cat(v, dim=1) for n, v in parts.items()}
    taps["audio"] = x[:, 0]
    kern = {}
    for stage, kernel in seq:
        kern.setdefault(stage, set()).add(kernel)
    return x, torch.cat(cs, dim=-1), taps, kern, seq


def assert_kernels(kern, want):
    for stage, prefix in want.items():
        assert stage in kern, (stage, sorted(kern))
        syms = sorted(kern[stage])
        assert len(syms) == 1 and syms[0].startswith(prefix), (stage, syms, prefix)


def test_step_kernels(staged):
    """The history and stream forms, under the lock-step names (the profiled step brings 5 frames to 2 items)."""
    _, _, taps, kern, seq = staged
    want = {"encs_carry": "mimi::stream_carry_kernel", "encs_conv0": "mimi::conv0_hist_kernel<64, 7>",
            "encs_res_s0": "mimi::resblock_hist_kernel<64,", "encs_res_s1": "mimi::resblock_hist_kernel<128,",
            "encs_res_s2": "mimi::resblock_hist_kernel<256,", "encs_res_s3": "mimi::resblock_hist_kernel<512,",
            # down conv 0 has 2400 rows per item, past run_auto's 1024
            "encs_down_s0": G128, "encs_down_s1": G64, "encs_down_s2": G64, "encs_down_s3": G64, "encs_final": G64,
            "encs_layernorm": "mimi::layernorm_kernel<512,", "encs_qkv": G64,
            "encs_attention": "mimi::attention_stream_kernel", "encs_kv_append": "mimi::attention_stream_append_kernel",
            "encs_o_proj": G64, "encs_fc1": G64, "encs_fc2": G64, "encs_ds_rows": "mimi::stream_ds_rows_kernel",
            "encs_downsample": G64, "encs_input_proj": G64, "encs_rvq": "mimi::rvq_level_h16_kernel<"}
    assert_kernels(kern, want)
    assert set(kern) == set(want), sorted(set(kern) ^ set(want))
    assert [s for s, _ in seq].count("encs_carry") == 2
    assert taps["conv0"].shape == (2, FRAME * 13, 64) and taps["downsample"].shape == (2, 13, 512)


def test_launch_count_does_not_depend_on_the_step(enc):
    counts = {}
    for B, n in ((1, 1), (3, 5)):
        x = torch.cat([esr.clip("t13")] * B)[..., :n * FRAME]
        with enc.encode_stream(batch=B, num_quantizers=8, max_step_frames=n) as st:
            _, seq = profiled_step(enc, st, x)
            # ... nor on the position, nor on the form (a slot step over a subset)
            _, seq2 = profiled_step(enc, st, x)
            enc.set_profiling(1)
            try:
                st.step(x[:1], slots=[B - 1])
                seq3 = enc.profile_sequence()
            finally:
                enc.set_profiling(0)
        counts[(B, n)] = len(seq)
        assert len(seq2) == len(seq) == len(seq3), (len(seq), len(seq2), len(seq3))
        assert [s for s, _ in seq] == [s for s, _ in seq3]
    # recorded stages: 2 carries, conv 0, 4 x (block, down conv), the final conv, 8 layers x (2 LayerNorms, q/k/v,
    # attention, append, o_proj, fc1, fc2), the downsample's rows and GEMM, the projections, the RVQ (one record: its
    # launches depend on num_quantizers alone)
    assert counts[(1, 1)] == counts[(3, 5)] == 2 + 1 + 4 * 2 + 1 + LAYERS * 8 + 2 + 1 + 1, counts


def check_stages(parity_log, staged, sd, names):
    _, _, taps, kern, _ = staged
    ar = stg.Arith("f32")
    bad = []
    for name in names:
        st = stg.STAGES[name]
        if name == "res0_elu":  # from the conv0 tap, which the stream's block reads
            rec = stg.measure("res1_elu", [taps["conv0"]], res0_view(sd), ar, taps["res0_elu"])
            rec["stage"] = "res0_elu (from the conv0 tap)"
        else:
            rec = stg.measure(name, [taps[s] for s in st.source], sd, ar, taps[st.out])
        rec.update(test="encode_stream_stage", case="stream_B2_T13_steps_1x5_3_5",
                   kernel=" + ".join(sorted(k for s in LAUNCHES[name] for k in kern.get(s, ()))))
        parity_log.append(rec)
        print(json.dumps(rec))
        bad.extend(f"{f} at {rec['worst']} ({rec['kernel']})" for f in stg.conditions(rec))
    assert not bad, bad


def test_seanet_stages_against_float64(staged, sd, parity_log):
    check_stages(parity_log, staged, sd, FRONT)


@pytest.mark.parametrize("l", range(LAYERS))
def test_transformer_layer_against_float64(staged, sd, parity_log, l):
    check_stages(parity_log, staged, sd, layer(l))


def test_downsample_and_projections_against_float64(staged, sd, parity_log):
    """``downsample`` is the replicate-padded conv of the whole concatenated transformer output: the fresh-slot fill
    and the carry, held to float64."""
    check_stages(parity_log, staged, sd, TAIL)


def test_staged_codes(staged, sd, parity_log):
    x, codes, taps, _, _ = staged
    tr = {}
    want = mimi_ref.encode(x, sd, 8, taps=tr)
    audit(parity_log, "encode_stream_B2_T13_steps_1x5_3_5", codes, taps["downsample"].transpose(1, 2), want,
          tr["pre_quantizer"], sd)


# ---- 6. items and streams are their own -----------------------------------------------------------------------------
def test_items_are_their_own(enc):
    x = torch.cat([esr.clip(n) for n in ("t13", "t13b", "t13c")])
    yb = run_stream(enc, x, [2, 3, 1, 7])[0]
    for i in range(3):
        assert torch.equal(yb[i], run_stream(enc, x[i:i + 1], [2, 3, 1, 7])[0][0]), i


def test_streams_and_interleaved_calls_are_their_own(state_dict):
    """Fresh engines (with decode weights), so that the decode between the steps does regrow the workspace the steps run
    in; the encodes run in f16x3 with graphs on."""
    full = dict(state_dict)
    full.update(synthetic.make_decoder_state_dict(seed=0))
    split = [2, 3, 1, 7]
    xa, xb = esr.clip("t13"), torch.cat([esr.clip("t13c"), esr.clip("t13d")])
    rng = np.random.default_rng(63)
    big = torch.from_numpy(rng.integers(0, 2048, (2, 8, 65)))
    dcodes = torch.from_numpy(rng.integers(0, 2048, (1, 8, 4)))
    wav = torch.from_numpy(np.stack([synthetic.speech_like(12000, 5, i) for i in range(2)]))
    lens = [12000, 7001]

    def ragged(m):  # (the frames past an item's own are unspecified)
        out = m.encode_ragged(wav.cuda(), lens, 8).cpu()
        return torch.cat([out[i, :, :encoded_length(n)].flatten() for i, n in enumerate(lens)])

    def calls(m, ds):
        return [lambda: m.encode_int32(wav.cuda(), 8).cpu(), lambda: m.decode(big).audio_values.cpu(),
                lambda: ds.step(dcodes).cpu(), lambda: ragged(m)]

    m = make_engine(full, decode=True)
    try:
        assert m.precision == "f16x3"
        m.set_graphs(True)
        with m.decode_stream(batch=1, num_quantizers=8, max_step_frames=4) as ds:
            want = [c() for c in calls(m, ds)]
        alone_a, alone_b = run_stream(m, xa, split)[0], run_stream(m, xb, split)[0]
    finally:
        m.close()
    m = make_engine(full, decode=True)
    try:
        m.set_graphs(True)
        ds = m.decode_stream(batch=1, num_quantizers=8, max_step_frames=4)
        m.encode_int32(wav.cuda(), 8)  # (the graph of this shape is captured before the streams start)
        sa = m.encode_stream(batch=1, num_quantizers=8, max_step_frames=7)
        sb = m.encode_stream(batch=2, num_quantizers=8, max_step_frames=7)
        ya, yb, got = [], [], []
        for a, b, call in zip(esr.chunks(xa, split), esr.chunks(xb, split), calls(m, ds)):
            before = m.graph_captures
            ya.append(sa.step(a).cpu())
            yb.append(sb.step(b).cpu())
            assert m.graph_captures == before, "a stream step captured or retired a graph"
            got.append(call())
        sa.close()
        sb.close()
        ds.close()
    finally:
        m.close()
    assert torch.equal(torch.cat(ya, dim=-1), alone_a)
    assert torch.equal(torch.cat(yb, dim=-1), alone_b)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"call {i} between the steps differs from the same call alone"


# ---- 8. ordinary extreme inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zeros", "negative_zeros", "square"])
def test_silence_and_full_scale(enc, sd, kind):
    n = 5 * FRAME
    if kind == "square":
        x = torch.where((torch.arange(n) // 60) % 2 == 0, 1.0, -1.0)[None, None]
    else:
        x = torch.zeros(1, 1, n) * (-1.0 if kind == "negative_zeros" else 1.0)
    want = mimi_ref.pre_quantizer(x.float(), sd, RefConfig())
    codes, emb = run_stream(enc, x.float(), [1, 3, 1], emb=True)
    assert torch.isfinite(emb).all()
    err = rel_err(emb, want)
    print(json.dumps(dict(test="encode_stream_extreme", kind=kind, rel_err=err)))
    assert err < ACT_TOL, (kind, err)
    assert torch.equal(codes, run_stream(enc, x.float(), [5])[0])


# ---- 9. the out buffer and the arguments ----------------------------------------------------------------------------
def test_out_is_fully_overwritten_and_nothing_past_it(enc):
    x = esr.clip("t13")[..., :3 * FRAME]
    want = run_stream(enc, x, [3])[0]
    n = 8 * 3
    buf = torch.full((n + 4096,), -7, dtype=torch.int32, device=enc.device)
    out = buf[:n].view(1, 8, 3)
    with enc.encode_stream(batch=1, num_quantizers=8, max_step_frames=3) as st:
        y = st.step(x, out=out)
        assert y.data_ptr() == buf.data_ptr()
        host = buf.cpu()
        assert torch.equal(host[:n].view(1, 8, 3), want) and bool((host[n:] == -7).all())
        for bad in (torch.empty((1, 8, 3), dtype=torch.int64, device=enc.device),
                    torch.empty((1, 8, 4), dtype=torch.int32, device=enc.device),
                    torch.empty((1, 8, 3), dtype=torch.int32),
                    torch.empty((1, 3, 8), dtype=torch.int32, device=enc.device).transpose(1, 2)):
            with pytest.raises(ValueError):
                st.step(x, out=bad)
        assert st.position == 1 * 3
    assert tuple(y.shape) == (1, 8, 3)


def test_audio_shapes_and_bad_step_lengths_leave_the_state_untouched(enc):
    x = esr.clip("t13")
    want = run_stream(enc, x, [2, 3, 8], max_step_frames=8)[0]
    with enc.encode_stream(batch=1, num_quantizers=8, max_step_frames=8) as st:
        assert st.frame_samples == FRAME
        out = [st.step(x[:, 0, :2 * FRAME]).cpu()]  # [B, F n] as well as [B, 1, F n]
        for bad in (x[..., :0], x[..., :FRAME - 1], x[..., :FRAME + 1], x[..., :9 * FRAME], x[0], torch.cat([x, x])):
            with pytest.raises(ValueError):
                st.step(bad)
        # and through the C entry itself
        a = x[0, 0, :9 * FRAME].to(enc.device).contiguous()
        buf = torch.empty(8 * 9, dtype=torch.int32, device=enc.device)
        for n in (0, 9, -1):
            assert enc._lib.mimi_encode_stream_step(st._h, ctypes.c_void_p(a.data_ptr()), n,
                                                    ctypes.c_void_p(buf.data_ptr()), enc._stream()) == 1
        assert enc._lib.mimi_encode_stream_step(st._h, None, 1, ctypes.c_void_p(buf.data_ptr()), enc._stream()) == 1
        assert enc._lib.mimi_encode_stream_step(st._h, ctypes.c_void_p(a.data_ptr()), 1, None, enc._stream()) == 1
        assert st.position == 2
        out.append(st.step(x[..., 2 * FRAME:5 * FRAME].numpy()).cpu())  # a host array
        out.append(st.step(x[..., 5 * FRAME:].double()).cpu())          # another dtype
    assert torch.equal(torch.cat(out, dim=-1), want)
    with pytest.raises(ValueError):
        enc.encode_stream(num_quantizers=33)
    with pytest.raises(ValueError):
        enc.encode_stream(batch=0)
    with pytest.raises(NotImplementedError):
        enc.encode(x.cuda(), use_streaming=True)
    st = enc.encode_stream()
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.step(x[..., :FRAME])


# ---- 10. round trip -------------------------------------------------------------------------------------------------
def test_round_trip_through_decode_stream(state_dict):
    """encode_stream -> decode_stream frame by frame: the plumbing (dtypes, layouts, positions), not the quality."""
    full = dict(state_dict)
    full.update(synthetic.make_decoder_state_dict(seed=0))
    x = esr.clip("t13")
    m = make_engine(full, decode=True)
    try:
        with m.encode_stream(batch=1, num_quantizers=8) as es, m.decode_stream(batch=1, num_quantizers=8,
                                                                               max_step_frames=1) as ds:
            codes, audio = [], []
            for a in esr.chunks(x, [1] * 13):
                c = es.step(a)
                assert_codes_in_range(c)
                codes.append(c.cpu())
                audio.append(ds.step(c).cpu())
            assert es.position == ds.position == 13
        codes = torch.cat(codes, dim=-1)
        with m.decode_stream(batch=1, num_quantizers=8, max_step_frames=13) as ds:
            want = ds.step(codes).cpu()
    finally:
        m.close()
    audio = torch.cat(audio, dim=-1)
    assert audio.shape == (1, 1, FRAME * 13) and torch.equal(audio, want)
