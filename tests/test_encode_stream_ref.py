"""Streaming encode without a GPU: the streamed reference (tests/encode_stream_ref.py) against ``mimi_ref`` of the whole
sequence, the mistakes it must catch, the installed ``transformers``' own streaming path, the clips' seeds, and the C
entry points' NULL handling.

* STREAMED = WHOLE.  For every split the GPU tests use, the streamed reference's concatenated embedding is within
  ``ACT_TOL`` = 1e-4 (the project's ``rel_err``) of ``mimi_ref.pre_quantizer`` of the whole clip, and its codes are
  ``mimi_ref.encode``'s; the measured values (1e-6-ish: another summation split of the same sums) are printed.
* MUTANTS.  Each likely mistake, switched on in the reference, misses ``ACT_TOL`` by >= 10 x on these same inputs: were
  one of them below that, the GPU tests' inputs could not tell a wrong kernel from a right one.  A mutant is run on the
  inputs that reach its mechanism: the window mutants where the sequence is longer than the window (T = 9 at a window of
  5 rows, and T = 130 at 250 on a clip built so that one row of the window matters), the two slot mutants on the slot
  schedule.
* TRANSFORMERS.  ``MimiModel.encode(use_streaming=True)`` over T = 13 in steps [2, 3, 1, 7] gives the streamed
  reference's codes: the replicate-on-first-call reading of the downsample is the reference's.
* SEEDS.  Every clip of ``encode_stream_ref.CLIPS`` streams to ``mimi_ref.encode``'s codes with no flip.
"""
import json

import pytest
import torch

import encode_stream_ref as esr
from mimi_hip import _lib
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

ACT_TOL = 1e-4
MISS = 10 * ACT_TOL
SPLITS_13 = ([13], [1] * 13, [2, 3, 1, 7], [12, 1])
SPLITS_9 = ([1] * 9, [4, 4, 1], [9])
SPLIT_130 = [7] * 18 + [4]


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def sid(s):
    return "x".join(map(str, s)) if len(s) < 5 else f"{s[0]}x{len(s)}"


def record(test, **kw):
    print(json.dumps(dict(test=test, **kw)))


@pytest.fixture(scope="module")
def sd(state_dict):
    return esr.as_tensors(state_dict)


def whole(name, sd, K=8):
    """(audio, pre-quantizer embedding, codes) of the one-shot reference."""
    x, cfg = esr.clip(name), esr.clip_cfg(name)
    taps = {}
    codes = mimi_ref.encode(x, sd, K, cfg, taps=taps)
    return x, taps["pre_quantizer"], codes


@pytest.fixture(scope="module")
def case13(sd):
    return whole("t13", sd)


@pytest.fixture(scope="module")
def case9(sd):
    return whole("t9w5", sd)


@pytest.fixture(scope="module")
def case130(sd):
    return whole("t130", sd)


# ---- streamed = whole ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", SPLITS_13, ids=sid)
def test_streamed_equals_whole_T13(sd, case13, split):
    x, want, codes = case13
    got = esr.embed_stream(x, sd, split)
    assert got.shape == want.shape == (1, 512, 13)
    err = rel_err(got, want)
    record("encode_stream_ref_T13", split=list(split), rel_err=err)
    assert err < ACT_TOL, err
    assert torch.equal(mimi_ref.rvq_from_embedding(got, sd, 8), codes)


@pytest.mark.parametrize("split", SPLITS_9, ids=sid)
def test_streamed_equals_whole_T9_window5(sd, case9, split):
    x, want, codes = case9
    cfg = esr.clip_cfg("t9w5")
    got = esr.embed_stream(x, sd, split, cfg)
    err = rel_err(got, want)
    record("encode_stream_ref_T9_w5", split=list(split), rel_err=err)
    assert err < ACT_TOL, err
    assert torch.equal(mimi_ref.rvq_from_embedding(got, sd, 8, cfg), codes)


def test_window_matters_at_T9(sd, case9):
    """The reference itself moves by far more than the tolerance when the window does: these inputs see the window."""
    x, want, _ = case9
    for w in (4, 6):
        assert rel_err(mimi_ref.pre_quantizer(x, sd, RefConfig(sliding_window=w)), want) > MISS


def test_real_window_T130(sd, case130):
    """T = 130 (260 rows, 10 past the window of 250) in steps of 7: the GPU tests' window case."""
    x, want, codes = case130
    got = esr.embed_stream(x, sd, SPLIT_130)
    err = rel_err(got, want)
    record("encode_stream_ref_T130", split="7x18+4", rel_err=err)
    assert err < ACT_TOL, err
    assert torch.equal(mimi_ref.rvq_from_embedding(got, sd, 8), codes)


# ---- mutants ---------------------------------------------------------------------------------------------------------
MUTANTS_13 = [
    ("rope_restart", esr.Mutant(rope_restart=True), [2, 3, 1, 7]),
    ("rope_restart", esr.Mutant(rope_restart=True), [12, 1]),
    ("down_short", esr.Mutant(down_short=True), [1] * 13),
    ("down_short", esr.Mutant(down_short=True), [2, 3, 1, 7]),
    ("final_short", esr.Mutant(final_short=True), [1] * 13),
    ("final_short", esr.Mutant(final_short=True), [2, 3, 1, 7]),
    ("ds_zero_fresh", esr.Mutant(ds_zero_fresh=True), [13]),
    ("ds_zero_fresh", esr.Mutant(ds_zero_fresh=True), [1] * 13),
    ("ds_replicate_every", esr.Mutant(ds_replicate_every=True), [1] * 13),
    ("ds_replicate_every", esr.Mutant(ds_replicate_every=True), [2, 3, 1, 7]),
    ("drop_conv0", esr.Mutant(drop_conv0=True), [1] * 13),
    ("drop_conv0", esr.Mutant(drop_conv0=True), [2, 3, 1, 7]),
]


@pytest.mark.parametrize("name,mutant,split", MUTANTS_13, ids=[f"{m[0]}-{len(m[2])}steps" for m in MUTANTS_13])
def test_mutants_miss_at_T13(sd, case13, name, mutant, split):
    x, want, _ = case13
    err = rel_err(esr.embed_stream(x, sd, split, mutant=mutant), want)
    record("encode_stream_ref_mutant", mutant=name, clip="t13", split=list(split), rel_err=err)
    assert err >= MISS, (name, split, err)


MUTANTS_9 = [(n, m, s) for n, m in (("window-1", esr.Mutant(window_delta=-1)), ("window+1", esr.Mutant(window_delta=1)),
                                    ("rope_restart", esr.Mutant(rope_restart=True)),
                                    ("down_short", esr.Mutant(down_short=True)),
                                    ("final_short", esr.Mutant(final_short=True)),
                                    ("ds_replicate_every", esr.Mutant(ds_replicate_every=True)),
                                    ("drop_conv0", esr.Mutant(drop_conv0=True)))
             for s in ([1] * 9, [4, 4, 1])] + [("ds_zero_fresh", esr.Mutant(ds_zero_fresh=True), [9])]


@pytest.mark.parametrize("name,mutant,split", MUTANTS_9, ids=[f"{m[0]}-{len(m[2])}steps" for m in MUTANTS_9])
def test_mutants_miss_at_T9_window5(sd, case9, name, mutant, split):
    x, want, _ = case9
    err = rel_err(esr.embed_stream(x, sd, split, esr.clip_cfg("t9w5"), mutant), want)
    record("encode_stream_ref_mutant", mutant=name, clip="t9w5", split=list(split), rel_err=err)
    assert err >= MISS, (name, split, err)


@pytest.mark.parametrize("delta", [-1, 1])
def test_window_mutants_miss_at_T130(sd, case130, delta):
    """The real window.  On natural input one key in 250 holds ~1/250 of a query's attention and a window off by one
    moves the embedding by 3e-4 .. 8e-4 only (62 speech-like clips, noise at three levels, bursts followed by silence,
    full-scale squares); the clip both this test and the GPU tests' T = 130 case use is built so that the rows which
    leave / enter the window matter (``encode_stream_ref.CLIPS``, tests/golden/make_window_clip.py)."""
    x, want, _ = case130
    err = rel_err(esr.embed_stream(x, sd, SPLIT_130, mutant=esr.Mutant(window_delta=delta)), want)
    record("encode_stream_ref_mutant", mutant=f"window{delta:+d}", clip="t130", split="7x18+4", rel_err=err)
    assert err >= MISS, (delta, err)


def test_window_clip_is_close_to_the_speech_clip():
    """The built clip stays audio: inside [-1, 1], exact in float16, within 5 % of full scale of the clip it started as."""
    from mimi_hip import synthetic
    x = esr.clip("t130")[0, 0]
    base = torch.from_numpy(synthetic.speech_like(esr.FRAME * 130, esr.CLIPS["t130"][1], esr.CLIPS["t130"][2]))
    assert float(x.abs().max()) <= 1.0 and torch.equal(x.half().float(), x)
    assert float((x - base).abs().max()) < 0.05


# ---- the slot schedule -----------------------------------------------------------------------------------------------
def sessions():
    return {name: esr.clip(name) for name in esr.SESSION_FRAMES}


def play_pool(sd, mutant=None):
    cfg = RefConfig(sliding_window=esr.WINDOW)
    pool = esr.SlotPool(sd, esr.BATCH, cfg, mutant)
    return esr.play(sessions(), pool.embed, pool.reset, lambda: pool.positions)


def test_slot_schedule_is_each_session_alone(sd):
    cfg = RefConfig(sliding_window=esr.WINDOW)
    assert {n: esr.CLIPS[n][0] for n in esr.SESSION_FRAMES} == esr.SESSION_FRAMES
    got = play_pool(sd)
    cut = esr.splits()
    for name, x in sessions().items():
        assert torch.equal(got[name], esr.embed_stream(x, sd, cut[name], cfg)), name
        err = rel_err(got[name], mimi_ref.pre_quantizer(x, sd, cfg))
        record("encode_stream_ref_slots", session=name, rel_err=err)
        assert err < ACT_TOL, (name, err)


@pytest.mark.parametrize("name,mutant,hit", [("reset_keeps_ds", esr.Mutant(reset_keeps_ds=True), "D"),
                                             ("carry_by_item", esr.Mutant(carry_by_item=True), "B")])
def test_slot_mutants_miss(sd, name, mutant, hit):
    """reset_keeps_ds: D starts on the slot A left.  carry_by_item: from call 3 on B is listed at a place that is not
    its slot."""
    cfg = RefConfig(sliding_window=esr.WINDOW)
    got = play_pool(sd, mutant)
    errs = {n: rel_err(got[n], mimi_ref.pre_quantizer(x, sd, cfg)) for n, x in sessions().items()}
    record("encode_stream_ref_mutant", mutant=name, clip="slot schedule", rel_err=errs)
    assert errs[hit] >= MISS, (name, errs)


# ---- the installed transformers' streaming path ----------------------------------------------------------------------
def test_transformers_streaming_gives_the_same_codes(state_dict, sd, case13):
    try:
        from transformers import MimiConfig as TMimiConfig, MimiModel
        model = MimiModel(TMimiConfig()).eval()
    except Exception as err:  # (no download is attempted: the config is the class's default)
        pytest.skip(f"transformers' MimiModel cannot be constructed offline: {err!r}")
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict.items()}, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith(("decoder", "upsample")) or "output_proj" in k for k in res.missing_keys), res.missing_keys
    x, _, codes = case13
    split = [2, 3, 1, 7]
    got, kv, pc = [], None, None
    with torch.no_grad():
        for a in esr.chunks(x, split):
            out = model.encode(a, num_quantizers=8, encoder_past_key_values=kv, padding_cache=pc, use_streaming=True)
            kv, pc = out.encoder_past_key_values, out.padding_cache
            got.append(out.audio_codes)
    got = torch.cat(got, dim=-1)
    ours = esr.encode_stream(x, sd, split)
    record("encode_stream_ref_vs_transformers", split=split, equal=bool(torch.equal(got, ours)),
           equal_to_whole=bool(torch.equal(got, codes)))
    assert torch.equal(got, ours)
    assert torch.equal(ours, codes)


# ---- seeds -----------------------------------------------------------------------------------------------------------
SEED_SPLITS = {13: [2, 3, 1, 7], 130: SPLIT_130, 133: [7] * 19, 9: [4, 4, 1], 11: [3, 1, 2, 2, 3], 10: [1, 2, 7]}


@pytest.mark.parametrize("name", list(esr.CLIPS))
def test_clips_have_no_flip(sd, name):
    """The streamed reference's codes are ``mimi_ref.encode``'s on every clip the GPU tests use (K = 32, so every
    prefix too): an explained flip on the GPU is then the GPU's rounding at a near tie, not the clip's."""
    cfg = esr.clip_cfg(name)
    x, emb, codes = whole(name, sd, 32)
    got = mimi_ref.rvq_from_embedding(esr.embed_stream(x, sd, SEED_SPLITS[esr.CLIPS[name][0]], cfg), sd, 32, cfg)
    _, margins = mimi_ref.rvq_from_embedding(emb, sd, 8, cfg, return_margins=True)
    record("encode_stream_ref_clip", clip=name, frames=esr.CLIPS[name][0], flips=int((got != codes).sum()),
           min_margin_K8=float(margins.min()))
    assert torch.equal(got, codes), name
    assert float(margins.min()) > 0.0


# ---- state and declarations ------------------------------------------------------------------------------------------
def test_state_is_bounded(sd):
    """The cache never holds more than W - 1 rows and the carries keep their sizes, however far the stream runs."""
    cfg = RefConfig(sliding_window=5)
    st = esr.StreamState(sd, 1, cfg)
    x = esr.clip("t13")
    sizes = None
    for t, a in enumerate(esr.chunks(x[..., :12 * esr.FRAME], [1] * 12)):
        st.embed(a)
        now = {k: tuple(v.shape) for k, v in st.carry.items()}
        assert sizes is None or now == sizes
        sizes = now
        assert all(k.shape[2] == min(2 * (t + 1), 4) for k in st.k)
    assert st.position == 12
    assert [(n, h, c) for n, h, c in esr.carry_plan(RefConfig())] == [
        ("conv0", 6, 1), ("res0", 2, 64), ("down0", 4, 64), ("res1", 2, 128), ("down1", 5, 128), ("res2", 2, 256),
        ("down2", 6, 256), ("res3", 2, 512), ("down3", 8, 512), ("final", 2, 1024), ("ds", 2, 512)]


def test_null_calls_fail_without_gpu_work():
    lib = _lib.load()
    assert lib.mimi_encode_stream_create(None, 1, 8, 1, None) == 1
    assert lib.mimi_encode_stream_step(None, None, 1, None, None) == 1
    assert b"null stream" in lib.mimi_last_error()
    assert lib.mimi_encode_stream_step_slots(None, None, 1, None, 1, None, None) == 1
    assert lib.mimi_encode_stream_reset(None) == 1
    assert lib.mimi_encode_stream_reset_slot(None, 0) == 1
    assert lib.mimi_encode_stream_position(None) == -1
    assert lib.mimi_encode_stream_slot_position(None, 0) == -1
    assert lib.mimi_encode_stream_state_bytes(None) == -1
    lib.mimi_encode_stream_destroy(None)
    assert lib.mimi_frame_samples_cfg(None) == 1920
