"""GPU: the RVQ kernels (proj -> codes) on adversarial residuals and codebooks, audited in float64.

tests/rvq_ref.py holds the audit (q = (d2(chosen) - min d2) / (2^-24 (|r| + |e|)^2) per level and frame, on the engine's
own ``proj`` tap and its own earlier codes; HARD q <= 2 n = 558, WORKING q <= 16 max(q_oracle, 1)), the exact rules (codes
in range, the lowest index of bitwise-equal rows, determinate codes = the float64 argmin), the crafted models and the
cases; tests/test_rvq_ref.py shows on the CPU which injected faults they catch.  Here every case runs on every kernel
form: the default form of a shape is audited, every other form and option must return the same bits (they share one
exact chain, so even near ties resolve identically), and every run pins the kernel from the profiled ``rvq`` stage's
symbol.  A retune that moves a threshold fails there: move the shape with it.

  frames                        option               symbol of the profiled rvq stage
  1, 31, 32, 33, 40, 128,       default              rvq_chain_h16_kernel<256, 16>
  129, 160, 256                 rvq_chain = 0        rvq_level_h16_kernel<256, 16, 32, false, 32, 8, 32, true>
  257, 264, 992                 default              <256, 16, 32, false, 32, 8, 32, true>
  40, 160, 264                  rvq_form = 1         <256, 16, 32, false, 32, 8, 32, false>
  993, 996, 1000                default (form 5)     <256, 8, 16, false, 64, 8, 32, true>
  996, 1000                     rvq_form = 1         <256, 2, 16, false, 64, 8, 32, false>
                                rvq_form = 2         <256, 2, 16, false, 64, 8, 32, true>
                                rvq_form = 3         <256, 2, 16, false, 64, 8, 64, true>
                                rvq_form = 4         <256, 4, 16, false, 64, 8, 32, true>
                                rvq_form = 6         <256, 16, 32, false, 32, 8, 32, true>
                                rvq_xcd = 0          the default's symbol
The persistent chain takes every grid of at most 128 workgroups, 64 ceil(2 ceil(frames / 32) / 8): up to 256 frames
(launch_rvq), so chain | per-level small form sits at 256 | 257 frames (not at 128 | 129, where the chain's grid grows
from 64 to 128 workgroups: both sides are run as well); small | large form at 992 | 993.  1000 = 31 x 32 + 8 gives the
64-frame form (3) a 40-frame tail; 264 = 8 x 32 + 8 and 996 = 31 x 32 + 4 give ``flat`` a tail tile of exactly 2048
candidates on 256- and on 512-code slices.

Shapes of the case runs: 40 frames (chain), 264 (small per-level form), 996 (large form); a case's frames are repeated
cyclically to the shape.  K = 2 on the crafted models (levels 0 and 1 see the crafted codebooks directly), K = 1, 3 and
32 on ``dup`` and ``zero``, K = 8 for ``embscale`` (x 2^-120 and ``tiny`` are the rs = inf cases); the stock model at 128 | 129, 256 | 257 and 992 | 993 frames with
K = 32, audited at all 32 levels.

q_oracle: on the crafted models oracle.mimi_ref.rvq_from_embedding on the embedding itself (the projection is exact, and
asserted so bitwise on the tap); on the stock model, whose projection rounds, the same oracle's quantizer loop on the
engine's own ``proj`` tap (rvq_ref.oracle_on_proj), so that both are measured on the same input.

Each audited run appends {test: "rvq", case, shape, kernel, K, q_engine, q_oracle, n, oracle_disagreements} to
``parity_log`` (parity_report.json; the baseline copy is profiles/rvq_parity.json).  Measured on an MI355X: see
profiles/rvq_parity.json and DESIGN 4.1.
"""
import json

import numpy as np
import pytest
import torch

import rvq_ref as R

pytestmark = pytest.mark.gpu

CHAIN = "mimi::rvq_chain_h16_kernel<256, 16>"


def lv(pf, ex, cw, ft, p1):
    return f"mimi::rvq_level_h16_kernel<256, {pf}, {ex}, false, {cw}, 8, {ft}, {'true' if p1 else 'false'}>"


SMALL, SMALL_3P = lv(16, 32, 32, 32, True), lv(16, 32, 32, 32, False)
LARGE = lv(8, 16, 64, 32, True)
LARGE_FORMS = {1: lv(2, 16, 64, 32, False), 2: lv(2, 16, 64, 32, True), 3: lv(2, 16, 64, 64, True),
               4: lv(4, 16, 64, 32, True), 6: SMALL}
DEFAULTS = {"rvq_chain": 1, "rvq_form": 0, "rvq_xcd": 1}
CHAIN_MAX, SMALL_MAX = 256, 992
SHAPES = (40, 264, 996)


def default_symbol(T):
    return CHAIN if T <= CHAIN_MAX else SMALL if T <= SMALL_MAX else LARGE


def variants(T):
    """[(options, symbol)] of every other form that runs T frames."""
    if T <= SMALL_MAX:
        out = [({"rvq_form": 1}, SMALL_3P)]
        if T <= CHAIN_MAX:
            out.append(({"rvq_chain": 0}, SMALL))
        return out
    return [({"rvq_form": f}, s) for f, s in LARGE_FORMS.items()] + [({"rvq_xcd": 0}, LARGE)]


@pytest.fixture(scope="module")
def sds():
    return R.state_dicts()


@pytest.fixture(scope="module")
def embs(sds):
    return {m: R.embeds(sd, 32) for m, sd in sds.items()}


def _engine(sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    return MimiHipModel(sd, device="cuda:0")


@pytest.fixture(scope="module")
def eng_stock(sds):
    m = _engine(sds["stock"])
    yield m
    m.close()


@pytest.fixture(scope="module")
def eng_pairs(sds):
    m = _engine(sds["pairs"])
    yield m
    m.close()


@pytest.fixture(scope="module")
def eng_degen(sds):
    m = _engine(sds["degen"])
    yield m
    m.close()


@pytest.fixture(scope="module")
def engines(eng_stock, eng_pairs, eng_degen):
    return {"stock": eng_stock, "pairs": eng_pairs, "degen": eng_degen}


@pytest.fixture(scope="module")
def natural(golden):
    """A natural embedding [512, 1000]: emb_speech60s (750 frames) repeated."""
    e = golden[0]["emb_speech60s"]
    return np.ascontiguousarray(np.tile(e, (1, 2))[:, :1000])


def run(m, emb, K, opts=None):
    """One profiled, taps-on quantize of emb [1, 512, T] -> (codes [K, T], the rvq stage's symbol, proj [T, 512])."""
    opts = opts or {}
    reruns = m.rvq_chain_reruns
    try:
        for k, v in opts.items():
            m.set_option(k, v)
        m.set_taps(True)
        m.set_profiling(1)
        codes = m.quantize(torch.from_numpy(np.ascontiguousarray(emb)).cuda(), K)[0].cpu().numpy()
        seq = m.profile_sequence()
        proj = m.get_tap("proj").copy()[0]
    finally:
        m.set_profiling(0)
        m.set_taps(False)
        for k in opts:
            m.set_option(k, DEFAULTS[k])
    # a chain that gave up (another process held the CUs) is answered by one re-run on the per-level small form: the
    # codes are that re-run's, the first symbol is still the form the shape and options select
    gave_up = m.rvq_chain_reruns - reruns
    syms = [k for s, k in seq if s == "rvq"]
    assert [s for s, _ in seq] == ["input_proj"] + ["rvq"] * (1 + gave_up) and gave_up in (0, 1), (seq, gave_up)
    if gave_up:
        assert syms == [CHAIN, SMALL], f"the chain gave up and was re-run: wanted {[CHAIN, SMALL]}, ran {syms}"
    return codes, syms[0], proj


def check(parity_log, m, sd, emb_levels, model, name, emb, K, bad):
    """The default form audited (both conditions, the exact rules, the crafted projection exact), every other form
    bitwise equal to it, every symbol pinned; failures are collected in ``bad``."""
    T = emb.shape[2]
    codes, sym, proj = run(m, emb, K)
    if sym != default_symbol(T):
        bad.append(f"{name} T = {T}: ran {sym}, wanted {default_symbol(T)}")
    if model != "stock" and not np.array_equal(proj.view(np.uint32), np.ascontiguousarray(emb[0].T).view(np.uint32)):
        bad.append(f"{name} T = {T}: the proj tap is not the embedding's halves bit for bit")
    a = R.audit(proj, codes, emb_levels)
    oc = R.oracle_codes(emb, sd, K) if model != "stock" else R.oracle_on_proj(proj, sd, K)
    ao = R.audit(proj, oc, emb_levels)
    rec = {"test": "rvq", "case": name, "shape": T, "kernel": sym, "K": K, "q_engine": a["q"], "q_oracle": ao["q"],
           "n": R.N_RVQ, "oracle_disagreements": int((oc != codes).sum()), "determinate": a["determinate"],
           "worst": a["worst"]}
    parity_log.append(rec)
    print(json.dumps(rec))
    bad += [f"{name} T = {T} ({sym}): {msg} at {a['worst']}" for msg in R.conditions(a["q"], ao["q"])]
    bad += [f"{name} T = {T} ({sym}): {msg}" for msg in a["bad"]]
    bad += [f"{name} T = {T}: oracle: {msg}" for msg in R.conditions(ao["q"], ao["q"]) + ao["bad"]]
    for opts, want in variants(T):
        c2, s2, _ = run(m, emb, K, opts)
        if s2 != want:
            bad.append(f"{name} T = {T} {opts}: ran {s2}, wanted {want}")
        if not np.array_equal(c2, codes):
            w = np.argwhere(c2 != codes)
            bad.append(f"{name} T = {T} {opts} ({s2}): {len(w)} codes differ from the default form's, first at "
                       f"(level, frame) {w[0].tolist()}: {c2[tuple(w[0])]} vs {codes[tuple(w[0])]}")
    return rec


# ---- a. the symbol table on natural data, both sides of every threshold -------------------------------------------------
@pytest.mark.parametrize("T", [1, 31, 32, 33, 40, 128, 129, 160, 256, 257, 992, 993, 996, 1000])
def test_symbols_and_forms_natural(engines, sds, embs, natural, parity_log, T):
    bad = []
    check(parity_log, engines["stock"], sds["stock"], embs["stock"], "stock", "natural", natural[None, :, :T], 8, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("T", [128, 129, 256, 257, 992, 993])
def test_stock_thresholds_all_levels(engines, sds, embs, natural, parity_log, T):
    bad = []
    check(parity_log, engines["stock"], sds["stock"], embs["stock"], "stock", "natural_K32", natural[None, :, :T], 32, bad)
    assert not bad, "\n".join(bad)


# ---- b. the crafted cases on the chain, the small and the large form ---------------------------------------------------
CASE_NAMES = ["dup", "midpoint", "scales", "flat40", "group8", "group65", "coherent_degen", "coherent_pairs", "tiny",
              "zero_K3", "zero_K32"]


@pytest.fixture(scope="module")
def cases():
    out = {c.name: c for c in R.crafted_cases() + [R.case_zero(32)]}
    assert sorted(out) == sorted(CASE_NAMES)
    return out


def assert_infinite_scale(m, emb, K):
    """The tap itself shows that the run took the rs = inf path: 0 < max |proj| < 2^-114 in both halves of every frame."""
    mx = np.abs(run(m, emb, K)[2]).reshape(-1, 2, R.D).max(2)
    assert (mx > 0).all() and (mx < R.RS_INF_BELOW).all(), (mx.min(), mx.max())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_crafted_case(engines, sds, embs, parity_log, cases, name):
    c = cases[name]
    bad = []
    for T in SHAPES:
        emb = R.case_flat(T).frames if name == "flat40" else c.tiled(T)
        check(parity_log, engines[c.model], sds[c.model], embs[c.model], c.model, name.replace("flat40", "flat"), emb,
              c.K, bad)
        if name == "tiny":
            assert_infinite_scale(engines[c.model], emb, c.K)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("K", [1, 3, 32])
def test_levels_on_every_form(engines, sds, embs, parity_log, cases, K):
    """K = 1 (the semantic level alone: ``sem_split`` with nothing behind it), 3 and 32 on every form (2: the cases)."""
    c = cases["dup"]
    bad = []
    for T in SHAPES:
        check(parity_log, engines["pairs"], sds["pairs"], embs["pairs"], "pairs", f"dup_K{K}", c.tiled(T), K, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("s", R.EMB_SCALES)
def test_embedding_scale(engines, sds, embs, natural, parity_log, s):
    """2^-120: max |proj| < 2^-114 in every frame (asserted on the tap), so rs = inf, every approximate distance is NaN
    and every code a candidate; 2^-60, 2^-50: small residuals at a finite scale; 2^24 and up: most codes tie in fp32."""
    c = R.case_embscale(natural[:, :40], s)
    bad = []
    for T in SHAPES:
        check(parity_log, engines["stock"], sds["stock"], embs["stock"], "stock", c.name, c.tiled(T), c.K, bad)
        if s <= -120:
            assert_infinite_scale(engines["stock"], c.tiled(T), c.K)
    assert not bad, "\n".join(bad)
