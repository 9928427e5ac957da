"""CPU: checks the checker of tests/test_rvq_kernels.py (tests/rvq_ref.py).

* The crafted projections are exact, and the oracle (torch CPU fp32) is within the HARD condition q <= 2 n on every
  case, with no exact rule broken; the largest q_oracle per case is printed.
* The CPU emulation of the one-product selection puts every case's (32-frame tile, slice) in its intended
  candidate-count class (<= 64: the chain's staged re-score; 65 .. 2048: the list path; > 2048: every code scored),
  passes the audit itself (``tiny`` and the embedding x 2^-120 have rs = inf at every frame and every (frame, code) pair
  a candidate; x 2^-60 and x 2^-50 do not: rs = 2^70, 2^60), and measures the ``coherent`` winner at >= 0.5 of the window above the approximate minimum
  (measured: 0.569 on both crafted models), so a window narrowed 2 x or more loses a determinate code there.
* Each injected fault fails the audit or an exact rule on at least one case (margins printed with -s):
      approx_only  the approximate argmin with no re-score          coherent_* (q = 3097: the rival the window is for)
      window/2, /4 the window narrowed                              coherent_* (the same determinate code lost)
      last_tie     the last index on equal distances in a slice     dup, flat40 (exact rule: a lower equal row exists)
      merge_later  equal distances: the later slice wins the merge  dup, flat40 (exact rule)
      truncate     the list cut at 2048, nothing else scored        group65 (the winner is the list's last code)
      skip_tail    the frames of a partial last tile left at 0      dup, flat40
      no_resid     the residual not updated after a level           zero_K3 (level 2 must see exactly 0), embscale+0
* ON THE GOLDEN EMBEDDING (emb_speech10s, the input of tests/test_gpu_parity.py's bit-exact quantizer tests) the same
  faults are emulated: approx_only, skip_tail and no_resid change codes there and so would fail those tests too;
  window/2, window/4, last_tie, merge_later and truncate leave every code as it is -- natural data has no equal rows,
  no crowded window and one candidate per frame and slice.  That is the gap tests/test_rvq_kernels.py closes.
"""
import numpy as np
import pytest

import rvq_ref as R


@pytest.fixture(scope="module")
def models():
    return R.state_dicts()


@pytest.fixture(scope="module")
def base_emb(golden):
    return np.ascontiguousarray(golden[0]["emb_speech10s"][:, :40])


@pytest.fixture(scope="module")
def cases(base_emb):
    out = R.crafted_cases() + [R.case_zero(32), R.case_flat(996)]
    out += [R.case_embscale(base_emb, s) for s in R.EMB_SCALES]
    return {c.name: c for c in out}


@pytest.fixture(scope="module")
def projs(cases, models):
    return {n: R.oracle_proj(c.frames, models[c.model]) for n, c in cases.items()}


@pytest.fixture(scope="module")
def embs(models):
    return {m: R.embeds(sd, 32) for m, sd in models.items()}


@pytest.fixture(scope="module")
def clean(cases, projs, embs):
    """The fault-free emulation of every case on 256-code slices."""
    return {n: R.emulate(projs[n], embs[c.model], c.K) for n, c in cases.items()}


def test_crafted_projection_is_exact(cases, projs):
    for n, c in cases.items():
        if c.model != "stock":
            assert np.array_equal(projs[n].view(np.uint32), np.ascontiguousarray(c.frames[0].T).view(np.uint32)), n


def test_oracle_within_hard_condition(cases, projs, embs, models):
    bad = []
    for n, c in cases.items():
        a = R.audit(projs[n], R.oracle_codes(c.frames, models[c.model], c.K), embs[c.model])
        print(f"{n}: T = {c.T} K = {c.K} q_oracle = {a['q']:.4g} determinate = {a['determinate']} worst = {a['worst']}")
        if not a["q"] <= R.HARD:
            bad.append(f"{n}: q_oracle = {a['q']:.4g} > {R.HARD} at {a['worst']}")
        bad += [f"{n}: {b}" for b in a["bad"]]
    assert not bad, "\n".join(bad)


def test_emulation_passes_the_audit(cases, projs, embs, clean):
    bad = []
    for n, c in cases.items():
        a = R.audit(projs[n], clean[n]["codes"], embs[c.model])
        print(f"{n}: q_emulation = {a['q']:.4g}")
        bad += [f"{n}: {m}" for m in R.conditions(a["q"], 0.0) + a["bad"]]
    assert not bad, "\n".join(bad)


def test_candidate_count_classes(cases, projs, embs, clean):
    bad = []
    for n, c in cases.items():
        if not c.expect:
            continue
        ems = {256: clean[n]}
        if any(e[4] == 512 for e in c.expect):
            ems[512] = R.emulate(projs[n], embs[c.model], c.K, slc=512)
        for level, t, s, cls, slc in c.expect:
            print(f"{n}: level {level} tile {t} ({slc}-code slices) candidates {ems[slc]['counts'][level][t].tolist()}"
                  f" wanted {cls}")
        bad += R.check_expect(c, ems)
    assert not bad, "\n".join(bad)


def test_infinite_scale_cases(cases, projs, clean):
    """rs = inf (max |r| < 2^-114) at both levels that read the projection, for every frame of ``tiny`` and of the
    embedding x 2^-120 -- and for no frame at 2^-60 and 2^-50, whose residuals are merely small.  With rs = inf every
    (frame, code) pair of every slice is a candidate."""
    for n in ("tiny", "embscale-120"):
        rs = R.first_scales(projs[n])
        mx = np.abs(projs[n]).reshape(-1, 2, R.D).max(2)
        assert np.isinf(rs).all() and (mx > 0).all() and (mx < R.RS_INF_BELOW).all(), (n, rs.min(), mx.max())
        T = projs[n].shape[0]
        for level in (0, 1):
            want = np.minimum(32, T - 32 * np.arange(-(-T // 32)))[:, None] * 256
            assert np.array_equal(clean[n]["counts"][level], np.broadcast_to(want, clean[n]["counts"][level].shape)), n
    for n in ("embscale-60", "embscale-50"):
        rs = R.first_scales(projs[n])
        print(f"{n}: rs = 2^{np.log2(rs.min()):.0f} .. 2^{np.log2(rs.max()):.0f}")
        assert np.isfinite(rs).all(), n
        assert (clean[n]["counts"][0] < 32 * 256).all(), n


@pytest.mark.parametrize("model", ["degen", "pairs"])
def test_coherent_winner_is_deep_in_the_window(cases, clean, model):
    c = cases[f"coherent_{model}"]
    level = c.expect[0][0]
    em = clean[c.name]
    assert (em["codes"][level] == R.COH_PAIRS[model][0]).all()
    ratio = float(em["pos"][level].min())
    print(f"coherent_{model}: the winner lies at {ratio:.3f} of the window above the approximate minimum")
    assert ratio >= 0.5, ratio


FAULT_CASES = {"approx_only": ["coherent_degen", "coherent_pairs"], "window/2": ["coherent_degen", "coherent_pairs"],
               "window/4": ["coherent_degen", "coherent_pairs"], "last_tie": ["dup", "flat40"],
               "merge_later": ["dup", "flat40"], "truncate": ["group65"], "skip_tail": ["dup", "flat40"],
               "no_resid": ["zero_K3", "embscale+0"]}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_fault_is_caught(cases, projs, embs, fault):
    caught = 0
    for n in FAULT_CASES[fault]:
        c = cases[n]
        a = R.audit(projs[n], R.emulate(projs[n], embs[c.model], c.K, fault=fault)["codes"], embs[c.model])
        misses = R.conditions(a["q"], 0.0) + a["bad"]
        print(f"{fault} on {n}: q = {a['q']:.4g} ({a['q'] / R.HARD:.3g} x the hard bound), {len(a['bad'])} exact-rule "
              f"violations{': ' + a['bad'][0] if a['bad'] else ''}")
        caught += bool(misses)
    assert caught, f"{fault}: passed on {FAULT_CASES[fault]}"


GOLDEN_CATCHES = {"approx_only": True, "window/2": False, "window/4": False, "last_tie": False, "merge_later": False,
                  "truncate": False, "skip_tail": True, "no_resid": True}


def test_which_faults_the_golden_embedding_shows(golden, models, embs):
    """The existing quantizer tests compare codes on natural embeddings with a fixture: a fault shows there only if it
    changes a code."""
    emb = golden[0]["emb_speech10s"][None]
    K = 4
    proj = R.oracle_proj(emb, models["stock"])
    ref = R.emulate(proj, embs["stock"], K)
    assert np.array_equal(ref["codes"], golden[0]["embcodes_speech10s"][:K])
    print("candidates per frame and slice:", float(np.mean([c.sum() for c in ref["counts"]])) / (proj.shape[0] * 8))
    got = {}
    for fault in R.FAULTS:
        codes = R.emulate(proj, embs["stock"], K, fault=fault)["codes"]
        got[fault] = bool((codes != ref["codes"]).any())
        print(f"{fault}: {int((codes != ref['codes']).sum())} of {codes.size} codes change on emb_speech10s")
    assert got == GOLDEN_CATCHES
