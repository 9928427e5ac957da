"""CPU: the restatement of the resampler's launcher and pass structure (tests/resample_pass_ref.py) against scipy, its
index invariants, and which shapes catch which injected fault.

The last point is the reason for tests/test_resample_kernels.py: the shapes of the GPU tests in tests/test_resample.py
run one pass per workgroup on every generic kernel, so a kernel whose pass hand-over is wrong -- (a) stale window in
load-then-compute, (b) dropped buffer toggle, (c) prefetch from the wrong window -- or whose register-FIR ``interior``
test is off by one (f) returns the same values on them as a correct one; the 256-clip ragged batches do not.
"""
import functools
import math

import numpy as np
import pytest

import resample_pass_ref as R

FORM_IDS = [f"{m}-{r}" for m, r, _ in R.FORM_TABLE]


@functools.lru_cache(maxsize=None)
def _mode_plan(mode, rate):
    return R.mode_plan(mode, rate)


def _batch(mode, rate):
    """the 256-clip ragged batch of a form, as tests/test_resample_kernels.py builds it"""
    up, down, hp, pre = _mode_plan(mode, rate)
    p1 = R.plan(len(hp), up, down, pre, R.NCLIPS, 1 << 20)
    lens = R.ragged_lengths(up, down, p1.pass_outputs, p1.fir)
    clips = [R.clip(rate + 7 * i, n) for i, n in enumerate(lens)]
    n_run = [R.api_lengths(n, rate)[1] for n in lens]
    return clips, n_run, (up, down, hp, pre)


@functools.lru_cache(maxsize=None)
def _clean(mode, rate):
    clips, n_run, (up, down, hp, pre) = _batch(mode, rate)
    return R.emulate(clips, hp, up, down, pre, n_outs=n_run)


def _differs(a, b):
    return any(not R.bits_equal(x, y) for x, y in zip(a, b))


def test_fir_constants():
    a, b = R.FIR_FORMS
    assert (a.LH, a.PRE, a.C0, a.W, a.PASS) == (63, 16, 2, 533, 768)
    assert (b.LH, b.PRE, b.C0, b.W, b.PASS) == (62, 31, 1, 277, 768)
    for f, rate in ((a, 16000), (b, 8000)):
        up, down, hp, pre = _mode_plan("polyphase", rate)
        assert (up, down, len(hp), pre) == (f.UP, f.DOWN, f.LH, f.PRE)


@pytest.mark.parametrize("mode,rate,form", R.FORM_TABLE, ids=FORM_IDS)
def test_form_table_and_pass_counts(mode, rate, form):
    clips, n_run, (up, down, hp, pre) = _batch(mode, rate)
    p = R.plan(len(hp), up, down, pre, len(clips), max(n_run))
    assert p.name == form and len(clips) == R.NCLIPS and p.grid == 16
    # four passes, the last holding a single output -- or, where up > down makes no clip that long (outputs come
    # ceil(up / down) at a time: 3 S + 1 is never a length at 8, 12 and 16 kHz), the fewest any clip can leave there
    last = max(n_run) - 3 * p.sweep
    assert R.passes(p, max(n_run)) == 4 and 1 <= last <= -(-up // down) and (last == 1 or up > down)
    got = sorted(set(n_run))
    whole = [k * p.sweep for k in (1, 2, 3) if k * p.sweep in got]                    # exact multiples of a sweep
    assert 0 in got and whole and (len(whole) == 3 or up > down)                     # (up > down skips some lengths)
    assert any(0 < n < p.pass_outputs for n in n_run) and any(R.passes(p, n, 15) == 0 for n in n_run if n)
    if p.wpt:
        assert p.W <= p.wpt * R.RS_BLOCK
    assert p.lds_bytes <= R.LDS_LIMIT


def test_known_windows_and_rejection():
    for rate, w in ((96000, 1106), (192000, 2210)):
        up, down, hp, pre = _mode_plan("polyphase", rate)
        assert R.plan(len(hp), up, down, pre, 32, 100000).W == w
    for name, up, down, taps, form, w in R.THRESHOLDS:
        p = R.plan(taps, up, down, R.threshold_pre_remove(taps, down), R.NCLIPS, 1 << 20)
        assert (p.name, p.W) == (form, w), name
    up, down, taps = R.IMPOSSIBLE
    with pytest.raises(R.Rejected):
        R.plan(taps, up, down, 0, R.NCLIPS, 1000)
    assert R.plan(63, 3, 2, 16, 0, 10) is None and R.plan(63, 3, 2, 16, 4, 0) is None


@pytest.mark.parametrize("mode,rate,form", R.FORM_TABLE, ids=FORM_IDS)
def test_emulation_bit_equal_scipy(mode, rate, form):
    """the fault-free emulation of the whole 256-clip batch (4 passes on the longest clip) equals scipy bit for bit"""
    from scipy.signal import resample_poly
    clips, n_run, (up, down, hp, pre) = _batch(mode, rate)
    outs, stats, p = _clean(mode, rate)
    assert p.name == form and stats["passes"] == 4 and not stats["violations"], stats
    assert stats["exited"] > 0
    if p.kind == "fir":
        assert stats["interior_late"] > 0 and stats["edge"] > 0
    for x, n, o in zip(clips, n_run, outs):
        want = resample_poly(x, up, down)[:n] if mode == "polyphase" and len(x) else R.upfirdn_ref(x, hp, up, down, pre, n)
        assert R.bits_equal(o, want), (mode, rate, len(x))


@pytest.mark.parametrize("name,up,down,taps,form,w", R.THRESHOLDS, ids=[t[0] for t in R.THRESHOLDS])
def test_emulation_thresholds_bit_equal_upfirdn(name, up, down, taps, form, w):
    h = R.random_filter(taps)
    pre = R.threshold_pre_remove(taps, down)
    lens = [R.n_in_for(t, up, down) for t in (3 * 256 + 1, 256, 255, 1)]
    clips = [R.clip(i, n) for i, n in enumerate(lens)]
    outs, stats, p = R.emulate(clips, h, up, down, pre, nclips=4096)   # a grid of one workgroup: 4 passes
    assert p.name == form and stats["passes"] == 4 and not stats["violations"]
    for x, o in zip(clips, outs):
        assert R.bits_equal(o, R.upfirdn_ref(x, h, up, down, pre, len(o))), (name, len(x))


@pytest.mark.parametrize("mode,rate", (("polyphase", 16000), ("polyphase", 8000), ("polyphase", 96000),
                                       ("soxr_hq", 22050)))
def test_emulation_adversarial_samples(mode, rate):
    """zeros, -0.0, full-scale alternation, subnormal products, Inf and NaN samples: the kernel's float32 arithmetic, as
    emulated, is scipy's.  scipy's upfirdn pads every filter phase to ceil(lh / up) taps, so where up does not divide lh
    (8 kHz, soxr_hq 22.05 kHz here) it multiplies one more input sample by a padding zero: +0 for a finite sample, NaN
    for a non-finite one.  The kernel runs that term too, so the non-finite positions are scipy's."""
    from scipy.signal import resample_poly
    up, down, hp, pre = _mode_plan(mode, rate)
    n = R.n_in_for(2 * 256 + 9, up, down)
    for name, x in R.adversarial_clips(n).items():
        outs, stats, p = R.emulate([x], hp, up, down, pre, nclips=4096)
        got, want = outs[0], R.upfirdn_ref(x, hp, up, down, pre, len(outs[0]))
        assert not stats["violations"]
        if mode == "polyphase":
            assert R.same_nonfinite_and_bits(want, resample_poly(x, up, down)), (rate, name)
        if name in R.NONFINITE:
            assert R.same_nonfinite_and_bits(got, want) and not np.isfinite(got).all(), (rate, name)
        else:
            assert R.bits_equal(got, want), (rate, name)
        if name == "subnormal":
            assert np.any(got != 0) and np.all(np.abs(got) < np.float32(2.0 ** -120))


@pytest.mark.parametrize("mode", ("polyphase", "soxr_hq"))
@pytest.mark.parametrize("rate", R.RATES)
def test_index_invariants(mode, rate):
    """every supported pair, over a full period of p0 mod up (p0 = (m0 + pre_remove) down at the pass starts m0 = 256 j)
    and at the clip edges: window reads in [0, W), filter indices in [0, lh), pr in 32 bits, W within the prefetch"""
    up, down, hp, pre = _mode_plan(mode, rate)
    lh = len(hp)
    P = R.plan(lh, up, down, pre, 4096, 1).pass_outputs
    period = up // math.gcd(P * down, up)
    n_long = P * (period + 2) + 17
    lens = [R.n_in_for(t, up, down) for t in (n_long, 1, 2, P - 1, P, P + 1, 2 * P + 188)] + [1, 2, 3]
    clips = [np.ones(n, np.float32) for n in lens]
    outs, stats, p = R.emulate(clips, hp, up, down, pre, nclips=4096, values=(lh < 100))
    assert p.grid == 1 and stats["passes"] == period + 3 >= 3
    assert not stats["violations"], stats["violations"]
    if p.kind == "poly":
        seen = {((P * j + pre) * down) % up for j in range(stats["passes"])}
        assert len(seen) == period                                     # every reachable p0 mod up was run
        assert stats["max_k_first"] < R.padded_len(lh, up) and stats["min_k_last"] >= 0   # (>= lh: the padding tap)
        assert stats["max_pr"] < up + 255 * down < 1 << 31
        kc = (R.padded_len(lh, up) - 1 + up - 1) // up
        assert up + 255 * down + kc * up + up < 1 << 31                 # the ceil identity's numerator
        # reads run to W - 1 with scipy's padded first term, to W - 2 (a spare sample) where up divides lh
        assert stats["max_window_read"] <= (p.W - 1 if lh % up else p.W - 2)
        if p.wpt:
            assert p.W <= p.wpt * 256
        assert p.lds_bytes <= R.LDS_LIMIT


def _fault_applies(p, fault):
    """a fault changes code of this form at all (elsewhere the faulty kernel text is the same text)"""
    return {"stale_pass": p.kind == "poly" and p.wpt == 0,
            "no_toggle": p.kind == "poly" and p.wpt > 0,
            "prefetch_w0": p.kind == "poly" and p.wpt > 0,
            "short_window": True,
            "trunc_ceil": True,
            "fir_interior": p.kind == "fir"}[fault]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_new_shapes_catch_every_fault(fault):
    """each injected fault changes output VALUES of the new 256-clip batches, on every form whose code it touches;
    the batches are the GPU tests' own (same lengths, same samples, same NaN tail behind the packed clips)"""
    caught = {}
    for mode, rate, form in R.FORM_TABLE:
        clips, n_run, (up, down, hp, pre) = _batch(mode, rate)
        clean, cstats, p = _clean(mode, rate)
        if not _fault_applies(p, fault):
            continue
        # the clips that sweep (the first 14) and the register-FIR edge clips (the last 3) suffice
        only = set(range(14)) | set(range(R.NCLIPS - 3, R.NCLIPS))
        outs, stats, _ = R.emulate(clips, hp, up, down, pre, n_outs=n_run, fault=fault, only=only)
        caught[(mode, rate, form)] = _differs([o for o in outs if o is not None],
                                               [c for c, o in zip(clean, outs) if o is not None])
        if fault == "short_window" and p.kind == "poly":
            # staged: [0, W - 1) where up does not divide lh, else [0, W - 2); seen exactly where a pass reads past it
            first_unstaged = p.W - 1 if len(hp) % up else p.W - 2
            assert caught[(mode, rate, form)] == (cstats["max_window_read"] == first_unstaged), (mode, rate)
    assert caught
    if fault in ("stale_pass", "no_toggle", "prefetch_w0", "fir_interior"):
        assert all(caught.values()), caught
    elif fault == "short_window":
        assert all(v for k, v in caught.items() if k[2].startswith("fir"))
        for wpt in "0124":   # at least one form of every prefetch depth
            assert any(v for k, v in caught.items() if k[2].startswith(f"poly<{wpt},")), wpt
    else:
        # trunc_ceil: exact for up = 1, clamped away on the register-FIR edge path.  Elsewhere it drops the first term of
        # every output whose numerator is not 1 (mod up): the terms with tap index in (lhp - up, lhp).  Where
        # lh = 1 (mod up) (32 kHz: 85 taps, up 3) those are all padding taps, x * 0, and finite samples cannot show it
        for (mode, rate, form), v in caught.items():
            up, _, hp, _ = _mode_plan(mode, rate)
            if form.startswith("fir") or up == 1:
                assert not v, (mode, rate)
            elif up >= 3:
                assert v == (len(hp) % up != 1), (mode, rate)
        for wpt in "0124":   # seen by at least one form of every prefetch depth
            assert any(v for k, v in caught.items() if k[2].startswith(f"poly<{wpt},")), wpt


@pytest.mark.parametrize("fault", ("stale_pass", "no_toggle", "prefetch_w0", "fir_interior"))
def test_todays_gpu_shapes_miss_the_pass_faults(fault):
    """the shapes of tests/test_resample.py's GPU tests (and of smoke()) return the same values from a kernel with
    fault (a), (b), (c) or (f) as from a correct one: no generic kernel runs a second pass on them, and the one
    register-FIR second pass (60 s at 16 kHz) is nowhere near the ``interior`` edge.

    This is about the pass structure, in program order.  Fault (b) as a kernel edit (xn from pass & 1) ALSO stores into
    the window the workgroup's other waves are still reading, with no barrier between: a race inside every pass, the
    first included (``stats["race"]``).  On an MI355X today's tests do catch that mutant, through the race, on the forms
    with several waves of window (profiles/resample_passes_parent.txt); with a barrier in front of the store -- the
    pass-structure fault alone -- they pass, and only the multi-pass batches fail."""
    ran = 0
    for mode, rate, lens in R.TODAY_SHAPES:
        up, down, hp, pre = _mode_plan(mode, rate)
        n_run = [R.api_lengths(n, rate)[1] for n in lens]
        p = R.plan(len(hp), up, down, pre, len(lens), max(n_run))
        if p.kind == "poly":
            assert R.passes(p, max(n_run)) == 1, (mode, rate)
        else:
            second = p.name == "fir<3,2,3>" and max(lens) == 16000 * 60      # the only later pass anywhere
            assert R.passes(p, max(n_run)) == (2 if second else 1), (mode, rate)
        if not _fault_applies(p, fault):
            continue
        clips = [R.clip(rate + i, n) for i, n in enumerate(lens)]
        clean, cstats, _ = R.emulate(clips, hp, up, down, pre, n_outs=n_run, tail=0)
        outs, stats, _ = R.emulate(clips, hp, up, down, pre, n_outs=n_run, tail=0, fault=fault)
        assert not cstats["violations"] and not stats["violations"], (mode, rate, stats["violations"])
        assert not _differs(outs, clean), (mode, rate, fault)
        assert stats["race"] == (fault == "no_toggle")
        ran += 1
    assert ran
