"""GPU: every form of the ingest resampler (csrc/resample.hip) on batches whose workgroups sweep their clips in several
passes, bit for bit against scipy computed live.

tests/test_resample.py is bit-exact too, but on its shapes every generic-kernel workgroup runs exactly one pass: the
register prefetch, the double-buffered LDS window, its toggle and the hand-over of q0 / r0 / w0 between passes never
execute (tests/test_resample_pass_ref.py asserts that, and that a kernel with a fault there returns the same values on
those shapes).  The launcher caps the grid at ceil(4096 / nclips) workgroups per clip, so here every batch has 256 clips:
16 workgroups, a sweep of S = 16 x 256 outputs (16 x 768 on the register FIR), and clips of up to 3 S + 1 outputs -- four
passes, asserted from the restated launch rule (tests/resample_pass_ref.py), as is the form each case runs (FORM_TABLE,
THRESHOLDS).  Lengths (resample_pass_ref.ragged_lengths): empty, 1 sample, under one pass, one pass -1 / 0 / +1, S and
2 S each -1 / 0 / +1, 3 S, 3 S + 1 (a last pass of one output; of ceil(up / down) where up > down skips that length),
ordinary short clips (workgroups 1..15 exit at once), and for the register FIR three clips that put workgroup 0's
pass 1 on each side of ``interior``'s right edge, the last of them directly in front of the NaN tail.

Every packed input buffer is longer than the clips and ends in NaN: a read past the last clip poisons an output.

Comparisons are bitwise against scipy.signal.resample_poly (polyphase mode) or scipy.signal.upfirdn over the same filter
with resample_poly's trim (soxr_hq mode, the C entry).  The one relaxation, on clips holding Inf / NaN samples: NaN
payloads are not compared (positions, and class and sign of every infinity, are).

Measured on an MI355X (profiles/resample_passes_parent.txt; 40 tests, 20 s with the module's scipy references): all
pass.  Subnormal samples (2^-130 amplitudes) are bit-equal on every form run: no exception to the bit-exact claim.

Inf / NaN samples found a difference, fixed in resample.hip: scipy's upfirdn pads every filter phase to ceil(lh / up)
taps, so where up does not divide lh it multiplies one more input sample by a padding zero than the kernels read.
That term is +0 for a finite sample and NaN for Inf / NaN: scipy returned a NaN where the kernels returned the finite sum
(or the infinity) of the real taps -- non-finite outputs kernel / scipy per clip, before: 8 kHz (fir<3,1,3>) +Inf 62 / 63,
NaN 62 / 63, -Inf and NaN 124 / 126; soxr_hq 22.05 kHz (poly<2,0,HG>) 205 / 206, 205 / 206, 412 / 413; equal at 16, 48 and
96 kHz (lh = 0 mod up), and at 44.1 kHz only because no non-finite sample landed on a padded phase.  The kernels now
derive jlo, w0 and the register FIR's constants from the padded length and compute that term as scipy does (x * 0, never
read from the filter); outputs on finite samples are bitwise what they were (0 + x 0 = +0 in front of the same sums).
"""
import numpy as np
import pytest
import torch

import resample_pass_ref as R
from mimi_hip import _lib, ingest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 257   # NaN samples behind the packed clips
FORM_IDS = [f"{m}-{r}" for m, r, _ in R.FORM_TABLE]


def _packed(clips):
    buf = np.concatenate([np.asarray(c, np.float32) for c in clips] + [np.full(TAIL, np.nan, np.float32)])
    return torch.from_numpy(buf).to(DEV)


def run_api(clips, rate, mode):
    """ingest.resample_packed on a buffer longer than the clips whose tail is NaN -> one numpy array per clip"""
    out, n_fix = ingest.resample_packed(_packed(clips), [len(c) for c in clips], rate, 24000, res_type=mode)
    out = out.cpu().numpy()
    offs = np.concatenate([[0], np.cumsum(n_fix)[:-1]]).astype(np.int64)
    return [out[o:o + n] for o, n in zip(offs, n_fix)]


def run_c(clips, h, up, down, pre_remove):
    """mimi_resample_poly itself with any filter: clips packed (NaN tail), outputs of ceil(n up / down) samples in a
    buffer pre-filled with NaN (an output never written stays NaN)"""
    n_in = np.asarray([len(c) for c in clips], np.int64)
    n_out = -(-n_in * up // down)
    in_off = np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(n_out)[:-1]]).astype(np.int64)
    x = _packed(clips)
    meta = torch.from_numpy(np.stack([in_off, n_in, out_off, n_out])).to(DEV)
    filt = torch.from_numpy(np.ascontiguousarray(h, np.float32)).to(DEV)
    out = torch.full((int(n_out.sum()) + 1,), float("nan"), dtype=torch.float32, device=DEV)
    lib = _lib.load()
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    _lib.check(lib.mimi_resample_poly(x.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), len(clips), out.data_ptr(),
                                      meta[2].data_ptr(), meta[3].data_ptr(), int(n_out.max()), filt.data_ptr(), len(h),
                                      up, down, pre_remove, stream))
    out = out.cpu().numpy()
    assert np.isnan(out[-1])
    return [out[o:o + n] for o, n in zip(out_off, n_out)]


def api_reference(x, rate, mode, plan4):
    """what librosa's mode returns for one clip: scipy, then fix_length"""
    from scipy.signal import resample_poly
    up, down, hp, pre = plan4
    n_fix, n_run = R.api_lengths(len(x), rate)
    if len(x) == 0:
        return np.zeros(n_fix, np.float32)
    y = resample_poly(x, up, down)[:n_run] if mode == "polyphase" else R.upfirdn_ref(x, hp, up, down, pre, n_run)
    assert len(y) == n_run
    return np.concatenate([y, np.zeros(n_fix - n_run, np.float32)])


def check_plan(plan4, lens, n_run, form):
    """the restated launch rule on this batch: the literal form, 16 workgroups, four passes on the longest clip"""
    up, down, hp, pre = plan4
    p = R.plan(len(hp), up, down, pre, len(lens), max(n_run))
    assert p.name == form, (p.name, form)
    assert len(lens) == R.NCLIPS and p.grid == 16
    assert R.passes(p, max(n_run)) == 4 >= 3
    return p


@pytest.mark.parametrize("mode,rate,form", R.FORM_TABLE, ids=FORM_IDS)
def test_forms_multi_pass_vs_scipy(mode, rate, form):
    plan4 = R.mode_plan(mode, rate)
    up, down, hp, pre = plan4
    p1 = R.plan(len(hp), up, down, pre, R.NCLIPS, 1 << 20)
    lens = R.ragged_lengths(up, down, p1.pass_outputs, p1.fir)
    n_run = [R.api_lengths(n, rate)[1] for n in lens]
    p = check_plan(plan4, lens, n_run, form)
    if p.kind == "fir":   # workgroup 0's pass 1 on each side of interior's right edge; the last clip is not interior
        mlast = p.sweep + p.pass_outputs - 1
        lhs = (mlast + p.fir.PRE) * p.fir.DOWN // p.fir.UP
        assert lens[-3:] == [lhs + 2, lhs + 1, lhs] and all(mlast < n for n in n_run[-3:])
    clips = [R.clip(rate + 7 * i, n) for i, n in enumerate(lens)]
    outs = run_api(clips, rate, mode)
    bad = [(i, len(x)) for i, (x, o) in enumerate(zip(clips, outs))
           if not R.bits_equal(o, api_reference(x, rate, mode, plan4))]
    assert not bad, (mode, rate, form, bad[:8])


@pytest.mark.parametrize("name,up,down,taps,form,w", R.THRESHOLDS, ids=[t[0] for t in R.THRESHOLDS])
def test_thresholds_through_the_c_entry(name, up, down, taps, form, w):
    """random dense filters on each side of W = 256 | 257, 512 | 513, 1024 | 1025 and of the 64 KB that move the
    filter from LDS to global memory, multi-pass, against upfirdn"""
    h = R.random_filter(taps)
    pre = R.threshold_pre_remove(taps, down)
    lens = R.ragged_lengths(up, down, R.RS_BLOCK)
    n_out = [-(-n * up // down) for n in lens]
    p = check_plan((up, down, h, pre), lens, n_out, form)
    assert p.W == w
    clips = [R.clip(taps + 3 * i, n) for i, n in enumerate(lens)]
    outs = run_c(clips, h, up, down, pre)
    bad = [(i, len(x)) for i, (x, o) in enumerate(zip(clips, outs))
           if not R.bits_equal(o, R.upfirdn_ref(x, h, up, down, pre, len(o)))]
    assert not bad, (name, bad[:8])


def test_impossible_pair_is_an_error_and_the_device_survives():
    """up 1, down 64, 1345 taps: a 17666-sample window, 70664 bytes even with the filter in global memory.  The launcher
    rejects it before any launch; the call returns an error and the next call on the device succeeds."""
    up, down, taps = R.IMPOSSIBLE
    with pytest.raises(R.Rejected):
        R.plan(taps, up, down, 0, 2, 100)
    clips = [R.clip(1, 6400), R.clip(2, 999)]
    with pytest.raises(_lib.MimiHipError) as e:
        run_c(clips, R.random_filter(taps), up, down, 0)
    assert e.value.status == 2   # MIMI_ERR_HIP: the launcher's hipErrorInvalidValue
    torch.cuda.synchronize()
    h = R.random_filter(255)
    outs = run_c(clips, h, 2, 1, 63)
    for x, o in zip(clips, outs):
        assert R.bits_equal(o, R.upfirdn_ref(x, h, 2, 1, 63, len(o)))


# one form of each kernel body: both register FIRs, prefetch with run-time and compile-time up, load-then-compute, and
# the filter in global memory
ADVERSARIAL_FORMS = (("polyphase", 16000, "fir<3,2,3>"), ("polyphase", 8000, "fir<3,1,3>"),
                     ("polyphase", 44100, "poly<2,0>"), ("polyphase", 48000, "poly<4,1>"),
                     ("polyphase", 96000, "poly<0,1>"), ("soxr_hq", 22050, "poly<2,0,HG>"))
ADV_IDS = [f"{m}-{r}" for m, r, _ in ADVERSARIAL_FORMS]


def _adversarial_batch(mode, rate, form, names):
    """256 clips: each adversarial clip (S + a pass + 9 outputs: two passes) followed by an ordinary one, then
    ordinary clips up to 3 S + 1 outputs.  Returns (clips, {index: pattern name})."""
    plan4 = R.mode_plan(mode, rate)
    up, down, hp, pre = plan4
    p1 = R.plan(len(hp), up, down, pre, R.NCLIPS, 1 << 20)
    S, P = 16 * p1.pass_outputs, p1.pass_outputs
    n_adv = R.n_in_for(S + P + 9, up, down)
    adv = R.adversarial_clips(n_adv)
    lens, which = [], {}
    for k in names:
        which[len(lens)] = k
        lens += [n_adv, R.n_in_for(S + 77, up, down)]
    lens += [R.n_in_for(3 * S + 1, up, down), 0, 1]
    rng = np.random.default_rng(5)
    lens += rng.integers(2, max(4, int(1.2 * P * down / up)), R.NCLIPS - len(lens)).tolist()
    clips = [adv[which[i]] if i in which else R.clip(rate + 11 * i, n) for i, n in enumerate(lens)]
    check_plan(plan4, lens, [R.api_lengths(n, rate)[1] for n in lens], form)
    return clips, which, plan4


@pytest.mark.parametrize("mode,rate,form", ADVERSARIAL_FORMS, ids=ADV_IDS)
def test_adversarial_finite(mode, rate, form):
    """all zeros, all -0.0, full-scale +-1 alternation and 2^-130 amplitudes (every product and sum subnormal) beside
    ordinary clips in one batch: every clip bit-equal to scipy, the subnormal one without exception"""
    clips, which, plan4 = _adversarial_batch(mode, rate, form, ("zeros", "negzeros", "alternate", "subnormal"))
    outs = run_api(clips, rate, mode)
    for i, (x, o) in enumerate(zip(clips, outs)):
        want = api_reference(x, rate, mode, plan4)
        assert R.bits_equal(o, want), (mode, rate, which.get(i, "ordinary"), i, len(x))
        if which.get(i) == "subnormal":
            assert np.any(want != 0) and np.all(np.abs(want) < np.float32(2.0 ** -120))


@pytest.mark.parametrize("mode,rate,form", ADVERSARIAL_FORMS, ids=ADV_IDS)
def test_adversarial_nonfinite(mode, rate, form):
    """one +Inf, one NaN, and a -Inf with a NaN, each in an otherwise ordinary clip beside ordinary clips: the
    non-finite positions and the class and sign of every infinity equal scipy's, every finite output is bit-equal, and
    the ordinary clips are bit-equal.  Where up does not divide the filter length this needs scipy's padded first term
    (module docstring): 8 kHz and soxr_hq 22.05 kHz here."""
    clips, which, plan4 = _adversarial_batch(mode, rate, form, R.NONFINITE)
    outs = run_api(clips, rate, mode)
    bad = []
    for i, (x, o) in enumerate(zip(clips, outs)):
        want = api_reference(x, rate, mode, plan4)
        if i in which:
            print(f"{mode} {rate} {which[i]}: non-finite outputs kernel {int((~np.isfinite(o)).sum())} / scipy "
                  f"{int((~np.isfinite(want)).sum())}, NaN kernel {int(np.isnan(o).sum())} / scipy "
                  f"{int(np.isnan(want).sum())}, finite-on-both bit-equal "
                  f"{R.same_nonfinite_and_bits(o[np.isfinite(o) & np.isfinite(want)], want[np.isfinite(o) & np.isfinite(want)])}")
            if not R.same_nonfinite_and_bits(o, want):
                bad.append((which[i], int((np.isnan(o) != np.isnan(want)).sum())))
        else:
            assert R.bits_equal(o, want), (mode, rate, "ordinary", i, len(x))
    assert not bad, (mode, rate, form, bad)
