"""TEST INFRASTRUCTURE, CPU only: a plain-numpy restatement of the ingest resampler's launcher and of the pass structure
of its kernels (tokenize-audio_amd/csrc/resample.hip), with injectable faults.

What the existing bit-exact tests cannot see is WHICH code ran: the launcher caps the grid at ceil(4096 / nclips)
workgroups per clip and every workgroup then sweeps its clip in passes of 256 outputs (768 for the register-FIR kernels),
handing the window state (q0, r0, w0), a register prefetch and a double-buffered LDS window from pass to pass.  A small
batch of short clips runs one pass per workgroup and never executes any of that.  This module restates

* ``plan``: the form the launcher picks -- ``fir<3,2,3>``, ``fir<3,1,3>`` or ``poly<WPT, UPC, HG>`` -- with the window W,
  the LDS bytes and the grid, from (lh, up, down, pre_remove, nclips, max_out); ``Rejected`` where the launcher returns an
  error before any launch;
* ``emulate``: every pass of every workgroup, THROUGH explicit window buffers that start as NaN, so a stale window, a
  buffer toggled wrongly or a sample never staged shows in the values; float32 products and sums rounded one by one in
  ascending input index, as the kernel (and scipy's upfirdn) adds them;
* ``passes``: how many passes a workgroup makes over a clip.

``emulate`` vectorises over the workgroups of a clip (axis 0) and the threads of a workgroup (axis 1); the pass loop and
the tap loop are the kernel's own.  It records index-invariant violations in ``stats`` instead of raising.

FAULTS (``fault=``), each a one-line change to the kernel text:
  stale_pass    (a) load-then-compute (WPT 0) never advances q0 / r0 / w0 past the first pass
  no_toggle     (b) the prefetched window is stored into the buffer just read (xn from pass & 1).  Emulated in program
                    order (the store after the pass's reads); on a device nothing orders that store against the reads of
                    the workgroup's other waves, so it also races WITHIN a pass (``stats["race"]``): values then depend on
                    the schedule even in a single pass
  prefetch_w0   (c) the prefetch reads from w0 (this pass's window start), not wn
  short_window  (d) the staged window is one sample short of what a pass can touch
  trunc_ceil    (e) ceil(n / up) written as (n + up - 1) / up under C's truncating division: wrong for n <= -up
  fir_interior  (f) the register-FIR ``interior`` test admits floor(p(mlast) / up) == n_in: one sample past the clip

The kernels run scipy's terms, padding included: upfirdn pads every filter phase with zeros to ceil(lh / up) taps, so with
lhp = ceil(lh / up) up an output's first term may carry a padding tap (index in [lh, lhp)): x[j] * 0, +0 for a finite
sample and NaN for Inf / NaN.  jlo, w0 and the register FIR's constants are therefore derived from lhp.

On (d): a pass reads window offsets up to ceil(255 down / up) + lhp / up - 1 <= W - 1 with W = (255 down + lh - 1) / up + 2;
where up divides lh the bound is W - 2 and W carries one spare sample.  "One short" is counted from what a pass can
touch: the fault stages W - 1 samples where lh != 0 (mod up), W - 2 where up divides lh (tests/test_resample_pass_ref.py
asserts the bound, and that the fault is seen exactly where a pass reads the first unstaged offset).  The register-FIR
window is exact, there the fault stages W - 1.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

RS_BLOCK = 256
GRID_TARGET = 4096          # workgroups in all: the cap per clip is ceil(4096 / nclips)
LDS_LIMIT = 64 * 1024       # default dynamic-LDS limit
FAULTS = ("stale_pass", "no_toggle", "prefetch_w0", "short_window", "trunc_ceil", "fir_interior")
POISON = np.float32(np.nan)  # never-written LDS and never-written outputs


class Rejected(ValueError):
    """The launcher returns hipErrorInvalidValue before any launch (window does not fit in LDS)."""


def _tdiv(a, b):
    """C integer division (truncates toward zero), b > 0; Python int or int64 array."""
    if isinstance(a, (int, np.integer)):
        a = int(a)
        return a // b if a >= 0 else -((-a) // b)
    return np.where(a >= 0, a // b, -((-a) // b))


class FirForm:
    """RsFir<UP, DOWN, R> of resample.hip: every constant of the register FIR."""

    def __init__(self, up, down, r):
        self.UP, self.DOWN, self.R = up, down, r
        self.MR = max(up, down)
        self.HALF = 10 * self.MR
        self.PREPAD = down - self.HALF % down
        self.LH = 2 * self.HALF + 1 + self.PREPAD
        self.LHP = -(-self.LH // up) * up                # with scipy's zero padding of every phase
        self.PRE = (self.HALF + self.PREPAD) // down
        self.C0 = (self.PRE * down) % up
        self.NT = max(self.cnt(0), self.cnt(up - 1))
        self.NX = self.off(r - 1) + self.cnt(r - 1)
        self.TSTEP = r // up * down
        self.W = self.TSTEP * (RS_BLOCK - 1) + self.NX
        self.PASS = RS_BLOCK * r
        assert r % up == 0

    def jlo(self, r):
        return -((-(self.C0 + r * self.DOWN - (self.LHP - 1))) // self.UP)  # ceil

    def jhi(self, r):
        return (self.C0 + r * self.DOWN) // self.UP                        # floor

    def off(self, r):
        return self.jlo(r) - self.jlo(0)

    def cnt(self, r):
        return self.jhi(r) - self.jlo(r) + 1

    def kfirst(self, r):
        return self.C0 + r * self.DOWN - self.UP * self.jlo(r)


FIR_FORMS = (FirForm(3, 2, 3), FirForm(3, 1, 3))   # RS_FIR(3, 2, 3), RS_FIR(3, 1, 3): in the launcher's order


@dataclass(frozen=True)
class Plan:
    name: str                  # "fir<3,2,3>" | "poly<WPT,UPC>" | "poly<WPT,0,HG>"
    kind: str                  # "fir" | "poly"
    lh: int
    up: int
    down: int
    pre: int
    W: int
    wpt: int                   # poly: 1 / 2 / 4 prefetch registers per thread, 0 = load-then-compute
    upc: int                   # poly: compile-time up (0: run time)
    hg: bool                   # poly: filter read from global memory
    lds_bytes: int
    grid: int                  # workgroups per clip (gridDim.x)
    pass_outputs: int          # outputs per workgroup pass
    fir: Optional[FirForm] = None

    @property
    def sweep(self):
        """outputs of one pass of the whole grid"""
        return self.grid * self.pass_outputs


def resample_window(lh, up, down):
    return ((RS_BLOCK - 1) * down + lh - 1) // up + 2


def plan(lh, up, down, pre_remove, nclips, max_out) -> Optional[Plan]:
    """launch_resample_poly, restated.  None: nothing to launch."""
    if nclips <= 0 or max_out <= 0:
        return None
    cap = (GRID_TARGET + nclips - 1) // nclips
    for f in FIR_FORMS:
        if up == f.UP and down == f.DOWN and lh == f.LH and pre_remove == f.PRE:
            b = min((max_out + f.PASS - 1) // f.PASS, cap)
            return Plan(f"fir<{f.UP},{f.DOWN},{f.R}>", "fir", lh, up, down, pre_remove, f.W, 0, up, False,
                        (f.LH + f.W) * 4, b, f.PASS, f)
    W = resample_window(lh, up, down)
    wpt = 1 if W <= RS_BLOCK else 2 if W <= 2 * RS_BLOCK else 4 if W <= 4 * RS_BLOCK else 0
    lds = (lh + (2 if wpt > 0 else 1) * W) * 4
    hg = lds > LDS_LIMIT
    if hg:
        lds -= lh * 4
    if lds > LDS_LIMIT:
        raise Rejected(f"window of {W} samples: {lds} bytes of LDS")
    bx = min((max_out + RS_BLOCK - 1) // RS_BLOCK, cap)
    upc = 0 if hg else up if up in (1, 3) else 0
    name = f"poly<{wpt},0,HG>" if hg else f"poly<{wpt},{upc}>"
    return Plan(name, "poly", lh, up, down, pre_remove, W, wpt, upc, hg, lds, bx, RS_BLOCK)


def passes(p: Plan, n_out: int, wg: int = 0) -> int:
    """passes workgroup ``wg`` makes over a clip of n_out outputs (0: it exits at once)"""
    left = n_out - wg * p.pass_outputs
    return 0 if left <= 0 else -(-left // p.sweep)


# ------------------------------------------------------------------------------------------------ emulation

def _new_stats():
    return {"violations": [], "max_window_read": -1, "max_k_first": -1, "min_k_last": 1 << 62, "max_pr": -1,
            "passes": 0, "exited": 0, "interior": 0, "edge": 0, "interior_late": 0, "race": False}


def _bad(stats, what):
    if len(stats["violations"]) < 16:
        stats["violations"].append(what)


def _ceil_div(n, up, kc, fault):
    """the kernel's ceil(n / up) for n that may be negative: (n + kc up + up - 1) / up - kc with kc up >= lh - 1"""
    if fault == "trunc_ceil":
        return _tdiv(n + up - 1, up)
    return _tdiv(n + kc * up + up - 1, up) - kc


def padded_len(lh, up):
    """lhp: the filter length with scipy's zero padding of every phase to ceil(lh / up) taps"""
    return -(-lh // up) * up


def _pass_w0(m0, p, kc, fault):
    p0 = (m0 + p.pre) * p.down
    q0 = p0 // p.up
    r0 = p0 - q0 * p.up
    return np.maximum(q0 + _ceil_div(r0 - (padded_len(p.lh, p.up) - 1), p.up, kc, fault), 0), q0, r0


def _gload(xbuf, off, n_in, j):
    """x[j] of the clip behind the kernel's guard (j < n_in ? xc[j] : 0); j >= 0"""
    ok = j < n_in
    return np.where(ok, xbuf[np.where(ok, off + j, 0)], np.float32(0))


def _poly_clip(p, xbuf, off, n_in, n_out, h, fault, stats, values, wgs):
    lh, up, down, W, wpt = p.lh, p.up, p.down, p.W, p.wpt
    nbuf = 2 if wpt else 1
    g = np.arange(p.grid, dtype=np.int64) if wgs is None else np.asarray(wgs, np.int64)
    m0 = g * RS_BLOCK
    stats["exited"] += int((m0 >= n_out).sum())          # if (m0 >= n_out) return;
    m0 = m0[m0 < n_out]
    y = np.full(n_out, POISON, np.float32)
    G = len(m0)
    if G == 0:
        return y
    lhp = padded_len(lh, up)
    kc = (lhp - 1 + up - 1) // up
    mstep = p.grid * RS_BLOCK
    tid = np.arange(RS_BLOCK, dtype=np.int64)[None, :]
    rows = np.arange(G)[:, None]
    w0, q0, r0 = _pass_w0(m0, p, kc, fault)
    Wst = (W - 1 if lh % up else W - 2) if fault == "short_window" else W       # samples staged
    lds = np.full((G, nbuf * W), POISON, np.float32)     # the window buffer(s), after the filter's lh floats
    lds_len = nbuf * W
    iw = np.arange(max(wpt, 1) * RS_BLOCK, dtype=np.int64)[None, :]
    if wpt:
        assert W <= wpt * RS_BLOCK
        lds[:, :Wst] = _gload(xbuf, off, n_in, w0[:, None] + iw)[:, :Wst]
    alive = np.ones(G, bool)
    pass_ = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        while alive.any():
            base = (pass_ & 1) * W if wpt else 0
            mn = m0 + mstep
            if wpt:
                nxt = alive & (mn < n_out)
                wn, qn, rn = _pass_w0(np.where(nxt, mn, 0), p, kc, fault)
                wn, qn, rn = np.where(nxt, wn, 0), np.where(nxt, qn, 0), np.where(nxt, rn, 0)
                j = (w0 if fault == "prefetch_w0" else wn)[:, None] + iw
                pf = np.where(nxt[:, None] & (iw < W), _gload(xbuf, off, n_in, j), np.float32(0))
            else:
                if fault != "stale_pass":
                    a, b, c = _pass_w0(m0, p, kc, fault)
                    w0, q0, r0 = np.where(alive, a, w0), np.where(alive, b, q0), np.where(alive, c, r0)
                stage = _gload(xbuf, off, n_in, w0[:, None] + np.arange(Wst, dtype=np.int64)[None, :])
                lds[alive, :Wst] = stage[alive]
            m = m0[:, None] + tid
            act = alive[:, None] & (m < n_out)
            pr = r0[:, None] + tid * down
            jhi = np.minimum(q0[:, None] + pr // up, n_in - 1)
            jlo = np.maximum(q0[:, None] + _ceil_div(pr - (lhp - 1), up, kc, fault), 0)
            k = pr - (jlo - q0[:, None]) * up
            xo = jlo - w0[:, None]
            cnt = jhi - jlo + 1
            use = act & (cnt > 0)
            if use.any():
                hi, klast = (xo + cnt - 1)[use], (k - (cnt - 1) * up)[use]
                stats["max_window_read"] = max(stats["max_window_read"], int(hi.max()))
                stats["max_k_first"] = max(stats["max_k_first"], int(k[use].max()))
                stats["min_k_last"] = min(stats["min_k_last"], int(klast.min()))
                stats["max_pr"] = max(stats["max_pr"], int(pr[act].max()))
                if int(xo[use].min()) < 0 or int(hi.max()) >= W:
                    _bad(stats, f"pass {pass_}: window read outside [0, {W}): {int(xo[use].min())}..{int(hi.max())}")
                second = (k - up)[use & (cnt > 1)]   # only a first term may be a padding tap (index in [lh, lhp))
                if int(k[use].max()) >= lhp or int(klast.min()) < 0 or (len(second) and int(second.max()) >= lh):
                    _bad(stats, f"pass {pass_}: filter index outside [0, {lh}): {int(klast.min())}..{int(k[use].max())}")
                if int(pr[act].max()) >= 1 << 31:
                    _bad(stats, f"pass {pass_}: pr = {int(pr[act].max())} does not fit 32 bits")
            if values:
                acc = np.zeros((G, RS_BLOCK), np.float32)
                for t in range(int(cnt[use].max()) if use.any() else 0):
                    sel = use & (t < cnt)
                    xi = base + xo + t
                    xin = (xi >= 0) & (xi < lds_len)
                    xv = np.where(xin, lds[rows, np.where(xin, xi, 0)], POISON)
                    kk = k - t * up
                    kin = (kk >= 0) & (kk < lh)
                    hv = np.where(kin, h[np.where(kin, kk, 0)], POISON)
                    if t == 0:   # k >= lh: scipy's padding tap, the constant 0 (never read from the filter)
                        hv = np.where(kk >= lh, np.float32(0), hv)
                    elif not p.hg:  # hs = lds: an index past the filter lands in the window buffers behind it
                        over = (kk >= lh) & (kk - lh < lds_len)
                        hv = np.where(over, lds[rows, np.where(over, kk - lh, 0)], hv)
                    acc = np.where(sel, acc + xv * hv, acc)
                y[m[act]] = acc[act]
            elif values:
                y[m[act]] = np.float32(0)
            if wpt:
                nb = ((pass_ if fault == "no_toggle" else pass_ + 1) & 1) * W
                if nb == base:   # stored into the buffer other waves may still be reading: no barrier in between
                    stats["race"] = True
                lds[alive, nb:nb + Wst] = pf[alive, :Wst]
                q0, r0, w0 = np.where(alive, qn, q0), np.where(alive, rn, r0), np.where(alive, wn, w0)
            pass_ += 1
            m0 = m0 + mstep
            alive = alive & (m0 < n_out)
    stats["passes"] = max(stats["passes"], pass_)
    return y


def _fir_clip(p, xbuf, off, n_in, n_out, h, fault, stats, values, wgs):
    F = p.fir
    UP, DOWN, R, LH, PRE, W, NT = F.UP, F.DOWN, F.R, F.LH, F.PRE, F.W, F.NT
    g = np.arange(p.grid, dtype=np.int64) if wgs is None else np.asarray(wgs, np.int64)
    m0 = g * F.PASS
    stats["exited"] += int((m0 >= n_out).sum())
    m0 = m0[m0 < n_out]
    y = np.full(n_out, POISON, np.float32)
    if len(m0) == 0:
        return y
    hs = np.asarray(h[:LH], np.float32)
    hr = np.zeros((UP, NT), np.float32)
    for r in range(UP):
        for i in range(F.cnt(r)):
            if F.kfirst(r) - i * UP < LH:               # (else a padding tap: zero)
                hr[r, i] = h[F.kfirst(r) - i * UP]
    kc = (F.LHP - 1 + UP - 1) // UP
    step = p.grid * F.PASS
    tid = np.arange(RS_BLOCK, dtype=np.int64)[None, :]
    Wst = W - 1 if fault == "short_window" else W
    pass_ = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        while len(m0):
            p0 = (m0 + PRE) * DOWN
            assert not ((p0 - F.C0) % UP).any()
            q0 = (p0 - F.C0) // UP
            w0 = q0 + F.jlo(0)
            mlast = m0 + F.PASS - 1
            edge = n_in if fault == "fir_interior" else n_in - 1
            interior = (w0 >= 0) & (mlast < n_out) & ((mlast + PRE) * DOWN // UP <= edge)
            stats["interior"] += int(interior.sum())
            stats["edge"] += int((~interior).sum())
            if pass_ > 0:
                stats["interior_late"] += int(interior.sum())
            if interior.any():
                mi, wi = m0[interior], w0[interior]
                Gi = len(mi)
                xs = np.full((Gi, W), POISON, np.float32)        # LDS window, staged unguarded
                j = wi[:, None] + np.arange(Wst, dtype=np.int64)[None, :]
                if int(j.max()) >= n_in:
                    _bad(stats, f"pass {pass_}: interior window reads x[{int(j.max())}] of a {n_in}-sample clip")
                inb = off + j < len(xbuf)
                if not inb.all():
                    _bad(stats, f"pass {pass_}: interior window reads past the packed buffer")
                xs[:, :Wst] = np.where(inb, xbuf[np.where(inb, off + j, 0)], POISON)
                if values:
                    rows = np.arange(Gi)[:, None]
                    mt = mi[:, None] + tid * R
                    for r in range(R):
                        acc = np.zeros((Gi, RS_BLOCK), np.float32)
                        for i in range(F.cnt(r % UP)):
                            acc = acc + xs[rows, tid * F.TSTEP + F.off(r) + i] * hr[r % UP, i]
                        y[(mt + r).ravel()] = acc.ravel()
            if (~interior).any() and values:
                me = m0[~interior]
                m = (me[:, None] + np.arange(F.PASS, dtype=np.int64)[None, :]).ravel()
                m = m[m < n_out]
                pp = (m + PRE) * DOWN
                jhi = np.minimum(pp // UP, n_in - 1)
                jlo = np.maximum(_ceil_div(pp - (F.LHP - 1), UP, kc, fault), 0)
                cnt = jhi - jlo + 1
                acc = np.zeros(len(m), np.float32)
                for t in range(int(cnt.max()) if len(m) else 0):
                    sel = t < cnt
                    jj = np.where(sel, jlo + t, 0)
                    kk = np.where(sel, pp - jj * UP, 0)
                    if int(kk.max()) >= F.LHP or int(kk.min()) < 0:
                        _bad(stats, f"pass {pass_}: edge filter index outside [0, {F.LHP})")
                    tap = np.where(kk < LH, hs[np.clip(kk, 0, LH - 1)], np.float32(0))   # >= LH: a padding tap
                    acc = np.where(sel, acc + xbuf[off + jj] * tap, acc)
                y[m] = acc
            pass_ += 1
            m0 = m0 + step
            m0 = m0[m0 < n_out]
    stats["passes"] = max(stats["passes"], pass_)
    return y


def emulate(clips, h, up, down, pre_remove, n_outs=None, nclips=None, fault=None, tail=8, values=True, only=None,
            wgs=None):
    """The launch, emulated: ``clips`` packed back to back with ``tail`` NaN samples behind them, clip c producing
    ``n_outs[c]`` outputs (default resample_poly's ceil(n up / down)).  ``nclips`` overrides the clip count the grid is
    sized by (default len(clips)); ``only`` restricts the emulation to some clips (the others come back as None) and
    ``wgs`` to some workgroups (outputs of the others stay NaN).  Returns (outputs, stats, plan)."""
    assert fault is None or fault in FAULTS
    h = np.asarray(h, np.float32)
    clips = [np.asarray(c, np.float32) for c in clips]
    n_in = [len(c) for c in clips]
    if n_outs is None:
        n_outs = [-(-n * up // down) for n in n_in]
    xbuf = np.concatenate(clips + [np.full(tail, POISON, np.float32)])
    offs = np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int64)
    stats = _new_stats()
    p = plan(len(h), up, down, pre_remove, len(clips) if nclips is None else nclips, max(n_outs, default=0))
    outs = []
    for c in range(len(clips)):
        if only is not None and c not in only:
            outs.append(None)
        elif p is None:
            outs.append(np.full(n_outs[c], POISON, np.float32))
        else:
            f = _fir_clip if p.kind == "fir" else _poly_clip
            outs.append(f(p, xbuf, int(offs[c]), n_in[c], n_outs[c], h, fault, stats, values, wgs))
    return outs, stats, p


# ------------------------------------------------------------------------------------------------ references, shapes

def bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def upfirdn_ref(x, h, up, down, pre_remove, n_out):
    """scipy.signal.upfirdn over the padded filter, trimmed as resample_poly trims (zeros past its end)."""
    from scipy.signal import upfirdn
    out = np.zeros(n_out, np.float32)
    if len(x):
        seg = upfirdn(np.asarray(h, np.float32), np.asarray(x, np.float32), up, down)[pre_remove:pre_remove + n_out]
        out[:len(seg)] = seg
    return out


def mode_plan(mode, rate, target=24000):
    """(up, down, padded filter, pre_remove) of a source rate in ``polyphase`` or ``soxr_hq`` mode"""
    from mimi_hip import ingest
    return (ingest.resample_plan if mode == "polyphase" else ingest.soxr_hq_plan)(rate, target)


def api_lengths(n_in, rate, target=24000):
    """(n_fix, n_run) of ingest.resample_packed: the returned length (librosa's fix_length) and the outputs the kernel
    computes (the rest is a zero tail)"""
    g = math.gcd(rate, target)
    up, down = target // g, rate // g
    n_fix = int(math.ceil(n_in * (float(target) / rate)))
    return n_fix, min(n_fix, -(-n_in * up // down))


# every source rate -> 24 kHz the resampler supports, both modes
RATES = (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 72000, 88200, 96000, 176400, 192000)

# the forms tests/test_resample_kernels.py runs through the Python API: (mode, source rate, form)
FORM_TABLE = (
    ("polyphase", 16000, "fir<3,2,3>"),
    ("polyphase", 8000, "fir<3,1,3>"),
    ("polyphase", 22050, "poly<1,0>"),
    ("polyphase", 12000, "poly<1,0>"),
    ("polyphase", 32000, "poly<2,3>"),
    ("polyphase", 44100, "poly<2,0>"),
    ("polyphase", 48000, "poly<4,1>"),
    ("polyphase", 88200, "poly<4,0>"),
    ("polyphase", 96000, "poly<0,1>"),
    ("polyphase", 176400, "poly<0,0>"),
    ("polyphase", 192000, "poly<0,1>"),
    ("soxr_hq", 16000, "poly<2,3>"),
    ("soxr_hq", 48000, "poly<4,1>"),
    ("soxr_hq", 22050, "poly<2,0,HG>"),
    ("soxr_hq", 44100, "poly<4,0,HG>"),
    ("soxr_hq", 72000, "poly<0,1>"),
    ("soxr_hq", 88200, "poly<0,0,HG>"),
)

NCLIPS = 256                # the multi-pass batches: a cap of ceil(4096 / 256) = 16 workgroups per clip


def n_in_for(n_out, up, down):
    """the shortest clip with at least n_out outputs (exactly n_out whenever some length gives n_out)"""
    return 0 if n_out <= 0 else (n_out - 1) * down // up + 1


def ragged_lengths(up, down, pass_outputs, fir: Optional[FirForm] = None, nclips=NCLIPS, seed=0):
    """Input lengths of one multi-pass batch of ``nclips`` clips.  With S = 16 pass_outputs (one sweep of the capped
    grid), the output lengths aimed at are: 0 and 1 sample in; shorter than a pass; a pass -1 / +0 / +1; S and 2 S, each
    -1 / +0 / +1 (an exact multiple of a sweep and its neighbours); 3 S; 3 S + 1 (four passes, the last holding one
    output).
    Each is the shortest clip with at least that many outputs: where up > down skips a length, the next one above it.
    Workgroups 1..15 of every clip under 15 passes exit at once.  The rest are ordinary short clips.  For a register-FIR
    form the last three clips put floor(p(mlast) / up) of workgroup 0's pass 1 at n_in - 2, n_in - 1 (interior, at
    equality) and n_in (not interior), the last one directly in front of whatever follows the packed clips."""
    S = (GRID_TARGET + nclips - 1) // nclips * pass_outputs
    P = pass_outputs
    outs = [40, P - 1, P, P + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 1]
    lens = [0, 1] + [n_in_for(t, up, down) for t in outs]
    edge = []
    if fir is not None:
        lhs = (S + P - 1 + fir.PRE) * fir.DOWN // fir.UP
        edge = [lhs + 2, lhs + 1, lhs]
    rng = np.random.default_rng(seed)
    top = max(4, int(1.2 * P * down / up))
    fill = rng.integers(2, top, nclips - len(lens) - len(edge)).tolist()
    return lens + fill + edge


def clip(seed, n):
    return np.random.default_rng(seed).normal(0.0, 0.3, n).astype(np.float32)


# the shapes of the GPU tests in tests/test_resample.py (and of smoke()): (mode, source rate, input lengths of one launch)
TODAY_SHAPES = (
    [("polyphase", r, (1, 2, 3, 37, 1001, 16001)) for r in (16000, 8000, 22050, 44100, 48000)]   # kernel_bit_exact
    + [("polyphase", 16000, (16000 * 60, 0, 7)),                                                  # full_size_vs_scipy
       ("polyphase", 16000, (16000,)),                                                            # load_then_encode
       ("polyphase", 16000, (8000, 333))]                                                         # smoke()
    + [("polyphase", r, (r * 3 + 17, 5, r // 3)) for r in (8000, 48000, 72000, 96000, 22050)]     # window_variants
    + [("soxr_hq", r, (1, 37, 1001, 3 * r + 17)) for r in (16000, 48000, 44100, 22050)]           # soxr_hq_kernel
)


# "any other FIR" through the C entry: random filters on each side of every threshold of the launcher.
# (case, up, down, taps, form, W): W = (255 down + taps - 1) / up + 2; LDS floats = taps + (2 or 1) W against 16384
THRESHOLDS = (
    ("W256", 2, 1, 255, "poly<1,0>", 256),
    ("W257", 2, 1, 256, "poly<2,0>", 257),
    ("W512", 3, 2, 1023, "poly<2,3>", 512),
    ("W513", 3, 2, 1024, "poly<4,3>", 513),
    ("W1024", 1, 2, 513, "poly<4,1>", 1024),
    ("W1025", 1, 2, 514, "poly<0,1>", 1025),
    ("lds64k_wpt0", 4, 3, 12953, "poly<0,0>", 3431),          # 12953 + 3431 = 16384 floats: the filter still in LDS
    ("lds64k_wpt0_hg", 4, 3, 12954, "poly<0,0,HG>", 3431),
    ("lds64k_wpt4", 16, 1, 14532, "poly<4,0>", 926),          # 14532 + 2 x 926 = 16384
    ("lds64k_wpt4_hg", 16, 1, 14533, "poly<4,0,HG>", 926),
)
IMPOSSIBLE = (1, 64, 1345)   # (up, down, taps): W = 17666 samples = 70664 bytes even with the filter in global memory


def random_filter(taps, seed=0):
    """a dense random FIR with no zero taps (every term of every output counts)"""
    rng = np.random.default_rng(1000 + seed)
    h = rng.normal(0.0, 1.0, taps).astype(np.float32) / np.float32(math.sqrt(taps))
    h[h == 0] = np.float32(1e-3)
    return h


def threshold_pre_remove(taps, down):
    return (taps // 2) // down   # as a centred filter would be aligned


def adversarial_clips(n, seed=0):
    """{name: n samples}: the sample patterns run beside ordinary clips.  2^-130 is below the smallest normal float32
    (2^-126): inputs, products and sums are all subnormal."""
    rng = np.random.default_rng(77 + seed)
    alt = np.where(np.arange(n) % 2 == 0, np.float32(1), np.float32(-1)).astype(np.float32)
    tiny = (np.ldexp(np.float32(1), -130) * rng.integers(-12, 13, n)).astype(np.float32)
    inf = clip(seed + 501, n)
    nan = clip(seed + 502, n)
    both = clip(seed + 503, n)
    if n:
        inf[n // 3] = np.inf
        nan[(2 * n) // 3] = np.nan
        both[n // 4] = -np.inf
        both[n // 2] = np.nan
    return {"zeros": np.zeros(n, np.float32), "negzeros": np.full(n, -0.0, np.float32), "alternate": alt,
            "subnormal": tiny, "inf": inf, "nan": nan, "inf_nan": both}


NONFINITE = ("inf", "nan", "inf_nan")


def same_nonfinite_and_bits(a, b):
    """the one relaxation: non-finite positions, and class and sign of each infinity, equal; every finite output
    bit-equal; NaN payloads not compared"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))
