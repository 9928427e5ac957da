"""Test infrastructure only (CPU): the float64 audit of the RVQ (proj -> codes), the crafted quantizers and the
adversarial residual cases behind tests/test_rvq_ref.py (CPU: checks this checker) and tests/test_rvq_kernels.py (GPU).

THE AUDIT, per level L and frame.  r_L is formed in numpy fp32 from the quantizer's own input (the ``proj`` tap) and the
audited chain's own earlier codes: r_0 = proj[:, :256] (semantic), r_1 = proj[:, 256:] (first acoustic),
r_{L+1} = r_L - embed_L[code_L] elementwise in fp32, embed = embed_sum / max(cluster_usage, eps) in fp32 -- both are
single IEEE operations per element, so bit-reproducible on any machine.  d2(c) = |r_L - e_c|^2 is evaluated for all
2048 codes in float64, and

    q = (d2(chosen) - min_c d2(c)) / (2^-24 (|r| + |e_chosen|)^2)

n, THE OPERATION COUNT (derived, not fitted).  The engine (ops.hip rvq_exact) and the reference both evaluate
d = sqrt(max((a + |r|^2) + |e|^2, 0)) with a = -2 r.e.  In units of u = 2^-24:
  * a is a chain of 256 fmas, one rounding each, every partial sum bounded by sum |2 r_k e_k| <= 2 |r||e|: 256 units of
    the 2|r||e| part of (|r| + |e|)^2 = |r|^2 + 2|r||e| + |e|^2;
  * |r|^2 and |e|^2 are sums of 256 squares in torch's order (8 lanes x 4 accumulators x 8 blocks): an element passes
    1 (square) + 8 (its accumulator) + 3 (the 4 accumulators) + 7 (the 8 lanes) = 19 roundings, each on a partial sum
    of at most the whole: 19 units of the |r|^2 and of the |e|^2 part, counted once on top of the chain's 256 (which
    already covers every part's share);
  * the two final adds round once each on at most (|r| + |e|)^2: 2 units;
  * the comparison is on d = sqrt(d2): one rounding, relative u on d, i.e. 2 u on d2: 2 units.
n = 256 + 19 + 2 + 2 = 279.  Both compared distances (the chosen code's and the true minimum's) carry this error, so
the HARD condition is q <= 2 n = 558.  The WORKING condition is q <= 16 max(q_oracle, 1) (the stage tests' rule),
q_oracle the same quantity for oracle.mimi_ref.rvq_from_embedding (torch CPU fp32) on the same input.

EXACT RULES (no tolerance): every code in [0, 2048); a chosen row that is bitwise equal to other rows of its level has
the lowest index of them; where the float64 margin between the best and the second-best code exceeds the hard bound
(taken with the level's largest |e|), the code is determinate and is the float64 argmin.

CRAFTED MODELS.  synthetic.make_state_dict(seed=0) with only the quantizer keys replaced: input_proj.weight becomes a
selection matrix (semantic [I_256 | 0], acoustic [0 | I_256]: products by 1 and 0 and sums with zeros round nothing, so
proj IS the two halves of the embedding), and levels 0 (semantic) and 1 (first acoustic) -- the two levels whose
residual a test controls directly -- get crafted codebooks as rows with cluster_usage = 1 (embed_sum / 1 = the rows).
Deeper levels keep the synthetic codebooks.
  model "pairs":  level 0 ``pairs_codebook`` (Gaussian directions, bitwise duplicate pairs, one coherent pair), level 1
                  ``scales_codebook`` (norms 2^0 .. 2^-24 of the largest, and copies of stock level-2 rows)
  model "degen":  level 0 ``flat_codebook`` (2048 equal rows), level 1 ``coherent_codebook`` (the window's worst case:
                  one coherent pair; and two groups of bitwise-equal rows)

POSITION CLASSES of a pair of special rows (i, j): "wave" (i, i + 1: one 32-code wave), "slice" (i, i + 40: two waves
of one 256-code slice), "half" (i, i + 300: two 256-slices of one 512-slice), "far" (i, i + 1500: two 512-slices).

``emulate`` is a CPU emulation of the kernels' one-product selection (the fp16 hi planes of r rs and e cs, the window
formula of rvq_level_h16_kernel<.., P1 = true> / rvq_chain_h16_kernel) followed by an fp32 re-score; it reports the
candidate count per (32-frame tile, slice) -- the class that decides which exact path a workgroup takes -- and each
frame's window position, and takes the injected faults of tests/test_rvq_ref.py.  It need not (and does not) match
the MFMA bit for bit.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from mimi_hip import synthetic
from oracle import mimi_ref
from oracle.mimi_ref import RefConfig

CFG = RefConfig()
D, NCODES, HID = 256, 2048, 512
U = 2.0 ** -24
N_RVQ = 256 + 19 + 2 + 2
HARD = 2 * N_RVQ
WORKING_FACTOR = 16.0
RVQ_CAND, RVQC_NSTG = 2048, 64      # ops.hip: the candidate list's capacity; the chain's staged re-score limit
POS = {"wave": 1, "slice": 40, "half": 300, "far": 1500}
SEM = "quantizer.semantic_residual_vector_quantizer."
ACO = "quantizer.acoustic_residual_vector_quantizer."


def cb_prefix(level: int) -> str:
    n = CFG.num_semantic_quantizers
    return f"{SEM}layers.{level}.codebook." if level < n else f"{ACO}layers.{level - n}.codebook."


def embeds(sd, K: int) -> np.ndarray:
    """embed = embed_sum / max(cluster_usage, eps) in fp32 for levels 0 .. K-1: [K, 2048, 256]."""
    out = []
    for l in range(K):
        es = np.asarray(sd[cb_prefix(l) + "embed_sum"], dtype=np.float32)
        us = np.asarray(sd[cb_prefix(l) + "cluster_usage"], dtype=np.float32)
        out.append(es / np.maximum(us, np.float32(CFG.codebook_eps))[:, None])
    return np.stack(out)


def first_equal(rows: np.ndarray) -> np.ndarray:
    """first[c] = the lowest index whose row is bitwise equal to row c."""
    _, inv = np.unique(np.ascontiguousarray(rows).view(np.uint32), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    lowest = np.full(inv.max() + 1, len(rows), dtype=np.int64)
    np.minimum.at(lowest, inv, np.arange(len(rows)))
    return lowest[inv]


def start_residual(proj: np.ndarray, level: int) -> np.ndarray:
    return np.ascontiguousarray(proj[:, :D] if level < CFG.num_semantic_quantizers else proj[:, D:2 * D])


def audit(proj, codes, emb) -> dict:
    """proj [F, 512] fp32 (the quantizer's input), codes [K, F], emb [K, 2048, 256] fp32 -> the worst q with where it
    fell, and the violations of the exact rules (``bad``: a list of strings, empty when every rule holds)."""
    proj = np.ascontiguousarray(np.asarray(proj, dtype=np.float32).reshape(-1, 2 * D))
    codes = np.asarray(codes).astype(np.int64)
    K, F = codes.shape
    nsem = CFG.num_semantic_quantizers
    rec = {"q": 0.0, "worst": None, "determinate": 0, "bad": []}
    if codes.min() < 0 or codes.max() >= NCODES:
        rec["bad"].append(f"code outside [0, {NCODES}): min {codes.min()}, max {codes.max()}")
        rec["q"] = float("inf")
        return rec
    r = None
    fr = np.arange(F)
    for L in range(K):
        e = emb[L]
        if L == 0 or L == nsem:
            r = start_residual(proj, L)
        c = codes[L]
        r64, e64 = r.astype(np.float64), e.astype(np.float64)
        rn, en = (r64 * r64).sum(1), (e64 * e64).sum(1)
        d2 = (rn[:, None] - 2.0 * (r64 @ e64.T)) + en[None, :]
        dmin, amin = d2.min(1), d2.argmin(1)
        dch = d2[fr, c]
        unit = U * (np.sqrt(rn) + np.sqrt(en[c])) ** 2
        q = np.where(dch > dmin, (dch - dmin) / np.maximum(unit, 1e-300), 0.0)
        w = int(q.argmax())
        if q[w] > rec["q"] or rec["worst"] is None:
            rec["q"] = float(max(q[w], rec["q"]))
            rec["worst"] = {"level": L, "frame": w, "chosen": int(c[w]), "argmin64": int(amin[w]),
                            "d2_chosen": float(dch[w]), "d2_min": float(dmin[w]), "unit": float(unit[w])}
        # determinate frames: the runner-up (of the rows that differ from the best one) is beyond the hard bound
        first = first_equal(e)
        part = np.partition(np.where(first[None, :] == first[amin][:, None], np.inf, d2), 0, axis=1)[:, 0]
        det = (part - dmin) > HARD * U * (np.sqrt(rn) + np.sqrt(en.max())) ** 2
        rec["determinate"] += int(det.sum())
        wrong = det & (first[c] != first[amin])
        for f in np.flatnonzero(wrong)[:4]:
            rec["bad"].append(f"level {L} frame {f}: determinate code {first[amin][f]}, got {c[f]} "
                              f"(d2 {dch[f]:.9g} vs {dmin[f]:.9g})")
        tie = first[c] != c
        for f in np.flatnonzero(tie)[:4]:
            rec["bad"].append(f"level {L} frame {f}: code {c[f]} chosen, its bitwise-equal row {first[c][f]} is lower")
        if L >= nsem or L + 1 < nsem:
            r = r - e[c]          # fp32, elementwise
    return rec


def conditions(q: float, q_oracle: float) -> List[str]:
    out = []
    if not q <= HARD:
        out.append(f"HARD q = {q:.4g} > 2 n = {HARD}")
    if not q <= WORKING_FACTOR * max(q_oracle, 1.0):
        out.append(f"WORKING q = {q:.4g} > {WORKING_FACTOR:g} max(q_oracle = {q_oracle:.4g}, 1)")
    return out


def oracle_codes(emb, sd, K: int) -> np.ndarray:
    """oracle.mimi_ref.rvq_from_embedding on emb [1, 512, T] -> [K, T]."""
    return mimi_ref.rvq_from_embedding(torch.as_tensor(np.asarray(emb)), sd, K)[0].numpy()


def oracle_on_proj(proj, sd, K: int) -> np.ndarray:
    """The oracle's quantizer on a given projection [T, 512] -> [K, T]: the loop of mimi_ref.rvq_encode (its
    ``codebook_embed``, its ``euclid_argmin`` = torch.cdist + argmin, its fp32 residual update) behind the engine's own
    input projection, for a model whose projection rounds (the stock one)."""
    proj = torch.as_tensor(np.ascontiguousarray(np.asarray(proj, dtype=np.float32).reshape(-1, 2 * D)))
    nsem = CFG.num_semantic_quantizers
    out = []
    with torch.no_grad():
        for pre, levels, x in ((SEM, range(nsem), proj[:, :D]), (ACO, range(max(K - nsem, 0)), proj[:, D:])):
            residual = x.contiguous()
            for l in levels:
                p = f"{pre}layers.{l}.codebook."
                embed = mimi_ref.codebook_embed({k: torch.as_tensor(np.asarray(sd[p + k]))
                                                 for k in ("embed_sum", "cluster_usage")}, "", CFG)
                idx = mimi_ref.euclid_argmin(residual, embed)
                residual = residual - torch.nn.functional.embedding(idx, embed)
                out.append(idx)
    return torch.stack(out).numpy()


def oracle_proj(emb, sd) -> np.ndarray:
    """The oracle's own projection (torch CPU fp32) of emb [1, 512, T] -> [T, 512]."""
    x = torch.as_tensor(np.asarray(emb)).float()
    with torch.no_grad():
        halves = [torch.nn.functional.conv1d(x, torch.as_tensor(np.asarray(sd[p + "input_proj.weight"])))
                  for p in (SEM, ACO)]
    return torch.cat(halves, dim=1)[0].T.contiguous().numpy()


# ---- crafted codebooks ------------------------------------------------------------------------------------------------
def _gauss(seed, n=NCODES):
    return (np.random.default_rng(seed).standard_normal((n, D)) / 16.0).astype(np.float32)


DUP_BASE = {"wave": 67, "slice": 133, "half": 10, "far": 200}
MID_BASE = {"wave": 70, "slice": 140, "half": 20, "far": 220}


def _sphere(seed, norm: float) -> np.ndarray:
    e = _gauss(seed)
    return (e * (norm / np.sqrt((e.astype(np.float64) ** 2).sum(1)))[:, None]).astype(np.float32)


def pairs_codebook() -> np.ndarray:
    """Gaussian directions at the norm of ``coherent_codebook``'s fillers; row DUP_BASE[c] + POS[c] is a bitwise copy of
    row DUP_BASE[c] in every class; and the coherent pair COH_PAIRS["pairs"] (``coherent_codebook``)."""
    r = coherent_r()[1]
    e = _sphere(101, 0.9 * COH_A * _norm(r))
    for c, i in DUP_BASE.items():
        e[i + POS[c]] = e[i]
    _coherent_pair(e, r, *COH_PAIRS["pairs"])
    return e


SCALE_POS = {"wave": 4, "slice": 40, "half": 300, "far": 1500}   # multiples of 4: both rows of one scale


ZERO_ANCHORS = {8: 100, 12: 101, 16: 102, 24: 103}   # level-1 row: the stock level-2 row it is a bitwise copy of


@functools.lru_cache(maxsize=1)
def stock_state_dict():
    """The stock model's weights: every model, codebook and case of this module starts from this one copy."""
    return synthetic.make_state_dict(seed=0)


def state_dicts() -> Dict[str, Dict[str, np.ndarray]]:
    return {"stock": stock_state_dict(), "pairs": crafted_state_dict("pairs"), "degen": crafted_state_dict("degen")}


def scales_codebook() -> np.ndarray:
    """Row c has norm ~ 8 x 2^(-8 (c mod 4)): 2^0, 2^-8, 2^-16, 2^-24 of the largest, interleaved so that every slice
    holds every scale.  The ZERO_ANCHORS rows (of the largest scale) are bitwise copies of stock level-2 rows (norm ~ 10):
    a frame equal to one leaves level 2 the residual 0, whose code is the level's smallest row, while a residual that
    was not updated sits on the copied level-2 row itself (``case_zero``; any other row of this codebook is nearer to
    level 2's smallest row than to the rest, with or without the update)."""
    e = _gauss(102) * np.float32(8.0)
    e = (e * np.exp2(-8.0 * (np.arange(NCODES) % 4)).astype(np.float32)[:, None]).astype(np.float32)
    lvl2 = embeds(stock_state_dict(), 3)[2]
    for i, k in ZERO_ANCHORS.items():
        e[i] = lvl2[k]
    return e


def flat_codebook() -> np.ndarray:
    return np.repeat(_gauss(103, 1), NCODES, axis=0)


# (winner i, rival j) per crafted model: one wave and the lower index wins | two waves of a slice and the higher one does.
# One pair per codebook: the rival -b r of a second pair would lie nearer to every frame than the tie,
# |r + b r'| <= (1 + b) |r|, and take the code.  So two of the four (position, role) combinations that can share a slice
# are held.  The window test is per code (the candidate test reads one code's approximate distance and the slice's
# minimum, wherever the two sit), and the tie and merge rules that the other two combinations would also pass through
# are exercised in every position class by ``dup``.
COH_PAIRS = {"degen": (1030, 1031), "pairs": (1190, 1150)}
COH_A, COH_B = 4.0, 2.0
COH_MARGIN = 2.0
GROUPS = {8: (300, 340), 65: (1540, 1700)}   # g: (first row of g equal rows, the distinct winner w), one slice each
GROUP_DELTA = 2.0 ** -5


def coherent_r() -> np.ndarray:
    """One r per pair (row 0: "degen", row 1: "pairs"): elements +-2^e (1 + 2^-11 - 2^-22), e in {-6 .. -3} -- every
    fp16 rounding (of r rs, a power of two times r, and of a r, b r) goes toward zero by all but 2^-11 of a half-ulp;
    the same multiset of exponents, so the same norm."""
    rng = np.random.default_rng(104)
    m = np.float32(1.0 + 2.0 ** -11 - 2.0 ** -22)
    out = []
    for _ in range(2):
        ex = rng.permutation(np.repeat(np.arange(-6, -2), D // 4))
        out.append((rng.choice([-1.0, 1.0], D) * np.exp2(ex)).astype(np.float32) * m)
    return np.stack(out)


def coherent_eta() -> float:
    """e_i = a (1 - eta) r: i wins by d2_j - d2_i = 2 (a - 1) a eta |r|^2 = COH_MARGIN x the hard bound at |e| = a |r|.
    Every multiple of the hard bound in that margin moves i 0.05 of the window towards the approximate minimum (and eta
    takes another 0.017 off the coherent rounding of e_i): at 4 x the emulation measures the winner at 0.44 of the
    window, at 2 x at 0.57 -- the code stays determinate, and a window narrowed 2 x still loses it."""
    return COH_MARGIN * HARD * U * (1.0 + COH_A) ** 2 / (2.0 * (COH_A - 1.0) * COH_A)


def _norm(v) -> float:
    return float(np.sqrt((np.asarray(v, dtype=np.float64) ** 2).sum()))


def _coherent_pair(e, r, i, j):
    e[i] = (np.float32(COH_A) * r) * np.float32(1.0 - coherent_eta())
    e[j] = np.float32(-COH_B) * r


def coherent_codebook() -> np.ndarray:
    """Fillers of norm 0.9 a |r|; the pair e_i = a (1 - eta) r and e_j = -b r, a = b + 2: without eta an exact tie at
    d2 = (a - 1)^2 |r|^2 whose one-product approximation favours j by (a + b) 2^-9 |r|^2, 0.71 of the window's leading
    term 1.06 2^-8 |r| a |r|; and the two GROUPS of g bitwise-equal rows (norm 0.8 a |r|: like the fillers, farther
    from r than the pair is) with a distinct row w at GROUP_DELTA of that norm from them."""
    r = coherent_r()[0]
    e = _sphere(105, 0.9 * COH_A * _norm(r))
    _coherent_pair(e, r, *COH_PAIRS["degen"])
    for g, (g0, w) in GROUPS.items():
        row = (e[g0] * np.float32(0.8 / 0.9)).astype(np.float32)
        off = _gauss(106 + g, 1)[0]
        off = off * np.float32(GROUP_DELTA * _norm(row) / _norm(off))
        e[g0:g0 + g] = row
        e[w] = row + off
    return e


def crafted_state_dict(kind: str) -> Dict[str, np.ndarray]:
    """kind: "pairs" | "degen": ``stock_state_dict`` (the one copy the codebooks and the cases are built from too) with
    the quantizer keys replaced."""
    sd = dict(stock_state_dict())
    eye, zero = np.eye(D, dtype=np.float32), np.zeros((D, D), dtype=np.float32)
    sd[SEM + "input_proj.weight"] = np.concatenate([eye, zero], axis=1)[:, :, None].copy()
    sd[ACO + "input_proj.weight"] = np.concatenate([zero, eye], axis=1)[:, :, None].copy()
    books = {"pairs": (pairs_codebook, scales_codebook), "degen": (flat_codebook, coherent_codebook)}[kind]
    for level, make in enumerate(books):
        sd[cb_prefix(level) + "embed_sum"] = make()
        sd[cb_prefix(level) + "cluster_usage"] = np.ones(NCODES, dtype=np.float32)
    return sd


# ---- cases ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    model: str                     # "stock" | "pairs" | "degen"
    frames: np.ndarray             # fp32 [1, 512, T]
    K: int = 2
    expect: List[Tuple[int, int, Optional[int], str, int]] = field(default_factory=list)
    # (level, tile, slice or None = every slice, class "low" <= 64 | "mid" 65..2048 | "over" > 2048, codes per slice)

    @property
    def T(self) -> int:
        return self.frames.shape[2]

    def tiled(self, T: int) -> np.ndarray:
        """The case's frames repeated cyclically to T frames."""
        reps = -(-T // self.T)
        return np.ascontiguousarray(np.tile(self.frames, (1, 1, reps))[:, :, :T])


def _pack(sem: np.ndarray, aco: np.ndarray) -> np.ndarray:
    """[T, 256] semantic and acoustic halves -> [1, 512, T]."""
    return np.ascontiguousarray(np.concatenate([sem, aco], axis=1).astype(np.float32).T[None])


def _filler(seed, T):
    return (np.random.default_rng(seed).standard_normal((T, D)) / 16.0).astype(np.float32)


def _midpoints(e, i, j, exps):
    out = []
    for k in exps:
        for sgn in (1.0, -1.0):      # +: i is the nearer row; -: j, the higher index
            out.append(((e[i] + e[j]) * np.float32(0.5) + np.float32(sgn * 2.0 ** -k) * (e[i] - e[j])).astype(np.float32))
    return out


def case_dup() -> Case:
    e = pairs_codebook()
    rng = np.random.default_rng(201)
    rows = []
    for c, i in DUP_BASE.items():
        for rel in (0.0, 1e-3, 3e-2):
            rows.append(e[i] + np.float32(rel) * (rng.standard_normal(D) / 16.0).astype(np.float32))
    sem = np.stack(rows).astype(np.float32)
    return Case("dup", "pairs", _pack(sem, _filler(202, len(sem))), expect=[(0, 0, None, "low", 256)])


def case_midpoint() -> Case:
    e = pairs_codebook()
    rows = []
    for c, i in MID_BASE.items():
        rows += _midpoints(e, i, i + POS[c], range(6, 23, 2))
    sem = np.stack(rows)
    return Case("midpoint", "pairs", _pack(sem, _filler(203, len(sem))))


def case_scales() -> Case:
    """Tile t holds the frames around rows of scale 2^(-8 t): midpoints of same-scale pairs in every position class
    and a noisy copy of a row."""
    e = scales_codebook()
    rng = np.random.default_rng(204)
    tiles = []
    for s in range(4):
        rows = []
        for c, off in SCALE_POS.items():
            i = 4 * (MID_BASE[c] // 4) + s
            rows += _midpoints(e, i, i + off, (8, 16))
            rows.append(e[i] + np.float32(2.0 ** (-8 * s - 3)) * (rng.standard_normal(D) / 16.0).astype(np.float32))
        rows = np.stack(rows)
        tiles.append(np.tile(rows, (2, 1))[:32])
    aco = np.concatenate(tiles).astype(np.float32)
    return Case("scales", "pairs", _pack(_filler(205, len(aco)), aco), expect=[(1, 0, None, "over", 256)])


def case_flat(T: int = 40) -> Case:
    """T = 40 on 256-code slices: tile 0 has 32 x 256 candidates (overflow), the tail 8 x 256 = 2048 (the cap: the list
    path, above the staged limit); T = 996 on 512-code slices: full tiles overflow, the 4-frame tail has 4 x 512 = 2048."""
    sem = _filler(206, T)
    exp = [(0, 0, None, "over", 256), (0, 1, None, "mid", 256)] if T == 40 else \
        [(0, 0, None, "over", 512), (0, T // 32, None, "mid", 512)]
    return Case(f"flat{T}", "degen", _pack(sem, _filler(207, T)), expect=exp)


def case_group(g: int) -> Case:
    """32 frames (one tile): even frames next to the winner w (the g equal rows are candidates GROUP_DELTA away), odd
    frames next to the equal rows (their lowest index wins; w is a candidate): (g + 1) x 32 candidates in the slice."""
    e = coherent_codebook()
    g0, w = GROUPS[g]
    rng = np.random.default_rng(208 + g)
    nrm = float(np.sqrt((e[g0].astype(np.float64) ** 2).sum()))
    rows = [(e[w] if t % 2 == 0 else e[g0]) + np.float32(1e-4 * nrm) * (rng.standard_normal(D) / 16.0).astype(np.float32)
            for t in range(32)]
    aco = np.stack(rows).astype(np.float32)
    cls = "mid" if RVQC_NSTG < (g + 1) * 32 <= RVQ_CAND else "over"
    return Case(f"group{g}", "degen", _pack(_filler(209, 32), aco), expect=[(1, 0, g0 // 256, cls, 256)])


def case_coherent(model: str) -> Case:
    """32 copies of the pair's r (2 x 32 = 64 candidates: the staged limit itself) on level 1 ("degen") or 0 ("pairs")."""
    r = np.tile(coherent_r()[0 if model == "degen" else 1], (32, 1)).astype(np.float32)
    fill = _filler(210, 32)
    level = 1 if model == "degen" else 0
    return Case(f"coherent_{model}", model, _pack(fill, r) if level else _pack(r, fill),
                expect=[(level, 0, COH_PAIRS[model][0] // 256, "low", 256)])


def case_zero(K: int) -> Case:
    """All-zero frames, and frames whose acoustic half is bitwise a level-1 row: the level-2 residual is exactly 0."""
    e = scales_codebook()
    aco = np.stack([np.zeros(D, np.float32)] * 4 + [e[i] for i in (*ZERO_ANCHORS, 1, 2, 3, 517, 1030, 1543, 2047, 40)])
    sem = _filler(211, len(aco))
    sem[:4] = 0.0
    return Case(f"zero_K{K}", "pairs", _pack(sem, aco), K=K)


# 2^-120 puts every frame's max |proj| under 2^-114, where rs = 2^(13 - ilogb(max|r|)) overflows to inf: every fp16
# plane element is +-inf (or NaN), every approximate distance NaN, every code a candidate.  (2^-60 and 2^-50 leave rs
# finite, 2^70 and 2^60: they are small-residual cases, no more.)
EMB_SCALES = (-120, -60, -50, -24, -12, 0, 12, 24, 50)
RS_INF_BELOW = 2.0 ** -114


def case_embscale(base: np.ndarray, s: int, K: int = 8) -> Case:
    """base [512, T] (a natural embedding) times 2^s on the stock model."""
    x = (np.asarray(base, dtype=np.float32) * np.float32(2.0 ** s)).astype(np.float32)
    assert np.isfinite(x).all()
    T = x.shape[1]
    exp = []
    if s <= -120:   # rs = inf: a full tile has 32 x 256 candidates in every slice, a tail of n frames n x 256
        exp = [(l, t, None, klass(min(32, T - 32 * t) * 256), 256) for l in (0, 1) for t in range(-(-T // 32))]
    return Case(f"embscale{s:+d}", "stock", np.ascontiguousarray(x[None]), K=K, expect=exp)


def case_tiny() -> Case:
    """The ``dup`` frames times 2^-120 on the "pairs" model, whose projection is exact: max |r| < 2^-114 at levels 0 and
    1 by construction, so rs = inf and all 12 x 256 (frame, code) pairs of every slice are candidates (the list
    overflows).  |r|^2 underflows to 0 in fp32 and every distance is |e| up to the chain's tiny a: the code is the
    level's smallest row."""
    x = (case_dup().frames * np.float32(2.0 ** -120)).astype(np.float32)
    assert np.isfinite(x).all() and 0 < np.abs(x).max() < RS_INF_BELOW
    return Case("tiny", "pairs", x, expect=[(0, 0, None, "over", 256), (1, 0, None, "over", 256)])


def first_scales(proj) -> np.ndarray:
    """rs of every frame at the two levels that read the projection: [2, F] (``_pow2_scale``; inf where it overflows)."""
    proj = np.asarray(proj, dtype=np.float32).reshape(-1, 2 * D)
    return np.stack([_pow2_scale(np.abs(start_residual(proj, l)).max(1)) for l in (0, CFG.num_semantic_quantizers)])


def crafted_cases() -> List[Case]:
    return [case_dup(), case_midpoint(), case_scales(), case_flat(40), case_group(8), case_group(65), case_coherent("degen"),
            case_coherent("pairs"), case_tiny(),
            case_zero(3)]


# ---- the CPU emulation of the selection ---------------------------------------------------------------------------------
def _pow2_scale(mx: np.ndarray) -> np.ndarray:
    """ops.hip rvq_norms: rs = 2^(13 - ilogb(mx)) in fp32 (inf when it overflows), 1 for mx = 0."""
    with np.errstate(all="ignore"):
        ex = np.floor(np.log2(np.where(mx > 0, mx, 1.0).astype(np.float64)))
        rs = np.exp2(13.0 - ex).astype(np.float32)        # > 2^127 -> inf, as ldexpf
    return np.where(mx > 0, rs, np.float32(1.0)).astype(np.float32)


FAULTS = ("approx_only", "window/2", "window/4", "last_tie", "merge_later", "truncate", "skip_tail", "no_resid")


def emulate(proj, emb, K: int, slc: int = 256, ft: int = 32, fault: Optional[str] = None) -> dict:
    """The engine's RVQ on the CPU: codes [K, F], the candidate counts per level [ntiles, nslices] and each frame's
    window position per level, pos = (approx d2 of the chosen code - the slice's approximate minimum) / window."""
    assert fault is None or fault in FAULTS, fault
    proj = np.ascontiguousarray(np.asarray(proj, dtype=np.float32).reshape(-1, 2 * D))
    F = proj.shape[0]
    nsem = CFG.num_semantic_quantizers
    nsl, ntl = NCODES // slc, -(-F // ft)
    wdiv = {"window/2": 2.0, "window/4": 4.0}.get(fault, 1.0)
    codes = np.zeros((K, F), dtype=np.int64)
    counts, pos = [], []
    fr = np.arange(F)
    tile = fr // ft
    r = None
    f32 = np.float32
    with np.errstate(all="ignore"):
        for L in range(K):
            e = emb[L]
            if L == 0 or L == nsem:
                r = start_residual(proj, L)
            uniq, inv = np.unique(e.view(np.uint32), axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            eu = uniq.view(np.float32)
            # exact fp32 distances (equal rows get equal values: computed once per distinct row); every sum is formed
            # in float64 and rounded once to fp32 -- an fp32 evaluation that does not depend on the BLAS at hand
            r64, eu64 = r.astype(np.float64), eu.astype(np.float64)
            xn = (r64 * r64).sum(1).astype(f32)
            ynu = (eu64 * eu64).sum(1).astype(f32)
            a = (-2.0 * (r64 @ eu64.T)).astype(f32)
            dex = np.sqrt(np.maximum((a + xn[:, None]) + ynu[None, :], f32(0.0)))[:, inv]
            yn = ynu[inv]
            # approximate: fp16 hi planes at power-of-two scales, fp32 accumulation
            rs = _pow2_scale(np.abs(r).max(1))
            amax = float(np.abs(e).max())
            cs = _pow2_scale(np.array([amax]))[0] if np.isfinite(amax) else f32(1.0)
            rh = (r * rs[:, None]).astype(np.float16).astype(f32)
            ehu = (eu * cs).astype(np.float16).astype(f32)
            acc = (rh.astype(np.float64) @ ehu.astype(np.float64).T).astype(f32)[:, inv]
            ur = (f32(1.0) / rs) * (f32(1.0) / cs)
            apx = (f32(-2.0) * (acc * ur[:, None]) + xn[:, None]) + yn[None, :]
            emax = f32(np.sqrt(yn.max()) * (1.0 + 1e-6))
            rnorm = np.sqrt(np.maximum(xn, f32(0.0)))
            cnt = np.zeros((ntl, nsl), dtype=np.int64)
            best_d = np.full((F, nsl), np.inf, dtype=f32)
            best_i = np.zeros((F, nsl), dtype=np.int64)
            best_p = np.zeros((F, nsl), dtype=np.float64)
            for s in range(nsl):
                sl = slice(s * slc, (s + 1) * slc)
                ap = apx[:, sl]
                m = np.fmin.reduce(np.where(np.isnan(ap), np.inf, ap), axis=1).astype(f32)
                rn = rnorm + emax
                win = (f32(1.06) * rnorm * emax * f32(2.0 ** -8) + rn * rn * f32(2.0 ** -18)
                       + np.abs(m) * f32(2.0 ** -20) + f32(1e-30)) / f32(wdiv)
                cand = ~(ap > (m + win)[:, None])
                c_t = np.zeros(ntl, dtype=np.int64)
                np.add.at(c_t, tile, cand.sum(1))
                cnt[:, s] = c_t
                over = c_t[tile] > RVQ_CAND
                if fault == "truncate":      # the list's first 2048 entries in (code, frame) order, nothing else
                    for t in np.flatnonzero(c_t > RVQ_CAND):
                        rows = np.flatnonzero(tile == t)
                        flat = cand[rows].T.copy()
                        keep = np.cumsum(flat.reshape(-1)).reshape(flat.shape) <= RVQ_CAND
                        cand[rows] = (flat & keep).T
                    use = cand
                else:
                    use = cand | over[:, None]
                dm = np.where(use, apx[:, sl] if fault == "approx_only" else dex[:, sl], np.inf)
                if fault == "last_tie":
                    ix = slc - 1 - np.argmin(dm[:, ::-1], axis=1)
                else:
                    ix = np.argmin(dm, axis=1)
                none = ~use.any(1)
                best_d[:, s] = np.where(none, np.nan, dm[fr, ix])
                best_i[:, s] = np.where(none, -1, ix + s * slc)
                best_p[:, s] = (ap[fr, ix].astype(np.float64) - m) / np.maximum(win.astype(np.float64), 1e-300)
            bd = np.where(np.isnan(best_d), np.inf, best_d)
            if fault == "merge_later":
                ws = nsl - 1 - np.argmin(bd[:, ::-1], axis=1)
            else:
                ws = np.argmin(bd, axis=1)      # equal distances: the earlier slice holds the lower indices
            c = best_i[fr, ws]
            c = np.where((c < 0) | (c >= NCODES) | np.isinf(bd[fr, ws]) & np.isnan(best_d[fr, ws]), 0, c)
            if fault == "skip_tail" and F % ft:
                c = np.where(fr >= F - F % ft, 0, c)
            codes[L] = c
            counts.append(cnt)
            pos.append(best_p[fr, ws])
            if (L >= nsem or L + 1 < nsem) and fault != "no_resid":
                r = r - e[c]
    return {"codes": codes, "counts": counts, "pos": pos}


def klass(n: int) -> str:
    return "low" if n <= RVQC_NSTG else "mid" if n <= RVQ_CAND else "over"


def check_expect(case: Case, em_by_slc: Dict[int, dict]) -> List[str]:
    """The case's intended candidate-count classes against the emulation's counts ({codes per slice: emulate(..)})."""
    bad = []
    for level, t, s, cls, slc in case.expect:
        cnt = em_by_slc[slc]["counts"][level][t]
        for sl in (range(len(cnt)) if s is None else [s * 256 // slc]):
            if klass(int(cnt[sl])) != cls:
                bad.append(f"{case.name}: level {level} tile {t} slice {sl} ({slc} codes): {int(cnt[sl])} candidates, "
                           f"wanted {cls}")
    return bad
