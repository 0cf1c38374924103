"""Per-draw acceptance rule for the sampler chain, derived from the restatement (tests/sampler_chain_ref.py) and the kernel's documented
quanta (csrc/kernels_sample.hip) alone -- test infrastructure.  No figure in here was tuned on device output.  It extends
tests/sampler_accept.py, whose reasoning and allowances (`cut_allowance`, `dev_allowance`, S_MARGIN) it reuses unchanged.

Paths G and top_k == 1: only comparisons and exact f32 operations decide them (the additive penalties are two f32 operations, done
alike on both sides), so `got` must equal the restatement's token.

Path S: the device runs min-p and typical-p over the k survivors in one lane, in the reference's order, so equal, or one of the
restatement's deciding comparisons lay within 2^-20 of flipping (`ChainRef.last_margin`, which for the chain also holds the distance
of every probability from the min-p threshold, of the typical-p running sum from typical_p on both sides of the cut, and of the first
deviation left out from the last one taken).

Path F with min-p.  Top-k, top-p and min-p are cuts of one stable descending order: min-p keeps a prefix of it, every tie of a value
included.  The device compares expf(x_i - M) < min_p; the reference compares f32(e_i / S) < f32(min_p * f32(1 / S)) with e_i its own
f32 exp.  Against the float64 e_i = exp(f32(x_i - M)) the device is off by expf's 2^-23 (relative) and the reference by 2^-23 for its
exp and 2^-24 for each of its three roundings, so both decide alike unless |e_i / min_p - 1| <= MINP_REL = 2^-23 + 3 * 2^-24.  An entry
equal to the maximum has e = 1 with no error on either side and is kept by both (min_p <= 1).  A draw with an entry inside that band
(and inside the largest admissible top-p cut) is UNDECIDED: the admissible cuts then run from the prefix without the band to the prefix
with it, combined with the admissible top-p cuts by taking the shorter prefix at either end, and the interval rule of
tests/sampler_accept.py (tolerance, eps_lo / eps_hi, membership in the largest admissible kept set) applies to that range of cuts
unchanged: its derivation only needs the admissible kept sets to be nested prefixes of one order.  min-p adds no sum, so `tol` is as
there.

Path F with typical-p.  The device does not take a logarithm per entry: with g_i = f32(M - x_i), -ln p_i = ln S + g_i, so the deviation
|(-ln p_i) - H| is |g_i - G| with G = sum p_i g_i, which it computes as f32(Sw / Sm) from two fixed-point sums (masses round(e_i * 2^40),
weighted gaps round(f32(e_i * g_i) * 2^40)) and keys as f32(|g_i - G|).  Against the float64 d_i = |g_i - G64| over the reference's own
survivors of the stages in front, the device's deviation of entry i is off by at most
    TAU_i = G * (2^-22 + 2^-23)            expf (2^-23) on numerator and denominator, the product's rounding, the f32 rounding of G
          + n_inexact * 2^-40 * (1 + G)    the fixed-point quanta of both sums (entries at the maximum are exact and count for nothing)
          + 2^-24 * d_i                    the rounding of the f32 difference
          + eps_up * (G + g_far)           when the cuts in front are themselves undecided: entries of mass share eps_up and gap <= g_far
                                           enter or leave the mean
          + ref_drift                      max |d_f32 - d_f64| of the restatement itself, so that its own kept set is admissible
and its cumulative masses by TAU_M = cut_allowance (as for top-p) + eps_up + the restatement's own drift along its order.  The cut falls
at a deviation level between t_lo (the level at which the earliest possible accumulation, every entry TAU_i early, reaches typical_p -
TAU_M) and t_hi (the latest possible one reaches typical_p + TAU_M).  Entries with d_i + TAU_i < t_lo are kept for sure, entries with
d_i - TAU_i > t_hi are removed for sure, the rest are ambiguous.  The draw is decided when exactly one entry is ambiguous (the mass below
t_lo cannot reach typical_p, so that entry is the one that crosses), or when all ambiguous entries hold one value -- then they tie bit for
bit on either side, go by ascending id, and their number follows from the masses alone -- and that number is the same at typical_p -
TAU_M and typical_p + TAU_M.  Otherwise the draw is UNDECIDED: the kept set lies between the sure set and the sure set with every ambiguous
entry.  With DELTA the mass between the two and D_small the mass of the smaller, no cumulative position moves by more than eps = 2 *
DELTA / D_small ((m' D - m D') / (D' D) with |m' - m|, |D' - D| <= DELTA), so `got` is accepted when it is in the larger set, has a
non-zero probability and u lies within tol + eps of its interval; `tol` is the draw tolerance of tests/sampler_accept.py."""
from __future__ import annotations

import numpy as np

import sampler_accept as sa
import sampler_ref as sr

MINP_REL = 2.0 ** -23 + 3 * 2.0 ** -24
G_REL = 2.0 ** -22 + 2.0 ** -23


def analyse_typ(ref, an, e, order, Cs, cuts, nk) -> None:
    """The typical-p part of the F rule: fills `an` (admit, undecided, ...) for a call whose typical-p stage ran."""
    rec = ref.last
    t = rec["typ"]
    xk = rec["xk"]
    n = xk.size
    c_lo, cut, c_hi = cuts
    u, ty = float(rec["u"]), float(ref.ty)
    M = np.float32(np.max(xk))
    with np.errstate(invalid="ignore", over="ignore"):
        g = (M - xk).astype(np.float32).astype(np.float64)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    up_ref = (rank < cut) & (e > 0)  # the reference's survivors of the cuts in front
    eps_up = (float(Cs[c_hi - 1]) - float(Cs[c_lo - 1])) / float(Cs[c_lo - 1])
    p = np.where(up_ref, e, 0.0)
    p = p / p.sum()
    G = float((p[up_ref] * g[up_ref]).sum())
    d = np.abs(np.where(np.isfinite(g), g, 1e300) - G)
    # the restatement's own drift, over the entries that carry any weight
    d32 = np.full(n, np.nan)
    d32[t["idx"]] = t["d"].astype(np.float64)
    heavy = up_ref & (p > 1e-12) & np.isfinite(d32)
    ref_drift = float(np.max(np.abs(d32[heavy] - d[heavy]))) if heavy.any() else 0.0
    inexact = up_ref & (e < 1)
    n_in, m_in = int(np.count_nonzero(inexact)), float(p[inexact].sum())
    g_far = float(g[order[min(c_hi, n) - 1]]) if c_hi != c_lo else 0.0
    tau = G * G_REL + n_in * sa.FIX_Q * (1 + G) + 2.0 ** -24 * np.minimum(d, 1e30) + eps_up * (G + g_far) + ref_drift
    ro = t["idx"][t["order"]]  # the reference's order
    C_ref = np.cumsum(p[ro])
    k = min(ro.size, t["cutoff"] + 1)
    tau_m = sa.cut_allowance(n_in, m_in) + eps_up + float(np.max(np.abs(t["cum"][:k].astype(np.float64) - C_ref[:k])))
    cand = (rank < c_hi) & (e > 0)  # whatever any admissible cut in front keeps
    ids = np.flatnonzero(cand)
    pc = np.where(up_ref, p, e / float(np.where(up_ref, e, 0.0).sum()))[ids]

    def level(shift, target):
        key = d[ids] + shift * tau[ids]
        o = np.argsort(key, kind="stable")
        cs = np.cumsum(pc[o])
        j = int(np.searchsorted(cs, target, side="left"))
        return float(key[o[j]]) if j < o.size else np.inf

    t_lo, t_hi = level(-1.0, ty - tau_m), level(+1.0, ty + tau_m)
    sure = np.zeros(n, bool)
    amb = np.zeros(n, bool)
    sure[ids] = (d[ids] + tau[ids] < t_lo) & (rank[ids] < c_lo)
    amb[ids] = ~sure[ids] & ~(d[ids] - tau[ids] > t_hi)
    keep_ref = t["keep"]
    small, big = sure.copy(), sure | amb
    na = int(np.count_nonzero(amb))
    undecided = True
    if c_lo == c_hi:
        if na == 1:
            undecided, small = False, big.copy()
        elif na > 1 and np.all(xk[amb] == xk[amb][0]):
            a_ids, pa, base = np.flatnonzero(amb), float(p[np.flatnonzero(amb)[0]]), float(p[sure].sum())
            j_lo = max(1, int(np.ceil((ty - tau_m - base) / pa - 1e-12)))
            j_hi = max(1, int(np.ceil((ty + tau_m - base) / pa - 1e-12)))
            if j_lo == j_hi and j_lo <= a_ids.size:
                undecided = False
                small = sure.copy()
                small[a_ids[:j_lo]] = True
                big = small.copy()
    an["typ_ok"] = bool(np.all(small <= keep_ref) and np.all(keep_ref <= big))
    an["undecided"] = undecided
    D = float(p[keep_ref].sum())
    q = np.where(keep_ref, p, 0.0) / D
    C = np.cumsum(q)
    cum32 = rec["cum"].astype(np.float64)
    inx = keep_ref & (e < 1)
    tol = float(np.max(np.abs(cum32 - C))) + sa.dev_allowance(int(np.count_nonzero(inx)), float(q[inx].sum()))
    pall = np.zeros(n)
    pall[ids] = pc
    d_small = float(pall[small].sum())
    delta = float(pall[big & ~small].sum())
    eps = 2 * delta / d_small if d_small > 0 else np.inf
    T = tol + eps
    lo = C - q
    width = np.where(big, pall, 0.0) / D
    hi = lo + width
    dist = np.maximum(0.0, np.maximum(lo - u, u - hi))
    admit = big & (width > 0) & (dist <= T)
    if u >= 1.0 - T:
        admit[n - 1] = True
    admit[int(rec["want"])] = True
    an.update(u=u, tol=tol, T=T, extra=eps, lo=lo, hi=hi, dist=dist, admit=admit, in_big=big, width=width, f32_total=float(cum32[-1]),
              n_kept=int(np.count_nonzero(q)), n_amb=na, tau_m=tau_m, ref_drift=ref_drift, cuts=cuts)


def analyse(ref) -> dict:
    """What the F rule needs about the last call of a ChainRef, float64; cached on the record.  Follows sampler_accept.analyse."""
    rec = ref.last
    if "_anc" in rec:
        return rec["_anc"]
    an: dict = {"undecided": False}
    rec["_anc"] = an
    xk = rec["xk"]
    n = xk.size
    M = np.float32(np.max(xk)) if n else np.float32(-np.inf)
    an["nan_row"] = not np.isfinite(M)
    if an["nan_row"]:
        return an
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((xk - M).astype(np.float32).astype(np.float64))
    pk = e / e.sum()
    u = float(rec["u"])
    inexact = (e > 0) & (e < 1)
    nk, mk = int(np.count_nonzero(inexact)), float(e[inexact].sum() / e.sum())
    order = rec["order"] if rec["order"] is not None else sr.stable_desc(xk)
    Cs = np.cumsum(pk[order])
    c_lo = cut = c_hi = n
    an["cut_ok"] = True
    if rec["cut"] is not None:
        cut, p = int(rec["cut"]), float(ref.p)
        drift = np.abs(rec["cum_sorted"].astype(np.float64) - Cs)

        def span(tc):
            return (min(n, int(np.searchsorted(Cs, p - tc, side="right")) + 1), min(n, int(np.searchsorted(Cs, p + tc, side="right")) + 1))

        _, c_hi0 = span(float(drift.max()) + sa.cut_allowance(nk, mk))
        tol_cut = float(drift[:c_hi0].max()) + sa.cut_allowance(nk, mk)
        c_lo, c_hi = span(tol_cut)
        an["cut_ok"] = c_lo <= cut <= c_hi
        c_lo, c_hi = min(c_lo, cut), max(c_hi, cut)
    an["topp_cuts"] = (c_lo, cut, c_hi)
    if rec["minp"] is not None:
        mp = float(ref.mp)
        es = e[order]  # descending
        m_ref = int(np.count_nonzero(rec["minp"]["keep"] & (rec["xp"] > -np.inf)))
        keep_ref = np.zeros(n, bool)
        keep_ref[order[:m_ref]] = True
        an["minp_prefix_ok"] = bool(np.array_equal(keep_ref, rec["minp"]["keep"] & (rec["xp"] > -np.inf)))
        m_hi = int(np.count_nonzero((es >= mp * (1 - MINP_REL)) | (es == 1)))
        m_lo = int(np.count_nonzero((es > mp * (1 + MINP_REL)) | (es == 1)))
        an["minp_ok"] = min(m_lo, cut) <= m_ref <= m_hi  # m_ref counts inside the reference's own top-p cut
        an["undecided"] = min(m_lo, c_hi) != min(m_hi, c_hi)
        m_lo, m_hi = min(m_lo, m_ref), max(m_hi, m_ref)
        c_lo, cut, c_hi = max(1, min(c_lo, m_lo)), min(cut, m_ref), min(c_hi, m_hi)
    an["cuts"] = (c_lo, cut, c_hi)
    if rec["typ"] is not None:
        analyse_typ(ref, an, e, order, Cs, (c_lo, cut, c_hi), nk)
        if c_lo != c_hi:
            an["undecided"] = True
        return an
    D = float(Cs[cut - 1])
    eps_hi = (float(Cs[c_hi - 1]) - D) / float(Cs[c_hi - 1])
    eps_lo = (D - float(Cs[c_lo - 1])) / float(Cs[c_lo - 1])
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    in_ref = rank < cut
    in_big = rank < c_hi
    q = np.where(in_ref, pk, 0.0) / D
    C = np.cumsum(q)
    cum32 = rec["cum"].astype(np.float64)
    inexact &= q > 0
    tol = float(np.max(np.abs(cum32 - C))) + sa.dev_allowance(int(np.count_nonzero(inexact)), float(q[inexact].sum()))
    extra = max(eps_lo, eps_hi)
    T = tol + extra
    lo = C - q
    width = np.where(in_big, pk, 0.0) / D
    hi = lo + width
    down = np.maximum(lo * eps_hi, (1 - lo) * eps_lo)
    up = np.maximum((1 - hi) * eps_hi, hi * eps_lo)
    dist = np.maximum(0.0, np.maximum(lo - u, u - hi))
    admit = in_big & (width > 0) & (lo - down - tol <= u) & (u <= hi + up + tol)
    if u >= 1.0 - T:
        admit[n - 1] = True
    admit[int(rec["want"])] = True
    an.update(u=u, tol=tol, T=T, extra=extra, lo=lo, hi=hi, dist=dist, admit=admit, in_big=in_big, width=width, f32_total=float(cum32[-1]),
              n_kept=int(np.count_nonzero(q)))
    return an


def accepts(ref, got: int) -> tuple[bool, str]:
    """Is `got` a defensible answer to the call `ref` (a ChainRef) just made?  -> (ok, reason).  `ref.last["undecided"]` tells whether an F
    draw had a min-p comparison inside the derived band."""
    rec = ref.last
    want, path = int(rec["want"]), ref.last_path
    got = int(got)
    rec["undecided"] = False
    if got == want and path != "F":
        return True, "equal"
    if path == "G" or ref.k == 1:
        return False, f"path {path}, top_k {ref.k}: only comparisons decide it, want {want}, got {got}"
    if path == "S":
        if ref.last_margin < sa.S_MARGIN:
            return True, f"S: deciding comparison within 2^-20 ({ref.last_margin:.3e})"
        return False, f"S: want {want}, got {got}, margin {ref.last_margin:.3e} >= 2^-20"
    if not 0 <= got < rec["vocab"]:
        return False, f"got {got} is outside the vocabulary"
    an = analyse(ref)
    if an["nan_row"]:
        return (got == want), f"the row has no finite maximum: only the fall-through to {want} is defensible, got {got}"
    rec["undecided"] = an["undecided"]
    if got == want:
        return True, "equal"
    if not an["admit"][got]:
        if not an["in_big"][got]:
            why = "top-k, or every admissible top-p and min-p cut, removed it"
        elif an["width"][got] <= 0:
            why = "its probability is 0"
        else:
            why = f"u {an['u']:.9g} is {an['dist'][got]:.3e} from its interval [{an['lo'][got]:.9g}, {an['hi'][got]:.9g}], T {an['T']:.3e}"
        return False, f"F: want {want}, got {got}: {why} (tol {an['tol']:.3e}, cuts {an['cuts']})"
    return True, f"F: u within {an['dist'][got]:.3e} of got's interval, T {an['T']:.3e}, undecided {an['undecided']}"
