"""Per-draw acceptance rule for the device sampler, derived from the restatement alone -- test infrastructure.

`accepts(ref, got)` decides whether the token a device returned is defensible, given what `RefSampler.sample` recorded of its
last call (`ref.last`).  No figure in here was tuned on device output.

Paths G and `top_k == 1`: only comparisons decide them, so `got` must equal the reference's token.  Path S (top_k <= SMALL_K): the
device sums in the reference's order, so equal, or the restatement's deciding comparison lay within 2^-20 of flipping.

Path F (parallel sums over the vocabulary) cannot be bit-equal to a reference that adds the vocabulary in f32 one term after
another.  `got == want` is accepted.  Otherwise the rule recomputes in float64 what the reference summed in f32:

  e_i = exp(f32(x_i - M)) over the entries top-k kept (x: the recorded tempered logits, M their maximum; the f32 difference is
  what both the reference and the device feed to exp), p_i = e_i / sum e.  Top-k itself is exact (comparisons; stable ties, first
  in index order, -0.0 == +0.0), so an entry top-k removed is never acceptable.

  Draw.  C = float64 cumulative sums of the renormalised kept probabilities in index order (the order `sample_from_probs` walks).
  `got` is accepted only if it is in the largest admissible kept set, has a non-zero probability, and u lies within T of
  [C[got-1], C[got]].  T = tol + (what the cut allowance adds, below), and

      tol = max_i |cumsum_f32[i] - C[i]|  +  DEV(n_kept)

  The first term is the reference's own drift on that row (its f32 interval contains u, and its endpoints are within the drift
  of the f64 ones, so the reference's token passes by construction).  DEV is the allowance for the device's arithmetic, from the
  kernel's documented quanta (csrc/kernels_sample.hip):
    * masses are round(expf(x - M) * 2^40): each is off by at most 2^-41 (half the 2^-40 quantum) plus expf's relative error
      EXPF_REL = 2^-23 (HIP documents expf at 1 ulp).  Integer sums add nothing.  In units of the total (>= 1, since the top entry
      contributes exactly 1) a partial sum is off by at most EXPF_REL + n_kept * 2^-41, and so is the denominator:
      2 * EXPF_REL + n_kept * 2^-40 for the quotient.  An entry equal to the maximum has mass expf(0) * 2^40 = 2^40 with no error
      at all, so both terms count only the entries below the maximum: n_inexact of them, holding the share mass_inexact of the
      total.  (On an all-equal row the device's sums are exact, and so is the rule: that is what tells `>` from `>=` at a
      cumulative sum that equals top_p.)
    * inside the draw's 1024-entry chunk the device scans f32 probabilities: the chunk's start is rounded to f32 once, every
      64-lane scan step is 6 additions plus 1 for the carry, 16 steps per chunk, and a rounding miss moves on into the next
      chunk: at most 1 + 2 * 16 * 7 = 225 roundings of at most 2^-25 each (the sums are below 1); each probability carries
      the f32 roundings of the denominator, the quotient and the conversion, 3 * 2^-24 over a mass of at most 1.
      DEV = 2 * 2^-23 * mass_inexact + n_inexact * 2^-40 + 225 * 2^-25 + 3 * 2^-24   (at most 8.1e-6 at n = 2^20, 7.1e-6 for small n).

  Top-p cut: a widened tolerance, not an enumeration (an enumeration walks the vocabulary once per admissible cut, thousands
  of them for top_p = 0.999999).  Cs = float64 sums of p over the stable descending order.  The reference cut where its f32 sums
  first exceeded top_p, so a device summing to within CUTDEV of exact (the first two terms of DEV) may cut at any c with
  Cs[c-1] > top_p - tol_cut and (c == 1 or Cs[c-2] <= top_p + tol_cut), tol_cut = max_{i < c_hi0} |cum_sorted_f32[i] - Cs[i]| +
  CUTDEV, where c_hi0 is the last admissible cut under the drift of the whole row (no cut of either side looks at sums beyond
  it, so the drift beyond it cannot matter; on a flat row with top_p = 1e-6 the whole-row drift would be a thousand times
  top_p).  These cuts c_lo..c_hi keep nested sets order[:c]; the largest, order[:c_hi], bounds membership.  A device that cut at
  c' != cut normalises by D' = Cs[c'-1] instead of D = Cs[cut-1].  With m the reference-kept mass below an entry and L = m / D:
    c' > cut adds entries of mass D' - D, some share r in [0, D' - D] of it below the entry: (m + r) / D' - m / D lies in
      [-L * eps_hi, (1 - L) * eps_hi], eps_hi = (Cs[c_hi-1] - D) / Cs[c_hi-1];
    c' < cut lacks entries of mass D - D': (m - r) / D' - m / D lies in [-(1 - L) * eps_lo, L * eps_lo],
      eps_lo = (D - Cs[c_lo-1]) / Cs[c_lo-1].
  So an entry's interval [L, H] may sit lower by down(L) = max(L * eps_hi, (1 - L) * eps_lo) or higher by up(H) =
  max((1 - H) * eps_hi, H * eps_lo) on the device, and the entry is accepted when u lies in [L - down - tol, H + up + tol].
  The total tolerance is T = tol + max(eps_hi, eps_lo); with a single admissible cut T = tol.  An entry of order[cut:c_hi]
  gets the interval it would have if it were inserted into the reference's sums.

  Fall-through: when the row has no finite maximum (all -inf, or a +inf: the reference's probabilities are NaN) only
  vocab - 1 is accepted.  Otherwise vocab - 1 is also accepted when u >= 1 - T (the f32 sums ended below u, or the device's f32
  scan did); the last kept entry, like any other, by the interval rule, which covers it when 1 - C_f32[-1] is within tol.
  When the reference fell through because its f32 total ended below u, an exact device lands on the entry whose f64
  interval holds u, which the interval rule accepts too."""
from __future__ import annotations

import math

import numpy as np

EXPF_REL = 2.0 ** -23
FIX_Q = 2.0 ** -40
S_MARGIN = 2.0 ** -20


def cut_allowance(n_inexact: int, mass_inexact: float) -> float:
    return 2 * EXPF_REL * mass_inexact + n_inexact * FIX_Q


def dev_allowance(n_inexact: int, mass_inexact: float) -> float:
    return cut_allowance(n_inexact, mass_inexact) + 225 * 2.0 ** -25 + 3 * 2.0 ** -24


def analyse(ref) -> dict:
    """Everything the F rule needs about the reference's last call, float64; cached on the record."""
    rec = ref.last
    if "_an" in rec:
        return rec["_an"]
    an: dict = {}
    rec["_an"] = an
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
    in_ref = np.ones(n, bool)
    in_big = np.ones(n, bool)
    D = 1.0
    eps_lo = eps_hi = 0.0
    an["cuts"] = None
    if rec["cut"] is not None:
        order, cut, p = rec["order"], int(rec["cut"]), float(ref.p)
        Cs = np.cumsum(pk[order])
        drift = np.abs(rec["cum_sorted"].astype(np.float64) - Cs)

        def span(tc):
            c_lo = min(n, int(np.searchsorted(Cs, p - tc, side="right")) + 1)
            c_hi = min(n, int(np.searchsorted(Cs, p + tc, side="right")) + 1)
            return c_lo, c_hi

        _, c_hi0 = span(float(drift.max()) + cut_allowance(nk, mk))
        tol_cut = float(drift[:c_hi0].max()) + cut_allowance(nk, mk)
        c_lo, c_hi = span(tol_cut)
        an["cuts"] = (c_lo, cut, c_hi)
        an["tol_cut"] = tol_cut
        an["cut_ok"] = c_lo <= cut <= c_hi
        c_lo, c_hi = min(c_lo, cut), max(c_hi, cut)
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
    n_final = int(np.count_nonzero(q))
    inexact &= q > 0
    tol = float(np.max(np.abs(cum32 - C))) + dev_allowance(int(np.count_nonzero(inexact)), float(q[inexact].sum()))
    extra = max(eps_lo, eps_hi)
    T = tol + extra
    lo = C - q  # C[i-1]
    width = np.where(in_big, pk, 0.0) / D
    hi = lo + width
    down = np.maximum(lo * eps_hi, (1 - lo) * eps_lo)
    up = np.maximum((1 - hi) * eps_hi, hi * eps_lo)
    dist = np.maximum(0.0, np.maximum(lo - u, u - hi))  # how far u lies from the float64 interval
    admit = in_big & (width > 0) & (lo - down - tol <= u) & (u <= hi + up + tol)
    if u >= 1.0 - T:
        admit[n - 1] = True
    admit[int(rec["want"])] = True
    an.update(u=u, tol=tol, T=T, extra=extra, lo=lo, hi=hi, dist=dist, admit=admit, in_big=in_big, width=width, pmax=float(q.max()),
              pmin=float(width[width > 0].min()), n_kept=n_final, f32_total=float(cum32[-1]))
    return an


def accepts(ref, got: int) -> tuple[bool, str]:
    """Is `got` a defensible answer to the call `ref` (a RefSampler) just made?  -> (ok, reason).  Details of an F decision are
    left in `ref.last["verdict"]`: dist (how far u lies from got's float64 interval), T, and the index distance to the reference's token."""
    rec = ref.last
    want, path = int(rec["want"]), ref.last_path
    got = int(got)
    rec["verdict"] = {"dist": 0.0, "T": 0.0, "idx": abs(got - want)}
    if got == want:
        return True, "equal"
    if path == "G" or ref.k == 1:
        return False, f"path {path}, top_k {ref.k}: only comparisons decide it, want {want}, got {got}"
    if path == "S":
        if ref.last_margin < S_MARGIN:
            return True, f"S: deciding comparison within 2^-20 ({ref.last_margin:.3e})"
        return False, f"S: want {want}, got {got}, margin {ref.last_margin:.3e} >= 2^-20"
    if not 0 <= got < rec["vocab"]:
        return False, f"got {got} is outside the vocabulary"
    an = analyse(ref)
    if an["nan_row"]:
        return False, f"the row has no finite maximum: only the fall-through to {want} is defensible, got {got}"
    T, u = an["T"], an["u"]
    if not an["admit"][got]:
        if not an["in_big"][got]:
            why = "top-k or every admissible top-p cut removed it"
        elif an["width"][got] <= 0:
            why = "its probability is 0"
        else:
            why = f"u {u:.9g} is {an['dist'][got]:.3e} from its interval [{an['lo'][got]:.9g}, {an['hi'][got]:.9g}], T {T:.3e}"
        return False, f"F: want {want}, got {got}: {why} (tol {an['tol']:.3e}, cuts {an['cuts']})"
    rec["verdict"] = {"dist": float(an["dist"][got]), "T": T, "idx": abs(got - want)}
    if an["width"][got] <= 0 or not an["in_big"][got]:
        return True, f"F: fall-through, u {u:.9g} >= 1 - T ({T:.3e})"
    return True, f"F: u within {an['dist'][got]:.3e} of got's interval, T {T:.3e}"


def admitted(ref) -> np.ndarray:
    """Every token `accepts` would pass for the last call (path F with a finite maximum)."""
    return np.flatnonzero(analyse(ref)["admit"])


def admitted_cap(ref) -> int:
    """2 * ceil(T / smallest kept probability) + 1; the kept set is the one the rule tests membership in (the largest admissible)."""
    an = analyse(ref)
    return 2 * math.ceil(an["T"] / an["pmin"]) + 1
