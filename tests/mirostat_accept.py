"""Per-draw acceptance rule for Mirostat v2 on the device, derived from the restatement (tests/mirostat_ref.py) and the roundings listed at
the top of csrc/kernels_sample.hip alone -- test infrastructure.  No figure in here was tuned on device output.

`judge(rec, u, got, mu_after, words)` decides one call.  `rec` is the record the restatement left when it ran the same row FROM THE MU THE
DEVICE HELD BEFORE THE CALL (read back), so state cannot drift between the two sides; `u` is the f32 of the sampler's next ChaCha20 word (the
caller takes it from the stream at the device's word counter, whether or not the restatement drew); `got`, `mu_after` and `words` (the
word-counter delta) are the device's.

The comparison both sides make.  With g_i = f32(M - x_i) (the same f32 on both sides) and S* = sum_j exp(-g_j) in float64, the exact
quantity is d_i = g_i + ln S* - mu: entry i is removed iff d_i > 0.  The reference evaluates f32(-ln p_i) > mu, the device g_i > f32(mu -
logf(S)).  Their distance from d_i, absolute (BAND_i):
  reference   exp of e_i: 2^-23 (0 for g_i = 0: exp(0) = 1)
              f32(1 / S) and the product: 2^-24 each (0 when S is a power of two: both are exact scalings)
              a subnormal p_i: 2^-150 / p_i
              ln: 2^-23 * |ln p_i| (0 at p_i = 1)
              its sequential f32 S against S*: |ln S_f32 - ln S*|, MEASURED from the record (0 on a row whose sums are exact)
  device      with n_in entries whose e is neither 0 nor 1: expf 2^-23, the quanta n_in * 2^-41 (S >= 1), the f32 of S 2^-24 -- all 0 when
              n_in = 0 (S is then an integer <= 2^20); logf: 2^-23 * |ln S|; the subtraction: 2^-24 * |mu - ln S| (0 when ln S = 0)
On a row with no finite maximum p_i = 1 / n for every id, both sides take the logarithm of the same f32: BAND = 2 * 2^-23 * ln n.
An entry is AMBIGUOUS when |d_i| <= BAND_i, SURE-kept when d_i < -BAND_i.  Where BAND_i is 0 (nothing rounds on either side: a single finite
entry, S = 1) the comparison itself decides, kept iff d_i <= 0: that is what tells `>` from `>=` at a surprise equal to mu.

Fallback decision.  The top entries (g = 0) have the smallest d; everything is removed iff they are.  Decided unless a top entry is
ambiguous.  Decided fallback: `got` must be the restatement's token exactly (the LAST maximum) and `words` 0.  Decided draw: `words` 1.
Undecided: either, each held to its own rule (a draw then kept at least the top entries).

A draw.  The admissible kept sets lie between LOWER = the sure set (with the top entries) and UPPER = LOWER plus the ambiguous entries; the
restatement's own set lies between them too (tests/test_mirostat_ref.py holds it to that).  The interval rule of tests/sampler_accept.py
applies with the restatement's set as the base: D its mass, C the float64 running sums of q = kept e / D, and `got` is accepted iff it is in
UPPER, has mass, and u lies in [C[got-1] - down - tol, C[got] + up + tol], where
  tol = max_i |cum_f32[i] - C[i]| (the restatement's own drift) + sampler_accept.dev_allowance(n_inexact, mass_inexact) (the device's sums
        and its f32 scan of the draw's chunk: the same structure as path F's, so the same allowance),
  eps_hi = (D_hi - D) / D_hi, eps_lo = (D - D_lo) / D_lo from the masses of UPPER and LOWER, and down / up as sampler_accept derives them.
u == 0 gives id 0 whatever its mass; n - 1 is also accepted when u >= 1 - (tol + max(eps_hi, eps_lo)).  With no ambiguous entry and u
farther than tol from both ends of the restatement's interval no other token passes.  A draw is LOOSE when the ambiguous mass exceeds 1e-4 of
the kept mass.

mu_after.  Held to the restatement's update for the device's token from the device's mu_before, evaluated in float64 on the recorded row:
surprise = -ln(e_got / D) for a draw, ln S* for the fallback (ln n on a uniform row), mu' = mu - eta * (surprise - tau).  Tolerance: eta times
the derived error of the device's surprise --
  draw      expf of e_got 2^-23 (0 at g = 0), the kept sum 2^-23 + n_in * 2^-41 + 2^-24 (0 with n_in = 0), the quotient 2^-24 (2^-150 / q more
            when q is subnormal), logf 2^-23 * |surprise|, and ln(D_hi / D_lo) for the set the device may have normalised by
  fallback  the sum as above, logf 2^-23 * |surprise|
-- plus the three f32 roundings of the update itself, 2^-24 * (2 * eta * |surprise - tau| + |mu'|).  Where the surprise is exact by
construction -- tau (the token has no mass in any admissible set), or 0 (a single entry carries all the mass: q = 1, S = 1) -- mu_after must
equal the f32 restatement bit for bit."""
from __future__ import annotations

import math

import numpy as np

import mirostat_ref as mr
import sampler_accept as sa

F = np.float32
LOOSE = 1e-4
R23, R24 = 2.0 ** -23, 2.0 ** -24


def u_of(rng, draws_before: int) -> np.float32:
    """the f32 the sampler's stream gives at word `draws_before`"""
    return F(rng.word(int(draws_before)) >> 8) * F(2.0 ** -24)


def _pow2(v: float) -> bool:
    return v > 0 and math.frexp(v)[0] == 0.5


def analyse(rec: dict) -> dict:
    if "_an" in rec:
        return rec["_an"]
    an: dict = {}
    rec["_an"] = an
    x, n = rec["x"], int(rec["vocab"])
    mu = float(rec["mu_before"])
    M = rec["M"]
    an["uniform"] = uniform = not np.isfinite(M)
    if uniform:
        pu = float(F(F(1) / F(n)))
        s = -math.log(pu)
        w = np.ones(n)
        d = np.full(n, s - mu)
        band = np.full(n, 2 * R23 * abs(s))
        tops = np.ones(n, bool)
        n_in, lnS, dS = 0, s, 0.0  # "S" of the uniform row: n, its surprise ln n
    else:
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            g = (M - x).astype(F).astype(np.float64)  # f32(M - x): what both sides feed to exp / compare
            w = np.where(np.isfinite(g), np.exp(-g), 0.0)
        S = float(w.sum())
        lnS = math.log(S)
        inexact = (w > 0) & (w < 1)
        n_in = int(np.count_nonzero(inexact))
        S32 = float(rec["S"])
        drift = abs(math.log(S32) - lnS)
        dS = (R23 + n_in * 2.0 ** -41 + R24) if n_in else 0.0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            p = rec["p"].astype(np.float64)
            lnp = np.where(p > 0, np.abs(np.log(np.where(p > 0, p, 1.0))), 0.0)
            sub = np.where((p > 0) & (p < 2.0 ** -126), 2.0 ** -150 / np.where(p > 0, p, 1.0), 0.0)
            d = np.where(np.isfinite(g), g + lnS - mu, np.inf)
        band = (np.where(g == 0, 0.0, R23) + (0.0 if _pow2(S32) else 2 * R24) + sub + R23 * lnp + drift  # the reference's side
                + dS + R23 * abs(lnS) + (R24 * abs(mu - lnS) if lnS != 0 else 0.0))  # the device's side
        band = np.where(np.isfinite(g), band, 0.0)
        tops = g == 0
    # with no rounding on either side (BAND_i = 0) the comparison itself decides: kept iff d_i <= 0 (`>` removes)
    sure = (d < -band) | ((band == 0) & (d <= 0))
    amb = (np.abs(d) <= band) & (band > 0) & (w > 0)
    top_amb = bool(np.any(amb & tops))
    top_kept = bool(np.all(sure[tops]))
    an.update(w=w, d=d, band=band, tops=tops, sure=sure, amb=amb, n_in=n_in, lnS=lnS, dS=dS,
              decided=not top_amb, fallback=(not top_kept and not top_amb))
    return an


def _draw(rec: dict, an: dict, u: float) -> dict:
    """the interval rule's arrays for a call that drew; cached"""
    if "draw" in an:
        return an["draw"]
    w, n = an["w"], int(rec["vocab"])
    lower = (an["sure"] | an["tops"]) & (w > 0)
    upper = lower | an["amb"]
    base = rec["kept"] & (w > 0) if not rec["fallback"] else lower
    base_ok = bool(np.all(lower <= base) and np.all(base <= upper))
    D, D_lo, D_hi = float(w[base].sum()), float(w[lower].sum()), float(w[upper].sum())
    q = np.where(base, w, 0.0) / D
    C = np.cumsum(q)
    inexact = (w > 0) & (w < 1) & upper
    dev = sa.dev_allowance(int(np.count_nonzero(inexact)), float(w[inexact].sum() / D))
    drift = float(np.max(np.abs(rec["cum"].astype(np.float64) - C))) if not rec["fallback"] else 0.0
    tol = drift + dev
    eps_hi, eps_lo = (D_hi - D) / D_hi, (D - D_lo) / D_lo
    T = tol + max(eps_hi, eps_lo)
    lo = C - q
    width = np.where(upper, w, 0.0) / D
    hi = lo + width
    down = np.maximum(lo * eps_hi, (1 - lo) * eps_lo)
    up = np.maximum((1 - hi) * eps_hi, hi * eps_lo)
    admit = upper & (width > 0) & (lo - down - tol <= u) & (u <= hi + up + tol)
    if u >= 1.0 - T:
        admit[n - 1] = True
    if u == 0.0:
        admit[0] = True
    if not rec["fallback"]:
        admit[int(rec["token"])] = True
    an["draw"] = dr = dict(lower=lower, upper=upper, base=base, base_ok=base_ok, D=D, D_lo=D_lo, D_hi=D_hi, tol=tol, T=T, lo=lo, hi=hi,
                           admit=admit, loose=(D_hi - D_lo) / D > LOOSE, amb_mass=(D_hi - D_lo) / D)
    return dr


def _mu_check(rec, mu_after, surprise64, tol_s, exact_surprise) -> tuple[bool, str]:
    mu, tau, eta = float(rec["mu_before"]), float(rec["tau"]), float(rec["eta"])
    got = F(mu_after)
    if exact_surprise is not None:
        want = mr.update(rec["mu_before"], rec["tau"], rec["eta"], exact_surprise)
        ok = got.tobytes() == want.tobytes()
        return ok, f"mu_after {got!r}: the surprise is exactly {float(exact_surprise)!r}, so the f32 update {want!r} bit for bit"
    want = mu - eta * (surprise64 - tau)
    tol = eta * tol_s + R24 * (2 * eta * abs(surprise64 - tau) + abs(want)) + 1e-45
    return abs(float(got) - want) <= tol, f"mu_after {float(got)!r} against {want!r}: off by {abs(float(got) - want):.3e}, tolerance {tol:.3e}"


def judge(rec: dict, u, got: int, mu_after, words: int) -> dict:
    """-> dict ok, reason, mode ('fallback' / 'draw'), decided, loose"""
    an = analyse(rec)
    n, got, words = int(rec["vocab"]), int(got), int(words)
    u = float(u)
    out = dict(ok=False, reason="", mode="", decided=an["decided"], loose=False)
    if not 0 <= got < n:
        out["reason"] = f"token {got} outside the vocabulary"
        return out
    if words not in (0, 1):
        out["reason"] = f"{words} words drawn"
        return out
    mode = "draw" if words else "fallback"
    out["mode"] = mode
    if an["decided"] and an["fallback"] != (mode == "fallback"):
        out["reason"] = f"the fallback decision is {'fallback' if an['fallback'] else 'draw'} (top entry {float(an['d'][an['tops']][0]):.3e} from mu, " \
                        f"band {float(an['band'][an['tops']][0]):.3e}), the device drew {words} word(s)"
        return out
    w = an["w"]
    sur_dev_S = an["dS"] + R23 * abs(an["lnS"])
    if mode == "fallback":
        want = mr.argmax_last(rec["x"])
        if got != want:
            out["reason"] = f"fallback: the token is the last maximum {want}, got {got}"
            return out
        if an["uniform"]:
            exact, s64, tol_s = None, an["lnS"], 2 * R23 * abs(an["lnS"])
        else:
            single = int(np.count_nonzero(w > 0)) == 1
            exact, s64, tol_s = (F(0) if single else None), an["lnS"], sur_dev_S
        ok, why = _mu_check(rec, mu_after, s64, tol_s, exact)
        out.update(ok=ok, reason="fallback: " + why)
        return out
    dr = _draw(rec, an, u)
    out["loose"] = bool(dr["loose"])
    if not dr["admit"][got]:
        out["reason"] = (f"draw: got {got}, the restatement {rec['token'] if not rec['fallback'] else 'fell back'}: u {u:.9g} against its interval "
                         f"[{dr['lo'][got]:.9g}, {dr['hi'][got]:.9g}], tol {dr['tol']:.3e}, T {dr['T']:.3e}, in the larger set: {bool(dr['upper'][got])}")
        return out
    # the surprise of the device's token
    in_upper, in_lower = bool(dr["upper"][got]), bool(dr["lower"][got])
    if not in_upper or w[got] == 0:
        ok, why = _mu_check(rec, mu_after, 0.0, 0.0, rec["tau"])  # q_got = 0 in every admissible set: tau
    else:
        q = w[got] / dr["D"]
        s64 = -math.log(q)
        single = int(np.count_nonzero(dr["upper"])) == 1 and w[got] == 1.0
        tol_s = ((0.0 if w[got] == 1.0 else R23) + an["dS"] + R24 + (2.0 ** -150 / q if q < 2.0 ** -126 else 0.0) + R23 * abs(s64)
                 + math.log(dr["D_hi"] / dr["D_lo"]))
        ok, why = _mu_check(rec, mu_after, s64, tol_s, F(0) if single else None)
        if not ok and not in_lower:  # an ambiguous entry reached by u == 0 or the fall-through: the device may have removed it (tau)
            ok, why = _mu_check(rec, mu_after, 0.0, 0.0, rec["tau"])
    out.update(ok=ok, reason="draw: " + why)
    return out
