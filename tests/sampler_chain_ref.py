"""numpy restatement of the sampler chain: the CLI sampler of tests/sampler_ref.py with the additive penalties, min-p and typical-p of
the reference's serving front ends around it -- test infrastructure.

The rules are the reference's, in f32 and in its order:
  additive penalties   crates/bitnet-sampling/src/strategies.rs `RepetitionPenaltyConfig::apply` :247-259 (two separate operations)
  min-p                crates/bitnet-logits/src/lib.rs `apply_min_p` :299-310, clamped as `MinPSampler::new`
  typical-p            crates/bitnet-logits/src/lib.rs `apply_typical` :337-381, clamped as `TypicalSampler::new`; the reference sorts
                       unstably, the library fixes equal deviations to ascending token id, and so does this file
The chain works in the CLI sampler's form: a stage removes entries by setting them to -inf and the next stage sees the softmax of the
survivors.  Order: counts, additive penalties, repetition penalty, NaN -> -inf, greedy shortcut, temperature, top-k, top-p, min-p,
typical-p, softmax, draw.  The occurrence count of the additive penalties is the count of the token in the list of the call at hand
(which, for a caller that passes the growing list, is how often the token was chosen so far); the repetition penalty keeps the
compounding exponent of `RefSampler`.

`ChainRef.sample` leaves the record of `RefSampler.sample` in `last` (same keys, so tests/sampler_accept.py reads it), plus: xp (the
logits after top-p), minp (None, or dict p, thr, keep), typ (None, or dict idx, p, d, order, cum, cutoff, keep)."""
from __future__ import annotations

import collections

import numpy as np

import sampler_ref as sr


def min_p_keep(probs: np.ndarray, min_p) -> tuple[np.ndarray, np.float32]:
    """`apply_min_p` on a probability slice -> (kept mask, threshold).  NaN compares false: kept."""
    p = np.asarray(probs, np.float32)
    mp = np.float32(min_p)
    if mp <= 0 or p.size == 0:
        return np.ones(p.size, bool), np.float32(0)
    with np.errstate(invalid="ignore"):
        pmax = np.float32(0)
        if np.any(p == p):
            pmax = np.float32(max(np.float32(0), np.nanmax(p)))  # fold(0.0, f32::max): NaN is ignored
        thr = np.float32(mp * pmax)
        return ~(p < thr), thr


def typical_keep(probs: np.ndarray, typical_p) -> dict | None:
    """`apply_typical` on a probability slice.  None when the stage is a no-op (typical_p >= 1, empty, nothing with p > 0); else a dict:
    idx (the entries with p > 0, ascending id), p, d (their deviations), order (positions in idx, ascending d then id), cum (f32 running sums
    in that order), cutoff, keep (mask over the slice: the entries the stage leaves non-zero)."""
    p = np.asarray(probs, np.float32)
    ty = np.float32(typical_p)
    if ty >= 1 or p.size == 0:
        return None
    with np.errstate(invalid="ignore", divide="ignore"):
        idx = np.flatnonzero(p > 0)
        if idx.size == 0:
            return None
        pi = p[idx]
        lnp = np.log(pi).astype(np.float32)
        terms = ((-pi) * lnp).astype(np.float32)
        H = np.add.accumulate(terms, dtype=np.float32)[-1]
        d = np.abs(((-lnp) - H).astype(np.float32))
    order = np.argsort(d, kind="stable")  # idx ascends, so ties go by ascending id
    cum = np.add.accumulate(pi[order], dtype=np.float32)
    over = np.flatnonzero(cum >= ty)
    cutoff = int(over[0]) + 1 if over.size else idx.size
    keep = np.zeros(p.size, bool)
    keep[idx[order[:cutoff]]] = True
    return dict(idx=idx, p=pi, d=d, H=H, order=order, cum=cum, cutoff=cutoff, keep=keep)


def additive(logits: np.ndarray, token_counts, frequency_penalty, presence_penalty) -> np.ndarray:
    """`RepetitionPenaltyConfig::apply` with count_penalty 1: x -= f * count, then x -= p, for every (token, count) with count > 0."""
    x = np.array(logits, np.float32)
    f, p = np.float32(frequency_penalty), np.float32(presence_penalty)
    with np.errstate(invalid="ignore", over="ignore"):
        for tok, c in token_counts:
            if tok >= x.size or c == 0:
                continue
            x[tok] = np.float32(x[tok] - np.float32(f * np.float32(c)))
            x[tok] = np.float32(x[tok] - p)
    return x


class ChainRef(sr.RefSampler):
    def __init__(self, temperature, top_k, top_p, repetition_penalty, seed=0, key=None, min_p=0.0, typical_p=1.0, frequency_penalty=0.0,
                 presence_penalty=0.0):
        super().__init__(temperature, top_k, top_p, repetition_penalty, seed, key)
        self.mp = np.float32(min(max(float(min_p), 0.0), 1.0))
        self.ty = np.float32(min(max(float(typical_p), 0.0), 1.0))
        self.fp, self.pp = np.float32(frequency_penalty), np.float32(presence_penalty)

    def is_greedy(self) -> bool:
        return bool(self.t == 0 or (self.t == 1 and self.k == 0 and self.p == 1 and self.mp <= 0 and self.ty >= 1))

    def exponent(self, tok: int) -> int:
        return self.counts.get(tok, 0)

    def sample(self, logits, generated) -> int:
        for g in generated:
            self.counts[int(g)] = self.counts.get(int(g), 0) + 1
        x = np.array(logits, np.float32)
        if self.fp != 0 or self.pp != 0:
            occ = collections.Counter(int(g) for g in generated)
            x = additive(x, sorted(occ.items()), self.fp, self.pp)
        x = self.penalise(x)
        x[np.isnan(x)] = -np.inf
        self.last_margin = np.inf
        self.last = rec = {"vocab": x.size}
        if self.is_greedy():
            self.last_path = "G"
            rec["want"] = sr.argmax(x)
            return rec["want"]
        self.last_path = "S" if 0 < self.k <= sr.SMALL_K and self.k < x.size else "F"
        ninf = np.float32(-np.inf)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.t != 1:
                x = (x / self.t).astype(np.float32)
            rec["xt"] = x
            if 0 < self.k < x.size:
                order = sr.stable_desc(np.where(np.isnan(x), -np.inf, x))
                f = np.full_like(x, -np.inf)
                f[order[: self.k]] = x[order[: self.k]]
                x = f
            rec["xk"] = x
            rec["order"] = rec["cum_sorted"] = rec["cut"] = None
            if self.p < 1:
                x = np.where(np.isnan(x), ninf, x).astype(np.float32)
                order = sr.stable_desc(x)
                cum = np.add.accumulate(sr.softmax(x)[order], dtype=np.float32)
                over = np.flatnonzero(cum > self.p)
                cut = int(over[0]) + 1 if over.size else x.size
                rec["order"], rec["cum_sorted"], rec["cut"] = order, cum, cut
                if over.size:
                    i = int(over[0])
                    lo = cum[i - 1] if i > 0 else np.float32(0)
                    self.last_margin = min(self.last_margin, float(cum[i]) - float(self.p), float(self.p) - float(lo))
                f = np.full_like(x, -np.inf)
                f[order[:cut]] = x[order[:cut]]
                x = f
            rec["xp"] = x
            rec["minp"] = rec["typ"] = None
            finite = bool(x.size) and bool(np.isfinite(np.max(x)))  # no finite maximum: every probability is NaN, both stages are no-ops
            if self.mp > 0 and finite:
                p = sr.softmax(x)
                keep, thr = min_p_keep(p, self.mp)
                rec["minp"] = dict(p=p, thr=thr, keep=keep)
                # an entry tied at the maximum has p == max p bit for bit on either side (exp(0) = 1 over one denominator), and
                # min_p <= 1: its comparison cannot flip
                live = (p > 0) & (p != np.max(p))
                if live.any():
                    self.last_margin = min(self.last_margin, float(np.min(np.abs(p[live].astype(np.float64) - float(thr)))))
                x = np.where(keep, x, ninf).astype(np.float32)
            if self.ty < 1 and finite:
                t = typical_keep(sr.softmax(x), self.ty)
                if t is not None:
                    rec["typ"] = t
                    c, cum, d, o = t["cutoff"], t["cum"], t["d"], t["order"]
                    # survivors of one value: one probability, one deviation, the order is the id order and the running sums add the
                    # same f32 value in the same order on either side, so nothing can flip and the stage adds no margin
                    exact = bool(np.all(t["p"] == t["p"][0]))
                    if not exact and cum[c - 1] >= self.ty:
                        lo = cum[c - 2] if c > 1 else np.float32(0)
                        self.last_margin = min(self.last_margin, float(cum[c - 1]) - float(self.ty), float(self.ty) - float(lo))
                    if c < o.size and not exact:  # the first entry left out against the last one taken
                        self.last_margin = min(self.last_margin, float(d[o[c]]) - float(d[o[c - 1]]))
                    x = np.where(t["keep"], x, ninf).astype(np.float32)
            probs = sr.softmax(x)
            u = self.rng.random_f32()
            cum = np.add.accumulate(probs, dtype=np.float32)
            rec["xf"], rec["u"], rec["probs"], rec["cum"] = x, u, probs, cum
            over = np.flatnonzero(cum > u)
            if not over.size:
                if np.isfinite(cum[-1]):
                    self.last_margin = min(self.last_margin, float(u) - float(cum[-1]))
                rec["want"] = x.size - 1
                return x.size - 1
            i = int(over[0])
            lo = cum[i - 1] if i > 0 else np.float32(0)
            self.last_margin = min(self.last_margin, float(cum[i]) - float(u), float(u) - float(lo))
            rec["want"] = i
            return i
