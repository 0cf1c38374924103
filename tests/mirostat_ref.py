"""numpy restatement of Mirostat v2 (crates/bitnet-sampling/src/strategies.rs `MirostatSampler::sample` :131-190 over
crates/bitnet-logits/src/lib.rs `softmax_in_place` :180-213) -- test infrastructure.

Every step is float32 in the reference's order; sequential sums are `np.add.accumulate` (one rounding per term, index order).  The front
stages (counts, additive penalties, repetition penalty, NaN -> -inf, temperature) and the RNG are `sampler_chain_ref.ChainRef`'s, which sits on
`sampler_ref.RefSampler`: the library draws u from the sampler's one ChaCha20 stream (the reference's type is ChaCha8Rng).

  1. p = softmax_in_place(x): M = fold(-inf, max); an entry equal to -inf gives 0, the others exp(x_i - M); S their sum in index order;
     S > 0: p_i = e_i * (1 / S), else every p_i = 1 / n (every row with no finite maximum: a +inf makes S NaN, and NaN > 0 is false)
  2. an entry with p_i > 0 and -ln(p_i) > mu becomes 0
  3. sum2 = the sum of what is left
  4. sum2 <= 0: the fallback, no random word: token = the LAST maximum of x (max_by), surprise = -ln(p_token) of the unfiltered p or tau if
     that is 0
  5. else q_i = p_i * (1 / sum2), u one random f32, the token is the first i with u <= the running f32 sum, n - 1 if none
  6. surprise = -ln(q_token) if q_token > 0 else tau (draw); mu -= eta * (surprise - tau), two f32 operations

`mirostat(x, mu, tau, eta, rng)` is the six steps on a tempered row and returns the record of the call: x, M, e, S, uniform, p, kept, sum2,
fallback, q, cum (the f32 running sums), u, token, surprise, mu_before, mu_after, words (random words drawn: 0 or 1).  `MirostatRef` puts the
front stages in front; `mu` is a plain attribute, so a test starts a call from any state."""
from __future__ import annotations

import numpy as np

import sampler_chain_ref as scr

F = np.float32


def softmax_in_place(x: np.ndarray) -> dict:
    """lib.rs:180-213 -> dict M, e, S, uniform, p (all f32)"""
    x = np.asarray(x, F)
    n = x.size
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = x[~np.isnan(x)]  # f32::max ignores NaN
        M = F(v.max()) if v.size else F(-np.inf)
        e = np.where(x == F(-np.inf), F(0), np.exp((x - M).astype(F)).astype(F)).astype(F)
        S = np.add.accumulate(e, dtype=F)[-1] if n else F(0)
        if S > 0:
            inv = F(F(1) / S)
            return dict(M=M, e=e, S=S, uniform=False, p=(e * inv).astype(F))
        return dict(M=M, e=e, S=S, uniform=True, p=np.full(n, F(F(1) / F(n)), F))


def argmax_last(x: np.ndarray) -> int:
    """the reference's argmax of the fallback: max_by keeps the LAST of equal maxima"""
    x = np.asarray(x, F)
    return int(np.flatnonzero(x == x.max())[-1])


def update(mu, tau, eta, surprise) -> np.float32:
    """mu -= eta * (surprise - tau): separate f32 operations"""
    with np.errstate(over="ignore", invalid="ignore"):
        return F(F(mu) - F(F(eta) * F(F(surprise) - F(tau))))


def mirostat(x, mu, tau, eta, rng) -> dict:
    x = np.asarray(x, F)
    n = x.size
    mu, tau, eta = F(mu), F(tau), F(eta)
    rec = softmax_in_place(x)
    p = rec["p"]
    with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
        s = (-np.log(p)).astype(F)  # f32 ln
        removed = (p > 0) & (s > mu)
        left = np.where(removed, F(0), p).astype(F)
        sum2 = np.add.accumulate(left, dtype=F)[-1]
        rec.update(x=x, surprises=s, kept=~removed & (p > 0), sum2=sum2, mu_before=mu, tau=tau, eta=eta, vocab=n)
        if sum2 <= 0:
            tok = argmax_last(x)
            pt = p[tok]
            sur = F(-np.log(pt)) if pt > 0 else tau
            rec.update(fallback=True, q=None, cum=None, u=None, words=0, token=tok, surprise=sur, mu_after=update(mu, tau, eta, sur))
            return rec
        q = (left * F(F(1) / sum2)).astype(F)
        u = rng.random_f32()
        cum = np.add.accumulate(q, dtype=F)
        hit = np.flatnonzero(u <= cum)
        tok = int(hit[0]) if hit.size else n - 1
        sur = F(-np.log(q[tok])) if q[tok] > 0 else tau
        rec.update(fallback=False, q=q, cum=cum, u=u, words=1, token=tok, surprise=sur, mu_after=update(mu, tau, eta, sur))
        return rec


class MirostatRef(scr.ChainRef):
    """`MirostatSampler::new(tau, eta, Some(seed))` behind the chain's front stages (penalties, NaN -> -inf, temperature)."""

    def __init__(self, tau, eta, seed=0, key=None, temperature=1.0, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0):
        super().__init__(temperature, 0, 1.0, repetition_penalty, seed, key, frequency_penalty=frequency_penalty, presence_penalty=presence_penalty)
        self.tau, self.eta = F(tau), F(eta)
        self.mu = F(F(2) * self.tau)
        self.fallbacks = 0

    def reset(self) -> None:
        """MirostatSampler::reset :192-195 (the library's reset also clears the counts and the word counter)"""
        self.mu = F(F(2) * self.tau)
        self.fallbacks = 0

    def front(self, logits, generated) -> np.ndarray:
        """counts, additive penalties, repetition penalty, NaN -> -inf, temperature: the row Mirostat sees"""
        import collections

        for g in generated:
            self.counts[int(g)] = self.counts.get(int(g), 0) + 1
        x = np.array(logits, F)
        if self.fp != 0 or self.pp != 0:
            occ = collections.Counter(int(g) for g in generated)
            x = scr.additive(x, sorted(occ.items()), self.fp, self.pp)
        x = self.penalise(x)
        x[np.isnan(x)] = -np.inf
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.t != 1:
                x = (x / self.t).astype(F)
        return x

    def sample(self, logits, generated, mu=None) -> int:
        """One call; `mu` (default: the state) is where it starts from.  The record stays in `last`."""
        x = self.front(logits, generated)
        rec = mirostat(x, self.mu if mu is None else mu, self.tau, self.eta, self.rng)
        self.last = rec
        self.mu = rec["mu_after"]
        self.fallbacks += int(rec["fallback"])
        return rec["token"]
