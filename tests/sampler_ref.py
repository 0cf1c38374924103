"""numpy restatement of the reference's sampler (crates/bitnet-cli/src/sampling.rs `Sampler::sample`) -- test infrastructure.

Every step is float32 in the reference's order: sequential sums are `np.add.accumulate` (one rounding per term, index
order), the sorts are stable and compare -0.0 equal to +0.0 as `partial_cmp` does.  The RNG is `ChaCha20Rng::seed_from_u64`
(rand_core 0.9 PCG32 seed expansion, rand_chacha 0.9 keystream: 64-bit block counter from 0, zero nonce) and
`rng.random::<f32>()` = (next_u32 >> 8) * 2^-24 (rand 0.9).  The keystream is pinned by a published test vector; the seed
expansion and the f32 conversion are restated from the crates' sources and have not been run against a Rust build.

`RefSampler.sample` also reports how close the deciding comparisons came to flipping (`last_margin`), and keeps what the call
decided in `last` (the tempered logits, the kept set after top-k, the top-p cut and its f32 sums, `u`, the f32 sums of the draw),
so that tests of the device's parallel-sum paths can tell a real mismatch from a rounding tie: tests/sampler_accept.py derives a
per-draw acceptance rule from that record."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def _rotl(x: int, n: int) -> int:
    return ((x << n) | (x >> (32 - n))) & M32


def chacha20_block(key: list[int], counter: int, nonce: tuple[int, int] = (0, 0)) -> list[int]:
    """One 64-byte ChaCha20 block as 16 little-endian words (rand_chacha layout: words 12-13 = 64-bit counter)."""
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *key, counter & M32, (counter >> 32) & M32, nonce[0], nonce[1]]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(x[i] + s[i]) & M32 for i in range(16)]


def pcg32_key(seed: int) -> list[int]:
    """rand_core 0.9 `SeedableRng::seed_from_u64`: eight PCG32 outputs, little-endian into the 32-byte seed."""
    state = seed & M64
    out = []
    for _ in range(8):
        state = (state * 6364136223846793005 + 11634580027462260723) & M64
        xs = ((((state >> 18) ^ state) >> 27)) & M32
        rot = state >> 59
        out.append(((xs >> rot) | (xs << ((32 - rot) & 31))) & M32)
    return out


class ChaCha20Rng:
    def __init__(self, seed: int | None = None, key: list[int] | None = None):
        self.key = list(key) if key is not None else pcg32_key(seed or 0)
        self.draws = 0
        self._blk = -1
        self._words: list[int] = []

    def word(self, n: int) -> int:
        b = n // 16
        if b != self._blk:
            self._blk, self._words = b, chacha20_block(self.key, b)
        return self._words[n % 16]

    def next_u32(self) -> int:
        w = self.word(self.draws)
        self.draws += 1
        return w

    def random_f32(self) -> np.float32:
        return np.float32(self.next_u32() >> 8) * np.float32(2.0 ** -24)


def powi(a: np.float32, b: int) -> np.float32:
    """compiler-builtins `__powisf2` (what `f32::powi` with a run-time exponent lowers to), b >= 0."""
    a = np.float32(a)
    r = np.float32(1.0)
    with np.errstate(over="ignore", under="ignore"):
        while True:
            if b & 1:
                r = np.float32(r * a)
            b //= 2
            if b == 0:
                break
            a = np.float32(a * a)
    return r


def count_exponent(generated: list[int], token: int) -> int:
    """Closed form of the count a call sees after the caller passed the growing list on every earlier call:
    at call c (the list holds g_0..g_{c-1}) token t has been added sum_{i<c, g_i=t} (c - i) times."""
    c = len(generated)
    return sum(c - i for i, g in enumerate(generated) if g == token)


def argmax(x: np.ndarray) -> int:
    """sampling.rs argmax: lowest index on ties, all -inf -> 0."""
    x = np.asarray(x, np.float32)
    m = x.max() if x.size else -np.inf
    if m == -np.inf:
        return 0
    return int(np.flatnonzero(x == m)[0])


def softmax(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.float32(np.max(x)) if x.size else np.float32(-np.inf)  # fold(NEG_INFINITY, f32::max)
        e = np.exp((x - mx).astype(np.float32)).astype(np.float32)
        s = np.add.accumulate(e, dtype=np.float32)[-1] if e.size else np.float32(0)
        return (e / s).astype(np.float32)


def stable_desc(x: np.ndarray) -> np.ndarray:
    """indices in `sort_by(|a, b| b.partial_cmp(a))` order: stable, -0.0 == +0.0."""
    return np.argsort(-np.asarray(x, np.float32), kind="stable")


class RefSampler:
    """`Sampler::new(temperature, top_k, top_p, repetition_penalty, Some(seed))`."""

    def __init__(self, temperature: float, top_k: int, top_p: float, repetition_penalty: float, seed: int = 0, key=None):
        self.t = np.float32(temperature)
        self.k = int(top_k)
        self.p = np.float32(top_p)
        self.rp = np.float32(repetition_penalty)
        self.rng = ChaCha20Rng(seed, key)
        self.counts: dict[int, int] = {}
        self.last_margin = np.inf  # smallest |cumsum - threshold| among the deciding comparisons of the last call
        self.last_path = ""
        self.last: dict = {}  # what the last call decided (see sample)

    def is_greedy(self) -> bool:
        return self.t == 0 or (self.t == 1 and self.k == 0 and self.p == 1)

    def penalise(self, logits: np.ndarray) -> np.ndarray:
        x = np.array(logits, np.float32)
        if self.rp == 1:
            return x
        with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
            for tok, cnt in self.counts.items():
                if tok < x.size and cnt > 0:
                    pen = powi(self.rp, cnt)
                    x[tok] = np.float32(x[tok] / pen) if x[tok] > 0 else np.float32(x[tok] * pen)
        return x

    def sample(self, logits, generated) -> int:
        for g in generated:
            self.counts[int(g)] = self.counts.get(int(g), 0) + 1
        x = self.penalise(logits)
        x[np.isnan(x)] = -np.inf
        self.last_margin = np.inf
        # `last`: vocab, want; and past the greedy shortcut: xt (tempered logits after penalty and NaN handling), xk (after top-k:
        # removed entries are -inf), order / cum_sorted / cut (top-p: stable descending order of xk, the f32 sums over it, entries
        # kept; None when top_p >= 1), xf (the logits the final softmax saw), u, probs and cum (f32, index order)
        self.last = rec = {"vocab": x.size}
        if self.is_greedy():
            self.last_path = "G"
            rec["want"] = argmax(x)
            return rec["want"]
        self.last_path = "S" if 0 < self.k <= SMALL_K and self.k < x.size else "F"
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.t != 1:
                x = (x / self.t).astype(np.float32)
            rec["xt"] = x
            if 0 < self.k < x.size:
                order = stable_desc(np.where(np.isnan(x), -np.inf, x))
                f = np.full_like(x, -np.inf)
                f[order[: self.k]] = x[order[: self.k]]
                x = f
            rec["xk"] = x
            rec["order"] = rec["cum_sorted"] = rec["cut"] = None
            if self.p < 1:
                x = np.where(np.isnan(x), np.float32(-np.inf), x).astype(np.float32)
                order = stable_desc(x)
                cum = np.add.accumulate(softmax(x)[order], dtype=np.float32)
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
            probs = softmax(x)
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


# the device's small-k bound (include/bitnet_hip.h BITNET_HIP_SAMPLE_SMALL_K); only labels paths here
SMALL_K = 64
