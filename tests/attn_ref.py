"""float64 model of the prompt attention (kernels_prefill_attn.hip: k_prefill_attn / k_prefill_attn_packed / k_prefill_merge), the inputs that
force its data-dependent paths, the tolerance its results are held to, and a float32 tile-by-tile emulation of its loop (CPU only).

Operands as the kernel makes them (k_prefill_prep, k_extend_prep, the attention kernel's own query path):
  * split-half RoPE at the absolute position, here in float64 on the f32 inputs (the tables are the f32 tables the device reads);
  * q times QMUL = float32(log2 e) * float32(1 / sqrt(128)): the softmax scale and the change to base 2 ride in the query image;
  * q, k and v each rounded to f16 ONCE.  Past keys of a continuation are the cache's values (exact f32, or already f16).
exact(): a float64 base-2 softmax over the visible keys (pos_k <= pos_q; all keys when not causal) times v -> (out, p).

Tolerance per output element (tol()):   2^-10 * sum_j p_j |v_jd|  +  2^-20 * max|v|
  * the probabilities pass through the matrix cores as f16: relative 2^-11 each, so sum_j p_j |v_jd| 2^-11 is the exact bound of that rounding;
    the factor 2 covers the f32 accumulation order, the hardware exp2 and the rare one-ulp difference between f32 and f64 RoPE before
    the f16 rounding of an operand;
  * the second term is an f32 floor for rows whose p is exactly 0 or 1;
  * f16 output rows add half an f16 ulp of the expected value.
It is not fitted to what the kernel gives: a kernel result above it is a finding.

Input families (family()): built as post-RoPE q', k' and rotated back to the f32 inputs (unrope()); v ~ N(0, 1.5).  See FAMILIES.

walk(): the kernel's loop in float32, 64 keys at a time, with the lazily moved reference point (it moves only when a tile's maximum outgrows
it by more than 8, or while it is unset), the optional key split with k_prefill_merge's combination, counters of the paths taken and
fault= switches that seed the mistakes the families exist to catch.
"""
from __future__ import annotations

import zlib

import numpy as np

D = 128
TILE = 64
LOG2E_F32 = np.float32(1.4426950408889634)
SCALE_F32 = np.float32(1.0) / np.sqrt(np.float32(D))
QMUL = np.float32(LOG2E_F32 * SCALE_F32)

FAMILIES = ("gauss", "ramp12", "ramp6", "steep", "fall12", "sunk", "needle")
# what each family forces:
#   gauss   q', k' ~ N(0, 1.5): the reference point is set in the first key tile and almost never moves again
#   ramp12  base-2 score trend 12 j / 64: the reference moves in EVERY tile (l and the 32 output accumulators rescaled by alpha)
#   ramp6   trend 6 j / 64: the reference goes stale (maximum above it, by less than 8), then moves
#   steep   trend min(1, 128 / T) per key: the mass sits on the last few visible keys; a mask or offset slip moves the output wholesale
#   fall12  trend -12 j / 64: the first tile dominates, later probabilities underflow
#   sunk    every real score near -30: a zero-padded key (score 0) would dominate if it were ever left unmasked
#   needle  k'_j = 4 u_j, q'_r = 4 u_t(r) (+-1 codes, t(r) a visible key), v on a 1/64 grid: the output is v_f16[t(r)]; any wrong key, slot
#           permutation, head -> KV head map or image offset shows exactly
FAULTS = ("alpha_l", "alpha_o", "mask", "merge_m")


def seed_of(*parts) -> int:
    """a seed that depends on the case's name only (not on the process: no hash())"""
    return zlib.crc32(repr(parts).encode())


def qmul_of(scale) -> np.float32:
    return np.float32(LOG2E_F32 * np.float32(scale))


def f16(x):
    """one rounding to f16, returned as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def rope(x, pos, sin, cos):
    """split-half RoPE in float64: x [n, heads, D] at positions pos [n]; sin / cos [max_pos, D / 2]"""
    x = np.asarray(x, np.float64)
    s, c = np.asarray(sin, np.float64)[pos][:, None, :], np.asarray(cos, np.float64)[pos][:, None, :]
    x0, x1 = x[..., : D // 2], x[..., D // 2:]
    return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1)


def rope_f32(x, pos, sin, cos, fused):
    """the same rotation in float32, as the device computes it: x0 c - x1 s and x0 s + x1 c, each either two rounded products and a sum or
    (fused) one product folded into a fused multiply-add -- which of the two a compiler emits is its choice.  -> float64 values of the f32 results"""
    x = np.asarray(x, np.float32)
    s, c = np.asarray(sin, np.float32)[pos][:, None, :], np.asarray(cos, np.float32)[pos][:, None, :]
    x0, x1 = x[..., : D // 2], x[..., D // 2:]
    if fused:
        lo = (x0.astype(np.float64) * c - (x1 * s).astype(np.float64)).astype(np.float32)
        hi = (x0.astype(np.float64) * s + (x1 * c).astype(np.float64)).astype(np.float32)
    else:
        lo, hi = x0 * c - x1 * s, x0 * s + x1 * c
    return np.concatenate([lo, hi], axis=-1).astype(np.float64)


def unrope(y, pos, sin, cos):
    """the inverse of rope() for the TABLE's rotation (sin^2 + cos^2 of f32 table entries is 1 only to 1e-7) -> float32 inputs"""
    y = np.asarray(y, np.float64)
    s, c = np.asarray(sin, np.float64)[pos][:, None, :], np.asarray(cos, np.float64)[pos][:, None, :]
    y0, y1 = y[..., : D // 2], y[..., D // 2:]
    n2 = s * s + c * c
    return np.concatenate([(y0 * c + y1 * s) / n2, (y1 * c - y0 * s) / n2], axis=-1).astype(np.float32)


def operands_q(q_in, pos, sin, cos, qmul=QMUL):
    """f32 query rows [n, heads, D] -> the f16 query image (float64 values); sin None: no RoPE (the host drop-in)"""
    q = np.asarray(q_in, np.float32)
    q = rope(q, pos, sin, cos) if sin is not None else q.astype(np.float64)
    return f16(q * np.float64(qmul))


def operands_k(k_in, pos, sin, cos):
    k = np.asarray(k_in, np.float32)
    return f16(rope(k, pos, sin, cos) if sin is not None else k)


def operands_v(v_in):
    return f16(np.asarray(v_in, np.float32))


def visible(pos_q, T, causal=True):
    """[n, T] bool: key j (at position j) is seen by the query at pos_q"""
    pos_q = np.asarray(pos_q)
    return (np.arange(T)[None, :] <= pos_q[:, None]) if causal else np.ones((len(pos_q), T), bool)


def exact(qh, kh, vh, pos_q, causal=True):
    """one head: qh [n, D], kh [T, D], vh [T, D] (the f16 operands as float64), pos_q [n] -> (out [n, D], p [n, T]) in float64"""
    s = qh @ kh.T
    s = np.where(visible(pos_q, kh.shape[0], causal), s, -np.inf)
    p = np.exp2(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return p @ vh, p


def tol(p, vh, want=None, out_f16=False):
    """[n, D]: the tolerance of one head's rows (module docstring); want: the expected rows, for f16 output rows"""
    t = 2.0 ** -10 * (p @ np.abs(vh)) + 2.0 ** -20 * np.max(np.abs(vh))
    if out_f16:
        t = t + 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    return t


def model(qh, kh, vh, pos_q, causal=True, out_f16=False):
    """all heads: qh [n, heads, D], kh / vh [T, kv, D] (f16 operands) -> (want [n, heads, D], tol [n, heads, D], p [heads, n, T])"""
    n, n_heads, _ = qh.shape
    group = n_heads // kh.shape[1]
    want, tl, ps = np.zeros((n, n_heads, D)), np.zeros((n, n_heads, D)), []
    for h in range(n_heads):
        o, p = exact(qh[:, h], kh[:, h // group], vh[:, h // group], pos_q, causal)
        want[:, h], tl[:, h] = o, tol(p, vh[:, h // group], o, out_f16)
        ps.append(p)
    return want, tl, np.stack(ps)


def scores(qh, kh, pos_q, causal=True):
    """base-2 scores of the visible (query, key) pairs of all heads, flat"""
    n_heads, group = qh.shape[1], qh.shape[1] // kh.shape[1]
    vis = visible(pos_q, kh.shape[0], causal)
    return np.concatenate([(qh[:, h] @ kh[:, h // group].T)[vis] for h in range(n_heads)])


# ---- the input families --------------------------------------------------------------------------------------------------------
def trend_of(name, T):
    """base-2 score trend over the key index of the ramp families"""
    j = np.arange(T, dtype=np.float64)
    if name == "ramp12":
        return 12.0 * j / TILE
    if name == "ramp6":
        return 6.0 * j / TILE
    if name == "fall12":
        return -12.0 * j / TILE
    if name == "steep":  # centred: |trend| <= 64 at any T
        return min(1.0, 128.0 / T) * (j - 0.5 * (T - 1))
    if name == "sunk":
        return np.full(T, -30.0)
    raise KeyError(name)


def family(name, rng, pos_q, T, n_heads, n_kv, causal=True):
    """-> (q' [n, heads, D], k' [T, kv, D], v [T, kv, D], needle target [n, heads] or None), post-RoPE, float64.  Key j sits at position j."""
    pos_q = np.asarray(pos_q)
    n, group = len(pos_q), n_heads // n_kv
    v = rng.normal(0, 1.5, (T, n_kv, D))
    if name == "gauss":
        return rng.normal(0, 1.5, (n, n_heads, D)), rng.normal(0, 1.5, (T, n_kv, D)), v, None
    if name == "needle":
        u = rng.choice([-1.0, 1.0], (T, n_kv, D))
        hi = np.where(causal, np.minimum(pos_q, T - 1), T - 1)
        t = rng.integers(0, hi[:, None] + 1, (n, n_heads))
        q = np.stack([4.0 * u[t[:, h], h // group] for h in range(n_heads)], axis=1)
        return q, 4.0 * u, np.round(v * 64.0) / 64.0, t
    # k'_j = n_j + b(j) w, q'_r = n_r + a w with q'_r . w = a exactly (the query's noise has no component along w): the base-2 score is
    # QMUL (n_r . n_j + a w . n_j) + trend(j), noise of sd ~0.5 around the trend.
    # The device rotates in f32, the model in f64: now and then (about 2e-4 of the elements) the two round an operand to different f16
    # neighbours, and that one element moves one score by q_d ulp16(k_d).  On a row whose mass sits on one or two keys this reaches the
    # output undiluted, so the construction keeps every such product small: w has equal components +-1/sqrt(128) (no dimension carries
    # more than 1/128 of the trend), the noise has sd 0.25, and a = 16 splits the trend's 64 at the ends of `steep` into query
    # components of QMUL (1.41 +- 0.9) <= 0.3 and key components of 2.8 +- 0.9 < 4 (f16 ulp 2^-9): one disagreement moves a score by
    # at most 6e-4 = 0.6 * 2^-10.  (With a = 8, Gaussian w and unit noise keys reached 18 and ONE disagreement cost 0.9 of the tolerance.)
    a, sd = 16.0, 0.25
    w = rng.choice([-1.0, 1.0], (n_kv, D)) / np.sqrt(D)
    b = trend_of(name, T) / (a * float(QMUL))
    k = rng.normal(0, sd, (T, n_kv, D)) + b[:, None, None] * w[None]
    q = rng.normal(0, sd, (n, n_heads, D))
    wq = w[np.arange(n_heads) // group]
    q = q - (q * wq[None]).sum(-1, keepdims=True) * wq[None] + a * wq[None]
    return q, k, v, None


# ---- the kernel's loop in float32 ----------------------------------------------------------------------------------------------
def _exp2(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(x.astype(np.float32)).astype(np.float32)


def walk(qh, kh, vh, pos_q, causal=True, parts=1, split_tiles=1, qg=TILE, fault=None):
    """One head in float32, as prefill_attn_body walks it.  qh [n, D], kh / vh [T, D]: the f16 operands; pos_q [n].  Rows are handled in
    workgroups of qg consecutive rows (the kernel's 32 / 64 / 128): a workgroup's last key tile is the last one any of its rows sees, and with
    parts > 1 (PrefillArgs::ksplit) its n_t tiles are cut into min(ceil(n_t / split_tiles), parts) shares of ceil(n_t / shares) tiles, each
    leaving a partial (o, m, l) that the merge combines; shares past the count only leave the mark m = -inf, as does a share whose tile range
    is empty.  fault: None | 'alpha_l' (l not rescaled) | 'alpha_o' (o not rescaled) | 'mask' (one key too many) | 'merge_m' (the merge
    ignores m).  -> (out [n, D] float64, counters {grow_mid, stale, unset_mid, tiles})"""
    assert fault in (None,) + FAULTS
    pos_q = np.asarray(pos_q)
    n, T = qh.shape[0], kh.shape[0]
    Tpad = (T + TILE - 1) // TILE * TILE
    k32, v32 = np.zeros((Tpad, D), np.float32), np.zeros((Tpad, D), np.float32)  # the images are zero-padded to whole tiles
    k32[:T], v32[:T] = kh, vh
    q32 = np.asarray(qh, np.float32)
    qlim = (pos_q if causal else np.full(n, T - 1)) + (1 if fault == "mask" else 0)
    out = np.zeros((n, D))
    cnt = dict(grow_mid=0, stale=0, unset_mid=0, tiles=0)
    NEG = np.float32(-np.inf)
    for r0 in range(0, n, qg):
        rows = slice(r0, min(r0 + qg, n))
        nr = rows.stop - rows.start
        top = int(pos_q[rows].max())
        n_t = ((min(top, T - 1) if causal else T - 1) // TILE) + 1
        shares = min((n_t + split_tiles - 1) // split_tiles, parts) if parts > 1 else 1
        per = (n_t + shares - 1) // shares
        partials = []
        for z in range(max(parts, 1)):
            first, last = z * per, min(z * per + per - 1, n_t - 1)
            if z >= shares or first > last:
                partials.append((np.zeros((nr, D), np.float32), np.full(nr, NEG), np.zeros(nr, np.float32)))
                continue
            m = np.full(nr, NEG)
            l = np.zeros(nr, np.float32)
            o = np.zeros((nr, D), np.float32)
            for kt in range(first, last + 1):
                kk, vv = k32[kt * TILE:(kt + 1) * TILE], v32[kt * TILE:(kt + 1) * TILE]
                unset = m < np.float32(-1.0e30)
                m_init = np.where(unset, np.float32(0), m).astype(np.float32)
                s = (q32.astype(np.float64)[rows] @ kk.astype(np.float64).T).astype(np.float32) - m_init[:, None]
                seen = (kt * TILE + np.arange(TILE))[None, :] <= qlim[rows][:, None]
                s = np.where(seen, s, NEG).astype(np.float32)
                mt = s.max(axis=1)
                grow = (mt > np.float32(8)) | unset
                shift = np.where(grow, np.maximum(mt, np.float32(-3.0e38)), np.float32(0)).astype(np.float32)
                with np.errstate(invalid="ignore", over="ignore"):  # (unset rows: -inf or -3e38 on the side np.where drops)
                    m_new = np.where(unset, shift, m + shift).astype(np.float32)
                    alpha = _exp2(m - m_new)
                alpha = np.where(np.isnan(alpha), np.float32(0), alpha)  # (-inf) - (-3e38): 2^-inf
                if fault != "alpha_l":
                    l = l * alpha
                if fault != "alpha_o":
                    o = o * alpha[:, None]
                m = m_new
                p = _exp2(s - shift[:, None])
                l = (l + p.sum(axis=1, dtype=np.float32)).astype(np.float32)
                p16 = p.astype(np.float16).astype(np.float32)
                o = (o + (p16.astype(np.float64) @ vv.astype(np.float64)).astype(np.float32)).astype(np.float32)
                live = seen.any(axis=1)
                cnt["tiles"] += int(live.sum())
                cnt["grow_mid"] += int((grow & ~unset & live).sum())
                cnt["stale"] += int((~grow & (mt > 0) & live).sum())
                cnt["unset_mid"] += int((unset & (kt > first)).sum())
            partials.append((o, m, l))
        if parts <= 1:
            o, m, l = partials[0]
            out[rows] = o.astype(np.float64) / l.astype(np.float64)[:, None]
            continue
        M = np.max(np.stack([pm for _, pm, _ in partials]), axis=0)
        L, acc = np.zeros(nr, np.float32), np.zeros((nr, D), np.float32)
        for o, m, l in partials:
            on = m != NEG
            with np.errstate(invalid="ignore"):
                wgt = np.ones(nr, np.float32) if fault == "merge_m" else _exp2(m - M)
            wgt = np.where(on, wgt, np.float32(0)).astype(np.float32)
            L = L + wgt * l
            acc = acc + wgt[:, None] * o
        out[rows] = acc.astype(np.float64) / L.astype(np.float64)[:, None]
    return out, cnt
