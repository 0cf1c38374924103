"""float64 model of the one-token decode attention (kernels_attn.hip: k_attn_partial<NH, KV16> / k_attn_partial_batch / k_attn_partial_rows and the
three k_attn_combine forms), the inputs that force its data-dependent paths, the tolerance its results are held to, and a float32 emulation of
its chunk algorithm with seeded faults (CPU only).

Operands as the kernel defines them (exact()):
  * split-half RoPE at `pos` on the f32 query rows and on the new key, here in float64 with the f32 tables the device reads;
  * past keys and values are the cache's own values (f32, or f16 converted exactly); under KV_F16 the new key and value are rounded ONCE to f16;
  * scale 1 / sqrt(128); head h reads KV head h // group.
exact() -> out, the probabilities p, the scores s and, for records of 64 and of 128 positions, the triples (m_c, l_c, o_c): the record's score
maximum, sum_j exp(s_j - m_c) and sum_j exp(s_j - m_c) v_j (un-normalised, relative to the record's OWN maximum) -- what k_attn_partial leaves in
`scratch`.

Tolerance per output element (tol()), derived, not fitted to what the kernel gives -- a kernel result above it is a finding:
    tol_d = sum_j p_j ds_j |v_jd - out_d|  +  2^-22 sum_j p_j |v_jd|  +  2^-23 |out_d|
  * a score error ds_j moves out_d by sum_j p_j ds_j (v_jd - out_d) (first order; ds is 1e-3 at the very most);
  * ds_j = 2^-24 (24 scale sum_d |q'_d k'_jd| + 4 |s_j|).  The 24 counts f32 roundings against the products' absolute sum (attn_partial_body):
    the 16-long FMA chain of one wave's partial sum (two chains per wave, even and odd dims), the adds that join the eight chains (the chain
    pair, then ((w0 + w1) + w2) + w3) and the three roundings of f32 RoPE (two products, one sum) on each operand.  Counted by depth, the
    deepest product passes 16 + 1 + 3 = 20 roundings of the sum and 3 + 3 of RoPE, 26 in all, but only two of the 128 products sit that deep: the
    mean depth is 8.5 + 1 + 2.25 + 6 = 17.75.  24 is kept: it is the smaller number, and a bound in which every rounding falls the same way is
    far from what f32 gives (walk() stays below a tenth of it).  4 |s_j| covers the f32 scale constant, the multiplication by it, the
    subtraction of the maximum and the argument of expf;
  * 2^-22 sum_j p_j |v_jd| covers expf, the accumulation of l and o (chains of 16, the class sums, enew * v), the 128-position half merge
    (__expf) and the online merge steps of the combine; 2^-23 |out_d| the division and the stored rounding;
  * KV_F16: the new token's key adds 2^-11 scale sum_d |q'_d k'_d| to its own ds -- hipcc may contract the RoPE expression into an FMA, and the
    key's f16 rounding can then fall on the neighbouring value;
  * f16 output rows (the rows form) add half an f16 ulp of the expected value;
  * 2^-126 sum_j |v_jd - out_d| is the floor of f32 underflow: a weight below the smallest normal f32 is lost whole (expf(s - m_c) in
    attn_partial_body, exp(m_c - M) in the half merge and in attn_combine_body's three merges), while float64 keeps it.  It matters only where
    the expected element is an exact 0 (needle: v on a grid), where every other term vanishes.
Records (rec_tol()): |m_c - m_ref| <= max_j ds_j over the record's positions; l_c exp(m_c - m_ref) and o_c exp(m_c - m_ref) against the model's,
under the same expression restricted to the record's positions (un-normalised: |v_jd| in place of |v_jd - out_d|, weights e_j = exp(s_j - m_ref)).

Input families (master() + token()), built in post-RoPE space; the query and the new key are rotated back to the raw qkv (attn_ref.unrope), past
keys go straight into the cache; v ~ N(0, 1.5).  See FAMILIES.  Stale slots at and past `pos` hold finite hostile values in every family (stale(); f32
keys are NaN except in `sunk`, which needs a finite winning score there).

walk(): the kernel's algorithm in float32: 64-position chunks with the 4 x 2 x 16 score chains, the stale-slot replacement, enew, the two (f32) or
four (f16) position classes of the P.V pass, the optional 128-position half merge, the combine's eight groups (record c -> group c % 8, merged in
index order) and the final eight-way join; fault= seeds the mistakes the families exist to catch (FAULTS).
"""
from __future__ import annotations

import numpy as np

from attn_ref import f16, rope, seed_of, unrope  # noqa: F401  (seed_of: re-exported for the tests)

D = 128
CHUNK = 64
SCALE = 1.0 / np.sqrt(128.0)
SCALE_F32 = np.float32(1.0) / np.sqrt(np.float32(D))

FAMILIES = ("gauss", "ramp12", "fall12", "newtok", "oldonly", "sunk", "needle")
# what each family forces:
#   gauss    q' ~ N(0, 1.5), k' ~ N(0, 1): the baseline; every record carries weight, so a lost key or record shows
#   ramp12   score trend +12 j / 64: every later record has the larger maximum -- the combine rescales l and a at every step, the NH == 2 merge has m1 > m0
#   fall12   trend -12 j / 64: record 0 dominates, later exp(m_c - M) underflow to exactly 0
#   newtok   the new token's score 30 above the rest: the mass sits on the enew / kn / vn path (the key from LDS, not its stale cache slot)
#   oldonly  the new token's score 30 below: the converse; a misplaced enew is invisible here and visible in newtok
#   sunk     every real score near -30; stale key slots hold 8 q', stale values the largest finite magnitude: one unmasked stale slot takes the output
#   needle   k'_j = 4 u_j, q'_h = 4 u_t(h) (+-1 codes), v on a 1/64 grid, a different visible target t(h) per head: out_h = v[t(h)] to the last bit
FAULTS = ("mask_tail", "new_twice", "enew_dropped", "merge_swap", "dead_record", "half_m", "head_map", "v_class")
# the mistake each fault seeds:
#   mask_tail     a stale slot (the one behind the new token) keeps its score
#   new_twice     the new token is counted in sc (against its stale value slot) and in enew
#   enew_dropped  the new token's weight is lost from the P.V sum
#   merge_swap    s_old and s_c are exchanged in the combine's online merge
#   dead_record   the combine merges one record past n_chunks
#   half_m        the 128-position half merge scales by m0, not by max(m0, m1)
#   head_map      head h reads KV head h % n_kv
#   v_class       two position classes of the P.V pass are exchanged

A_W, SD_NOISE = 16.0, 0.25  # the trend families: query component along w, noise sd (attn_ref.family's construction, natural-log scores)
BIG = {False: 1.0e30, True: 6.0e4}  # stale values: the largest magnitudes that stay finite (f32 after a product with a weight <= 1; f16)
UNDERFLOW = 2.0 ** -126  # the smallest normal f32: a weight below it may be lost whole
DEAD_RECORD = (1.0e4, 1.0e3, 1.0e6)  # (m, l, o) of the hostile records behind the live ones


def cache_dtype(kv_f16):
    return np.float16 if kv_f16 else np.float32


def rope1(x, pos, sin, cos):
    """float64 RoPE of [heads, D] rows at one position"""
    return rope(np.asarray(x)[None], np.array([pos]), sin, cos)[0]


def unrope1(y, pos, sin, cos):
    return unrope(np.asarray(y)[None], np.array([pos]), sin, cos)[0]


# ---- the input families --------------------------------------------------------------------------------------------------------
def trend_of(name, T):
    j = np.arange(T, dtype=np.float64)
    if name == "ramp12":
        return 12.0 * j / CHUNK
    if name == "fall12":
        return -12.0 * j / CHUNK
    if name == "sunk":
        return np.full(T, -30.0)
    if name in ("newtok", "oldonly"):
        return np.zeros(T)
    raise KeyError(name)


def master(name, rng, T, n_kv):
    """one family's keys and values for positions 0 .. T - 1, post-RoPE, float64: what the cache holds below `pos` and, at `pos`, the new token.
    -> dict(name, k [T, kv, D], v [T, kv, D], w [kv, D] | None, u [T, kv, D] | None)"""
    v = rng.normal(0, 1.5, (T, n_kv, D))
    if name == "gauss":
        return dict(name=name, k=rng.normal(0, 1.0, (T, n_kv, D)), v=v, w=None, u=None)
    if name == "needle":
        u = rng.choice([-1.0, 1.0], (T, n_kv, D))
        return dict(name=name, k=4.0 * u, v=np.round(v * 64.0) / 64.0, w=None, u=u)
    # k'_j = n_j + b(j) w, q'_h = n_h + a w with the query's noise orthogonal to w: score = scale (n_h . n_j + a w . n_j) + trend(j), noise sd ~0.36
    w = rng.choice([-1.0, 1.0], (n_kv, D)) / np.sqrt(D)
    b = trend_of(name, T) / (A_W * SCALE)
    return dict(name=name, k=rng.normal(0, SD_NOISE, (T, n_kv, D)) + b[:, None, None] * w[None], v=v, w=w, u=None)


def needle_targets(pos):
    """0, the new token, and both sides of every 64 (hence every 128) boundary below pos"""
    c = {0, pos}
    for b in range(CHUNK, pos + 1, CHUNK):
        c.update((b - 1, b))
    return sorted(c)


def token(m, rng, pos, n_heads):
    """the step at `pos` -> (q' [heads, D], new key' [kv, D], new value [kv, D], needle targets [heads] | None), float64"""
    name, n_kv = m["name"], m["k"].shape[1]
    group = n_heads // n_kv
    kn, vn = m["k"][pos].copy(), m["v"][pos].copy()
    if name == "gauss":
        return rng.normal(0, 1.5, (n_heads, D)), kn, vn, None
    if name == "needle":
        cand = needle_targets(pos)
        t = rng.choice(cand, n_heads, replace=len(cand) < n_heads)
        t[rng.integers(n_heads)] = pos  # one head always looks at the new token
        if n_heads > 1:
            t[(int(np.argmax(t == pos)) + 1) % n_heads] = cand[-2] if len(cand) > 1 else 0  # and one at the last cached boundary slot
        q = np.stack([4.0 * m["u"][t[h], h // group] for h in range(n_heads)])
        return q, kn, vn, t
    w = m["w"]
    if name in ("newtok", "oldonly"):
        kn = kn + (30.0 if name == "newtok" else -30.0) / (A_W * SCALE) * w
    wq = w[np.arange(n_heads) // group]
    q = rng.normal(0, SD_NOISE, (n_heads, D))
    q = q - (q * wq).sum(-1, keepdims=True) * wq + A_W * wq
    return q, kn, vn, None


def raw_qkv(q1, kn1, vn, pos, sin, cos):
    """post-RoPE query and new key rotated back -> the f32 qkv row the kernel reads: q | k | v"""
    return np.concatenate([unrope1(q1, pos, sin, cos).ravel(), unrope1(kn1, pos, sin, cos).ravel(), vn.astype(np.float32).ravel()])


def stale(name, q1, n_kv, kv_f16):
    """hostile contents of the slots at and past pos -> (key [kv, D], value [kv, D]) in the cache's dtype, the same for every stale slot.
    Keys: 8 q' of the KV head's first query head (its score beats every real one) -- f32 caches outside `sunk` hold NaN instead (any score there is
    replaced).  Values: the largest finite magnitude, alternating in sign (finite: the zero-filled-cache contract of include/bitnet_hip.h)."""
    group = q1.shape[0] // n_kv
    k = 8.0 * q1[::group]
    if not kv_f16 and name != "sunk":
        k = np.full((n_kv, D), np.nan)
    v = BIG[bool(kv_f16)] * np.where(np.arange(n_kv * D).reshape(n_kv, D) % 2, -1.0, 1.0)
    dt = cache_dtype(kv_f16)
    return k.astype(dt), v.astype(dt)


def host_caches(m, q1, pos, slots, kv_f16):
    """the logical caches [kv, slots, D] of one step: the master's keys / values below pos, stale() from pos on"""
    dt = cache_dtype(kv_f16)
    n_kv = m["k"].shape[1]
    ks, vs = stale(m["name"], q1, n_kv, kv_f16)
    kc, vc = np.empty((n_kv, slots, D), dt), np.empty((n_kv, slots, D), dt)
    kc[:, :pos], vc[:, :pos] = m["k"][:pos].transpose(1, 0, 2).astype(dt), m["v"][:pos].transpose(1, 0, 2).astype(dt)
    kc[:, pos:], vc[:, pos:] = ks[:, None], vs[:, None]
    return kc, vc


# ---- the model -----------------------------------------------------------------------------------------------------------------
def exact(qkv, k_past, v_past, pos, sin, cos, n_heads, n_kv, kv_f16, recs=(64, 128)):
    """qkv: the f32 row; k_past / v_past [kv, >= pos, D]: the cache's values (only slots below pos are read).
    -> dict(out [H, D], p [H, t_k], s [H, t_k], ds [H, t_k], q [H, D], K / V [kv, t_k rounded up to 128, D]: the operands, zeros behind t_k,
    rec {64 | 128: (m [H, R], l [H, R], o [H, R, D])}, t_k, group, kv_f16)"""
    qkv = np.asarray(qkv, np.float32)
    group = n_heads // n_kv
    q = rope1(qkv[: n_heads * D].reshape(n_heads, D), pos, sin, cos)
    kn = rope1(qkv[n_heads * D:(n_heads + n_kv) * D].reshape(n_kv, D), pos, sin, cos)
    vn = qkv[(n_heads + n_kv) * D:].reshape(n_kv, D).astype(np.float64)
    if kv_f16:
        kn, vn = f16(kn), f16(vn)
    t_k = pos + 1
    Tp = (t_k + 127) // 128 * 128
    K, V = np.zeros((n_kv, Tp, D)), np.zeros((n_kv, Tp, D))
    K[:, :pos], V[:, :pos] = k_past[:, :pos], v_past[:, :pos]
    K[:, pos], V[:, pos] = kn, vn
    aK, aV = np.abs(K), np.abs(V)
    out, p, s, ds = np.zeros((n_heads, D)), np.zeros((n_heads, t_k)), np.zeros((n_heads, t_k)), np.zeros((n_heads, t_k))
    rec = {r: [] for r in recs}
    for h in range(n_heads):
        g = h // group
        s[h] = K[g, :t_k] @ q[h] * SCALE
        qk = aK[g, :t_k] @ np.abs(q[h])
        ds[h] = 2.0 ** -24 * (24.0 * SCALE * qk + 4.0 * np.abs(s[h]))
        if kv_f16:
            ds[h, pos] += 2.0 ** -11 * SCALE * qk[pos]
        e = np.exp(s[h] - s[h].max())
        p[h] = e / e.sum()
        out[h] = p[h] @ V[g, :t_k]
        sp = np.full(Tp, -np.inf)
        sp[:t_k] = s[h]
        for r in rec:
            R = (t_k + r - 1) // r
            sr = sp[: R * r].reshape(R, r)
            m = sr.max(axis=1)
            e = np.exp(sr - m[:, None])
            rec[r].append((m, e.sum(axis=1), np.matmul(e[:, None, :], V[g, : R * r].reshape(R, r, D))[:, 0]))
    recs = {r: tuple(np.stack([x[i] for x in rec[r]]) for i in range(3)) for r in rec}
    return dict(out=out, p=p, s=s, ds=ds, q=q, K=K, V=V, aV=aV, rec=recs, pos=pos, t_k=t_k, group=group, kv_f16=bool(kv_f16))


def tol(ex, out_f16=False):
    """[H, D]: the tolerance of the output rows (module docstring)"""
    group, t_k = ex["group"], ex["t_k"]
    t = np.zeros_like(ex["out"])
    for h in range(t.shape[0]):
        g, p, o = h // group, ex["p"][h], ex["out"][h]
        dev = np.abs(ex["V"][g, :t_k] - o[None])
        t[h] = (p * ex["ds"][h]) @ dev + 2.0 ** -22 * (p @ ex["aV"][g, :t_k]) + 2.0 ** -23 * np.abs(o) + UNDERFLOW * dev.sum(axis=0)
    return t + half_ulp_f16(ex["out"]) if out_f16 else t


def half_ulp_f16(want):
    """what one rounding of the expected rows to f16 may add"""
    return 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)


def rec_tol(ex, rec):
    """-> (tol_m [H, R], tol_l [H, R], tol_o [H, R, D]) for records of `rec` positions, in the scale of the model's own (m, l, o)"""
    group, t_k = ex["group"], ex["t_k"]
    m_ref, l_ref, o_ref = ex["rec"][rec]
    H, R = m_ref.shape
    tm, tl, to = np.zeros((H, R)), np.zeros((H, R)), np.zeros((H, R, D))
    live = (np.arange(R * rec) < t_k).reshape(R, rec)
    for h in range(H):
        aV = ex["aV"][h // group, : R * rec].reshape(R, rec, D)
        sp, dp = np.full(R * rec, -np.inf), np.zeros(R * rec)
        sp[:t_k], dp[:t_k] = ex["s"][h], ex["ds"][h]
        sp, dp = sp.reshape(R, rec), dp.reshape(R, rec)
        e = np.exp(sp - m_ref[h][:, None])
        tm[h] = dp.max(axis=1)
        tl[h] = (e * dp).sum(axis=1) + 2.0 ** -22 * e.sum(axis=1) + 2.0 ** -23 * l_ref[h] + UNDERFLOW * live.sum(axis=1)
        to[h] = (np.matmul((e * dp)[:, None, :], aV)[:, 0] + 2.0 ** -22 * np.matmul(e[:, None, :], aV)[:, 0] + 2.0 ** -23 * np.abs(o_ref[h])
                 + UNDERFLOW * aV.sum(axis=1))
    return tm, tl, to


def ratio(got, want, bound):
    """max |got - want| / bound; anything not finite counts as infinitely wrong"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0.0, 0.0, err / bound)))  # (a bound of 0 -- one key, an expected 0 -- asks for equality)


def rec_ratio(ex, rec, m, l, o):
    """the records (m [H, R], l [H, R], o [H, R, D]) a kernel or walk() left, against the model -> max(err / tol) over m, l and o"""
    m_ref, l_ref, o_ref = ex["rec"][rec]
    tm, tl, to = rec_tol(ex, rec)
    m, l, o = (np.asarray(x, np.float64) for x in (m, l, o))
    if not (np.isfinite(m).all() and np.isfinite(l).all() and np.isfinite(o).all()):
        return float("inf")
    with np.errstate(over="ignore"):
        f = np.exp(m - m_ref)
    return max(ratio(m, m_ref, tm), ratio(l * f, l_ref, tl), ratio(o * f[..., None], o_ref, to))


# ---- the kernel's algorithm in float32 ---------------------------------------------------------------------------------------------
F32 = np.float32


def _fma(a, b, c):
    """one fused multiply-add in f32 (the product of two f32 is exact in f64)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _exp(x):
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, F32)).astype(F32)


def _head_chunks(q, K, V, kn, vn, pos, kv_f16, fault):
    """one head over all its 64-position chunks.  q [D] rotated f32; K / V [C, 64, D] f32 images of the cache tiles (stale slots included);
    kn / vn [D]: the new token's key and value as the kernel holds them in LDS.  -> (m [C], l [C], o [C, D]) f32"""
    C = K.shape[0]
    t_k = pos + 1
    K = K.copy()
    K[pos // CHUNK, pos % CHUNK] = kn  # the new token's key comes from LDS (its cache slot was read before it was written)
    # scores: wave = 32-dim slice, two chains per wave (even / odd dims) of 16 FMAs; chain pair, then ((w0 + w1) + w2) + w3
    Kw, qw = K.reshape(C, CHUNK, 4, 16, 2), q.reshape(4, 16, 2)
    acc = np.zeros((C, CHUNK, 4, 2), F32)
    for i in range(16):
        acc = _fma(qw[None, None, :, i, :], Kw[:, :, :, i, :], acc)
    with np.errstate(invalid="ignore"):
        part = acc[..., 0] + acc[..., 1]
        s = ((part[..., 0] + part[..., 1]) + part[..., 2]) + part[..., 3]
        j = np.arange(C * CHUNK).reshape(C, CHUNK)
        seen = j < t_k + (1 if fault == "mask_tail" else 0)
        s = np.where(seen, s * SCALE_F32, F32(-np.inf)).astype(F32)
        m = s.max(axis=1)
        e = np.where(seen, _exp(s - m[:, None]), F32(0)).astype(F32)
    l = e.sum(axis=1, dtype=F32)
    enew = F32(0) if fault == "enew_dropped" else e[pos // CHUNK, pos % CHUNK]
    sc = e if fault == "new_twice" else np.where(j == pos, F32(0), e).astype(F32)  # the new token's value is not in the cache registers
    # un-normalised P.V: position p = NPQ * k + class; f32: two classes, each two chains (k even / odd) of 16; f16: four classes, one chain of 16
    if kv_f16:
        w, Vc = sc.reshape(C, 16, 4), V.reshape(C, 16, 4, D)  # [step][class]
        if fault == "v_class":
            w = w[:, :, [1, 0, 2, 3]]
        a = np.zeros((C, 4, D), F32)
        for i in range(16):
            a = _fma(w[:, i, :, None], Vc[:, i], a)
        a[pos // CHUNK, 0] += enew * vn
        o = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
    else:
        w, Vc = sc.reshape(C, 16, 2, 2), V.reshape(C, 16, 2, 2, D)  # [step][chain][class]
        if fault == "v_class":
            w = w[:, :, :, ::-1]
        a = np.zeros((C, 2, 2, D), F32)
        for i in range(16):
            a = _fma(w[:, i, :, :, None], Vc[:, i], a)
        ar = a[:, 0] + a[:, 1]  # [C][class][D]
        ar[pos // CHUNK, 0] += enew * vn
        o = ar[:, 0] + ar[:, 1]
    return m, l, o.astype(F32)


def _half_merge(m, l, o, fault):
    """pairs of 64-position halves -> one record per 128 positions; a dead second half has m = -inf, l = 0, o = 0"""
    C = m.shape[0]
    if C % 2:
        m, l, o = np.append(m, F32(-np.inf)), np.append(l, F32(0)), np.concatenate([o, np.zeros((1, D), F32)])
    m0, m1 = m[0::2], m[1::2]
    M = m0 if fault == "half_m" else np.maximum(m0, m1)
    e0, e1 = _exp(m0 - M), _exp(m1 - M)
    with np.errstate(invalid="ignore", over="ignore"):
        return M.astype(F32), (e0 * l[0::2] + e1 * l[1::2]).astype(F32), (e0[:, None] * o[0::2] + e1[:, None] * o[1::2]).astype(F32)


def _combine(m, l, o, fault):
    """records -> the output row: eight groups, record c to group c % 8, merged online in index order; then the eight-way join"""
    R = m.shape[0]
    n = R + (1 if fault == "dead_record" else 0)
    if fault == "dead_record":
        m, l, o = np.append(m, F32(DEAD_RECORD[0])), np.append(l, F32(DEAD_RECORD[1])), np.concatenate([o, np.full((1, D), DEAD_RECORD[2], F32)])
    trips = (n + 7) // 8
    pad = trips * 8 - n
    mp = np.append(m, np.full(pad, -np.inf, F32)).reshape(trips, 8)
    lp = np.append(l, np.zeros(pad, F32)).reshape(trips, 8)
    op = np.concatenate([o, np.zeros((pad, D), F32)]).reshape(trips, 8, D)
    valid = (np.arange(trips * 8) < n).reshape(trips, 8)
    gm, gl, ga = np.full(8, -np.inf, F32), np.zeros(8, F32), np.zeros((8, D), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(trips):
            m_new = np.maximum(gm, mp[u])
            s_old, s_c = _exp(gm - m_new), _exp(mp[u] - m_new)
            if fault == "merge_swap":
                s_old, s_c = s_c, s_old
            ok = valid[u]
            gl = np.where(ok, gl * s_old + lp[u] * s_c, gl).astype(F32)
            ga = np.where(ok[:, None], ga * s_old[:, None] + op[u] * s_c[:, None], ga).astype(F32)
            gm = np.where(ok, m_new, gm).astype(F32)
        w = _exp(gm - gm.max())  # groups without a record: exp(-inf) = 0
        L, acc = F32(0), np.zeros(D, F32)
        for p in range(8):
            L = F32(L + w[p] * gl[p])
            acc = (acc + w[p] * ga[p]).astype(F32)
        return (acc / L).astype(np.float64)


def walk(qkv, kc, vc, pos, sin, cos, n_heads, n_kv, kv_f16, rec=64, fault=None):
    """The whole op in float32.  qkv: the f32 row; kc / vc [kv, slots, D]: the logical caches in their own dtype, stale slots included (slots a
    multiple of 64, > pos).  rec: 64 | 128 positions per record.  -> (out [H, D] float64, (m [H, R], l [H, R], o [H, R, D]) float32)"""
    assert fault in (None,) + FAULTS and rec in (64, 128)
    group = n_heads // n_kv
    raw = np.asarray(qkv, F32)
    sn, cs = np.asarray(sin, F32)[pos], np.asarray(cos, F32)[pos]

    def rot(x):  # two rounded products and a sum (hipcc may fuse one product: within the tolerance's RoPE count either way)
        x0, x1 = x[..., : D // 2], x[..., D // 2:]
        return np.concatenate([x0 * cs - x1 * sn, x0 * sn + x1 * cs], axis=-1).astype(F32)

    q = rot(raw[: n_heads * D].reshape(n_heads, D))
    kn = rot(raw[n_heads * D:(n_heads + n_kv) * D].reshape(n_kv, D))
    vn = raw[(n_heads + n_kv) * D:].reshape(n_kv, D)
    if kv_f16:  # rounded as the cache will hold them
        kn, vn = kn.astype(np.float16).astype(F32), vn.astype(np.float16).astype(F32)
    C = pos // CHUNK + 1
    out, ms, ls, os_ = np.zeros((n_heads, D)), [], [], []
    for h in range(n_heads):
        g = h % n_kv if fault == "head_map" else h // group
        K = np.asarray(kc[g, : C * CHUNK], F32).reshape(C, CHUNK, D)
        V = np.asarray(vc[g, : C * CHUNK], F32).reshape(C, CHUNK, D)
        m, l, o = _head_chunks(q[h], K, V, kn[g], vn[g], pos, kv_f16, fault)
        if rec == 128:
            m, l, o = _half_merge(m, l, o, fault)
        out[h] = _combine(m, l, o, fault)
        ms.append(m), ls.append(l), os_.append(o)
    return out, (np.stack(ms), np.stack(ls), np.stack(os_))
