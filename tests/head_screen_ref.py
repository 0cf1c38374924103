"""numpy model of the screened greedy head (csrc/kernels_head.hip): the int8 screening image of the f16 table, the interval [lb, ub] it proves
around each f32 logit of the full head, and the candidate set that is rescored.

  image      per row v: s_v = f32(max|E_v|) / 127 (f32 division), q_vk = clip(rint(E_vk / s_v), -127, 127) (f32 division, ties to even) -- the
             builder's own f32 operations, so codes and scales are the device's bit for bit -- and, in float64, the coefficient
             c_v = ((1 + 2^-10)^2 rho_v + K 2^-24 (1 + 2^-10) |E_v| + 2^-55) (1 + 2^-20), rho_v = |E_v - s_v q_v|_2, K = hidden / 32 + 16
             (the builder's formula on exact norms: its f32 value lies within 2^-15 of this one).  A row with a non-finite entry: codes 0,
             scale 0, c_v = +inf.
  interval   r = |y|_2 (1 + 2^-10) + 2^-55, +inf where that is not a number <= 2^60;  a_v = s_v * sum_k q_vk y_k;  w_v = c_v r (1 + 2^-20) + 2^-100;
             ub_v = t + 2^-22 |t|, t = a_v + w_v;  lb_v = t' - 2^-22 |t'|, t' = a_v - w_v
  keep       L = max of the lb that are numbers (-inf if none); row v is kept unless ub_v < L (a NaN keeps the row)
  head_f32   the full head's logit in ITS f32 order: lane l of 64 chains fused multiply-adds over columns 512 c + 8 l + i (c, then i), then the
             xor butterfly 32, 16, 8, 4, 2, 1 -- what the interval must contain.  (Each fused multiply-add is taken in float64 and rounded to f32:
             the product of an f32 and an f16 is exact there, the sum is rounded twice, which moves a result by one f32 unit in about one
             operation of 2^29.)

`cases(hidden, vocab)` are the inputs both test files run."""
import numpy as np

UP10, UP20 = 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -20


def build(table):
    """-> (q int8 [vocab, hidden], s f32 [vocab], c f64 [vocab], rho f64, norm f64)"""
    e16 = np.asarray(table, np.float16)
    e = e16.astype(np.float32)
    bad = ~np.isfinite(e).all(axis=1)
    e = np.where(bad[:, None], np.float32(0), e)
    mx = np.abs(e).max(axis=1)
    s = (mx / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(s[:, None] > 0, np.clip(np.rint(e / s[:, None]), -127, 127), 0).astype(np.float32)
    e64, q64, s64 = e.astype(np.float64), q.astype(np.float64), s.astype(np.float64)
    rho = np.sqrt(((e64 - s64[:, None] * q64) ** 2).sum(axis=1))
    norm = np.sqrt((e64 * e64).sum(axis=1))
    k = e.shape[1] / 32 + 16
    c = (UP10 * UP10 * rho + k * 2.0 ** -24 * UP10 * norm + 2.0 ** -55) * UP20
    c = np.where(bad, np.inf, c)
    return q.astype(np.int8), np.where(bad, np.float32(0), s), c, rho, norm


def interval(y, q, s, c):
    """-> (lb f64 [vocab], ub f64 [vocab]) for the f32 activations y"""
    y = np.asarray(y, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.sqrt((y * y).sum()) * UP10 + 2.0 ** -55
        r = nrm if nrm <= 2.0 ** 60 else np.inf
        a = s.astype(np.float64) * (q.astype(np.float64) @ y)
        w = c * r * UP20 + 2.0 ** -100
        t, t2 = a + w, a - w
        return t2 - 2.0 ** -22 * np.abs(t2), t + 2.0 ** -22 * np.abs(t)


def keep(lb, ub):
    """-> (bool [vocab], L)"""
    good = lb[~np.isnan(lb)]
    L = good.max() if good.size else -np.inf
    with np.errstate(invalid="ignore"):
        return ~(ub < L), L


def head_f32(y, table):
    """the full head's f32 logits in the kernel's summation order -> f32 [vocab]"""
    y = np.asarray(y, np.float32)
    e = np.asarray(table, np.float16)
    vocab, hidden = e.shape
    nch = hidden // 512
    yl = y.reshape(nch, 64, 8).astype(np.float64)
    el = e.reshape(vocab, nch, 64, 8).astype(np.float64)
    acc = np.zeros((vocab, 64), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for ch in range(nch):
            for i in range(8):
                acc = (yl[ch, :, i][None, :] * el[:, ch, :, i] + acc.astype(np.float64)).astype(np.float32)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, lanes ^ off]).astype(np.float32)
    return acc[:, 0]


def pick(logits) -> int:
    v = np.asarray(logits, np.float64)
    v = np.where(np.isnan(v), -np.inf, v)
    m = v.max()
    return 0 if m == -np.inf else int(np.flatnonzero(v == m)[0])


def tables(hidden, vocab, seed=0):
    """name -> f16 table [vocab, hidden]"""
    rng = np.random.default_rng([11, hidden, vocab, seed])
    normal = rng.normal(0.0, 1.0, (vocab, hidden)).astype(np.float16)
    out = {"normal": normal}
    t = normal.copy()
    t[np.arange(vocab), rng.integers(0, hidden, vocab)] = np.float16(6.0e4)  # one huge entry per row: a coarse scale for all the others
    out["outlier"] = t
    t = normal.copy()
    t[::3] = 0  # all-zero rows
    t[1::3] = (rng.integers(-1023, 1024, t[1::3].shape) * 2.0 ** -24).astype(np.float16)  # subnormal rows
    out["zero_subnormal"] = t
    t = normal.copy()
    t[:] = t[0]  # every row the same: every row a candidate
    out["identical"] = t
    t = normal.copy()
    if vocab > 2:
        t[vocab // 2:] = t[: vocab - vocab // 2]  # duplicated rows ...
        one = t[-1].view(np.uint16).copy()
        one[hidden // 3] ^= 1  # ... and one that differs from its twin in one last f16 bit
        t[-1] = one.view(np.float16)
    out["duplicates"] = t
    t = normal.copy()
    t[0, 5], t[vocab // 2, 7], t[vocab - 1, hidden - 1] = np.inf, -np.inf, np.nan
    out["nonfinite"] = t
    return out


def activations(hidden, seed=0):
    """name -> f32 [hidden]"""
    rng = np.random.default_rng([12, hidden, seed])
    out = {"normal": rng.normal(0.0, 1.0, hidden).astype(np.float32)}
    out["range40"] = (rng.normal(0.0, 1.0, hidden) * 2.0 ** rng.integers(-20, 21, hidden)).astype(np.float32)  # a 2^40 dynamic range
    out["zero"] = np.zeros(hidden, np.float32)
    out["tiny"] = (rng.normal(0.0, 1.0, hidden) * 2.0 ** -70).astype(np.float32)  # squares below the normal range
    x = out["normal"].copy()
    x[3] = np.inf
    out["inf"] = x
    x = out["normal"].copy()
    x[hidden - 2] = np.nan
    out["nan"] = x
    out["huge"] = (out["normal"] * np.float32(2.0 ** 70)).astype(np.float32)  # beyond the overflow-free range: everything is kept
    return out


def cases(hidden, vocab):
    """(table name, activation name, table, y): every table with the plain activations, the plain table with every activation, and the
    non-finite table with the non-finite activations"""
    ts, ys = tables(hidden, vocab), activations(hidden)
    out = [(tn, "normal", t, ys["normal"]) for tn, t in ts.items()]
    out += [("normal", yn, ts["normal"], y) for yn, y in ys.items() if yn != "normal"]
    out += [("nonfinite", yn, ts["nonfinite"], ys[yn]) for yn in ("inf", "zero")]
    out += [("zero_subnormal", "tiny", ts["zero_subnormal"], ys["tiny"])]
    return out
