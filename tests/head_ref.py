"""numpy / float64 restatement of the decode head (csrc/kernels_decode.hip: k_logits_f16 + k_argmax_final; csrc/kernels_batch.hip: k_logits_f16_batch
+ k_argmax_final_batch): what bitnet_hip_logits_f16_dev and bitnet_hip_logits_f16_batch_dev are held to.

  norm    xn = (x - mean(x)) / sqrt(var(x) + eps) * gamma, var the mean of the squared deviations; gamma None = no norm (xn = x), as in the kernel
  logits  logits[v] = sum_k xn[k] * float(E[v, k])
  pick    NaN counts as -inf, the lowest index wins a tie (-0.0 == +0.0), all -inf gives token 0
  state   history[p + 1] = token iff a history is given and (n_forced is absent or p + 1 >= n_forced); the position advances whenever a position
          pointer is given

Everything is float64 on the f32 / f16 values the kernel reads.  `bound` is the acceptance bound of the float path (derived in tests/test_head_gpu.py);
the `perturb` forms are deliberately wrong heads that tests/test_head_ref.py uses to show that the bound discriminates."""
import numpy as np

FLOAT_CASES = ("rand", "mean3", "const", "gamma")


def layernorm(x, gamma, eps, center=True):
    """center=False: the (wrong) form without the mean subtraction"""
    x = np.asarray(x, np.float32).astype(np.float64)
    if gamma is None:
        return x
    d = x - x.mean() if center else x
    return d / np.sqrt((d * d).mean() + eps) * np.asarray(gamma, np.float32).astype(np.float64)


def logits(x, gamma, eps, table, center=True):
    """-> (logits [vocab] f64, magnitude [vocab] f64 = sum_k |xn[k] * E[v, k]|)"""
    xn = layernorm(x, gamma, eps, center)
    e = np.asarray(table, np.float16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return e @ xn, np.abs(e) @ np.abs(xn)


def pick(l) -> int:
    v = np.asarray(l, np.float64)
    v = np.where(np.isnan(v), -np.inf, v)
    m = v.max()
    return 0 if m == -np.inf else int(np.flatnonzero(v == m)[0])  # -0.0 == +0.0: a tie


def advance(p, token, history=None, n_forced=None, has_pos=True):
    """-> (position after, history after or None); `history` is not modified"""
    if not has_pos:
        return p, None if history is None else np.array(history)
    h = None if history is None else np.array(history)
    if h is not None and (n_forced is None or p + 1 >= n_forced):
        h[p + 1] = token
    return p + 1, h


def bound(hidden: int, magnitude):
    """per-logit acceptance bound of the float path: (hidden / 64 + 16) * 2^-23 * sum_k |xn_k * E_vk|"""
    return (hidden / 64 + 16) * 2.0 ** -23 * np.asarray(magnitude, np.float64)


def mean_shift_term(x, gamma, eps, table):
    """The one error of the f32 head that is not relative to the products: the f32 mean is off by at most (hidden / 256 + 8) * 2^-24 * mean|x|
    (a thread's hidden / 256 - 1 additions, 6 butterfly steps, 2 across the waves, the division), which moves EVERY xn_k by that / sigma * gamma_k.
    -> [vocab] that shift's worst effect on each logit, in absolute terms.  0 without a norm, and 0 for a constant row every multiple of which
    (up to hidden) is an f32 value: then each partial sum, in any order, and the division are exact."""
    if gamma is None:
        return np.zeros(len(table))
    x = np.asarray(x, np.float32).astype(np.float64)
    multiples = x[0] * np.arange(1, x.size + 1)
    if np.all(x == x[0]) and np.array_equal(multiples.astype(np.float32).astype(np.float64), multiples):
        return np.zeros(len(table))
    d = x - x.mean()
    sigma = np.sqrt((d * d).mean() + eps)
    dm = (x.size / 256 + 8) * 2.0 ** -24 * np.abs(x).mean()
    return dm / sigma * np.abs(np.asarray(table, np.float16).astype(np.float64) @ np.asarray(gamma, np.float32).astype(np.float64))


def relative_units(hidden: int) -> float:
    """roundings (units of 2^-24) that act on a product xn_k * E_vk relative to itself: see the derivation in tests/test_head_gpu.py"""
    return hidden / 64 + 6 + hidden / 512 + 11


def float_case(name: str, hidden: int, vocab: int, seed: int = 0):
    """-> (x f32 [hidden], gamma f32 [hidden], table f16 [vocab, hidden]) of one of FLOAT_CASES"""
    rng = np.random.default_rng([FLOAT_CASES.index(name), hidden, vocab, seed])
    table = rng.normal(0.0, 1.0, (vocab, hidden)).astype(np.float16)
    gamma = np.ones(hidden, np.float32)
    if name == "rand":
        x = rng.normal(0.1, 1.0, hidden)
    elif name == "mean3":
        x = rng.normal(3.0, 0.5, hidden)
    elif name == "const":
        # 1.5 sums, divides and subtracts exactly in f32 at every hidden used (1.5 * hidden < 2^24, few mantissa bits): mean = 1.5, every deviation 0
        x = np.full(hidden, 1.5)
    else:
        x = rng.normal(0.1, 1.0, hidden)
        gamma = rng.uniform(0.5, 1.5, hidden).astype(np.float32)
    return x.astype(np.float32), gamma, table


def int_case(hidden: int, vocab: int, seed: int = 0):
    """x integers in [-3, 3] as f32, table integers in [-4, 4] as f16: every product and partial sum is an integer below 2^24 in magnitude
    (12 * 8192 < 2^17), so the f32 head is exact in any summation order.  -> (x, table, logits f32 exact)"""
    rng = np.random.default_rng([7, hidden, vocab, seed])
    x = rng.integers(-3, 4, hidden).astype(np.float32)
    if not x.any():
        x[0] = 1.0
    table = rng.integers(-4, 5, (vocab, hidden)).astype(np.float16)
    return x, table, int_logits(x, table)


def int_logits(x, table):
    want = np.asarray(table, np.float16).astype(np.int64) @ np.asarray(x, np.float32).astype(np.int64)
    assert np.abs(want).max(initial=0) < 2 ** 24
    return want.astype(np.float32)


# ---- deliberately wrong heads --------------------------------------------------------------------------------------------------------------
def perturb(kind: str, x, gamma, eps, table, lane: int = 13, chunk: int = 0):
    """-> logits [vocab] f64 of a head with one seeded mistake:
    drop   lane `lane`'s 8 columns of 512-column chunk `chunk` are left out of every row's sum
    chunk  a row reads its chunk `chunk` from chunk 0 (hidden 512 has only chunk 0: there the row reads chunk 0 of the row half a table on, the same
           slip one level up).  Every row is misread -- the rows share the kernel's code -- and each row's logit moves on its own: entry v of the
           result is what row v's misread alone would give, so the caller can judge one row or all.
    mean   the mean is not subtracted"""
    e = np.asarray(table, np.float16).astype(np.float64)
    hidden = e.shape[1]
    if kind == "mean":
        return logits(x, gamma, eps, table, center=False)[0]
    xn = layernorm(x, gamma, eps)
    if kind == "drop":
        xn = xn.copy()
        xn[512 * chunk + 8 * lane:512 * chunk + 8 * lane + 8] = 0.0
        return e @ xn
    if kind == "chunk":
        e = e.copy()
        if hidden == 512:
            e = np.roll(e, len(e) // 2, axis=0)
        else:
            c = max(chunk, 1)
            e[:, 512 * c:512 * c + 512] = e[:, :512]
        return e @ xn
    raise ValueError(kind)
