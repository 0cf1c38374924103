"""numpy restatement of the reference's teacher-forced scoring (crates/bitnet-cli/src/score.rs:96-119, log_softmax_stable :160-173;
commands/eval.rs compute_nll_stats) and of the greedy argmax rule (sampling.rs:45-49,189-202), one logits row at a time.

  row_nll(logits, target)  non-finite logits -> -inf; m = max; sum = f32 sum of exp(v - m) in index order; lse = m + ln(sum);
                           nll = -(logits[target] - lse).  A target < 0 means "no target" (0); a target >= len is NaN (eval.rs refuses
                           it, score.rs would index out of bounds: the device contract writes NaN).
  argmax(logits)           NaN counts as -inf, lowest index on ties.
  totals(nlls)             score.rs's f64 total over the f32 per-position values: mean_nll, ppl = exp(mean_nll); eval.rs's std_nll.
  head_rows(x, gamma, ...) the device head's operand: f16(LN(x) * gamma) in the f32 op order of k_logits_f16, as float32."""
import numpy as np


def row_nll(logits, target: int) -> float:
    l = np.asarray(logits, np.float32)
    if target < 0:
        return 0.0
    if target >= l.size:
        return float("nan")
    v = np.where(np.isfinite(l), l, np.float32(-np.inf)).astype(np.float32)
    m = np.float32(v.max())
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((v - m).astype(np.float32)).astype(np.float32)
        s = np.cumsum(e, dtype=np.float32)[-1]  # the reference's sequential f32 sum (cumsum keeps the index order; np.sum is pairwise)
        lse = np.float32(m + np.float32(np.log(s)))
        return float(-(np.float32(v[target]) - lse))


def argmax(logits) -> int:
    l = np.asarray(logits, np.float32)
    v = np.where(np.isnan(l), np.float32(-np.inf), l)
    return int(np.argmax(v))  # numpy returns the first (lowest) index of the maximum


def nll_rows(logits2d, targets) -> np.ndarray:
    return np.array([row_nll(r, int(t)) for r, t in zip(logits2d, targets)], np.float32)


def totals(nlls) -> dict:
    v = np.asarray(nlls, np.float32)
    n = int(v.size)
    total = float(np.sum(v.astype(np.float64)))
    mean = total / n if n else 0.0
    var = float(np.sum((v.astype(np.float64) - mean) ** 2)) / n if n else 0.0
    return {"tokens": n, "mean_nll": mean, "ppl": float(np.exp(mean)), "std_nll": float(np.sqrt(var))}


def head_rows(x, gamma, eps: float) -> np.ndarray:
    """f16(LN(x) * gamma) row by row, as float32 (gamma None: f16(x))."""
    x = np.asarray(x, np.float32)
    if gamma is None:
        return x.astype(np.float16).astype(np.float32)
    h = np.float32(x.shape[1])
    mean = (x.sum(axis=1, dtype=np.float32) / h).astype(np.float32)[:, None]
    d = (x - mean).astype(np.float32)
    var = ((d * d).sum(axis=1, dtype=np.float32) / h).astype(np.float32)[:, None]
    denom = np.sqrt(var + np.float32(eps)).astype(np.float32)
    return (((d / denom).astype(np.float32) * np.asarray(gamma, np.float32)).astype(np.float16)).astype(np.float32)
