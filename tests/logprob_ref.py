"""numpy / float64 restatement of the logits tap (include/bitnet_hip.h: bitnet_hip_logprob_record): what csrc/kernels_logprob.hip is held to.

Top list: the CLI's rule (crates/bitnet-cli/src/main.rs:1344-1350) -- finite entries first, by descending logit (-0.0 == +0.0), then ascending id;
every non-finite entry after every finite one, by ascending id.  lse: M = max_i l_i with NaN read as -inf, lse = M + log(sum_i exp(l_i - M)) in
float64; +inf if M is +inf, -inf if M is -inf (inf - inf is never evaluated)."""
import collections

import numpy as np

TOP_MAX = 20
Ref = collections.namedtuple("Ref", "token n_top logit lse top_id top_logit")


def top_order(l: np.ndarray) -> np.ndarray:
    """ids of the whole row in the tap's order"""
    l = np.asarray(l, np.float32)
    fin = np.isfinite(l)
    key = np.where(fin, -l.astype(np.float64), 0.0)  # non-finite entries tie among themselves: ascending id; -0.0 and +0.0 tie too
    return np.lexsort((np.arange(l.size), key, ~fin))


def lse64(l: np.ndarray) -> float:
    x = np.asarray(l, np.float32).astype(np.float64)
    x = np.where(np.isnan(x), -np.inf, x)
    m = float(x.max())
    if m == np.inf or m == -np.inf:
        return m
    return m + float(np.log(np.exp(x - m).sum()))


def record(l: np.ndarray, token: int, top_n: int, order=None) -> Ref:
    """order: top_order(l) computed before (a row checked under several top_n)"""
    l = np.asarray(l, np.float32)
    n_top = min(int(top_n), l.size)
    ids = (top_order(l) if order is None else order)[:n_top].astype(np.int32)
    if 0 <= token < l.size:
        logit = np.float32(-np.inf) if np.isnan(l[token]) else l[token]
    else:
        logit = np.float32(np.nan)
    return Ref(int(token), n_top, np.float32(logit), lse64(l), ids, l[ids].copy())


def geometry(vocab: int):
    """(slice width, workgroups) of csrc/kernels_logprob.hip's partition: a function of the vocabulary alone"""
    s = (-(-vocab // 64) + 3) // 4 * 4
    s = min(max(s, 1024), 8192)
    return s, -(-vocab // s)


def chain(vocab: int) -> int:
    """D: the longest chain of f32 additions behind one lse, from the kernel as written (logprob_body): a thread's run over its slice entries
    (ceil(slice / 512), the first onto 0), the wave's xor tree (6), the eight wave sums one after another (7), then the merge: a lane's two
    workgroups (2) and the wave's xor tree (6)."""
    s, _ = geometry(vocab)
    return -(-min(s, vocab) // 512) + 6 + 7 + 2 + 6


def lse_bound(vocab: int, lse: float) -> float:
    """2 * (D + 4) * 2^-24 * max(1, |lse|): each addition rounds once (relative 2^-24 of a partial sum that never exceeds the total), + 4 for expf
    of the entries, expf of the workgroup maxima, logf and the final M + log S; doubled."""
    return 2.0 * (chain(vocab) + 4) * 2.0 ** -24 * max(1.0, abs(lse))


def same_bits(a, b) -> bool:
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
