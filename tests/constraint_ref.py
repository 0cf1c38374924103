"""numpy float32 restatement of the sampler's CONSTRAINTS stage (include/bitnet_hip.h, bitnet_hip_sampler_set_constraints): the element-wise
edit of the logits row that sits directly behind "counts" and in front of every other stage.

    apply(logits, cfg, g, seq) -> logits'

cfg is a dict with any of: bias ({id: value} or (id, value) pairs, in order), allowed (ids), hold (ids), min_tokens, no_repeat_ngram.
g is the number of tokens chosen so far, seq the token history h[0..P] (prompt included).  A sampler WITHOUT constraints that is given logits'
must then do exactly what a sampler WITH them does on logits: that equivalence is what the GPU tests hold, bit for bit."""
import numpy as np

F = np.float32
NEG_INF = F(-np.inf)


def bias_pairs(cfg):
    b = cfg.get("bias") or ()
    return list(b.items()) if isinstance(b, dict) else list(b)


def is_on(cfg):
    return bool(cfg) and bool(bias_pairs(cfg) or cfg.get("allowed") or cfg.get("hold") or cfg.get("min_tokens") or cfg.get("no_repeat_ngram"))


def ngram_banned(seq, n, vocab=None):
    """Tokens banned by no_repeat_ngram = n after the sequence seq = h[0..P]: for every j with j + n - 1 <= P and h[j .. j+n-2] == h[P-n+2 .. P],
    token h[j+n-1].  n = 1: every token of seq.  Fewer than n tokens in seq: nothing.  Ids outside [0, vocab) are skipped."""
    seq = [int(t) for t in seq]
    P = len(seq) - 1
    out = set()
    if n <= 0:
        return out
    for j in range(0, P - n + 2):  # j + n - 1 <= P
        if seq[j:j + n - 1] == seq[P - n + 2:P + 1]:
            t = seq[j + n - 1]
            if vocab is None or 0 <= t < vocab:
                out.add(t)
    return out


def apply(logits, cfg, g, seq):
    """The stage on one row; float32 in, float32 out, the input left unchanged."""
    x = np.array(logits, dtype=F, copy=True)
    V = x.size
    if not cfg:
        return x
    pairs = bias_pairs(cfg)
    allowed = list(cfg.get("allowed") or ())
    if pairs or allowed:
        b = np.zeros(V, F)
        for i, v in pairs:  # a duplicate id: the last entry wins
            b[int(i)] = F(v)
        with np.errstate(invalid="ignore"):
            x = (x + b).astype(F)  # one f32 addition per entry; +inf + -inf = NaN, which the ban below (or NaN -> -inf) catches
    ban = np.zeros(V, bool)
    if allowed:
        ban[:] = True
        ban[np.asarray(allowed, dtype=np.int64)] = False
    # a -inf bias is a ban: it wins over a +inf logit (x + -inf is NaN there, and NaN -> -inf follows)
    if pairs:
        last = {}
        for i, v in pairs:
            last[int(i)] = F(v)
        for i, v in last.items():
            if v == NEG_INF:
                ban[i] = True
    if int(cfg.get("min_tokens") or 0) > 0 and g < int(cfg["min_tokens"]):
        for i in cfg.get("hold") or ():
            ban[int(i)] = True
    n = int(cfg.get("no_repeat_ngram") or 0)
    if n > 0 and seq is not None:
        for t in ngram_banned(seq, n, V):
            ban[t] = True
    x[ban] = NEG_INF
    return x
