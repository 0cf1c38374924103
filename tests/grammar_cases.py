"""Inputs the grammar tests share between the CPU and the GPU files: the launch geometry restated, and the masked rows of path F.

A masked row is -inf everywhere but at k survivors -- what a grammar state that allows k tokens leaves of a logits row.  The survivors' logits
lie 0.25 apart (the row is a ladder from 6.0 down), so no comparison of the chain's analysis (tests/sampler_chain_accept.py) falls inside a
rounding band: tests/test_grammar_ref.py shows on the CPU that the restatement reports every draw of every row decided, which makes the GPU
test's cap on undecided draws one the restatement alone meets."""
import numpy as np

F = np.float32
MASKED_VOCABS = [4097, 128256]
MASKED_K = [1, 2, 3, 65, 1000]
MASKED_STEPS = 4
# the F configs the masked rows run under: name -> (temperature, top_k, top_p, repetition_penalty), chain stages
MASKED_CFGS = {
    "F-top_p": ((0.7, 0, 0.9, 1.1), {}),
    "F-temperature": ((0.7, 0, 1.0, 1.0), {}),
    "F-min_p": ((0.9, 0, 1.0, 1.0), dict(min_p=0.05)),
    "F-typical_p": ((0.9, 0, 1.0, 1.0), dict(typical_p=0.9)),
    # top-k beyond the one-lane path's 64: with fewer survivors than k the k-th largest lies among the -inf entries, so the later radix passes
    # of the top-k select run inside -inf's own bin
    "F-top_k300": ((0.8, 300, 0.95, 1.0), {}),
}


def geometry(vocab):
    """(workgroups, slice) of a sampling launch: csrc/kernels_sample.hip `geometry`"""
    nwg = min(64, (vocab + 1023) // 1024)
    return nwg, (vocab + nwg - 1) // nwg


def edge_ids(vocab):
    """0, vocab - 1, the middle, and both sides of the first and the last boundary between two workgroups' slices"""
    nwg, sl = geometry(vocab)
    ids = {0, vocab - 1, vocab // 2}
    if nwg > 1:
        ids |= {sl - 1, sl, (nwg - 1) * sl - 1, (nwg - 1) * sl}
    return sorted(i for i in ids if 0 <= i < vocab)


_MASKED = {}


def masked_row(vocab, k):
    """(raw row, survivor ids): a random row whose k survivors -- the edge ids first, then random ones -- carry a ladder of logits 0.25 apart in
    a shuffled order.  Made once per (vocab, k) and shared; callers must not write to it."""
    if (vocab, k) not in _MASKED:
        rng = np.random.default_rng(9100 + vocab + k)
        x = (2.5 * rng.standard_normal(vocab)).astype(F)
        e = edge_ids(vocab)[:k]
        rest = np.setdiff1d(np.arange(vocab), np.asarray(e))
        ids = np.concatenate([np.asarray(e, dtype=np.int64), rng.choice(rest, size=k - len(e), replace=False)]).astype(np.int64)
        x[ids[rng.permutation(k)]] = (6.0 - 0.25 * np.arange(k)).astype(F)
        x.setflags(write=False)
        _MASKED[(vocab, k)] = (x, np.sort(ids))
    return _MASKED[(vocab, k)]


def masked_desc(vocab, ids):
    """the two-state automaton whose state 0 allows exactly `ids` (and stays), and whose state 1 allows nothing"""
    tc = np.zeros(vocab, np.uint16)
    tc[ids] = 1
    return tc, np.array([[-1, 0], [-1, -1]], np.int32)
