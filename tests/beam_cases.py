"""Inputs of the beam search tests, shared by the CPU tests of the rule (tests/test_beam_ref.py) and the GPU tests of the select launch
(tests/test_beam_gpu.py): crafted searches, one per property of the rule, and seeded random ones.  A search is a dict: B, eos, max_new, lw (the
length weights), P (the prompt position) and steps[s][b] = (lse, ids [2B], logits [2B]), the part of beam b's tap record the rule reads."""
import numpy as np

import beam_ref as br

F = np.float32


def _search(B, eos, max_new, lw, P, steps):
    return dict(B=B, eos=eos, max_new=max_new, lw=np.asarray(lw, F), P=P,
                steps=[[(F(l), np.asarray(i, np.int32), np.asarray(g, F)) for l, i, g in step] for step in steps])


_dead2 = (0.0, [1, 2, 3, 4], [0, 0, 0, 0])
_dead3 = (0.0, [1, 2, 3, 4, 5, 6], [0] * 6)
_eos3 = (0.0, [9, 1, 2, 3, 4, 5], [-0.125, -7, -8, -9, -10, -11])
_keep = (0.0, [1, 2, 3, 4], [-1, -5, -6, -7])
inf, nan = np.inf, np.nan

CRAFTED = {
    # equal scores: ascending j inside a beam (step 0), ascending b across beams (step 1)
    "tie_orders": _search(2, -1, 8, br.len_weights(8, 0.0), 3, [
        [(0.0, [5, 6, 7, 8], [-1, -1, -2, -3]), _dead2],
        [(0.0, [10, 11, 12, 13], [-0.5, -0.5, -4, -5]), (0.0, [20, 21, 22, 23], [-0.5, -0.5, -4, -5])]]),
    # NaN and -inf candidates read as -inf and come last in (b, j) order; a NaN lse sinks a whole beam; +inf - +inf is NaN
    "non_finite_last": _search(2, -1, 8, br.len_weights(8, 0.0), 0, [
        [(0.0, [5, 6, 7, 8], [-0.25, -0.5, -2, -3]), _dead2],
        [(0.0, [5, 6, 7, 8], [nan, -1, -inf, -2]), (nan, [1, 2, 3, 4], [-0.1, -0.2, -0.3, -0.4])],
        [(0.0, [5, 6, 7, 8], [-inf, nan, nan, inf]), (inf, [1, 2, 3, 4], [inf, -0.2, -0.3, -0.4])]]),
    # an EOS at walk index 0 < B is pooled, an EOS at walk index 2 >= B is skipped
    "eos_walk_index": _search(2, 9, 8, br.len_weights(8, 0.0), 0, [
        [(0.0, [5, 6, 7, 8], [-1, -1, -2, -3]), _dead2],
        [(0.0, [9, 5, 6, 7], [-0.1, -1, -2, -3]), (0.0, [5, 9, 6, 7], [-0.2, -0.3, -5, -6])]]),
    # a full pool replaces its worst entry for a strictly greater key, and the search ends by the pool
    "pool_replaces_worst": _search(3, 9, 3, [1, 4, 1, 1], 0, [
        [(0.0, [1, 2, 9, 3, 4, 5], [-1, -2, -3, -4, -5, -6]), _dead3, _dead3],
        [_eos3, _eos3, _eos3]]),
    "done_by_budget": _search(2, 9, 2, br.len_weights(2, 1.0), 0, [
        [(0.0, [5, 6, 7, 8], [-1, -1.5, -2, -3]), _dead2],
        [(0.0, [1, 2, 3, 4], [-1, -2, -3, -4]), (0.0, [1, 2, 3, 4], [-1, -2, -3, -4])]]),
    # two beams whose lineages part at step 0, continue themselves at step 1 and are both replaced by beam 1's children at step 2
    "from_is_div_before": _search(2, -1, 8, br.len_weights(8, 0.0), 10, [
        [(0.0, [5, 6, 7, 8], [-1, -2, -3, -4]), _dead2],
        [_keep, _keep],
        [(0.0, [1, 2, 3, 4], [-9, -9, -9, -9]), (0.0, [1, 2, 3, 4], [-0.1, -0.2, -6, -7])]]),
}


def random_search(rng, B=None):
    """quantised values give ties, some rows are non-finite, some length weights zero (-inf * 0: a NaN key); max_new steps of records"""
    B = int(rng.integers(1, 9)) if B is None else B
    vocab = max(2 * B, int(rng.integers(6, 41)))
    eos = int(rng.integers(0, vocab)) if rng.random() < 0.8 else -1
    max_new = int(rng.integers(1, 7))
    lw = br.len_weights(max_new, float(rng.choice([0.0, 0.6, 1.0, 2.5])))
    if rng.random() < 0.1:
        lw[int(rng.integers(1, max_new + 1))] = 0.0
    steps = []
    for _ in range(max_new):
        step = []
        for _ in range(B):
            ids = rng.permutation(vocab)[:2 * B].astype(np.int32)
            logits = np.sort((rng.integers(-24, 1, size=2 * B) * 0.25).astype(F))[::-1].copy()
            lse = F(rng.integers(0, 4) * 0.25)
            r = rng.random()
            if r < 0.15:
                logits[rng.integers(0, 2 * B, size=2)] = rng.choice(np.array([nan, -inf, inf], F), size=2)
            elif r < 0.2:
                lse = F(rng.choice(np.array([nan, -inf, inf], F)))
            step.append((lse, ids, logits))
        steps.append(step)
    return dict(B=B, eos=eos, max_new=max_new, lw=lw, P=int(rng.integers(0, 200)), steps=steps)


def new_ref(search, cls=br.BeamRef):
    return cls(search["B"], search["eos"], search["max_new"], search["lw"], prompt_pos=search["P"])


def ref_step(ref, search, s):
    """step s of the search on the restatement"""
    step = search["steps"][s]
    ref.step([r[0] for r in step], np.array([r[1] for r in step]), np.array([r[2] for r in step]), search["P"] + s)
