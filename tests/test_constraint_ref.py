"""CPU: the numpy restatement of the CONSTRAINTS stage (tests/constraint_ref.py) against its own definition -- the n-gram rule against a
brute-force enumeration of all n-grams, ban over bias, duplicate ids, the hold-off boundary, an allowed list with a bias on an allowed id."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_ref as cr  # noqa: E402

F = np.float32
INF = F(np.inf)


def brute_force_banned(seq, n, alphabet):
    """token t is banned iff appending it would make the sequence end in an n-gram that it already contains"""
    seq = list(seq)
    have = {tuple(seq[j:j + n]) for j in range(len(seq) - n + 1)}
    return {t for t in alphabet if len(seq) >= n - 1 and tuple(seq[len(seq) - (n - 1):] + [t]) in have}


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_the_ngram_rule_against_all_ngrams(n):
    rng = np.random.default_rng(100 + n)
    hits = 0
    for length in range(0, 41):
        for _ in range(8):
            seq = rng.integers(0, 5, length).tolist()
            got = cr.ngram_banned(seq, n, 5)
            want = brute_force_banned(seq, n, range(5))
            assert got == want, (n, seq, got, want)
            hits += bool(got)
    assert hits > 40  # the rule was exercised, not vacuously empty


def test_ngram_edges():
    assert cr.ngram_banned([], 1) == set() and cr.ngram_banned([], 3) == set()
    assert cr.ngram_banned([4], 3) == set()          # shorter than n - 1
    assert cr.ngram_banned([4, 4], 3) == set()       # exactly n - 1 tokens: no j with j + n - 1 <= P
    assert cr.ngram_banned([4, 4, 4], 3) == {4}      # the match at j = 0 overlaps the suffix
    assert cr.ngram_banned([1, 2, 9, 1, 2], 3) == {9}
    assert cr.ngram_banned([1, 2, 7, 1, 2, 8, 1, 2], 3) == {7, 8}
    assert cr.ngram_banned([3, 1, 2], 1) == {1, 2, 3}
    assert cr.ngram_banned([1, 99, 1], 2, vocab=10) == set() and cr.ngram_banned([1, 99, 1], 2) == {99}  # ids past the vocabulary are skipped
    assert cr.ngram_banned([-5, 2, -5], 2, vocab=10) == {2}  # ... but still take part in the match


def test_ban_beats_bias():
    x = np.array([1.0, 2.0, np.inf, -1.0, np.nan], F)
    got = cr.apply(x, dict(bias={1: 5.0, 3: 100.0, 2: -np.inf}, allowed=[0, 1, 2, 4]), 0, [])
    assert got[0] == F(1.0) and got[1] == F(7.0)
    assert got[2] == -INF  # +inf logit, -inf bias: banned, not NaN
    assert got[3] == -INF  # a large bias on an id outside the allowed list
    assert np.isnan(got[4])  # a NaN logit that nothing bans stays for NaN -> -inf
    got = cr.apply(x, dict(bias={0: 50.0}, no_repeat_ngram=1), 0, [0])
    assert got[0] == -INF and got[1] == F(2.0)
    got = cr.apply(x, dict(bias={0: 50.0}, hold=[0], min_tokens=1), 0, [])
    assert got[0] == -INF


def test_duplicate_ids_the_last_wins():
    x = np.zeros(4, F)
    got = cr.apply(x, dict(bias=[(1, 3.0), (2, -np.inf), (1, -1.5), (2, 0.25)]), 0, [])
    assert got.tolist() == [0.0, -1.5, 0.25, 0.0]
    got = cr.apply(x, dict(bias=[(2, 0.25), (2, -np.inf)]), 0, [])
    assert got[2] == -INF


def test_bias_is_one_f32_addition():
    x = np.array([0.1, 16777216.0, -0.0], F)
    got = cr.apply(x, dict(bias={0: 0.2, 1: 1.0}), 0, [])
    assert got[0] == F(0.1) + F(0.2) and got[1] == F(16777216.0)  # 2^24 + 1 rounds back in f32
    assert got.dtype == F and x[0] == F(0.1)  # the input is left alone


def test_the_hold_off_boundary():
    x = np.arange(6, dtype=F)
    cfg = dict(hold=[5, 2], min_tokens=4)
    for g in range(0, 4):
        got = cr.apply(x, cfg, g, [])
        assert got[5] == -INF and got[2] == -INF and got[4] == F(4), g  # g = min_tokens - 1 still holds
    for g in (4, 5, 100):
        assert np.array_equal(cr.apply(x, cfg, g, []), x), g            # g = min_tokens: live
    assert np.array_equal(cr.apply(x, dict(hold=[5], min_tokens=0), 0, []), x)


def test_allowed_list_with_a_bias_on_an_allowed_id():
    x = np.linspace(-2, 2, 9).astype(F)
    got = cr.apply(x, dict(allowed=[8, 0, 3], bias={3: 1.25, 4: 9.0}), 7, [1, 2, 3])
    want = np.full(9, -INF, F)
    want[[0, 8]] = x[[0, 8]]
    want[3] = x[3] + F(1.25)
    assert np.array_equal(got, want)
    assert np.argmax(got) == 8


def test_off_and_empty_configs_change_nothing():
    x = np.array([1.0, -0.0, np.nan, np.inf], F)
    for cfg in (None, {}, dict(bias={}, allowed=[], hold=[], min_tokens=0, no_repeat_ngram=0)):
        assert cr.apply(x, cfg, 3, [1, 1, 1]).tobytes() == x.tobytes()
        assert not cr.is_on(cfg)
    assert cr.is_on(dict(no_repeat_ngram=2)) and cr.is_on(dict(bias={1: 0.0}))
