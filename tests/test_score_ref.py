"""Hand cases for tests/score_ref.py, the numpy restatement of score.rs's per-position NLL and of the greedy argmax rule."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

INF, NAN = np.inf, np.nan


def f32(*v):
    return np.array(v, np.float32)


def test_uniform_row_is_log_vocab():
    assert math.isclose(sr.row_nll(np.zeros(8, np.float32), 3), math.log(8), rel_tol=1e-6)


def test_matches_float64_log_softmax():
    rng = np.random.default_rng(1)
    l = (5 * rng.standard_normal(1000)).astype(np.float32)
    want = -(l[17] - (l.max() + np.log(np.exp(l.astype(np.float64) - l.max()).sum())))
    assert abs(sr.row_nll(l, 17) - want) < 1e-4


def test_non_finite_logits_are_minus_inf():
    base = f32(1.0, 2.0, 3.0)
    with_bad = f32(1.0, 2.0, 3.0, NAN, INF, -INF)
    for t in range(3):
        assert sr.row_nll(with_bad, t) == sr.row_nll(base, t)
    assert sr.row_nll(with_bad, 3) == INF  # NaN target logit
    assert sr.row_nll(with_bad, 4) == INF  # +inf is non-finite too
    assert sr.row_nll(with_bad, 5) == INF


def test_all_non_finite_row_is_nan():
    assert math.isnan(sr.row_nll(f32(NAN, INF, -INF), 0))
    assert math.isnan(sr.row_nll(f32(-INF, -INF), 1))


def test_targets_out_of_range():
    assert sr.row_nll(f32(1.0, 2.0), -1) == 0.0
    assert math.isnan(sr.row_nll(f32(1.0, 2.0), 2))


def test_argmax_ties_and_nan():
    assert sr.argmax(f32(1.0, 3.0, 3.0, 2.0)) == 1
    assert sr.argmax(f32(NAN, -5.0, NAN)) == 1
    assert sr.argmax(f32(NAN, NAN)) == 0  # every entry -inf: the lowest index
    assert sr.argmax(f32(1.0, INF, INF)) == 1
    assert sr.argmax(f32(-INF, -INF, -1.0)) == 2


def test_totals_are_score_rs_keys():
    t = sr.totals(f32(1.0, 2.0, 3.0))
    assert t["tokens"] == 3 and t["mean_nll"] == 2.0
    assert math.isclose(t["ppl"], math.exp(2.0), rel_tol=1e-15)
    assert math.isclose(t["std_nll"], math.sqrt(2.0 / 3.0), rel_tol=1e-12)
    assert sr.totals(f32())["mean_nll"] == 0.0


def test_head_rows_round_once_to_f16():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 64)).astype(np.float32)
    g = rng.uniform(0.5, 1.5, 64).astype(np.float32)
    a = sr.head_rows(x, g, 1e-5)
    ln = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * g
    assert np.all(a == a.astype(np.float16).astype(np.float32))
    assert np.max(np.abs(a - ln)) <= 2.0 ** -10 * np.max(np.abs(ln))
    assert np.array_equal(sr.head_rows(x, None, 0.0), x.astype(np.float16).astype(np.float32))
