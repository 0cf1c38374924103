"""The screened greedy head's bound on the CPU (tests/head_screen_ref.py): for every row the interval the int8 screening image proves contains the
f32 logit the full head computes in its own summation order, and the rows that survive the screen include every row that attains the maximum --
so the pick among the rescored rows is the full head's pick.  No GPU."""
import numpy as np
import pytest

import head_screen_ref as ref

SHAPES = [(512, 257), (1024, 5), (2560, 1031), (512, 1)]


def _all_cases():
    for hidden, vocab in SHAPES:
        for tn, yn, table, y in ref.cases(hidden, vocab):
            yield pytest.param(table, y, id=f"{hidden}x{vocab}-{tn}-{yn}")


@pytest.mark.parametrize("table,y", _all_cases())
def test_interval_contains_the_f32_logit_and_the_maximum_survives(table, y):
    q, s, c, rho, norm = ref.build(table)
    lb, ub = ref.interval(y, q, s, c)
    f = ref.head_f32(y, table).astype(np.float64)
    number = ~np.isnan(f)
    kept, L = ref.keep(lb, ub)
    open_ = np.isnan(lb) | np.isnan(ub)  # no interval at all (inf - inf under a non-finite input): such a row must simply be kept
    assert kept[open_].all()
    number &= ~open_
    assert np.all(lb[number] <= f[number]) and np.all(f[number] <= ub[number])
    assert kept[~number].all()  # a NaN logit is never screened away (it counts as -inf in the pick, and may be the lowest index of all)
    v = np.where(number, f, -np.inf)
    assert kept[v == v.max()].all()
    cand = np.flatnonzero(kept)
    assert cand[ref.pick(f[cand])] == ref.pick(f)


def test_image_codes_reproduce_the_rows_within_half_a_step():
    table = ref.tables(512, 257)["normal"]
    q, s, c, rho, norm = ref.build(table)
    e = table.astype(np.float64)
    # the f32 quotient E / s is off by at most 2^-24 of its size (<= 127 steps), and so is the point at which it rounds
    assert np.abs(q.astype(np.int32)).max() == 127 and np.all(np.abs(e - s[:, None].astype(np.float64) * q) <= (0.5 + 127 * 2.0 ** -23) * s[:, None])
    assert np.all(c > rho) and np.all(c < 1.01 * rho + 1e-3 * norm + 1e-15)


def test_screen_screens_on_the_benchmarks_distribution():
    """standard normal rows rounded to f16, as bench.py draws them: few rows survive, or the screened head would save nothing"""
    hidden, vocab = 2560, 4099
    table = ref.tables(hidden, vocab)["normal"]
    q, s, c, _, _ = ref.build(table)
    for y in (ref.activations(hidden)["normal"], ref.activations(hidden, 1)["normal"]):
        kept, _ = ref.keep(*ref.interval(y, q, s, c))
        assert 1 <= kept.sum() <= vocab // 16


def test_degenerate_inputs_keep_every_row():
    hidden, vocab = 512, 257
    ts, ys = ref.tables(hidden, vocab), ref.activations(hidden)
    q, s, c, _, _ = ref.build(ts["identical"])
    assert ref.keep(*ref.interval(ys["normal"], q, s, c))[0].all()
    q, s, c, _, _ = ref.build(ts["normal"])
    for yn in ("inf", "nan", "huge"):
        assert ref.keep(*ref.interval(ys[yn], q, s, c))[0].all(), yn
    q, s, c, _, _ = ref.build(ts["nonfinite"])
    assert np.isinf(c[[0, vocab // 2, vocab - 1]]).all() and ref.keep(*ref.interval(ys["normal"], q, s, c))[0][[0, vocab // 2, vocab - 1]].all()
