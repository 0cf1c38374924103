"""CPU: tests/head_ref.py (the float64 head the GPU tests compare with) against the oracle's LayerNorm and a plain matvec, its pick and state rules,
and the proof that the float path's acceptance bound discriminates: three seeded mistakes each move a logit by at least ten bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as H  # noqa: E402

EPS = 1e-5
HIDDENS = (512, 8192)
VOCAB = 48


@pytest.mark.parametrize("hidden", [512, 1536, 2560])
def test_layernorm_matches_the_oracle_and_logits_a_plain_matvec(oracle, hidden):
    rng = np.random.default_rng(hidden)
    x = rng.normal(0.3, 2.0, hidden).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, hidden).astype(np.float32)
    table = rng.normal(0, 1, (33, hidden)).astype(np.float16)
    xn = H.layernorm(x, gamma, EPS)
    want = oracle.layernorm(x, gamma, EPS).astype(np.float64)  # f32 arithmetic
    assert np.max(np.abs(xn - want)) <= 1e-5 * np.max(np.abs(want))
    got, mag = H.logits(x, gamma, EPS, table)
    plain = np.array([sum(float(xn[k]) * float(table[v, k]) for k in range(hidden)) for v in range(3)])
    assert np.allclose(got[:3], plain, rtol=0, atol=1e-10 * mag[:3].max())
    assert np.allclose(got, table.astype(np.float64) @ xn, rtol=0, atol=1e-10 * mag.max())
    assert np.all(mag >= np.abs(got))
    # no norm without a gamma, as in the kernel
    assert np.array_equal(H.layernorm(x, None, EPS), x.astype(np.float64))
    assert np.array_equal(H.logits(x, None, EPS, table)[0], table.astype(np.float64) @ x.astype(np.float64))


def test_pick_rule():
    inf, nan = np.inf, np.nan
    assert H.pick([1.0, 3.0, 3.0, 2.0]) == 1          # lowest index of a tie
    assert H.pick([-0.0, 0.0, -1.0]) == 0 and H.pick([-1.0, 0.0, -0.0]) == 1  # -0.0 == +0.0
    assert H.pick([1.0, nan, inf, inf]) == 2           # NaN is -inf, +inf wins
    assert H.pick([nan, nan, nan]) == 0 and H.pick([-inf, nan, -inf]) == 0  # nothing above -inf: token 0
    assert H.pick([nan, -5.0]) == 1
    assert H.pick(np.array([2.0], np.float32)) == 0


def test_history_and_position_rule():
    h = [-7] * 8
    p, got = H.advance(3, 42, h)
    assert p == 4 and list(got) == [-7, -7, -7, -7, 42, -7, -7, -7] and h == [-7] * 8
    assert H.advance(3, 42, h, n_forced=5)[0] == 4 and list(H.advance(3, 42, h, n_forced=5)[1]) == h   # p + 1 = n_forced - 1: kept
    assert list(H.advance(3, 42, h, n_forced=4)[1])[4] == 42                                              # p + 1 = n_forced: written
    assert list(H.advance(3, 42, h, n_forced=0)[1])[4] == 42
    assert H.advance(3, 42, None) == (4, None)                                                            # a position alone still advances
    p, got = H.advance(3, 42, h, has_pos=False)                                                          # no position pointer: nothing moves
    assert p == 3 and list(got) == h


def test_integer_case_is_exact_in_f32():
    for hidden in (512, 8192):
        x, table, want = H.int_case(hidden, 17)
        assert np.abs(x).max() <= 3 and np.abs(table.astype(np.float32)).max() <= 4
        assert np.array_equal(x, np.round(x)) and np.array_equal(table, np.round(table.astype(np.float32)).astype(np.float16))
        assert (np.abs(table.astype(np.float64)) @ np.abs(x.astype(np.float64))).max() < 2 ** 24  # every partial sum of every order is an exact f32
        assert np.array_equal(want.astype(np.float64), H.logits(x, None, EPS, table)[0])
        assert np.array_equal(want, (table.astype(np.float32)[:, ::-1] @ x[::-1]).astype(np.float32))  # another order, in f32


@pytest.mark.parametrize("hidden", HIDDENS)
@pytest.mark.parametrize("case", H.FLOAT_CASES)
def test_the_derived_error_terms_fit_inside_the_acceptance_bound(case, hidden):
    """The derivation (tests/test_head_gpu.py) has two terms: roundings relative to each product, relative_units(hidden) * 2^-24 * magnitude, and
    the common shift the f32 mean's own error gives every xn_k, which is not relative to the products and so is evaluated on the inputs.  Their sum
    must stay inside the bound the GPU test asserts (which repeats this check on its own, larger tables)."""
    x, gamma, table = H.float_case(case, hidden, VOCAB)
    _, mag = H.logits(x, gamma, EPS, table)
    derived = H.relative_units(hidden) * 2.0 ** -24 * mag + H.mean_shift_term(x, gamma, EPS, table)
    assert np.all(derived <= H.bound(hidden, mag))
    if case == "const":
        assert not mag.any() and not derived.any()  # LayerNorm of a constant row is 0: every logit exactly 0
    else:
        assert np.all(derived >= 0.25 * H.bound(hidden, mag))  # and the bound is no more than four times the derived error


@pytest.mark.parametrize("hidden", HIDDENS)
@pytest.mark.parametrize("case", H.FLOAT_CASES)
def test_bound_catches_each_seeded_mistake_tenfold(case, hidden):
    x, gamma, table = H.float_case(case, hidden, VOCAB)
    want, mag = H.logits(x, gamma, EPS, table)
    b = H.bound(hidden, mag)
    assert H.pick(want) == (0 if case == "const" else int(np.argmax(want)))
    kinds = ("drop", "chunk", "mean") if case == "mean3" else ("drop", "chunk")
    for kind in kinds:
        for chunk in sorted({0, hidden // 512 - 1}):
            moved = np.abs(H.perturb(kind, x, gamma, EPS, table, chunk=chunk) - want)
            ratio = moved / np.where(b > 0, b, 1.0)
            print(case, hidden, kind, chunk, "moved / bound: max %.3g, median %.3g" % (ratio.max(), np.median(ratio)))
            if case == "const":
                # xn = 0: a head that drops or misreads table columns still gives 0, and the bound there is 0 (exact equality is what the GPU test
                # asserts); only the missing mean could show, and that is not required of this case
                assert not moved.any() and not b.any()
                continue
            assert np.any(moved >= 10.0 * b), (case, hidden, kind, chunk, ratio.max())
            # not one lucky row: the typical row shows it tenfold too (a single row can hide a misread when two sums happen to agree)
            assert np.median(ratio) >= 10.0, (case, hidden, kind, chunk, np.median(ratio))
    if case == "const":  # ... and the missing mean does show on the constant row, though nothing requires it
        assert np.abs(H.perturb("mean", x, gamma, EPS, table) - want).max() > 0
