"""CPU: tests/logprob_ref.py against a literal Python transcription of the reference CLI's comparator (crates/bitnet-cli/src/main.rs:1344-1350),
on rows with ties, +-0.0, NaN and +-inf.  The comparison covers what the rule claims: the order of the finite entries, and finite before
non-finite (among non-finite entries the Rust comparator is no total order; the restatement fixes ascending id there)."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_ref as ref  # noqa: E402


def partial_cmp(a, b):
    """f32::partial_cmp: None when either is NaN"""
    if math.isnan(a) or math.isnan(b):
        return None
    return -1 if a < b else (1 if a > b else 0)


def cli_cmp(a, b):
    """indexed.sort_by(|a, b| match (a.1.is_finite(), b.1.is_finite()) { (false, true) => Greater, (true, false) => Less,
    _ => { let cmp = b.1.partial_cmp(&a.1).unwrap_or(Equal); if cmp == Equal { a.0.cmp(&b.0) } else { cmp } } })"""
    fa, fb = math.isfinite(a[1]), math.isfinite(b[1])
    if not fa and fb:
        return 1
    if fa and not fb:
        return -1
    c = partial_cmp(b[1], a[1])
    c = 0 if c is None else c
    return (a[0] > b[0]) - (a[0] < b[0]) if c == 0 else c


def rows():
    rng = np.random.default_rng(7)
    out = []
    for n in (1, 2, 7, 33, 200):
        r = rng.standard_normal(n).astype(np.float32)
        out.append(r)
        q = np.round(r * 2) / 2  # many ties
        out.append(q.astype(np.float32))
        z = q.copy().astype(np.float32)
        z[::3] = -0.0
        z[1::3] = 0.0
        out.append(z)
        s = r.copy()
        s[rng.integers(0, n, max(1, n // 4))] = np.nan
        s[rng.integers(0, n, max(1, n // 5))] = np.inf
        s[rng.integers(0, n, max(1, n // 5))] = -np.inf
        out.append(s)
    out.append(np.full(9, np.nan, np.float32))
    out.append(np.full(9, -np.inf, np.float32))
    out.append(np.array([np.inf, 1.0, np.nan, 1.0, -0.0, 0.0, -np.inf], np.float32))
    return out


@pytest.mark.parametrize("i", range(len(rows())))
def test_order_is_the_cli_comparators(i):
    l = rows()[i]
    got = ref.top_order(l)
    assert sorted(got.tolist()) == list(range(l.size))
    want = [k for k, _ in sorted(((k, float(v)) for k, v in enumerate(l)), key=functools.cmp_to_key(cli_cmp))]
    nf = int(np.isfinite(l).sum())
    assert got[:nf].tolist() == want[:nf]  # the finite entries, in the CLI's order
    assert np.isfinite(l[got[:nf]]).all() and not np.isfinite(l[got[nf:]]).any()  # finite before non-finite, in both
    assert not np.isfinite(l[want[nf:]]).any()
    assert got[nf:].tolist() == sorted(got[nf:].tolist())  # ascending id among the non-finite


def test_lse_rules():
    assert ref.lse64(np.array([np.nan, np.nan], np.float32)) == -np.inf
    assert ref.lse64(np.array([-np.inf, -np.inf], np.float32)) == -np.inf
    assert ref.lse64(np.array([1.0, np.inf, np.nan], np.float32)) == np.inf
    assert ref.lse64(np.array([0.0, 0.0], np.float32)) == pytest.approx(math.log(2.0), abs=1e-15)
    assert ref.lse64(np.array([np.nan, 3.0, -np.inf], np.float32)) == 3.0
    l = np.array([1000.0, 999.0], np.float32)
    assert ref.lse64(l) == pytest.approx(1000.0 + math.log1p(math.exp(-1.0)), abs=1e-12)


def test_record_fields():
    l = np.array([0.5, np.nan, 2.0, 2.0, -0.0, 0.0], np.float32)
    r = ref.record(l, 1, 4)
    assert r.n_top == 4 and r.top_id.tolist() == [2, 3, 0, 4] and r.logit == -np.inf
    assert ref.same_bits(r.top_logit, l[[2, 3, 0, 4]])
    assert math.isnan(ref.record(l, 6, 0).logit) and math.isnan(ref.record(l, -1, 0).logit)
    assert ref.record(l, 0, 20).n_top == 6 and ref.record(l, 0, 20).top_id.tolist() == [2, 3, 0, 4, 5, 1]
