"""bitnet_hip_score_topn_f16_dev (csrc/kernels_score.hip: k_topn_head, k_topn_combine, k_score_topn) against a float64 reference written
here: the final norm as tests/score_ref.py states it, the f16-rounded operands, a float64 dot, np.argsort in the key order (larger value
first, lower id on equal values, NaN read as -inf).

Families, every one a table built by planting rows: gauss (a Gaussian background, min(top_n + 1, vocab) planted ranks at random ids), block (the
planted ranks inside ONE 128-entry block: its certificate fails, the escape has to run), spread (one per block, round robin), ties (small
integers without a norm: every dot product exact in f32, ties within and across blocks, duplicated rows), equal (one integer row repeated:
every block fails its certificate), nonfin (integers, positive x, table rows of NaN, +inf and -inf).
gauss / block / spread: consecutive ranks down to rank n_top + 1 lie more than twice the bound apart -- asserted on the reference first -- so
ids must be equal; values within the bound of tests/test_score_gpu.py check_rows (5e-5 max|l| + 1e-4, the head's f32 accumulation).  ties /
equal / nonfin: ids and top values exactly equal.  nll and argmax: the bytes bitnet_hip_score_f16_dev leaves on the same inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5
FAMILIES = ("gauss", "block", "spread", "ties", "equal", "nonfin")
EXACT = FAMILIES[3:]


def make_case(family, h, v, n, top_n):
    """(table f16 [v, h], x f32 [n, h], gamma or None)"""
    rng = np.random.default_rng([h, v, n, top_n, FAMILIES.index(family)])
    if family in EXACT:
        x = rng.integers(1 if family == "nonfin" else -4, 5, (n, h)).astype(np.float32)
        table = rng.integers(-3, 4, (v, h)).astype(np.float32)
        if family == "equal":
            table[:] = table[0]
        if family == "ties":
            for group in ((5, 6, 130, 260, v - 1), (7, 131, 290)):
                ids = [i for i in group if i < v]
                table[ids] = table[ids[:1]]
        if family == "nonfin":
            for val, group in ((np.nan, (2, 131, v - 1)), (np.inf, (9, 129)), (-np.inf, (4, 257))):
                table[[i for i in group if i < v]] = val
        return table.astype(np.float16), x, None
    gamma = rng.uniform(0.5, 1.5, h).astype(np.float32)
    # The planted rows lie along LN(x) * gamma: ONE element of it rounding to the other f16 neighbour would move a logit past the bound.  Rows
    # of small integers that sum to zero keep the norm's sums exact in f32 in any order, so the device's operands are the reference's bits.
    half = rng.integers(1, 13, h // 2)
    base = rng.permutation(np.concatenate([half, -half])).astype(np.float32)
    unit = np.concatenate([np.ones(h // 4), -np.ones(h // 4), np.zeros(h - h // 4 * 2)])
    x = (base + np.stack([rng.permutation(unit) for _ in range(n)])).astype(np.float32)
    a = sr.head_rows(base[None], gamma, EPS)[0].astype(np.float64)
    u = a / (a @ a)  # a . u = 1: table row s u scores about s on every row
    s = 3.0 * rng.standard_normal(v)
    planted = min(top_n + 1, v)
    if family == "gauss":
        ids = rng.choice(v, planted, replace=False)
    elif family == "block":
        b0 = (v - 1) // 128 // 2 * 128  # a middle block; the ranks run against the id order inside it
        ids = b0 + np.arange(min(128, v - b0))[::-1][:planted]
    else:
        nb = (v + 127) // 128
        ids = np.array(sorted(range(v), key=lambda i: (i % 128, i // 128))[:planted]) if nb > 1 else np.arange(planted)
    s[ids] = 100.0 - 2.0 * np.arange(planted)
    table = s[:, None] * u[None, :] + 0.01 * rng.standard_normal((v, h))
    return table.astype(np.float16), x, gamma


def run(hip, torch, pkg, table, x, gamma, targets, top_n):
    n, h = x.shape
    v = table.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    t, xd, gd, td = dev(table.view(np.int16)), dev(x), dev(gamma) if gamma is not None else None, dev(targets)
    out = []
    for topn in (True, False):
        nll = torch.zeros(n, dtype=torch.float32, device="cuda")
        am = torch.zeros(n, dtype=torch.int32, device="cuda")
        wsb = hip.score_topn_workspace_bytes(n, h, v) if topn else hip.score_workspace_bytes(n, h, v)
        ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
        if topn:
            rec = torch.zeros(n * pkg.LOGPROB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            hip.score_topn_f16_dev(t, xd, gd, EPS, h, v, n, td, nll, am, rec, top_n, ws, wsb)
        else:
            hip.score_f16_dev(t, xd, gd, EPS, h, v, n, td, nll, am, None, 0, ws, wsb)
        torch.cuda.synchronize()
        out += [nll.cpu().numpy(), am.cpu().numpy()]
    return rec.cpu().numpy().view(pkg.LOGPROB_DTYPE), out


@pytest.mark.parametrize("top_n", [1, 5, 20])
@pytest.mark.parametrize("n", [1, 127, 130])
@pytest.mark.parametrize("v", [1, 127, 129, 300])
@pytest.mark.parametrize("h", [128, 192])
@pytest.mark.parametrize("family", FAMILIES)
def test_topn_against_f64(pkg, hip, family, h, v, n, top_n):
    import torch
    table, x, gamma = make_case(family, h, v, n, top_n)
    targets = np.random.default_rng(n + v).integers(0, v, n).astype(np.int32)
    if n > 1:
        targets[1] = -1
    rec, (nll, am, nll0, am0) = run(hip, torch, pkg, table, x, gamma, targets, top_n)
    assert nll.tobytes() == nll0.tobytes() and am.tobytes() == am0.tobytes()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = sr.head_rows(x, gamma, EPS).astype(np.float64) @ table.astype(np.float64).T
    key = np.where(np.isnan(ref), -np.inf, ref)
    n_top = min(top_n, v)
    for r in range(n):
        fin = ref[r][np.isfinite(ref[r])]
        bound = 0.0 if family in EXACT else 5e-5 * float(np.max(np.abs(fin))) + 1e-4
        order = np.argsort(-key[r], kind="stable")
        if family not in EXACT:  # the reference's ranking is unambiguous at the bound, down to rank n_top + 1
            ranked = key[r][order[:n_top + 1]]
            assert np.all(ranked[:-1] - ranked[1:] > 2 * bound), (r, ranked)
        got = rec[r]
        assert got["n_top"] == n_top and got["token"] == targets[r]
        assert np.array_equal(got["top_id"][:n_top], order[:n_top]), (r, got["top_id"][:n_top], order[:n_top])
        want = key[r][order[:n_top]]
        inf = np.isinf(want)
        assert np.array_equal(got["top_logit"][:n_top][inf], want[inf]) and np.all(np.abs(got["top_logit"][:n_top][~inf] - want[~inf]) <= bound), r
        if fin.size:
            lse = float(fin.max() + np.log(np.sum(np.exp(fin - fin.max()))))
            assert abs(float(got["lse"]) - lse) <= 5e-5 * float(np.max(np.abs(fin))) + 1e-4, (r, got["lse"], lse)
        else:
            assert np.isnan(got["lse"])
        tl = ref[r][targets[r]] if targets[r] >= 0 else np.nan
        if np.isfinite(tl):
            assert abs(float(got["logit"]) - tl) <= bound, (r, got["logit"], tl)
        else:
            assert np.array_equal(np.float32(got["logit"]), np.float32(tl), equal_nan=True), (r, got["logit"], tl)
