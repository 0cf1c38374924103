"""CPU: tests/gemm_ref.py, the model tests/test_gemm_instances_gpu.py holds the tiled matmul's kernels against.

1. the model is the oracle's operation: its dense weights, its quantised products and its LayerNorm against oracle.gemv_qk256 / gemv_qk256_f64 /
   i2s_matmul / layernorm at the tolerances tests/test_gemm_parity.py uses.
2. the bounds are tight enough to catch real faults: each fault below is injected into the model and must leave the bound behind TENFOLD in at least
   one output (where the bound is 0 -- the exact forms -- it must change an output): digit plane 0 dropped, two tokens of a 16-token group swapped,
   the last 256-column block taken from the one before (a stale tile), one 32-block read with its neighbour's scale, the last row tile not written,
   one row block computed from another's weights.
3. the exact inputs ARE exact: for every case of the GPU file the largest partial sum any summation order can reach stays below 2^24 units.
4. the records' fast reader agrees with tests/qb32_ref.decode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402
import qb32_ref  # noqa: E402
import test_gemm_instances_gpu as G  # noqa: E402  (its case table and input generators; nothing there touches a GPU at import)


def approx_tol(cols):
    return min(2e-4 * np.sqrt(cols / 256.0), 1e-3)


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("rows,cols,m", [(48, 256, 3), (100, 300, 5), (64, 1100, 4)])
def test_model_matches_the_oracle_on_qk256(oracle, rows, cols, m):
    mat = R.make_matrix("qk256", rows, cols, rows + cols)
    qs, stride = mat.upload["qs"].reshape(-1), mat.upload["stride"]
    rng = np.random.default_rng(cols)
    x = rng.uniform(-10, 10, (m, cols)).astype(np.float32)
    x[m // 2] *= 1e-3
    f64 = np.stack([oracle.gemv_qk256_f64(qs, x[i], rows, cols, stride) for i in range(m)])
    assert np.allclose(x.astype(np.float64) @ mat.dense.T, f64, rtol=1e-12, atol=1e-9)  # the dense matrix IS the oracle's weights
    want = np.stack([oracle.gemv_qk256(qs, x[i], rows, cols, stride) for i in range(m)])
    for digits in (4, 3, 2):
        p = R.product_int8(*R.quant_rows(x, digits), mat, digits)
        if digits >= 3:  # test_gemm_parity.test_qk256_gemm_matches_oracle_rows' gate
            scale = np.maximum(1.0, np.abs(x).sum(axis=1, keepdims=True) * 2e-7 / approx_tol(cols))
            assert np.all((np.abs(p.want - want) <= approx_tol(cols) * scale) | (np.abs(p.want - want) <= 2e-2 * np.abs(want))), digits
        for i in range(m):
            a, b = p.want[i], want[i].astype(np.float64)
            assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b)) >= 0.99999, (digits, i)
    pf = R.product_fp6(*R.quant_rows(x, 2), mat)
    assert np.array_equal(pf.want, R.product_int8(*R.quant_rows(x, 2), mat, 2).want)  # the same integer, the same scale


@pytest.mark.parametrize("kind,block", [("i2s256", 256), ("i2s32", 32), ("i2s32h", 32)])
def test_model_matches_the_oracle_on_block_scales(oracle, kind, block):
    n, k, m = 48, 512, 5
    mat = R.make_matrix(kind, n, k, 11 + block)
    x = np.random.default_rng(block).uniform(-4, 4, (m, k)).astype(np.float32)
    want = oracle.i2s_matmul(x.reshape(-1), mat.upload["packed"].reshape(-1), mat.upload["scales"].reshape(-1), m, n, k, block).reshape(m, n)
    for digits in (4, 3):  # test_gemm_parity.test_ternary_scaled_gemm's gates
        p = R.product_int8(*R.quant_rows(x, digits), mat, digits)
        assert np.max(np.abs(p.want - want)) <= 2e-5 * np.max(np.abs(want)) + 1e-6, digits
    p = R.product_int8(*R.quant_rows(x, 2), mat, 2)
    assert np.max(np.abs(p.want - want)) <= 2e-4 * np.max(np.abs(want)) + 1e-6
    if kind == "i2s32h":  # f16 activations: 7 sigma of the element roundings, as there
        p = R.product_f16(*R.quant_rows_f16(x), mat)
        sigma = 2.0 ** -11.5 / np.sqrt(3.0) * np.sqrt((x.astype(np.float64) ** 2) @ (mat.dense ** 2).T)
        assert np.all(np.abs(p.want - want) <= 7.0 * sigma + 1e-6)
        pc = R.product_f16(R.rows_to_f16(x), np.ones(m), mat)
        assert np.all(np.abs(pc.want - want) <= 7.0 * sigma + 1e-6)
        q, s = R.quant_qb32(x)
        assert np.max(np.abs(R.qb32_values(q, s) - x)) <= 2.0 ** -13 * np.abs(x).max()  # a QB32 value is within half a step of its unit


def test_model_layernorm_matches_the_oracle(oracle):
    rng = np.random.default_rng(3)
    m, k = 6, 300
    x = rng.normal(0.1, 1.0, (m, k)).astype(np.float32)
    g = (rng.uniform(0.5, 1.5, k) / 80).astype(np.float32)
    got = R.layernorm_rows(x, g, 1e-5)
    want = np.stack([oracle.layernorm(x[i], g, 1e-5) for i in range(m)])
    assert np.max(np.abs(got - want)) <= 3e-5 * np.max(np.abs(want)) + 1e-6  # test_gemm_fusions_ln_residual_silu's gate
    q, inv = R.quant_rows(x, 4, (g, 1e-5))
    assert np.max(np.abs(q * inv[:, None] - want)) <= 3e-5 * np.max(np.abs(want)) + 1e-6


def test_digits_recombine_and_tiles_interleave():
    q = np.random.default_rng(1).integers(-(1 << 14), (1 << 14) + 1, (7, 64))
    d = R.digits256(q, 2)
    assert np.array_equal(d[0] + 256 * d[1], q) and np.abs(d[0]).max() <= 128 and np.abs(d[1]).max() <= 64
    d = R.digits32(q)
    assert np.array_equal(d[0] + 32 * d[1] + 1024 * d[2], q) and np.abs(d).max() <= 16
    q4 = np.random.default_rng(2).integers(-(1 << 30), (1 << 30) + 1, (7, 64))
    d = R.digits256(q4, 4)
    assert np.array_equal(sum(d[i] << (8 * i) for i in range(4)), q4) and np.abs(d).max() <= 128
    a, b = np.arange(32).reshape(32, 1), 100 + np.arange(32).reshape(32, 1)
    t = R.interleave16(a, b)[:, 0]
    assert list(t[:16]) == list(range(16)) and list(t[16:32]) == list(range(100, 116)) and list(t[32:48]) == list(range(16, 32))


# ---------------------------------------------------------------- 2. the bounds catch real faults
FK, FM, FROWS = 512, 48, 512  # two 256-column blocks, three 16-token groups, two row blocks
FORMS = [("int8", "qk256", 2), ("int8", "qk256", 3), ("int8", "qk256", 4), ("int8", "i2s256", 2), ("int8", "i2s256", 3), ("int8", "i2s256", 4),
         ("int8", "i2s32", 2), ("int8", "i2s32", 3), ("int8", "i2s32", 4), ("int8", "i2s32h", 3), ("int8", "i2s32h", 4), ("f16q", "i2s32h", 2),
         ("f16q", "qk256", 2), ("chain", "qk256", 2), ("chain", "i2s32h", 2), ("fp6", "qk256", 2), ("qb32", "qk256", 2)]
FAULTS = ["plane0", "tokens", "stale", "scale", "row_tile", "row_block"]


def quantise(form, x, digits):
    if form in ("int8", "fp6"):
        return R.quant_rows(x, digits)
    if form == "f16q":
        return R.quant_rows_f16(x)
    return (R.rows_to_f16(x), np.ones(x.shape[0])) if form == "chain" else R.quant_qb32(x)


def product(form, a, b, mat, digits):
    if form == "int8":
        return R.product_int8(a, b, mat, digits)
    if form == "fp6":
        return R.product_fp6(a, b, mat)
    return R.product_qb32(a, b, mat) if form == "qb32" else R.product_f16(a, b, mat)


def faulty_output(form, fault, a, b, mat, digits):
    """the model's output under one fault (None: the form has nothing the fault could touch)"""
    a, wint, scale = a.copy(), mat.wint.copy(), None if mat.scale is None else mat.scale.copy()
    if fault == "plane0":
        if form in ("f16q", "chain"):
            return None  # f16 rows have no digit planes
        a = a - (R.digits32(a)[0] if form in ("fp6", "qb32") else R.digits256(a, digits)[0])
    elif fault == "stale":
        a[:, 256:] = a[:, :256]
    elif fault == "scale":
        if scale is None:
            return None
        blk = mat.block
        scale[:, blk:2 * blk] = scale[:, 2 * blk:3 * blk] if blk == 32 else scale[:, :blk]
    elif fault == "row_block":
        wint[256:] = wint[:256]
        if scale is not None:
            scale[256:] = scale[:256]
    out = product(form, a, b, R.Matrix(mat.kind, wint, scale, mat.block, {}), digits).want.copy()
    if fault == "tokens":
        out[[17, 22]] = out[[22, 17]]
    elif fault == "row_tile":
        out[:, -16:] = np.nan  # what the buffer held before the launch
    return out


@pytest.mark.parametrize("form,kind,digits", FORMS)
def test_every_fault_leaves_the_bound_behind_tenfold(form, kind, digits):
    mat = R.make_matrix(kind, FROWS, FK, G.seed_of("fault", kind))
    x = R.float_rows(FM, FK, G.seed_of("fault", form, digits))
    # the last 16-token group carries an outlier channel, 2^21 times the others: its rows live on the low digit planes, which is where the 4-digit
    # forms' plane 0 is visible at all in an f32 output (beside a full-scale sum it is 2^-22 of the value: under one rounding)
    x[32:, 5] *= 2.0 ** 21
    a, b = quantise(form, x, digits)
    p = product(form, a, b, mat, digits)
    target = np.where(p.bound == 0, p.exact32.astype(np.float64), p.want)
    assert np.all(np.abs(p.want - target) <= p.bound + R.U * np.abs(p.want))  # (the exact value is the want, rounded once)
    for fault in FAULTS:
        bad = faulty_output(form, fault, a, b, mat, digits)
        if bad is None:
            continue
        with np.errstate(over="ignore"):
            got = bad.astype(np.float32).astype(np.float64)  # what an f32 buffer would hold
        err = np.abs(got - target)
        caught = ~(err <= 10.0 * p.bound)
        print(form, kind, digits, fault, "outputs beyond 10 x bound:", int(caught.sum()), "of", caught.size)
        assert caught.any(), (form, kind, digits, fault)


# ---------------------------------------------------------------- 3. the exact inputs are exact
def _all_cases():
    seen, out = set(), []
    for name, case in list(G.CASES.items()) + [(n, c) for _, cs in G.ENV_CASES.values() for n, c in cs.items()]:
        key = (G.form_of(name, case), case[1], case[2], case[3], case[4])
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(name, case, id=name))
    return out


@pytest.mark.parametrize("name,case", _all_cases())
def test_exact_inputs_stay_below_2_24_units(name, case):
    units = G.exact_units(name, case)
    if units is None:
        # 2 digits, unscaled int8 planes: |digit| <= 128, |w| <= 2, K = 256: |D_d| <= 2^16 -- exact int32 sums, exact conversions, one rounding
        form, mat = G.form_of(name, case), G.matrix_for(case[1], case[2], case[2], "pow2")
        assert form == "int8" and mat.scale is None and np.abs(mat.wint).max() <= 2 and 128 * 2 * G.K < 1 << 24
        return
    print(name, "largest partial sum:", float(units.max()), "units")
    assert units.max() < R.EXACT_UNITS, (name, float(units.max()))
    # ... and the model draws the same conclusion: bound 0 everywhere
    entry, kind, rows, m, digits, flags, _ = case
    x = G.rows_of(G.form_of(name, case), digits, m, "exact")[:64]
    p = G.model(G.form_of(name, case), x, G.matrix_for(kind, rows, rows, "pow2"), digits)
    assert not p.bound.any() and p.exact32 is not None


def test_exact_inputs_quantise_to_the_integers_they_were_built_from():
    m = 40
    x = G.rows_of("int8", 2, m, "exact")
    q, inv = R.quant_rows(x, 2)
    assert np.array_equal(q * inv[:, None], x.astype(np.float64)) and np.abs(q).max() == 8192
    for digits in (3, 4):
        q, inv = R.quant_rows(G.rows_of("int8", digits, m, "exact"), digits)
        d = R.digits256(q, digits)
        assert not d[:-1].any() and np.abs(d[-1]).max() == 32  # the top plane alone
    xh, inv = R.quant_rows_f16(G.rows_of("f16q", 2, m, "exact"))
    assert np.array_equal(xh * inv[:, None], G.rows_of("f16q", 2, m, "exact").astype(np.float64))
    assert np.array_equal(R.rows_to_f16(G.rows_of("chain", 2, m, "exact")), G.rows_of("chain", 2, m, "exact").astype(np.float64))
    xq = G.rows_of("qb32", 2, m, "exact")
    q, s = R.quant_qb32(xq)
    assert np.array_equal(R.qb32_values(q, s), xq.astype(np.float64))
    live = np.abs(xq).max(axis=1) > 0
    assert np.all(s[live] == s[live][:, :1])  # one exponent per row: every unit holds a peak


# ---------------------------------------------------------------- 4. the records' reader
def test_fast_record_reader_agrees_with_qb32_ref():
    rng = np.random.default_rng(9)
    m, cols = 70, 512
    mp, nblk = 128, 2
    mag = rng.integers(0, 17, (mp, nblk, 4, 3, 2, 32))
    code = (mag | (rng.integers(0, 2, mag.shape) << 5)).astype(np.uint8)
    bits = ((code[..., None] >> np.arange(6)) & 1).astype(np.uint8).reshape(mp, nblk, 4, 3, 2, 192)
    rec = np.zeros((mp, nblk, 592), np.uint8)
    rec[:, :, :576] = np.packbits(bits, axis=-1, bitorder="little").reshape(mp, nblk, 576)
    rec[:, :, 576:584] = rng.integers(100, 160, (mp, nblk, 8))
    buf = rec.reshape(-1)
    vals, exps = qb32_ref.decode(buf, m, cols)
    q, s = R.decode_fp6_records(buf, m, cols, 592)
    assert np.array_equal(s, exps.astype(np.int64)) and np.array_equal(R.qb32_values(q, s), vals)
