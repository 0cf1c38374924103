"""Pins the CPU oracle to the reference's own known-answer tests.

Each test names the reference test it replays (file:line under /root/reference).
CPU only; runs in seconds.
"""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q = "crates/bitnet-quantization/src"
K = "crates/bitnet-kernels/src"
M = "crates/bitnet-models/src"


# ---------------------------------------------------------------- QK256 ----


def test_unpack_block_smoke(oracle):
    """Q/i2s_qk256.rs:379-396"""
    qs = np.array([(0b11100100 + (i & 3)) & 0xFF for i in range(64)], np.uint8)
    codes = oracle.unpack_qk256_block(qs)
    assert (codes < 4).all()
    assert list(codes[:4]) == [0, 1, 2, 3]


def test_gemv_row_smoke(oracle):
    """Q/i2s_qk256.rs:399-416  all code 2 -> dot == sum(x)"""
    cols = 512
    row = np.full(128, 0xAA, np.uint8)
    x = (np.arange(cols, dtype=np.float32) * np.float32(0.01)).astype(np.float32)
    expected = np.float32(0)
    for v in x:  # sequential f32 sum, as iter().sum()
        expected = np.float32(expected + v)
    got = oracle.gemv_qk256_row(row, x, cols)
    assert abs(got - float(expected)) < 1e-3


def test_gemv_row_with_tail(oracle):
    """Q/i2s_qk256.rs:419-437  cols=300"""
    cols = 300
    row = np.full(2 * 64, 0xAA, np.uint8)
    x = (np.arange(cols) % 7).astype(np.float32)
    assert abs(oracle.gemv_qk256_row(row, x, cols) - float(x.sum())) < 1e-3


@pytest.mark.parametrize("impl", ["dispatch", "scalar", "avx2"])
def test_gemv_multi_row(oracle, impl):
    """Q/i2s_qk256.rs:440-465  0x55 -> -sum(x)"""
    if impl == "avx2" and not oracle.have_avx2():
        pytest.skip("no AVX2")
    rows, cols = 3, 256
    qs = np.full(rows * 64, 0x55, np.uint8)
    x = np.arange(cols, dtype=np.float32)
    y = oracle.gemv_qk256(qs, x, rows, cols, 64, impl=impl)
    assert np.all(np.abs(y + x.sum()) < 1e-3)


def test_code_to_f32_lut(oracle):
    """Q/i2s_qk256.rs:468-474, :560-565"""
    assert [oracle.code_to_f32(c) for c in range(4)] == [-2.0, -1.0, 1.0, 2.0]


def test_size_tolerance(oracle):
    """Q/i2s_qk256.rs:499-541  I2SQk256NoScale::new +-128 B"""
    rows, cols = 512, 1024
    exact = rows * 256
    assert oracle.i2s_qk256_new(rows, cols, exact) == 256
    assert oracle.i2s_qk256_new(rows, cols, exact + 32) == 256
    assert oracle.i2s_qk256_new(rows, cols, exact + 128) == 256
    with pytest.raises(oracle.OracleError, match="data size mismatch"):
        oracle.i2s_qk256_new(rows, cols, exact + 129)
    with pytest.raises(oracle.OracleError):
        oracle.i2s_qk256_new(rows, cols, exact // 2)


def test_block_decode_golden(oracle):
    """Q/i2s_qk256.rs:575-621  cycling codes"""
    qs = np.zeros(64, np.uint8)
    for i in range(64):
        base = i * 4
        qs[i] = (base % 4) | (((base + 1) % 4) << 2) | (((base + 2) % 4) << 4) | (((base + 3) % 4) << 6)
    codes = oracle.unpack_qk256_block(qs)
    assert np.array_equal(codes, np.arange(256) % 4)
    w = np.array([oracle.code_to_f32(int(c)) for c in codes], np.float32)
    rms = float(np.sqrt((w * w).sum() / 256))
    assert 0.1 <= rms <= 5.0
    assert {-2.0, -1.0, 1.0, 2.0} <= set(w[:16].tolist())


def test_tiny_gemv_e2e(oracle):
    """Q/i2s_qk256.rs:630-677  1x256 ones -> 256.0"""
    y = oracle.gemv_qk256(np.full(64, 0xAA, np.uint8), np.ones(256, np.float32), 1, 256, 64)
    assert abs(y[0] - 256.0) < 1e-4


def test_negatives_dimension_checks(oracle):
    """Q/i2s_qk256.rs:691-742 (+ :476-484) error substrings"""
    with pytest.raises(oracle.OracleError, match="x length"):
        oracle.gemv_qk256(np.zeros(64, np.uint8), np.ones(246, np.float32), 1, 256, 64)
    with pytest.raises(oracle.OracleError, match="too short"):
        oracle.gemv_qk256(np.zeros(64, np.uint8), np.ones(256, np.float32), 2, 256, 64)
    with pytest.raises(oracle.OracleError, match="y_out length"):
        oracle.gemv_qk256(np.zeros(128, np.uint8), np.ones(256, np.float32), 2, 256, 64, y_len=1)
    with pytest.raises(oracle.OracleError, match="y_out length"):
        oracle.gemv_qk256(np.zeros(64, np.uint8), np.zeros(256, np.float32), 1, 256, 64, y_len=2)
    # :749-762 stride mismatch (debug_assert "row bytes mismatch")
    with pytest.raises(oracle.OracleError, match="row bytes mismatch"):
        oracle.gemv_qk256(np.zeros(128, np.uint8), np.ones(256, np.float32), 1, 256, 128)


def test_dispatch_smoke_minus_128(oracle):
    """Q/qk256_dispatch.rs:106-119  0x55, act 0.5, 256x256 -> all -128.0"""
    rows = cols = 256
    packed = np.full(rows * cols // 4, 0x55, np.uint8)
    y = oracle.gemv_qk256(packed, np.full(cols, 0.5, np.float32), rows, cols, 64)
    assert np.all(y == -128.0)
    # the legacy scalar map (:83-89) sends code 1 -> 0
    y2 = oracle.qk256_dispatch_gemv_scalar(rows, cols, packed, np.ones(rows, np.float32), np.full(cols, 0.5, np.float32))
    assert np.all(y2 == 0.0)


def _avx2_tol(cols):
    """Q/i2s_qk256_avx2.rs:411-429"""
    return min(1e-5 * np.sqrt(cols // 256), 5e-4), 1e-4


@pytest.mark.parametrize("rows,cols,seed", [(4, 256, 42), (16, 512, 1), (8, 1024, 2), (3, 300, 3), (5, 2560, 4), (2, 6912, 5), (7, 263, 6)])
def test_avx2_matches_scalar(oracle, rows, cols, seed):
    """Q/i2s_qk256_avx2.rs:370-429 and
    crates/bitnet-models/tests/qk256_avx2_correctness.rs (random bytes, x in
    [-10,10), tol abs min(1e-5*sqrt(blocks),5e-4) or rel 1e-4)."""
    if not oracle.have_avx2():
        pytest.skip("no AVX2")
    rng = np.random.default_rng(seed)
    stride = -(-cols // 256) * 64
    qs = rng.integers(0, 256, rows * stride, dtype=np.uint8)
    x = rng.uniform(-10, 10, cols).astype(np.float32)
    ys = oracle.gemv_qk256(qs, x, rows, cols, stride, impl="scalar")
    ya = oracle.gemv_qk256(qs, x, rows, cols, stride, impl="avx2")
    yt = oracle.gemv_qk256_f64(qs, x, rows, cols, stride)
    abs_tol, rel_tol = _avx2_tol(max(cols, 256))
    for s, a in zip(ys, ya):
        d = abs(float(s) - float(a))
        rel = d / abs(float(s)) if abs(s) > 1e-12 else d
        assert d <= max(abs_tol, 1e-3) or rel <= rel_tol  # reference smoke tol; sizes >256 use rel
    # both within f32 rounding of the f64 truth
    assert np.max(np.abs(ys - yt)) < 2e-2
    assert np.max(np.abs(ya - yt)) < 2e-2
    ym = oracle.gemv_qk256(qs, x, rows, cols, stride, impl="avx2_mt", threads=3)
    assert np.array_equal(ym, ya)


def test_qk256_vs_f32_reference_correlation(oracle):
    """crossval/tests/qk256_crossval.rs:245-326  64x1024, corr >= 0.998 vs a
    dequantize-then-f32 GEMV (here: exact 1.0 modulo rounding)."""
    rng = np.random.default_rng(42)
    rows, cols = 64, 1024
    qs = rng.integers(0, 256, rows * 256, dtype=np.uint8)
    x = rng.uniform(-1, 1, cols).astype(np.float32)
    y = oracle.gemv_qk256(qs, x, rows, cols, 256)
    lut = np.array([-2, -1, 1, 2], np.float32)
    codes = ((qs.reshape(rows, 256, 1) >> np.array([0, 2, 4, 6])) & 3).reshape(rows, cols)
    yref = lut[codes] @ x
    corr = np.corrcoef(y, yref)[0, 1]
    assert corr >= 0.998


# ------------------------------------------------------------- ternary ----


def _pack_weight_matrix(w, k, n, bs):
    """K/cpu/quantized_matmul.rs:268-292"""
    packed_k = -(-k // 4)
    packed = np.zeros(packed_k * n, np.uint8)
    for col in range(n):
        for row in range(k):
            v = w[row * n + col]
            code = 1 if v == 1 else 3 if v == -1 else 0
            packed[col * packed_k + row // 4] |= code << ((row % 4) * 2)
    return packed, np.ones(n * -(-k // bs), np.float32)


def _naive(a, w, m, n, k):
    a = np.asarray(a, np.float32).reshape(m, k)
    w = np.asarray(w, np.float32).reshape(k, n)
    out = np.zeros((m, n), np.float32)
    for i in range(m):
        for j in range(n):
            s = np.float32(0)
            for l in range(k):
                s = np.float32(s + np.float32(a[i, l] * w[l, j]))
            out[i, j] = s
    return out.reshape(-1)


_SHAPES = [
    # (m, n, k, bs, weight pattern, act fn, tol)  -- K/cpu/quantized_matmul.rs:343-493
    (2, 2, 2, 32, lambda i: [1, 0, 0, 1][i], lambda i: [3.0, -2.0, 5.0, 7.0][i], 1e-6),
    (2, 2, 2, 256, lambda i: [1, 0, 0, 1][i], lambda i: [3.0, -2.0, 5.0, 7.0][i], 1e-6),
    (4, 4, 4, 32, lambda i: 1, lambda i: float(i), 1e-5),
    (3, 3, 4, 32, lambda i: -1, lambda i: 1.0, 1e-5),
    (4, 4, 8, 32, lambda i: 0, lambda i: 42.0, 1e-6),
    (3, 5, 8, 32, lambda i: 1, lambda i: 0.0, 1e-6),
    (16, 16, 16, 32, lambda i: [1, -1, 0, 1][i % 4], lambda i: np.float32(i) * np.float32(0.1), 1e-4),
    (7, 5, 11, 32, lambda i: [-1, 0, 1][i % 3], lambda i: np.float32(i) * np.float32(0.05) - np.float32(1.0), 1e-4),
    (13, 9, 17, 256, lambda i: [0, 1, -1][i % 3], lambda i: float((i * 7 + 3) % 10) - 5.0, 1e-4),
    (32, 64, 32, 32, lambda i: [1, 0, -1, 0][i % 4], lambda i: np.sin(np.float32(i)), 1e-3),
    (64, 32, 256, 256, lambda i: [1, -1][i % 2], lambda i: np.float32(i) * np.float32(0.001), 1e-3),
    (1, 1, 1, 32, lambda i: 1, lambda i: 7.5, 1e-6),
    (1, 8, 4, 32, lambda i: [1, -1, 0, 1][i % 4], lambda i: float(i + 1), 1e-5),
    (6, 1, 4, 32, lambda i: [1, -1, 1, -1][i], lambda i: float(i), 1e-5),
    (3, 2, 5, 32, lambda i: [1, 0, -1, 1, 0, 1, -1, 0, 1, -1][i], lambda i: float(i) + 0.5, 1e-5),
    (4, 4, 8, 32, lambda i: [1, -1, 0][i % 3], lambda i: float(i % 5), 0.0),  # :618-631 bit-exact
]


@pytest.mark.parametrize("case", range(len(_SHAPES)))
def test_ternary_shape_sweep(oracle, case):
    m, n, k, bs, wf, af, tol = _SHAPES[case]
    w = [wf(i) for i in range(k * n)]
    act = np.array([af(i) for i in range(m * k)], np.float32)
    packed, scales = _pack_weight_matrix(w, k, n, bs)
    expected = _naive(act, w, m, n, k)
    for impl in ("f32", "blocked", "dequant"):
        out = oracle.i2s_matmul(act, packed, scales, m, n, k, bs, impl=impl)
        assert np.max(np.abs(out - expected)) <= tol, impl


def test_snapshot_identity_weights(oracle):
    """crates/bitnet-kernels/tests/snapshot_kernel_outputs.rs:151-163 ->
    snapshots/...i2s_matmul_identity_weights.snap = [10.000000, 10.000000]"""
    wp = np.array([oracle.pack_i2s([1, 1, 1, 1])] * 2, np.uint8)
    out = oracle.i2s_matmul([1.0, 2.0, 3.0, 4.0], wp, [1.0, 1.0], 1, 2, 4, 4)
    assert "[" + ", ".join(f"{v:.6f}" for v in out) + "]" == "[10.000000, 10.000000]"


def test_snapshot_mixed_ternary(oracle):
    """snapshot_kernel_outputs.rs:165-177 -> ...mixed_ternary.snap = [6.000000]"""
    wp = np.array([oracle.pack_i2s([1, -1, 0, 1])], np.uint8)
    out = oracle.i2s_matmul([1.0, 2.0, 3.0, 4.0], wp, [2.0], 1, 1, 4, 4)
    assert "[" + ", ".join(f"{v:.6f}" for v in out) + "]" == "[6.000000]"


def test_non_unit_scales(oracle):
    """K/cpu/quantized_matmul.rs:555-613"""
    packed = np.full(2, 0b01010101, np.uint8)
    out = oracle.i2s_matmul(np.ones(8, np.float32), packed, [2.0, 0.5], 2, 2, 4, 32)
    assert np.allclose(out, [8.0, 2.0, 8.0, 2.0], atol=1e-5)
    packed = np.full(16, 0b01010101, np.uint8)
    out = oracle.i2s_matmul(np.ones(64, np.float32), packed, [1.0, 3.0], 1, 1, 64, 32)
    assert np.allclose(out, [128.0], atol=1e-4)


def test_pack_i2s_roundtrip(oracle):
    """K/cpu/quantized_matmul.rs:675-701"""
    b = oracle.pack_i2s([1, -1, 0, 1])
    assert [oracle.decode_i2s((b >> (2 * i)) & 3) for i in range(4)] == [1, -1, 0, 1]
    assert oracle.pack_i2s([0, 0, 0, 0]) == 0x00
    assert oracle.pack_i2s([1, 1, 1, 1]) == 0b01010101
    assert oracle.pack_i2s([-1, -1, -1, -1]) == 0b11111111
    assert oracle.decode_i2s(2) == 0


def test_ternary_validation(oracle):
    """K/cpu/quantized_matmul.rs:705-742"""
    a4, p4, s4 = np.ones(4, np.float32), np.zeros(4, np.uint8), np.ones(4, np.float32)
    for m, n, k in [(0, 2, 2), (2, 0, 2), (2, 2, 0)]:
        with pytest.raises(oracle.OracleError, match="dimensions must be > 0"):
            oracle.i2s_matmul(a4, p4, s4, m, n, k, 32, out_len=4)
    with pytest.raises(oracle.OracleError, match="block_size must be > 0"):
        oracle.i2s_matmul(a4, p4[:2], s4[:2], 2, 2, 2, 0)
    with pytest.raises(oracle.OracleError, match="activations too small"):
        oracle.i2s_matmul(a4[:2], p4, s4, 2, 2, 4, 32)
    with pytest.raises(oracle.OracleError, match="output too small"):
        oracle.i2s_matmul(a4, p4[:2], s4[:2], 2, 2, 2, 32, out_len=1)


def test_three_kernels_agree_large(oracle):
    """K/cpu/quantized_matmul.rs:746-768"""
    m, n, k = 16, 8, 48
    for bs in (32, 256):
        w = [[1, 0, -1, 1, -1][i % 5] for i in range(k * n)]
        packed, scales = _pack_weight_matrix(w, k, n, bs)
        act = np.sin(np.arange(m * k, dtype=np.float32) * np.float32(0.03)).astype(np.float32)
        o1 = oracle.i2s_matmul(act, packed, scales, m, n, k, bs, impl="f32")
        o2 = oracle.i2s_matmul(act, packed, scales, m, n, k, bs, impl="blocked")
        o3 = oracle.i2s_matmul(act, packed, scales, m, n, k, bs, impl="dequant")
        assert np.max(np.abs(o1 - o2)) <= 1e-4 and np.max(np.abs(o1 - o3)) <= 1e-4


# ------------------------------------------------------------ provider ----


def test_fallback_matmul_identity(oracle):
    """K/cpu/fallback.rs:306-318  A . I = A"""
    c = oracle.matmul_i2s([1, 2, 3, 4], [1, 0, 0, 1], 2, 2, 2)
    assert c.tolist() == [1.0, 2.0, 3.0, 4.0]


def test_fallback_matmul_dimension_validation(oracle):
    """K/cpu/fallback.rs:320-331"""
    with pytest.raises(oracle.OracleError, match="dimension mismatch"):
        oracle.matmul_i2s([1, 2], [1, 0], 2, 2, 2, c_len=4)


def test_fallback_quantize_i2s(oracle):
    """K/cpu/fallback.rs:334-360"""
    out, scales = oracle.quantize_i2s([1.5, -1.0, 0.5, -0.5, 0.0, 2.0, -2.0, 0.1])
    assert scales[0] > 0 and out.any()
    # scale = 2.0/1.5; codes: 1.5/s=1.125->1, -1/s=-.75->3, .5/s=.375->0, -.375->0 | 0->0, 1.5->1, -1.5->3, .075->0
    assert np.isclose(scales[0], 2.0 / 1.5)
    assert out.tolist() == [1 | (3 << 2), (1 << 2) | (3 << 4)]
    with pytest.raises(oracle.OracleError, match="too small"):
        oracle.quantize_i2s(np.ones(32, np.float32), out_len=1)


# -------------------------------------------------------- block dequant ----


def _pack_codes(codes):
    out = []
    for i in range(0, len(codes), 4):
        b = 0
        for j, c in enumerate(codes[i : i + 4]):
            b |= (c & 3) << (2 * j)
        out.append(b)
    return np.array(out, np.uint8)


F16_ONE, F16_TWO = 0x3C00, 0x4000


def test_i2s_lut_mapping_sym_k1(oracle):
    """M/quant/i2s.rs:922-945  codes 0..3, f16 1.0 -> -2,-1,1,2"""
    dst = oracle.i2s_dequant_block(_pack_codes([0, 1, 2, 3]), 4, F16_ONE)
    assert dst.tolist() == [-2.0, -1.0, 1.0, 2.0]


def test_i2s_extreme_scale_values(oracle):
    """M/quant/i2s.rs:1006-1057  clamp [1e-3, 1e3]"""
    q = _pack_codes([0, 1, 2, 3])
    z = oracle.i2s_dequant_block(q, 4, 0x0000)
    assert np.all(np.abs(z) <= 2e-3 + 1e-6) and np.allclose(np.abs(z), [2e-3, 1e-3, 1e-3, 2e-3])
    inf = oracle.i2s_dequant_block(q, 4, 0x7C00)
    assert np.all(np.isfinite(inf)) and np.allclose(np.abs(inf), [2e3, 1e3, 1e3, 2e3])
    assert np.all(np.isfinite(oracle.i2s_dequant_block(q, 4, 0x7BFF)))
    # negative scale -> abs()
    assert oracle.i2s_dequant_block(q, 4, 0xC000).tolist() == [-4.0, -2.0, 2.0, 4.0]


def test_i2s_code_boundary_values(oracle):
    """M/quant/i2s.rs:1172-1201"""
    lut = [-2.0, -1.0, 1.0, 2.0]
    for code in range(4):
        assert oracle.i2s_dequant_block(_pack_codes([code] * 4), 4, F16_ONE).tolist() == [lut[code]] * 4


def _create_i2s_test_data(rows, cols, block):
    """M/quant/i2s.rs:1238-1268"""
    bpr = -(-cols // block)
    qbits = -(-block // 4)
    out = bytearray()
    for _ in range(rows * bpr):
        out += bytes(((0b11100100 + i) & 0xFF) for i in range(qbits))
        out += bytes([0x00, 0x3C])
    return np.frombuffer(bytes(out), np.uint8)


def test_i2s_infer_block_and_sizes(oracle):
    """M/quant/i2s.rs:1143-1170"""
    assert oracle.i2s_infer_block_size(66, 1, 256) == 256
    assert oracle.i2s_infer_block_size(34, 1, 128) == 128
    assert oracle.i2s_infer_block_size(1, 1, 256) is None
    assert oracle.i2s_expected_bytes(1, 1024 * 1024, 256) > 0
    assert oracle.i2s_expected_bytes(2, 64, 32) == 40  # BitNet32-F16: 10 B / 32 elems


@pytest.mark.parametrize("rows,cols,block", [(1, 256, 256), (1, 128, 128), (1, 64, 64), (2, 32, 32), (6, 256, 256), (2, 64, 32)])
def test_i2s_block_sizes_and_transpose_parity(oracle, rows, cols, block):
    """M/quant/i2s.rs:1084-1107, :1203-1236, :947-1004 (transposed parity)"""
    data = _create_i2s_test_data(rows, cols, block)
    a = oracle.i2s_dequantize_to_f32(data, rows, cols)
    bt = oracle.i2s_dequantize_to_f32(data, rows, cols, transposed=True)
    assert np.all(np.isfinite(a)) and a.size == rows * cols
    assert np.array_equal(a.reshape(rows, cols), bt.reshape(cols, rows).T)
    # independent numpy decode
    lut = np.array([-2, -1, 1, 2], np.float32)
    per = block // 4 + 2
    blocks = data.reshape(-1, per)
    codes = ((blocks[:, : block // 4, None] >> np.array([0, 2, 4, 6])) & 3).reshape(-1, block)
    assert np.array_equal(a, lut[codes].reshape(-1))


def test_i2s_transposed_parity_small(oracle):
    """M/quant/i2s.rs:947-1004: 3x10 'block=8' bytes match no inferable block
    size -> both walkers take the partial path with block 256 and 0 available
    blocks -> all zeros, MSE 0 (the reference test passes this way)."""
    rows, cols = 3, 10
    one = _pack_codes(([0, 1, 2, 3] * 8)[:8])
    data = np.concatenate([np.concatenate([one[:2], np.array([0x00, 0x40], np.uint8)])] * 6)
    a = oracle.i2s_dequantize_to_f32(data, rows, cols)
    bt = oracle.i2s_dequantize_to_f32(data, rows, cols, transposed=True)
    assert np.all(a == 0) and np.all(bt == 0)


def test_i2s_partial_block_processing(oracle):
    """M/quant/i2s.rs:1109-1141: half the rows present -> decoded then zero fill"""
    full = _create_i2s_test_data(2, 256, 256)
    out = oracle.i2s_dequantize_to_f32(full, 4, 256).reshape(4, 256)
    ref = oracle.i2s_dequantize_to_f32(full, 2, 256).reshape(2, 256)
    # :425-429 quirk: a row's last block is not counted, so all present rows decode
    assert np.array_equal(out[:2], ref) and np.all(out[2:] == 0)
    assert np.all(oracle.i2s_dequantize_to_f32(np.zeros(0, np.uint8), 1, 256) == 0)


def test_i2s_tail_block_consumes_fewer_bytes(oracle):
    """M/quant/i2s.rs:300-321: a tail block of n elems stores ceil(n/4)+2 bytes."""
    # 1 row x 40 cols, block 32 -> expected_bytes says 2*(8+2)=20, walker reads 8+2 then 2+2
    data = np.array([0xE4] * 8 + [0x00, 0x3C] + [0xE4] * 2 + [0x00, 0x40] + [0] * 6, np.uint8)
    assert oracle.i2s_infer_block_size(20, 1, 40) == 32
    out = oracle.i2s_dequantize_to_f32(data, 1, 40)
    assert out[:4].tolist() == [-2, -1, 1, 2] and out[32:36].tolist() == [-4, -2, 2, 4]


# ------------------------------------------------------- Q/utils.rs -----


def test_pack_unpack_2bit(oracle):
    """Q/utils.rs:266-272"""
    vals = [-2, -1, 0, 1, -2, 1]
    packed = oracle.pack_2bit_values(vals)
    assert oracle.unpack_2bit_values(packed, len(vals)).tolist() == vals
    assert oracle.pack_2bit_values([5, -9, 0, 1]).tolist() == [3 | (0 << 2) | (2 << 4) | (3 << 6)]
    d = oracle.dequantize_blocks(oracle.unpack_2bit_values(packed, 6), [0.5], 32)
    assert d.tolist() == [-1.0, -0.5, 0.0, 0.5, -1.0, 0.5]


# -------------------------------------------- oracle/_ref (real reference) ----


def test_vendored_ggml_pins_lut_and_bit_order(oracle):
    """The reference's own C (ggml-quants.c:59-72) pins: sizeof(block_iq2_s)=82, LSB-first extraction, qmap {-2,-1,1,2},
    f16 d conversion.  Its outputs are recorded in tests/golden/iq2s_ref_dequant.npz (tests/golden/make_iq2s_ref_fixture.py)
    and compared against the oracle's restatement; where oracle/_ref is built, the live library must reproduce the recording."""
    golden = np.load(os.path.join(GOLDEN, "iq2s_ref_dequant.npz"))
    d_all, qs_all, y_all = golden["d_bits"], golden["qs"], golden["y"]
    assert d_all[0] == F16_ONE and np.all(qs_all[0] == 0xE4)
    assert y_all[0, :4].tolist() == [-2.0, -1.0, 1.0, 2.0]
    if oracle.ref_available():
        for d_bits, qs, y in zip(d_all, qs_all, y_all):
            assert np.array_equal(oracle.ref_dequantize_row_iq2_s(int(d_bits), qs), y)
    for d_bits, qs, y in zip(d_all[1:], qs_all[1:], y_all[1:]):
        d_bits = int(d_bits)
        codes = oracle.unpack_qk256_block(qs)
        d = np.float32(oracle.f16_to_f32(d_bits))
        mine = np.array([np.float32(d * np.float32(oracle.code_to_f32(int(c)))) for c in codes], np.float32)
        assert np.array_equal(y, mine)
        if 1e-3 <= float(d) <= 1e3:  # inside M/quant/i2s.rs's clamp the Sym dequant agrees too
            assert np.array_equal(oracle.i2s_dequant_block(qs, 256, d_bits), y)
    # f16 conversion agrees with numpy on every bit pattern
    allbits = np.arange(65536, dtype=np.uint16)
    np_f = allbits.view(np.float16).astype(np.float32)
    mine = np.array([oracle.f16_to_f32(int(b)) for b in allbits[::7]], np.float32)
    ok = (mine == np_f[::7]) | (np.isnan(mine) & np.isnan(np_f[::7]))
    assert ok.all()


# ------------------------------------------ transformer half of the oracle ----
# oracle/transformer_oracle.c restates the decode step's host-side operators.  The reference pins them with the
# tests replayed here (VERDICT r1 "pins for the transformer oracle"): LayerNorm properties
# (crates/bitnet-models/tests/layernorm_fix_tests.rs), split-half RoPE against the closed form
# (crates/bitnet-models/tests/rope_parity.rs), the RoPE table unit tests, property tests and snapshots
# (crates/bitnet-rope/src/lib.rs:108-163, tests/property_tests.rs, tests/snapshot_tests.rs) and RotaryEmbedding's
# behavioural tests (crates/bitnet-transformer/tests/rope_tests.rs).


def _mean_var(row):
    row = np.asarray(row, np.float32)
    mean = np.float32(row.sum(dtype=np.float32) / np.float32(row.size))
    var = np.float32(((row - mean) ** 2).sum(dtype=np.float32) / np.float32(row.size))
    return float(mean), float(var)


def test_layernorm_normalizes_over_last_dimension(oracle):
    """layernorm_fix_tests.rs:205-265: [6, 64] with a different mean per position -> every row mean ~ 0, variance ~ 1."""
    B, H = 6, 64
    i = np.arange(B * H, dtype=np.float32)
    x = ((np.sin(i / np.float32(H) * 5.0) + np.cos(i / np.float32(H) * 3.0)) * 2.0 + (i // H).astype(np.float32)).astype(np.float32).reshape(B, H)
    g = np.ones(H, np.float32)
    for r in range(B):
        mean, var = _mean_var(oracle.layernorm(x[r], g, 1e-5))
        assert abs(mean) < 1e-3 and abs(var - 1.0) < 0.1, (r, mean, var)


def test_layernorm_normalizes_per_position_independently(oracle):
    """layernorm_fix_tests.rs:268-326: two vectors with very different statistics."""
    H = 32
    i = np.arange(H, dtype=np.float32)
    v1 = (i / np.float32(H)) * np.float32(10.0)
    v2 = -(i / np.float32(H)) * np.float32(5.0) + np.float32(20.0)
    for v in (v1, v2):
        mean, var = _mean_var(oracle.layernorm(v.astype(np.float32), np.ones(H, np.float32), 1e-5))
        assert abs(mean) < 1e-3 and abs(var - 1.0) < 0.1


def test_layernorm_output_differs_from_rmsnorm(oracle):
    """layernorm_fix_tests.rs:328-400: the mean-subtracting LayerNorm the transformer uses is NOT RMSNorm."""
    H = 128
    xx = np.arange(H, dtype=np.float32) / np.float32(H)
    x = (np.sin(xx * 8.0) * 3.0 + 5.0).astype(np.float32)
    g = np.ones(H, np.float32)
    ln, rms = oracle.layernorm(x, g, 1e-5), oracle.rmsnorm(x, g, 1e-5)
    assert abs(float(ln.mean())) < 1e-3
    assert abs(float(rms.mean())) > 0.5
    assert float(np.abs(ln - rms).mean()) > 0.1
    # the RMSNorm of K/rocm/rmsnorm.rs is x / sqrt(mean(x^2) + eps) * gamma
    want = x / np.sqrt(np.float32((x.astype(np.float64) ** 2).mean()) + np.float32(1e-5))
    assert np.allclose(rms, want, rtol=1e-6)


def _rope_closed_form(x, pos, theta=10000.0):
    """apply_rope_reference of rope_parity.rs:16-52 in f32 numpy."""
    x = np.asarray(x, np.float32)
    D = x.shape[-1]
    half = D // 2
    i = np.arange(half)
    freq = (i * 2).astype(np.float32) / np.float32(D)
    th = (np.float32(pos) / np.power(np.float32(theta), freq, dtype=np.float32)).astype(np.float32)
    c, s = np.cos(th, dtype=np.float32), np.sin(th, dtype=np.float32)
    x0, x1 = x[..., :half], x[..., half:]
    return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1)


def test_rope_split_halves_parity(oracle):
    """rope_parity.rs:54-166: identity at position 0, the worked position-1 values, batch x heads, distinct positions."""
    q = np.arange(8, dtype=np.float32)
    assert np.allclose(oracle.rope_apply(q, 0), q, atol=1e-6)
    q = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.float32)
    got = oracle.rope_apply(q, 1)
    c0, s0 = np.cos(np.float32(1.0)), np.sin(np.float32(1.0))
    assert abs(got[0] - (1.0 * c0 - 5.0 * s0)) < 1e-5 and abs(got[4] - (1.0 * s0 + 5.0 * c0)) < 1e-5
    qb = np.arange(2 * 2 * 1 * 8, dtype=np.float32).reshape(2, 2, 1, 8)
    rb = oracle.rope_apply(qb, 1)
    assert rb.shape == qb.shape and np.isfinite(rb).all()
    assert np.allclose(rb, _rope_closed_form(qb, 1), atol=1e-4)
    qs = np.arange(4 * 8, dtype=np.float32).reshape(4, 8)
    rows = [oracle.rope_apply(qs[p], p) for p in range(4)]
    for p in range(1, 4):
        assert np.abs(rows[p] - rows[p - 1]).max() > 1e-6
    # split halves (i, i + D/2), not interleaved pairs (i, i + 1): rope_parity.rs:168-
    q8 = np.arange(8, dtype=np.float32)
    inter = q8.copy()
    th = np.float32(1.0) / np.power(np.float32(10000.0), (np.arange(4) * 2).astype(np.float32) / np.float32(8))
    inter[0::2] = q8[0::2] * np.cos(th) - q8[1::2] * np.sin(th)
    inter[1::2] = q8[0::2] * np.sin(th) + q8[1::2] * np.cos(th)
    assert np.abs(oracle.rope_apply(q8, 1) - inter).max() > 1e-3
    # general positions / thetas against the closed form (theta 500000: rope_tests.rs:95-98, LLaMA-3's base)
    rng = np.random.default_rng(0)
    for D, pos, theta in ((8, 3, 10000.0), (64, 17, 10000.0), (128, 255, 500000.0), (32, 5, 10000.0)):
        x = rng.normal(0, 1, (3, D)).astype(np.float32)
        assert np.allclose(oracle.rope_apply(x, pos, theta), _rope_closed_form(x, pos, theta), atol=2e-4), (D, pos)


def test_rope_tables_unit_tests_and_snapshots(oracle):
    """crates/bitnet-rope/src/lib.rs:108-147 (shape, identity row, known values) and tests/snapshot_tests.rs
    (DEFAULT_ROPE_BASE = 10000; 4-dim x 8-seq table: half_dim=2 sin_len=16 cos_len=16)."""
    sin, cos = oracle.rope_tables(8, 3, 10000.0)
    assert sin.shape == (3, 4) and cos.shape == (3, 4)
    sin, cos = oracle.rope_tables(8, 2, 10000.0)
    assert np.abs(sin[0]).max() <= 1e-7 and np.abs(cos[0] - 1.0).max() <= 1e-7
    sin, cos = oracle.rope_tables(4, 2, 10000.0)
    assert abs(sin[1, 0] - np.sin(np.float32(1.0))) <= 1e-6 and abs(cos[1, 0] - np.cos(np.float32(1.0))) <= 1e-6
    assert abs(sin[1, 1] - np.sin(np.float32(0.01))) <= 1e-6 and abs(cos[1, 1] - np.cos(np.float32(0.01))) <= 1e-6
    sin, cos = oracle.rope_tables(4, 8, 10000.0)
    assert f"half_dim={sin.shape[1]} sin_len={sin.size} cos_len={cos.size}" == "half_dim=2 sin_len=16 cos_len=16"


def test_rope_tables_properties(oracle):
    """crates/bitnet-rope/tests/property_tests.rs:30-62: dimensions and sin^2 + cos^2 = 1 over (dim, seq_len, base)."""
    rng = np.random.default_rng(1)
    for _ in range(40):
        dim, seq, base = int(rng.integers(1, 65)) * 2, int(rng.integers(1, 65)), float(rng.uniform(1.0, 1e6))
        sin, cos = oracle.rope_tables(dim, seq, base)
        assert sin.size == seq * (dim // 2) == cos.size
        assert np.abs(sin * sin + cos * cos - 1.0).max() < 1e-5


def test_rotary_embedding_behaviour(oracle):
    """crates/bitnet-transformer/tests/rope_tests.rs:28-78: shape, finiteness, positions differ, determinism."""
    x = np.ones((1, 4, 1, 64), np.float32)
    assert oracle.rope_apply(x, 0).shape == x.shape
    x = np.ones((2, 8, 4, 32), np.float32)
    assert oracle.rope_apply(x, 0).shape == x.shape and np.isfinite(oracle.rope_apply(x, 0)).all()
    x = np.ones((1, 2, 1, 32), np.float32)
    assert np.abs(oracle.rope_apply(x, 0) - oracle.rope_apply(x, 5)).max() > 1e-7
    assert np.array_equal(oracle.rope_apply(x, 3), oracle.rope_apply(x, 3))


def test_quantized_matmul_i2s_composite_worked_example(oracle):
    """QuantizedLinear::quantized_matmul_i2s (quantized_linear.rs:704-802) by hand: m=1, k=4, n=2.
    input [0.4, 1.7, -3.0, -0.5] -> clamp(-2,1).round() = [0, 1, -2, -1] (-0.5 rounds away from zero);
    packed 0b11100100, 0b00011011 -> raw codes [0,1,2,3, 3,2,1,0] = B[4,2] rows (0,1),(2,3),(3,2),(1,0);
    C = [0*0 + 1*2 - 2*3 - 1*1, 0*1 + 1*3 - 2*2 - 1*0] = [-5, -1]; one scale per output feature [0.5, 2] -> [-2.5, -2]."""
    x = np.array([0.4, 1.7, -3.0, -0.5], np.float32)
    packed = np.array([0b11100100, 0b00011011], np.uint8)
    assert oracle.quantized_matmul_i2s(x, packed, np.array([0.5, 2.0], np.float32), 32, 1, 2, 4).tolist() == [-2.5, -2.0]
    # block-indexed scales (scales.len() != out_features): idx = min(col * k / block_size, len - 1) -> col 0 -> 0, col 1 -> min(4 / 2, 2) = 2
    got = oracle.quantized_matmul_i2s(x, packed, np.array([10.0, 100.0, 1000.0], np.float32), 2, 1, 2, 4)
    assert got.tolist() == [-50.0, -1000.0]
    # NaN input quantises to 0; a weight buffer that is too short fails matmul_i2s's B check
    assert oracle.quantized_matmul_i2s(np.array([np.nan, 1, 1, 1], np.float32), packed, np.array([1.0, 1.0], np.float32), 32, 1, 2, 4).tolist() == [2 + 3 + 1, 3 + 2 + 0]
    with pytest.raises(oracle.OracleError, match="Matrix B dimension mismatch"):
        oracle.quantized_matmul_i2s(x, packed[:1], np.array([1.0, 1.0], np.float32), 32, 1, 2, 4)
