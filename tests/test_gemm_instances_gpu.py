"""GPU: every kernel instance the tiled matmul's launch layer can reach (kernels_gemm.hip), its VALUES against tests/gemm_ref.py -- the exact
float64 / int64 model of what each form carries into its product -- on every output element.  tests/test_gemm_dispatch_gpu.py pins which tile a
launch takes; this file takes its CASES (and adds the instances it lacks), asserts the same report first and then the numbers.

Instance -> case (the reported tile {digits, wave_tokens, waves, scale_mode} / wave rows / resident image is the last field of the case's row):

  k_gemm_mfma<2, {1, 2, 4}, 0, 2, 1>     i8_m2048 / i8_m6400, i8_m16640 (the tail rule) / i8_m12288, i8_flag_m12288, walk_i8
  k_gemm_mfma<3, 2, 0, 2, 1>             i8_3dig                         k_gemm_mfma<4, 2, 0, 2, 1>   i8_4dig
  k_gemm_mfma<{2, 3, 4}, 2, 1>           i8_block256 / i8_block256_3dig / i8_block256_4dig                                (8 waves, mode 1)
  k_gemm_mfma<{2, 3}, 2, 2>, <4, 1, 2>   i8_block32_f32 / i8_block32_f32_3dig / i8_block32_f32_4dig                      (8 waves, mode 2)
  k_gemm_mfma<{2, 3}, 2, 3, 2, 1>,       i8_block32_f16_int8_flag, i8_block32_f16_3dig_silu / i8_block32_f16_3dig /
             <4, 1, 3, 2, 1>             i8_block32_f16_4dig                                                              (mode 3)
  k_gemm_f16a<1, {1, 2, 4}, 0, 4>        f16q_m2048, f16q_silu / f16q_m4096 / f16q_m8192                                   (mode 4)
  k_gemm_f16a<0, {1, 2, 4}, 0, 4>        f16a_m2048 / f16a_m4096 / f16a_m8192        (BITNET_HIP_GEMM_F16A=1: a child process; mode 5)
  k_gemm_fp6<{1, 2, 4}, 4, 1, 0>         fp6_m2048, fp6_m1000, fp6_silu / fp6_m8192 / fp6_resident_m16384 at 500 and 499 rows (k_gemm_fp6w takes
                                         rows % 256 == 0 only), and whole under BITNET_HIP_GEMM_FP6W=0 (a child process)
  k_gemm_fp6<{1, 2, 4}, 4, 0, 0>         fp6_m2048_expand / fp6_m8192_expand / fp6_expand_m16384, walk_fp6_expand
  k_gemm_fp6<4, 5, {1, 0}, 0>            fp6_rows1280_m8192 / fp6_rows1280_m8192_expand                                   (wave rows 80)
  k_gemm_fp6w                            fp6_resident_m16384, walk_fp6                                                    (wave rows 128)
  k_gemm_f16a<0, {1, 2, 4}, 1, 4>        chain_m1024 / chain_m2048 / chain_m4096, chain_m8192_silu, walk_chain, the rest of f16h_split (bx_off 16)
  k_gemm_f16a<1, {1, 2, 4}, 1, 4>        chain_scaled_m1024 / chain_scaled_m2048 / chain_scaled_m4096, the rest of f16h_split_scaled
  k_gemm_f16a<{0, 1}, 4, 1, 5>           chain_m8192 / chain_scaled_m8192                                                 (wave rows 80)
  k_gemm_f16a<{0, 1}, 4, 2, {4, 5}>      chain_qb32_m4096, chain_qb32_m8192 / chain_scaled_qb32_m4096, chain_scaled_qb32_m8192   (their f32 rows)
  k_gemm_f16h<0>, <1>                    f16h_whole, f16h_split (row blocks 0 .. 15) / f16h_whole_scaled, f16h_split_scaled
  k_gemm_fp6<{1, 2, 4}, 4, 1, 1>         qb32_m2048, qb32_m2048_silu / qb32_m8192, qb32_m8192_silu / qb32_m16384, walk_qb32   (mode 8)
  k_gemm_fp6<{1, 2, 4}, 4, 0, 1>         the same cases under BITNET_HIP_FP4_RESIDENT=0 (a child process)
  k_quant_rows<{2, 3, 4}, {3, 8}, 0>,    test_quantiser_edges (K up to 3072: NV 3, from 3076: NV 8), test_layernorm_prologue_carries_the_model_integer;
  k_quant_rows<2, {3, 8}, 1>             every fused case of under 2048 padded rows; at 2048 rows and more under BITNET_HIP_QUANT_W=0 (a child process)
  k_quant_rows_w<0>, <1>                 every 2-digit / fp6 fused case of 2048 padded rows and more; test_wave_per_row_quantiser_by_value (ragged m)
  k_quant_rows_f16<3>, <8>               the f16q cases; test_quantiser_edges at K = 256, 3072 / 6912, 8192
  k_rows_to_f16, k_rows_to_qb32          the chain and QB32 cases' inputs, compared by value before the product is
 No input reaches through the ABI:
  store_wave_tiles' scalar silu path     (:494-499) half rows that are no multiple of 4: weights_concat(.., interleave16) takes parts of rows % 16 == 0 only
  k_gemm_f16a<.., 2, ..> below 64 tokens, k_gemm_fp6<.., 5, .., 1>: not built (pick_f16a / pick_fp6 hold no such row; the first is the refusal
                                         test_gemm_dispatch_gpu's chain_qb32_m1024 pins)
  k_gemm_mfma<NDIG, TTW, 0>, <NDIG, TT32, 3> with 8 waves: launch_gemm_t names them first (:2124) and replaces them in every launch that could
                                         take them (:2132-2134: unscaled and f16-scale-tile launches run the 4-wave form)
 The weight-group walk (gemm_weight_group): the walk_* cases have 24 row blocks and take it by default -- as ONE group of 24 at K = 256; under
 BITNET_HIP_GEMM_WGROUP=8 (a child process) the same cases walk three groups of 8.

a. exact inputs (gemm_ref.int_rows: integers times one power of two per row, a peak that fixes the exponent the quantiser takes; power-of-two block
   scales within a factor of 8): every product and every partial sum of any order is below 2^24 units, so the f32 result is the exact one and is
   compared BY VALUE.  tests/test_gemm_ref.py proves that condition for the inputs of every case here.  2 digits on the int8 planes round the exact
   integer once (combine_digits<2>): by value for ARBITRARY rows.  3 and 4 digits: rows on the top digit plane.
b. float inputs (gemm_ref.float_rows: a magnitude per row from exp(uniform(-3, 3)), one zero row; arbitrary block scales) against float64 within the
   bound gemm_ref derives per form -- a count of f32 roundings x 2^-24 x the magnitudes that enter them, stated at gemm_ref.product_*: NDIG - 1
   (combine_digits), NDIG + folds (scale modes 1 - 3), K (f16 accumulator), 3 K (fp6 accumulator; at K = 256 its sums stay below 2^24 and the form
   is exact).  Every case asserts that its bound IS that count on its own inputs, and prints max |got - want| / bound.
   Elements whose partial sums stay below 2^24 units are exact in float inputs too, and are asserted by value (bound 0).
c. edges on every case: a ragged token count (m - 37: the same padded count, the same tile), 64 NaN guard rows behind row m that must stay NaN, y
   starts as NaN (every live element must be written); on the fused entry rows = 512, 500 (paired store, short last tile) and 499 (scalar store).
d. epilogues: residual, in-place residual, silu(gate) * up on interleave16 handles (half rows 256 and 240), the f16 hand-over.
e. quantiser edges through a 48-row matmul, the planes read back from the workspace (GemmArgs::planes / inv_scale, launch_gemm_mfma :2387-2390).
f. the LayerNorm prologue on integer-valued rows: the f64 sums are exact in any order, f32 subtraction, IEEE division and multiplication are
   reproducible operation for operation (numpy rounds as the device does), so the planes hold the model's q in every column -- by value.
g. environment switches, one child process each (the switches are read once per process)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402
import test_gemm_dispatch_gpu as D  # noqa: E402

pytestmark = pytest.mark.gpu

SILU, X_F16, Y_F16, INT8, FP6, FP6_EXPAND, YH_QB32 = 1, 2, 4, 8, 16, 32, 64
K = 256
GUARD = 64
T = D.T

# id -> (entry, matrix, rows, m, digits, flags, expected): test_gemm_dispatch_gpu.CASES' rows, for the instances it does not launch
NEW_CASES = {
    "i8_block256_3dig": ("fused", "i2s256", 512, 2048, 3, 0, T(3, 32, 8, 1)),
    "i8_block256_4dig": ("fused", "i2s256", 512, 2048, 4, 0, T(4, 32, 8, 1)),
    "i8_block32_f32_3dig": ("fused", "i2s32", 512, 2048, 3, 0, T(3, 32, 8, 2)),
    "i8_block32_f32_4dig": ("fused", "i2s32", 512, 2048, 4, 0, T(4, 16, 8, 2)),
    "f16q_m4096": ("fused", "i2s32h", 512, 4096, 2, 0, T(2, 32, 4, 4)),
    "fp6_m8192_expand": ("fused", "qk256", 512, 8192, 2, FP6 | FP6_EXPAND, T(2, 32, 4, 6, 64, False)),
    "chain_scaled_m1024": ("f16", "i2s32h", 1280, 1024, 2, 0, T(2, 16, 4, 4)),
    "chain_scaled_m2048": ("f16", "i2s32h", 1280, 2048, 2, 0, T(2, 32, 4, 4)),
    "chain_scaled_qb32_m4096": ("f16", "i2s32h", 1280, 4096, 2, YH_QB32, T(2, 64, 4, 4)),
    "chain_scaled_qb32_m8192": ("f16", "i2s32h", 1280, 8192, 2, YH_QB32, T(2, 64, 4, 4, 80)),
    "f16h_split_scaled": ("f16", "i2s32h", 6144, 4096, 2, 0, T(2, 128, 4, 4)),
    "qb32_m2048": ("qb32", "qk256", 512, 2048, 2, 0, T(2, 16, 4, 8, 64, True)),
    "qb32_m2048_silu": ("qb32", "qk256+pair", 512, 2048, 2, SILU, T(2, 16, 4, 8, 64, True)),
    # silu(gate) * up on the fused entry: half rows 256, and 240 (a multiple of 4, no multiple of 16: the pair's last tile is short)
    "i8_silu": ("fused", "qk256+pair", 512, 2048, 2, SILU, T(2, 16, 4, 0)),
    "i8_silu_480": ("fused", "qk256+pair", 480, 2048, 2, SILU, T(2, 16, 4, 0)),
    "i8_block32_f16_3dig_silu": ("fused", "i2s32h+pair", 512, 2048, 3, SILU, T(3, 32, 4, 3)),
    "f16q_silu": ("fused", "i2s32h+pair", 480, 2048, 2, SILU, T(2, 16, 4, 4)),
    "fp6_silu": ("fused", "qk256+pair", 480, 2048, 2, SILU | FP6, T(2, 16, 4, 6, 64, True)),
    # 6144 rows = 24 row blocks: the weight-group walk; m = the fewest tokens at which the form keeps its 64-token tile
    "walk_i8": ("fused", "qk256", 6144, 1024, 2, 0, T(2, 64, 4, 0)),
    "walk_fp6": ("fused", "qk256", 6144, 2048, 2, FP6, T(2, 64, 4, 6, 128, True)),
    "walk_fp6_expand": ("fused", "qk256", 6144, 2048, 2, FP6 | FP6_EXPAND, T(2, 64, 4, 6, 64, False)),
    "walk_chain": ("f16", "qk256", 6144, 1024, 2, 0, T(2, 64, 4, 5)),
    "walk_qb32": ("qb32", "qk256", 6144, 2048, 2, 0, T(2, 64, 4, 8, 64, True)),
}
CASES = {**{k: v for k, v in D.CASES.items() if "error" not in v[-1]}, **NEW_CASES}


def _with(name, expected=None, **kw):
    entry, kind, rows, m, digits, flags, exp = CASES[name]
    return (entry, kind, rows, m, digits, flags, expected or exp)


# switch -> (environment, {id: case}): what each child process runs; `form` overrides the model's form where only the switch selects it
ENV_CASES = {
    "f16a": ({"BITNET_HIP_GEMM_F16A": "1"}, {"f16a_m2048": ("fused", "qk256", 512, 2048, 2, 0, T(2, 16, 4, 5)),
                                             "f16a_m4096": ("fused", "qk256", 512, 4096, 2, 0, T(2, 32, 4, 5)),
                                             "f16a_m8192": ("fused", "qk256", 512, 8192, 2, 0, T(2, 64, 4, 5))}),
    "f16h_off": ({"BITNET_HIP_GEMM_F16H": "0"}, {"f16h_split": _with("f16h_split", T(2, 64, 4, 5))}),
    "fp6w_off": ({"BITNET_HIP_GEMM_FP6W": "0"}, {"fp6_resident_m16384": _with("fp6_resident_m16384", T(2, 64, 4, 6, 64, True))}),
    "fp4_resident_off": ({"BITNET_HIP_FP4_RESIDENT": "0"}, {"qb32_m2048": _with("qb32_m2048", T(2, 16, 4, 8, 64, False)),
                                                            "qb32_m8192": _with("qb32_m8192", T(2, 32, 4, 8, 64, False)),
                                                            "qb32_m8192_silu": _with("qb32_m8192_silu", T(2, 32, 4, 8, 64, False)),
                                                            "qb32_m16384": _with("qb32_m16384", T(2, 64, 4, 8, 64, False))}),
    "quant_w_off": ({"BITNET_HIP_QUANT_W": "0"}, {"i8_m2048": _with("i8_m2048"), "fp6_m2048": _with("fp6_m2048"), "fp6_m2048_expand": _with("fp6_m2048_expand")}),
    "wgroup_8": ({"BITNET_HIP_GEMM_WGROUP": "8"}, {n: _with(n) for n in ("walk_i8", "walk_fp6", "walk_fp6_expand", "walk_chain", "walk_qb32")}),
}
F16A_FORM = {"f16a_m2048", "f16a_m4096", "f16a_m8192"}


# ---------------------------------------------------------------- inputs and the model, shared with tests/test_gemm_ref.py
def form_of(name, case):
    entry, kind, rows, m, digits, flags, _ = case
    if entry == "f16":
        return "chain"
    if entry == "qb32":
        return "qb32"
    if flags & FP6:
        return "fp6"
    if name in F16A_FORM or (kind.startswith("i2s32h") and digits == 2 and not flags & INT8):
        return "f16q"
    return "int8"


def seed_of(*parts):
    return sum(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def matrix_of(kind, rows, scales):
    """the case's matrix: a pair = two matrices of rows / 2 interleaved in 16-row tiles; unscaled matrices are the same for both scale kinds"""
    if kind.endswith("+pair"):
        base = kind[:-5]
        return R.pair(matrix_of(base + "#a", rows // 2, scales), matrix_of(base + "#b", rows // 2, scales))
    base = kind.split("#")[0]
    return R.make_matrix(base, rows, K, seed_of(kind, rows, K), "float" if base == "qk256" else scales)


@functools.lru_cache(maxsize=None)
def matrix_for(kind, rows, full_rows, scales):
    """rows < full_rows: the first rows of the full matrix (the row-tail launches)"""
    mat = matrix_of(kind, full_rows, "float" if kind.startswith("qk256") else scales)
    return mat if rows == full_rows else mat.head(rows)


@functools.lru_cache(maxsize=4)
def rows_of(form, digits, m, inputs):
    if inputs == "float":
        return R.float_rows(m, K, seed_of("float", form, m))
    s = seed_of("exact", form, digits, m)
    if form == "int8" and digits > 2:
        return R.int_rows(m, K, s, top=15, peak=16)          # q = 2 n 256^(NDIG - 1): the top digit plane alone
    if form in ("int8", "fp6"):
        return R.int_rows(m, K, s, top=1000, peak=8192)      # q = n
    if form == "qb32":
        return R.int_rows(m, K, s, top=1000, peak=1023, every=32)  # every unit's exponent is the same: q = 16 n
    return R.int_rows(m, K, s, top=1000, peak=1023)          # f16 rows: n 2^-9 behind the row quantiser, n 2^e on the chain


def model(form, x, mat, digits, flags=0, ln=None):
    """-> gemm_ref.Product of the launch's f32 output (before a residual)"""
    if form == "int8":
        p = R.product_int8(*R.quant_rows(x, digits, ln), mat, digits)
    elif form == "fp6":
        p = R.product_fp6(*R.quant_rows(x, 2, ln), mat)
    elif form == "f16q":
        p = R.product_f16(*R.quant_rows_f16(x, ln), mat)
    elif form == "chain":
        p = R.product_f16(R.rows_to_f16(x), np.ones(x.shape[0]), mat)
    else:
        p = R.product_qb32(*R.quant_qb32(x), mat)
    return R.silu_mul(p) if flags & SILU else p


def derived_roundings(form, digits, mat):
    """the count gemm_ref's bound must carry (restated here from the table in the header, b.)"""
    if form == "int8":
        return digits - 1 if mat.scale is None else digits + (8 if mat.block == 32 else 1) * (-(-K // 256))
    return K if form in ("f16q", "chain") else 3 * K


def variants(case):
    """(m, rows, inputs) of the launches of one case: aligned on exact and on float inputs, the ragged token tail (the same padded count: every
    form pads to 32, 64 or 128 tokens), and on the fused entry's 512-row matrices the two row tails.  Launches of more than 2^23 outputs share
    the two input kinds between the aligned and the ragged launch."""
    entry, kind, rows, m, digits, flags, _ = case
    assert -(-(m - 37) // 128) == -(-m // 128)
    v = [(m, rows, "exact"), (m - 37, rows, "float")] if m * rows > 1 << 23 else [(m, rows, "exact"), (m, rows, "float"), (m - 37, rows, "exact")]
    if entry == "fused" and rows == 512 and not kind.endswith("+pair"):
        v += [(m - 37, 500, "float"), (m - 37, 499, "float")]
    return v


def report_for(want_report, vrows):
    """the report of a row-tail launch: the case's own, except that k_gemm_fp6w takes rows % 256 == 0 only (launch_gemm_fp6 :2262) -- the tails of
    its cases run k_gemm_fp6<4, 4, 1, 0>, wave rows 64"""
    if vrows % 256 != 0 and want_report["wave_rows"] == 128:
        return dict(want_report, wave_rows=64)
    return want_report


def exact_units(name, case):
    """the exactness condition of a case's exact inputs, from the model alone: the largest number of units any partial sum of any order can reach
    (gemm_ref.max_units) -- tests/test_gemm_ref.py asserts it stays below 2^24 for every case.  None: 2 digits on unscaled int8 planes, whose
    int32 digit sums and single rounding need no condition."""
    entry, kind, rows, m, digits, flags, _ = case
    form, mat, x = form_of(name, case), matrix_for(kind, rows, rows, "pow2"), rows_of(form_of(name, case), digits, m, "exact")
    if form == "int8":
        return None if digits == 2 and mat.scale is None else R.max_units(np.abs(R.quant_rows(x, digits)[0]).astype(np.float64), mat.dense)
    if form in ("fp6", "qb32"):
        q, s = R.quant_qb32(x) if form == "qb32" else (R.quant_rows(x, 2)[0], None)
        d = np.abs(R.digits32(q)).astype(np.float64)
        lsb = 1.0 if s is None else np.repeat(np.exp2(s.astype(np.float64) - 130.0), 32, axis=1)
        return R.max_units((d[0] + 32.0 * d[1] + 1024.0 * d[2]) * lsb, mat.dense)
    xh = R.rows_to_f16(x) if form == "chain" else R.quant_rows_f16(x)[0]
    return R.max_units(np.abs(xh), mat.dense)


# ---------------------------------------------------------------- launches
_handles = {}


def handle_of(hip, mat):
    key = id(mat)
    if key not in _handles:
        up = mat.upload
        if "parts" in up:
            h = hip.weights_concat([handle_of(hip, p) for p in up["parts"]], interleave16=True)
        elif mat.kind == "qk256":
            h = hip.weights_upload_qk256(up["qs"].reshape(-1), mat.rows, mat.cols, up["stride"])
        else:
            h = hip.weights_upload_i2s(up["packed"].reshape(-1), up["scales"].reshape(-1), mat.rows, mat.cols, up["block"])
        _handles[key] = (h, mat)  # (the matrix is kept: its id stays its own)
    return _handles[key][0]


@pytest.fixture(scope="module", autouse=True)
def _free_handles(hip):
    yield
    for h, _ in reversed(list(_handles.values())):
        hip.weights_free(h)
    _handles.clear()


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(torch_, m, cols, dtype=None):
    """[m + GUARD, cols] of NaN: rows m .. are the guard rows"""
    return torch_.full((m + GUARD, cols), float("nan"), device="cuda", dtype=dtype or torch_.float32)


def launch(hip, torch_, entry, h, mat, x, digits, flags, residual=None, inplace=False, ln=None, want_yh=False, gout=None, cols=K):
    """one launch on fresh buffers -> dict(y [m, out], tail [GUARD, out], report, and what the entry's input conversion left: xh / qb, ws)"""
    m, out_cols = x.shape[0], mat.rows // 2 if flags & SILU else mat.rows
    mp = -(-m // 64) * 64
    xd = dev(torch_, x)
    y = guarded(torch_, m, out_cols)
    res = None
    if residual is not None:
        if inplace:
            y[:m] = dev(torch_, residual)
            res = y
        else:
            res = dev(torch_, residual)
    out = {}
    if entry == "fused":
        wsb = hip.matmul_workspace_bytes(m, cols, digits)
        ws = torch_.zeros(wsb, dtype=torch_.uint8, device="cuda")
        assert ws.data_ptr() % 256 == 0
        if flags & Y_F16:
            y = guarded(torch_, m, out_cols, torch_.float16)
        kw = {} if ln is None else dict(ln_gamma=dev(torch_, ln[0]), ln_eps=float(ln[1]))
        hip.matmul_fused_dev(h, xd, y, m, ws, wsb, residual=res, flags=flags, digits=digits, **kw)
        out["ws"] = ws
    elif entry == "f16":
        xh = torch_.zeros(mp, cols, dtype=torch_.float16, device="cuda")
        hip.rows_to_f16_dev(xd, None, m, cols, xh, None)
        yh = None
        if flags & YH_QB32:
            yh = torch_.zeros(hip.qb32_bytes(m, mat.rows), dtype=torch_.uint8, device="cuda")
        elif want_yh:
            yh = torch_.full((mp + GUARD, out_cols), float("nan"), dtype=torch_.float16, device="cuda")
        hip.matmul_f16_dev(h, xh, m, y=y, residual=res, flags=flags, yh=yh, gamma_out=None if gout is None else dev(torch_, gout))
        out["xh"], out["yh"] = xh, yh
    else:
        qb = torch_.zeros(hip.qb32_bytes(m, cols), dtype=torch_.uint8, device="cuda")
        hip.rows_to_qb32_dev(xd, None, m, cols, qb, None)
        yh = torch_.full((mp + GUARD, out_cols), float("nan"), dtype=torch_.float16, device="cuda") if want_yh else None
        hip.matmul_qb32_dev(h, qb, m, y=y, residual=res, flags=flags, yh=yh, gamma_out=None if gout is None else dev(torch_, gout))
        out["qb"], out["yh"] = qb, yh
    torch_.cuda.synchronize()
    out["report"] = {"tile": dict(hip.matmul_last_tile()), "wave_rows": hip.matmul_last_wave_rows(), "resident": hip.matmul_last_resident_fp4()}
    got = y.float().cpu().numpy() if flags & Y_F16 else y.cpu().numpy()
    out["y"], out["tail"] = got[:m], got[m:]
    return out


def check_inputs(entry, out, x):
    """the chain's and the QB32 consumer's inputs are what the model says they are -- by value, every element"""
    m = x.shape[0]
    if entry == "f16":
        assert np.array_equal(out["xh"][:m].cpu().numpy().astype(np.float64), R.rows_to_f16(x))
        assert not out["xh"][m:].cpu().numpy().any()
    elif entry == "qb32":
        q, s = R.decode_fp6_records(out["qb"].cpu().numpy(), m, K, 592)
        mq, ms = R.quant_qb32(x)
        assert np.array_equal(q, mq) and np.array_equal(s, ms)


RATIOS = {}


def check_values(tag, form, out, p, exact_inputs=False):
    """every live element within the model's bound (by value where the bound is 0), the guard rows untouched -> max error / bound"""
    got = out["y"]
    assert np.isnan(out["tail"]).all(), (tag, "guard rows written")
    exact = (p.bound == 0) if p.exact32 is not None else np.zeros(p.bound.shape, bool)
    target = np.where(exact, p.exact32.astype(np.float64), p.want) if p.exact32 is not None else p.want
    err = np.abs(got.astype(np.float64) - target)
    ratio = float(np.max(np.where(p.bound > 0, err / np.where(p.bound > 0, p.bound, 1.0), 0.0), initial=0.0))
    RATIOS[form] = max(RATIOS.get(form, 0.0), ratio)
    print(f"GEMMRATIO {tag} form={form} exact_elements={float(np.mean(exact)):.3f} max_err={np.nanmax(err):.3e} max_err/bound={ratio:.4f}")
    bad = ~(err <= p.bound)  # (a NaN -- an element nobody wrote -- is bad)
    assert not bad.any(), (tag, int(bad.sum()), [(int(i), int(j), float(got[i, j]), float(target[i, j]), float(p.bound[i, j])) for i, j in np.argwhere(bad)[:6]])
    if exact_inputs and p.exact32 is not None:
        assert exact.all(), (tag, "the exact inputs left the exact range")
        assert np.array_equal(got, p.exact32), tag
    return ratio


def check_bound_is_derived(tag, form, digits, mat, p):
    n = derived_roundings(form, digits, mat)
    assert p.roundings == n, (tag, p.roundings, n)
    exact = p.units < R.EXACT_UNITS if p.units is not None else np.zeros(p.bound.shape, bool)
    if form == "int8" and digits == 2 and mat.scale is None:
        exact = np.ones(p.bound.shape, bool)
    assert np.array_equal(p.bound, np.where(exact, 0.0, R.gamma(n) * p.mag)), tag


def check_instance(hip, torch_, name, case):
    """every variant of one case; -> its largest error / bound"""
    entry, kind, rows, m, digits, flags, want_report = case
    form = form_of(name, case)
    worst = 0.0
    for vm, vrows, inputs in variants(case):
        mat = matrix_for(kind, vrows, rows, "pow2" if inputs == "exact" else "float")
        x = rows_of(form, digits, m, inputs)[:vm]
        tag = f"{name} m={vm} rows={vrows} {inputs}"
        out = launch(hip, torch_, entry, handle_of(hip, mat), mat, x, digits, flags)
        assert out["report"] == report_for(want_report, vrows), (tag, out["report"], want_report)
        check_inputs(entry, out, x)
        p = model(form, x, mat, digits, flags)
        check_bound_is_derived(tag, form, digits, mat, getattr(p, "source", p))  # (silu * up: the bound of the product it is built from)
        worst = max(worst, check_values(tag, form + ("+silu" if flags & SILU else ""), out, p, exact_inputs=inputs == "exact"))
    return worst


# ---------------------------------------------------------------- a. - c. one case per instance
@pytest.mark.parametrize("name", list(CASES))
def test_instance_values(hip, torch_, name):
    t0 = time.time()
    check_instance(hip, torch_, name, CASES[name])
    print(f"GEMMTIME {name} {time.time() - t0:.2f} s")


# ---------------------------------------------------------------- d. epilogues
# one token-tile width per form at least; the fused entry's residual also on the scalar store path (499 rows) and the fifth tile of the 320-row form
EPILOGUE_CASES = ["i8_m2048", "i8_3dig", "i8_block256", "i8_block32_f32", "i8_block32_f16_4dig", "f16q_m2048", "fp6_m2048", "fp6_m2048_expand",
                  "fp6_rows1280_m8192", "fp6_resident_m16384", "chain_m1024", "chain_m8192", "chain_scaled_m4096", "f16h_whole", "qb32_m2048"]


@pytest.mark.parametrize("name", EPILOGUE_CASES)
def test_residual_and_in_place_residual(hip, torch_, name):
    entry, kind, rows, m, digits, flags, want_report = case = CASES[name]
    form = form_of(name, case)
    vm = m - 37
    for vrows in ((rows, 499) if entry == "fused" and rows == 512 else (rows,)):
        for inputs in ("exact", "float"):
            mat = matrix_for(kind, vrows, rows, "pow2" if inputs == "exact" else "float")
            x = rows_of(form, digits, m, inputs)[:vm]
            rng = np.random.default_rng(seed_of("res", name, vrows, inputs))
            res = (rng.integers(-512, 513, (vm, vrows)) / 8.0 if inputs == "exact" else rng.normal(0, 1, (vm, vrows))).astype(np.float32)
            p = R.add_residual(model(form, x, mat, digits), res)
            for inplace in (False, True):
                tag = f"{name} m={vm} rows={vrows} {inputs} residual{' in place' if inplace else ''}"
                out = launch(hip, torch_, entry, handle_of(hip, mat), mat, x, digits, flags, residual=res, inplace=inplace)
                assert out["report"] == report_for(want_report, vrows), (tag, out["report"])
                check_values(tag, form + "+residual", out, p)


F16_HANDOVER_FUSED = ["i8_silu", "i8_silu_480", "fp6_silu"]  # FUSE_Y_F16: the digit forms' silu * up as f16 rows


@pytest.mark.parametrize("name", F16_HANDOVER_FUSED)
def test_f16_handover_of_the_fused_entry(hip, torch_, name):
    entry, kind, rows, m, digits, flags, want_report = case = CASES[name]
    form, vm = form_of(name, case), m - 37
    mat = matrix_for(kind, rows, rows, "float")
    x = rows_of(form, digits, m, "float")[:vm]
    h = handle_of(hip, mat)
    f32 = launch(hip, torch_, entry, h, mat, x, digits, flags)
    f16 = launch(hip, torch_, entry, h, mat, x, digits, flags | Y_F16)
    assert f32["report"] == f16["report"] == want_report
    assert np.isnan(f16["tail"]).all()
    assert np.array_equal(f16["y"].astype(np.float16), np.clip(f32["y"], -65504.0, 65504.0).astype(np.float16))  # the f32 value, clamped, rounded once
    check_values(f"{name} m={vm} y_f16", form + "+f16", f16, R.to_f16(model(form, x, mat, digits, flags)))


F16_HANDOVER_CHAIN = ["chain_m1024", "chain_m8192", "chain_m8192_silu", "chain_scaled_m2048", "f16h_whole", "qb32_m2048", "qb32_m2048_silu"]


@pytest.mark.parametrize("name", F16_HANDOVER_CHAIN)
def test_f16_handover_of_the_chain_entries(hip, torch_, name):
    """yh = f16(clamp(gamma_out * y)) beside y (silu * up: no gamma_out in the kernel's paired branch): the f32 rows by the model, the f16 rows by value
    from the f32 rows the same launch wrote, and by the model's bound"""
    entry, kind, rows, m, digits, flags, want_report = case = CASES[name]
    form, vm = form_of(name, case), m - 37
    mat = matrix_for(kind, rows, rows, "float")
    x = rows_of(form, digits, m, "float")[:vm]
    out_cols = rows // 2 if flags & SILU else rows
    gout = None if flags & SILU else np.random.default_rng(seed_of("gout", name)).uniform(0.5, 1.5, out_cols).astype(np.float32)
    out = launch(hip, torch_, entry, handle_of(hip, mat), mat, x, digits, flags, want_yh=True, gout=gout)
    assert out["report"] == want_report
    p = model(form, x, mat, digits, flags)
    check_values(f"{name} m={vm} y beside yh", form, out, p)
    yh = out["yh"].cpu().numpy()
    mp = -(-vm // 64) * 64
    assert np.isnan(yh[mp:]).all()  # rows up to m_pad belong to the buffer (include/bitnet_hip.h); the guard rows behind them do not
    scaled = out["y"] if gout is None else out["y"] * gout[None, :]
    assert scaled.dtype == np.float32
    assert np.array_equal(yh[:vm], np.clip(scaled, -65504.0, 65504.0).astype(np.float16)), name
    check_values(f"{name} m={vm} yh", form + "+f16", dict(y=yh[:vm].astype(np.float32), tail=yh[mp:].astype(np.float32)), R.to_f16(p, gout))


# ---------------------------------------------------------------- e. quantiser edges
def workspace_views(ws, m, m_pad, kp):
    """(inv_scale [m_pad], the plane bytes) of a fused launch's workspace: launch_gemm_mfma :2387-2390"""
    buf = ws.cpu().numpy()
    off = -(-m_pad * 4 // 256) * 256
    return buf[: m_pad * 4].view(np.float32), buf[off:]


def padded_rows(m, digits, mat):
    ws_mode = 0 if mat.scale is None else 2 if mat.block == 32 else 1
    ttw = (2 if digits <= 3 else 1) if ws_mode >= 2 else 4 if digits == 2 and not ws_mode else 2  # gemm_ttw :2001
    return -(-m // (32 * ttw)) * (32 * ttw)


def check_quantiser(hip, torch_, tag, x, mat, digits, flags, ln=None):
    """one fused launch; the planes and the inverse scales in the workspace are the model's by value, the outputs within the form's bound"""
    m, cols = x.shape
    kp = -(-cols // 256) * 256
    form = "fp6" if flags & FP6 else "f16q" if mat.kind == "i2s32h" and digits == 2 else "int8"
    out = launch(hip, torch_, "fused", handle_of(hip, mat), mat, x, digits, flags, ln=ln, cols=cols)
    mp = padded_rows(m, digits, mat)
    inv, planes = workspace_views(out["ws"], m, mp, kp)
    if form == "f16q":
        mq, minv = R.quant_rows_f16(x, ln)
        got_q = planes[: mp * kp * 2].view(np.float16).reshape(mp, kp)[:m].astype(np.float64)
    else:
        mq, minv = R.quant_rows(x, digits, ln)
        got_q = R.decode_fp6_records(planes, m, kp, 576)[0] if form == "fp6" else R.decode_int8_planes(planes, m, kp, digits)
    assert np.array_equal(inv[:m].astype(np.float64), minv), tag
    assert not inv[m:mp].any(), (tag, "padding rows carry scale 0")
    assert not got_q[:, cols:].any(), (tag, "zero padding behind the last column")
    bad = np.argwhere(got_q[:, :cols] != mq)
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist(), [(float(got_q[i, j]), float(mq[i, j])) for i, j in bad[:4]])
    p = model(form, x, mat, digits, 0, ln)
    assert p.roundings == (digits - 1 if form == "int8" else cols if form == "f16q" else 3 * cols), tag
    check_values(tag, form + "/quantiser", out, p)


QUANT_K = [256, 300, 1100, 3072, 3076, 6912, 8192]


@functools.lru_cache(maxsize=None)
def edge_matrix(kind, cols):
    return R.make_matrix(kind, 48, cols, seed_of("edge", kind, cols))


@pytest.mark.parametrize("cols", QUANT_K)
def test_quantiser_edges(hip, torch_, cols):
    """300, 1100: ragged last blocks; 3072 | 3076: NV = 3 | 8; 8192: the largest K.  2 digits by value, the others within their bound"""
    for m in (1, 33):
        x = R.float_rows(max(m, 3), cols, seed_of("edge", m, cols))[:m]
        for digits, flags in ((2, 0), (3, 0), (4, 0), (2, FP6), (2, FP6 | FP6_EXPAND)):
            check_quantiser(hip, torch_, f"edge K={cols} m={m} digits={digits} flags={flags}", x, edge_matrix("qk256", cols), digits, flags)
        if cols % 256 == 0:
            mat = edge_matrix("i2s32h", cols)
            check_quantiser(hip, torch_, f"edge K={cols} m={m} f16 rows", x, mat, 2, 0)
            assert hip.matmul_last_tile()["scale_mode"] == 4


@pytest.mark.parametrize("cols", [1100, 2560])
def test_wave_per_row_quantiser_by_value(hip, torch_, cols):
    """k_quant_rows_w<0>, <1> without LayerNorm (denom = 1: the workgroup-per-row arithmetic), 2085 rows: 27 padding rows in the last workgroups"""
    m = 2085
    x = R.float_rows(m, cols, seed_of("wave", cols))
    for flags in (INT8, FP6):
        check_quantiser(hip, torch_, f"wave-per-row K={cols} flags={flags}", x, edge_matrix("qk256", cols), 2, flags)


# ---------------------------------------------------------------- f. the LayerNorm prologue
@pytest.mark.parametrize("cols", [256, 1100, 3076])
def test_layernorm_prologue_carries_the_model_integer(hip, torch_, cols):
    """k_quant_rows<NDIG, NV, FP6> with ln_gamma, integer-valued rows: the kernel's q is the model's in every column (the docstring's f.)"""
    m = 33
    rng = np.random.default_rng(seed_of("ln", cols))
    x = R.int_rows(m, cols, seed_of("lnx", cols), top=1000, peak=8192)
    ln = (rng.uniform(0.5, 1.5, cols).astype(np.float32), np.float32(1e-5))
    for digits, flags in ((2, 0), (3, 0), (4, 0), (2, FP6)):
        check_quantiser(hip, torch_, f"layernorm K={cols} digits={digits} flags={flags}", x, edge_matrix("qk256", cols), digits, flags, ln=ln)
    if cols % 256 == 0:
        check_quantiser(hip, torch_, f"layernorm K={cols} f16 rows", x, edge_matrix("i2s32h", cols), 2, 0, ln=ln)


# ---------------------------------------------------------------- g. environment switches
def child_main(hip, torch_, switch):
    for name, case in ENV_CASES[switch][1].items():
        worst = check_instance(hip, torch_, name, case)
        print("CHILD_OK", name, f"{worst:.4f}")
    for h, _ in _handles.values():
        hip.weights_free(h)


_CHILD = r"""
import importlib, sys
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
import test_gemm_instances_gpu as G
G.child_main(hip, torch, {switch!r})
print("CHILD_DONE")
"""


@pytest.mark.parametrize("switch", list(ENV_CASES))
def test_values_under_an_environment_switch(switch):
    env, cases = ENV_CASES[switch]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=root, switch=switch)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    print(p.stdout[-6000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert "CHILD_DONE" in lines and [l.split()[1] for l in lines if l.startswith("CHILD_OK ")] == list(cases), p.stdout[-3000:]
