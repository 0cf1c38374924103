"""GPU: every reachable instance of k_gemv_mfma (csrc/kernels_mfma.hip), the library's public GEMV on f32 activations, by value against the
float64 / int64 model of tests/gemv_mfma_ref.py.  Each case first asserts what bitnet_hip_gemv_geometry reports of the launch, then the values:

  exact vectors  one per digit plane p = 0..3: a pin pair +-2^29 u per 256-block fixes every K range's exponent and cancels in the integer sums,
                 every other element is n 2^(8 p) u (plane p alone), block scales are two neighbouring powers of two: nothing rounds, the output
                 must EQUAL u 2^(8 p) sum w n (times the scales) on every element (behind the LayerNorm-after-product epilogue: the once-rounded
                 value; behind silu * up: within the bound of its two instructions); and `rpi`: plane 0 plus a cancelling pair of odd integers
                 between 2^23 and 2^24 per block, which a conversion rounding x + 1/2 in f32 would move;
  float vectors  mixed (per-column magnitudes over 2^+-12), range (K-range maxima 2^20 apart), zero_range (one K range all zero), tiny (maxima
                 below 2^-95: the exponent clamp), edge (range maxima exactly 2^e and 2^e (2 - 2^-23)), zero, mean (LayerNorm only: mean 50 x the
                 deviation): every element within the bound gemv_mfma_ref derives (a count of f32 roundings x 2^-24 x the magnitudes that enter
                 them).  The three large shapes run `mixed` alone (their model is tens of millions of integer products per vector).
Epilogues: y only; residual; m = 3 rows with a residual (33x5); silu * up on the paired shapes; each with LayerNorm 0, 1 (prologue; float vectors)
and 2 (after the product, bound gamma).  The merging cases add the QAct output + gamma_out + statistics.  y lies between NaN guards, QAct and
statistics between 0xA5 guards; the kernel choice is set to MFMA for the module and restored.

Instances k_gemv_mfma<8, RING, NV, LN, BS32, MERGE>.  Every shape runs every scale form it can take: qk256 (BS32 0), i2s256 (BS32 0 + the runtime
256-block fold), i2s32 (BS32 1), i2s32h (BS32 2); NV is 1 without LayerNorm and the NV column with LN 1 and LN 2:

  shape      rows x cols    K split  K ranges (blocks)         blocks/wave RING NV  tiles/wg grid  what it is there for
  16x1         16 x 256     1        1                         1           2    2   8        1     one block, seven surplus waves
  3x2           3 x 512     2        1 1                       1           2    2   4        1     rows % 16 != 0 inside the only tile
  33x5         33 x 1280    4        1 1 1 2                   2           2    2   2        2     a ragged last tile and a surplus tile; m = 3
  48x11        48 x 2816    8        1 1 2 1 1 2 1 2           2           2    2   1        3     ranges shorter than RING behind the 11 - wave remap
  16x17        16 x 4352    8        2 2 2 2 2 2 2 3           3           3    4   1        1
  16x32        16 x 8192    8        4 4 4 4 4 4 4 4           4           4    4   1        1     LN 1 above 64 KiB of dynamic LDS (66688 / 75008 bytes)
  16x300c      16 x 300     2        1 1                       1           2    2   4        1     cols % 256 = 44: a ragged last block (qk256)
  48x2564c     48 x 2564    8        1 1 2 1 1 2 1 2           2           2    2   1        3     cols % 256 = 4: one float4 in the last block (qk256)
  P160x1      160 x 256     1        1                         1           2    2   8        2     5 pairs over 4 per workgroup
  P32x10       32 x 2560    4        2 3 2 3                   3           3    2   2        1
  P32x13       32 x 3328    4        3 3 3 4                   4           4    2   2        1
  P32x17       32 x 4352    4        4 4 4 5                   5           5    4   2        1     LN 1 above 64 KiB with 32-block scales (69888 bytes)
  4112x9     4112 x 2304    4        2 2 2 3                   3           3    2   2        129   257 tiles: the first shape off split 8
  8208x9     8208 x 2304    2        4 5                       5           5    2   4        129   513 tiles: off split 4
  16400x5   16400 x 1280    1        5                         5           5    2   8        129   1025 tiles: off split 2
(P = an interleave16 (gate, up) handle run with FUSE_SILU_MUL: at most 4 K ranges.)  A matrix with 256-block scales and ragged columns has no
QK256-shaped rows: bitnet_hip_gemv_geometry reports that it leaves the MFMA kernel (kernel = VALU), which the two ragged-column shapes assert.

Reached: LN 0: RING 2, 3, 4, 5 x 3 scale forms = 12; LN 1 and LN 2: (RING, NV) = (2, 2), (3, 2), (4, 2), (5, 2), (3, 4), (4, 4), (5, 4) x 3 scale forms
= 21 each; MERGE: 3.  57 of 63.
Unreachable (no shape the entries accept selects them; removing them is not this file's business): RING 2 with NV 4, LN 1 and LN 2 x 3 scale forms
= 6: NV 4 needs more than 4096 columns = 17 blocks or more, which no K split brings to 2 per wave (8 ranges of 17 blocks hold 3).

Merging instances k_gemv_mfma<8, 2, 1, 0, BS32, 1> (16 rows; records WRITTEN BY THE TEST; bitnet_hip_gemv_attn_merge_dev for qk256, i2s32, i2s32h
and bitnet_hip_gemv_attn_merge_q_dev -- QAct out, gamma_out, statistics -- for i2s256, which the QAct GEMV does not take):
  heads / KV heads (group)   columns  K split
  2 / 2 (1)                  256      1
  4 / 2 (2)                  512      2
  20 / 5 (4)                 2560     8       ranges 1 1 1 2 1 1 1 2: skipped merge slots
at 1, 2 and 4 live records, chunk maxima 0, 40 and 90 apart (e^-90 underflows to 0), dead records holding stale finite values with a large m,
and a record buffer of 2 records (the index clamp)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_mfma_ref as M  # noqa: E402
import gemvq_ref as Q  # noqa: E402
from qact_ref import quantize_qact  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> rows, cols, paired (run with silu * up), what the geometry entry must report without LayerNorm, NV with LayerNorm
SHAPES = {
    "16x1": (16, 256, False, dict(k_split=1, blocks=1, blocks_per_wave=1, ring=2, tiles_per_workgroup=8, grid=1), 2),
    "3x2": (3, 512, False, dict(k_split=2, blocks=2, blocks_per_wave=1, ring=2, tiles_per_workgroup=4, grid=1), 2),
    "33x5": (33, 1280, False, dict(k_split=4, blocks=5, blocks_per_wave=2, ring=2, tiles_per_workgroup=2, grid=2), 2),
    "48x11": (48, 2816, False, dict(k_split=8, blocks=11, blocks_per_wave=2, ring=2, tiles_per_workgroup=1, grid=3), 2),
    "16x17": (16, 4352, False, dict(k_split=8, blocks=17, blocks_per_wave=3, ring=3, tiles_per_workgroup=1, grid=1), 4),
    "16x32": (16, 8192, False, dict(k_split=8, blocks=32, blocks_per_wave=4, ring=4, tiles_per_workgroup=1, grid=1), 4),
    "16x300c": (16, 300, False, dict(k_split=2, blocks=2, blocks_per_wave=1, ring=2, tiles_per_workgroup=4, grid=1), 2),
    "48x2564c": (48, 2564, False, dict(k_split=8, blocks=11, blocks_per_wave=2, ring=2, tiles_per_workgroup=1, grid=3), 2),
    "P160x1": (160, 256, True, dict(k_split=1, blocks=1, blocks_per_wave=1, ring=2, tiles_per_workgroup=8, grid=2), 2),
    "P32x10": (32, 2560, True, dict(k_split=4, blocks=10, blocks_per_wave=3, ring=3, tiles_per_workgroup=2, grid=1), 2),
    "P32x13": (32, 3328, True, dict(k_split=4, blocks=13, blocks_per_wave=4, ring=4, tiles_per_workgroup=2, grid=1), 2),
    "P32x17": (32, 4352, True, dict(k_split=4, blocks=17, blocks_per_wave=5, ring=5, tiles_per_workgroup=2, grid=1), 4),
    "4112x9": (4112, 2304, False, dict(k_split=4, blocks=9, blocks_per_wave=3, ring=3, tiles_per_workgroup=2, grid=129), 2),
    "8208x9": (8208, 2304, False, dict(k_split=2, blocks=9, blocks_per_wave=5, ring=5, tiles_per_workgroup=4, grid=129), 2),
    "16400x5": (16400, 1280, False, dict(k_split=1, blocks=5, blocks_per_wave=5, ring=5, tiles_per_workgroup=8, grid=129), 2),
}
LARGE = ("4112x9", "8208x9", "16400x5")
ROWS3 = "33x5"  # the shape that also runs m = 3 with a residual
# every (shape, kind) the table runs by value: ragged columns take no scaled kind (2 x 1), every other shape all four (13 x 4)
CASES = [(n, k) for n in SHAPES for k in M.KINDS if not (SHAPES[n][1] % 256 and k != "qk256")]
N_CASES = 54
LEAVES_MFMA = [(n, "i2s256") for n in SHAPES if SHAPES[n][1] % 256]  # asserted from the geometry entry alone
# heads, KV heads -> K split
MERGES = {(2, 2): 1, (4, 2): 2, (20, 5): 8}
MERGE_ROWS = 16
EPS = 1e-5
WORST = {}  # epilogue kind -> largest error / bound seen (printed; EXPERIMENTS.md keeps the figures of one run)


def lds_bytes(name, kind, ln):
    """dynamic LDS of a launch (kernels_mfma.hip :147-152): 8 waves x (4, or 5 with 32-block scales) planes of RING 256 + 16 bytes, the statistics
    and partial sums, and with LN 1 the normalised row"""
    _, cols, _, expect, _ = SHAPES[name]
    return 8 * (5 if M.FOLD[kind] == 32 else 4) * (expect["ring"] * 256 + 16) + 128 + 512 + (4 * cols if ln == 1 else 0)


def seed_of(*parts):
    return sum((i + 1) * sum(map(ord, str(p))) for i, p in enumerate(parts)) % (1 << 31)


def weights_for(name, kind, scales):
    rows, cols, paired, _, _ = SHAPES[name]
    mk = lambda r, tag: M.pin_codes(Q.make_weights(kind, r, cols, seed_of(name, kind, scales, tag), scales, any_shape=True))
    if not paired:
        return mk(rows, "w")
    return Q.pair(mk(rows // 2, "gate"), mk(rows // 2, "up"))


def ln_gamma_for(cols, mode, seed):
    rng = np.random.default_rng(seed)
    if mode == "exact":  # one of two neighbouring powers of two per 256-block: x * gamma and W . gamma are exact, and a pin pair shares one
        return np.repeat(rng.choice(np.array([0.25, 0.125], np.float32), -(-cols // 256)), 256)[:cols]
    return (rng.uniform(0.5, 1.5, cols) / (1.58 * np.sqrt(cols))).astype(np.float32)


def log2_unit(kind):
    return 10 if kind == "i2s32" else -20  # (the exact i2s32 matrices carry block scales of 2^-30, 2^-31)


def vectors(name, kind, mode, ln, ln_gamma):
    """[(tag, x f32 [cols])]: the activation rows a case runs"""
    rows, cols, _, expect, _ = SHAPES[name]
    if mode == "exact":
        out = [(f"plane{p}", M.plane_vector(cols, p, seed_of(name, "plane", p), log2_unit(kind))) for p in range(4)]
        out.append(("rpi", M.rpi_vector(cols, seed_of(name, "rpi"), log2_unit(kind))))
        if ln == 2:  # the un-normalised vectors whose product with gamma is the exact vector (powers of two: exact)
            out = [(t, (u.astype(np.float64) / ln_gamma.astype(np.float64)).astype(np.float32)) for t, u in out]
        return out
    kinds = ["mixed"] if name in LARGE else ["mixed", "range", "zero_range", "tiny", "edge", "zero"] + (["mean"] if ln else [])
    rg = M.column_ranges(cols, expect["k_split"])
    return [(k, M.float_vector(cols, seed_of(name, k), k, rg)) for k in kinds]


def exact_products(name, kind):
    """[(tag, Product)] of the plane vectors of a case without LayerNorm and with LN 2 (tests/test_gemv_mfma_ref.py asserts bound 0 from here)"""
    wts = weights_for(name, kind, "pow2")
    ks = SHAPES[name][3]["k_split"]
    g = ln_gamma_for(wts.cols, "exact", seed_of(name, "gamma"))
    out = [(tag, M.product(wts, x, ks)) for tag, x in vectors(name, kind, "exact", 0, None)]
    out += [(tag + "*gamma", M.product(wts, x * g, ks)) for tag, x in vectors(name, kind, "exact", 2, g)]
    out.append(("gamma", M.product(wts, g, ks)))
    return out


# ---------------------------------------------------------------- device helpers
@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


@pytest.fixture(scope="module")
def mfma(hip, pkg):
    """the process-wide kernel choice set to MFMA for this module, and restored"""
    before = hip.get_kernel()
    hip.set_kernel(pkg.KERNEL_MFMA)
    yield hip
    hip.set_kernel(before)


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(hip, wts):
    if "parts" in wts.upload:
        parts = [upload(hip, p) for p in wts.upload["parts"]]
        h = hip.weights_concat(parts, interleave16=True)
        for p in parts:
            hip.weights_free(p)
        return h
    if wts.kind == "qk256":
        return hip.weights_upload_qk256(wts.upload["qs"].reshape(-1), wts.rows, wts.cols, wts.upload["stride"])
    return hip.weights_upload_i2s(wts.upload["packed"].reshape(-1), wts.upload["scales"].reshape(-1), wts.rows, wts.cols, wts.upload["block"])


class Guarded:
    """a device buffer of n elements between two 64-byte guards (NaN for floats, 0xA5 for bytes) that must survive the launch"""

    def __init__(self, torch_, n, dtype, interior):
        self.pad = 64 // {torch_.float32: 4, torch_.float64: 8, torch_.uint8: 1}[dtype]
        self.fill = 0xA5 if dtype == torch_.uint8 else float("nan")
        self.buf = torch_.full((n + 2 * self.pad,), self.fill, dtype=dtype, device="cuda")
        self.view = self.buf[self.pad: self.pad + n]
        self.view.fill_(interior)

    def read(self):
        """the interior as numpy; asserts the guards"""
        a = self.buf.cpu().numpy()
        want = np.full(self.pad, self.fill, a.dtype).view(np.uint8)
        assert np.array_equal(a[: self.pad].view(np.uint8), want) and np.array_equal(a[-self.pad:].view(np.uint8), want), "guard overwritten"
        return a[self.pad: -self.pad].copy()


def hold(got, p, tag, kind):
    """every element within the model's bound; where the bound is 0, equal by value.  -> the worst error / bound"""
    tgt, bound = M.target(p)[0], p.bound[0]
    err = np.abs(got.astype(np.float64) - tgt)
    assert not np.isnan(got).any(), tag
    exact = bound == 0
    print(*tag, end=" ")
    assert np.array_equal(got[exact].astype(np.float64), tgt[exact]), (tag, "exact elements differ", int((err[exact] > 0).sum()), float(err[exact].max()))
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print(f"worst error / bound {ratio:.4f}", f"({int(exact.sum())} of {exact.size} elements exact)")
    assert ratio <= 1.0, (tag, ratio, int(np.argmax(np.where(exact, 0.0, err / np.where(exact, 1.0, bound)))))
    return ratio


def hold_qact(q, s, v, gam, tag):
    """the QAct and statistics the kernel left of its own f32 output v: the quantiser's bits; the pairs are f32 sums over 16 values"""
    assert np.array_equal(q, quantize_qact(v, gam)), (tag, "qact")
    v64 = v.astype(np.float64).reshape(-1, 16)
    st = s.reshape(-1, 2)
    assert np.all(np.abs(st[:, 0] - v64.sum(1)) <= M.R.gamma(15) * np.abs(v64).sum(1) + M.TINY), (tag, "sum")
    assert np.all(np.abs(st[:, 1] - (v64 * v64).sum(1)) <= M.R.gamma(16) * (v64 * v64).sum(1) + 16 * M.TINY), (tag, "sum of squares")


def check_geometry(pkg, geo, name, kind, ln, merge=0):
    """what bitnet_hip_gemv_geometry reports against the table"""
    _, cols, _, expect, nv = SHAPES[name]
    want = dict(expect, kernel=pkg.KERNEL_MFMA, unfused=0, stat_vectors=nv if ln else 1, layernorm=ln, scale_form=M.SCALE_FORM[kind],
                wscale=int(kind == "i2s256"), merge=merge, lds_bytes=lds_bytes(name, kind, ln), lds_raised=int(lds_bytes(name, kind, ln) > 65536))
    assert geo == want, (name, kind, ln, geo, want)


# ---------------------------------------------------------------- the plain instances
@pytest.mark.parametrize("name,kind", CASES)
def test_instance_by_value(mfma, pkg, torch_, name, kind):
    hip = mfma
    rows, cols, paired, expect, _ = SHAPES[name]
    out_rows, flags, ks = rows // 2 if paired else rows, 1 if paired else 0, expect["k_split"]  # flags: BITNET_HIP_FUSE_SILU_MUL
    rng = np.random.default_rng(seed_of(name, kind, "epilogue"))
    res = rng.normal(0, 1, (3, out_rows)).astype(np.float32)
    res_d = dev(torch_, res)
    for mode in ("float",) if name in LARGE else ("exact", "float"):
        wts = weights_for(name, kind, "pow2" if mode == "exact" else "float")
        h = upload(hip, wts)
        g_np = ln_gamma_for(cols, mode, seed_of(name, "gamma"))
        g_d, g_unbound = dev(torch_, g_np), dev(torch_, g_np)
        check_geometry(pkg, hip.gemv_geometry(h, flags), name, kind, 0)
        check_geometry(pkg, hip.gemv_geometry(h, flags, ln_gamma=g_unbound), name, kind, 1)
        bind_ks = hip.gemv_geometry(h, 0)["k_split"]  # the binding launch is the unpaired one
        hip.weights_bind_ln(h, g_d)
        check_geometry(pkg, hip.gemv_geometry(h, flags, ln_gamma=g_d), name, kind, 2)
        check_geometry(pkg, hip.gemv_geometry(h, flags, ln_gamma=g_unbound), name, kind, 1)  # another pointer: the prologue form
        for ln in (0, 1, 2):
            if ln == 1 and mode == "exact":
                continue  # (the prologue's three f32 operations leave no exact value: LN 1 runs the float vectors)
            lnk = ("" if ln == 0 else f"+ln{ln}") + (", exact vectors" if mode == "exact" else "")
            kw = dict(flags=flags)
            if ln:
                kw.update(ln_gamma=g_unbound if ln == 1 else g_d, ln_eps=EPS)
            for vtag, x in vectors(name, kind, mode, ln, g_np):
                x_d = dev(torch_, x)
                base = M.launch(wts, x, ks, ln=(ln, g_np, EPS, bind_ks) if ln else None, silu=paired)
                tag = (name, kind, mode, f"ln{ln}", vtag)
                # y only: a buffer of whole tiles behind the rows, so a surplus store shows
                y = Guarded(torch_, out_rows, torch_.float32, float("nan"))
                hip.gemv_fused_dev(h, x_d, y.view, **kw)
                torch_.cuda.synchronize()
                hold(y.read(), base, tag + ("silu" if paired else "y",), ("silu" if paired else "product") + lnk)
                if ln == 0 and not paired:  # the same launch through the unfused entries
                    y = Guarded(torch_, out_rows, torch_.float32, float("nan"))
                    hip.gemv_dev(h, x_d, y.view)
                    torch_.cuda.synchronize()
                    hold(y.read(), base, tag + ("gemv_dev",), "product")
                if not paired:  # residual (the paired form has none)
                    y = Guarded(torch_, out_rows, torch_.float32, float("nan"))
                    hip.gemv_fused_dev(h, x_d, y.view, residual=res_d[0], **kw)
                    torch_.cuda.synchronize()
                    hold(y.read(), Q.add_residual(base, res[0]), tag + ("residual",), "residual" + lnk)
                assert np.array_equal(x_d.cpu().numpy(), x), (tag, "input overwritten")
            if name == ROWS3 and mode == "float":  # m = 3: grid.y walks the rows, each with its own residual row
                xs = np.stack([x for _, x in vectors(name, kind, mode, ln, g_np)[:3]])
                ps = M.launch_rows(wts, xs, ks, residual=res, ln=(ln, g_np, EPS, bind_ks) if ln else None)
                y = Guarded(torch_, 3 * out_rows, torch_.float32, float("nan"))
                hip.gemv_fused_dev(h, dev(torch_, xs.reshape(-1)), y.view, m=3, residual=res_d.reshape(-1), **kw)
                torch_.cuda.synchronize()
                got = y.read().reshape(3, out_rows)
                for i, p in enumerate(ps):
                    hold(got[i], p, (name, kind, f"ln{ln}", "m=3 row", i), "residual m=3" + lnk)
                if ln == 0:  # bitnet_hip_matmul_dev rows (m < 16 stays on the GEMV)
                    y = Guarded(torch_, 3 * out_rows, torch_.float32, float("nan"))
                    hip.matmul_dev(h, dev(torch_, xs.reshape(-1)), y.view, 3)
                    torch_.cuda.synchronize()
                    got = y.read().reshape(3, out_rows)
                    for i, p in enumerate(M.launch_rows(wts, xs, ks)):
                        hold(got[i], p, (name, kind, "matmul_dev row", i), "product")
        hip.weights_free(h)
    print("worst error / bound so far:", {k: round(r, 4) for k, r in sorted(WORST.items())})


@pytest.mark.parametrize("name,kind", LEAVES_MFMA)
def test_ragged_columns_with_block_scales_leave_the_mfma_kernel(mfma, pkg, name, kind):
    """a scaled matrix of cols % 256 != 0 keeps cols / 4 bytes per row, not whole 64-byte blocks: no tiles, and the entry says which kernel runs"""
    rows, cols, _, _, _ = SHAPES[name]
    rng = np.random.default_rng(seed_of(name, kind))
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(rows, cols))
    s = rng.uniform(0.05, 2.0, (rows, -(-cols // 256))).astype(np.float32)
    h = mfma.weights_upload_i2s(M.R.pack_codes(codes).reshape(-1), s.reshape(-1), rows, cols, 256)
    geo = mfma.gemv_geometry(h)
    assert geo["kernel"] in (pkg.KERNEL_VALU, pkg.KERNEL_EXACT) and geo["unfused"] == 0 and geo["k_split"] == 0 and geo["ring"] == 0, geo
    mfma.weights_free(h)


# ---------------------------------------------------------------- the merging instances
def write_records(rng, n_kv, group, chunks_max, live, apart):
    """the chunk records of launch_attn_decode(.., combine = false), written by the test: per KV head and chunk (m, l)[4] and o[4][128] for the
    group's heads.  Live records: m = a base per head, `apart` lower in every record but one, l in 1 .. 30, |o| <= l; dead records: stale finite values and m = 1e4."""
    s = np.zeros((n_kv, chunks_max, Q.REC_FLOATS), np.float32)
    for kv in range(n_kv):
        for c in range(chunks_max):
            rec = s[kv, c]
            for j in range(4):
                if c < live and j < group:
                    top = c == (kv + j) % live  # the record that holds the head's maximum
                    rec[2 * j] = 2.0 * (kv - j) + rng.normal(0, 0.5) - (0.0 if top else apart)
                    rec[2 * j + 1] = rng.uniform(1.0, 30.0)
                    rec[8 + 128 * j: 8 + 128 * (j + 1)] = rng.normal(0, 0.4, 128) * rec[2 * j + 1]
                else:
                    rec[2 * j], rec[2 * j + 1] = 1e4, 7.0
                    rec[8 + 128 * j: 8 + 128 * (j + 1)] = rng.normal(0, 50.0, 128)
    return s.reshape(-1)


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("n_heads,n_kv", list(MERGES))
def test_merging_instance_by_value(mfma, pkg, torch_, n_heads, n_kv, kind):
    hip = mfma
    cols, rows, group = n_heads * 128, MERGE_ROWS, n_heads // n_kv
    wts = Q.make_weights(kind, rows, cols, seed_of("merge", n_heads, kind), any_shape=True)
    h = upload(hip, wts)
    geo = hip.gemv_geometry(h, merge=group)
    assert (geo["kernel"], geo["merge"], geo["ring"], geo["stat_vectors"], geo["layernorm"], geo["scale_form"], geo["wscale"], geo["k_split"]) == \
        (pkg.KERNEL_MFMA, 1, 2, 1, 0, M.SCALE_FORM[kind], int(kind == "i2s256"), MERGES[(n_heads, n_kv)]), geo
    assert geo["blocks_per_wave"] <= 2 and geo["lds_raised"] == 0
    rng = np.random.default_rng(seed_of("merge", n_heads, n_kv, kind))
    res = rng.normal(0, 1, rows).astype(np.float32)
    gam = rng.uniform(0.5, 1.5, rows).astype(np.float32)
    res_d, gam_d = dev(torch_, res), dev(torch_, gam)
    # (max_pos, pos, chunk maxima apart): 1, 2 and 4 live records; a buffer of 2 records, shorter than the 4 requested: the index clamp
    for max_pos, pos, apart in [(256, 10, 0.0), (256, 100, 40.0), (256, 255, 90.0), (256, 200, 0.0), (128, 100, 90.0)]:
        chunks_max, live = -(-max_pos // 64), (pos + 64) >> 6
        records = write_records(rng, n_kv, group, chunks_max, live, apart)
        scratch = Guarded(torch_, records.size, torch_.float32, 0.0)
        scratch.view.copy_(dev(torch_, records))
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        v, delta = M.merged_row(records, pos, n_heads, n_kv, chunks_max)
        p = Q.add_residual(M.product(wts, v, geo["k_split"], spread=delta), res)
        tag = ("merge", f"{n_heads}/{n_kv}", kind, f"max_pos {max_pos}", f"pos {pos}", f"apart {apart}")
        y = Guarded(torch_, rows, torch_.float32, float("nan"))
        if kind == "i2s256":  # the QAct-producing entry stays on this kernel for a matrix the QAct GEMV does not take
            q = Guarded(torch_, hip.qact_bytes(rows), torch_.uint8, 0)
            s = Guarded(torch_, rows // 16 * 2, torch_.float64, float("nan"))
            hip.gemv_attn_merge_q_dev(h, scratch.view, n_heads, n_kv, max_pos, pos_d, y.view, q.view, residual=res_d, gamma_out=gam_d, stats_out=s.view)
            torch_.cuda.synchronize()
            got = y.read()
            hold_qact(q.read(), s.read(), got, gam, tag)
        else:
            hip.gemv_attn_merge_dev(h, scratch.view, n_heads, n_kv, max_pos, pos_d, y.view, residual=res_d)
            torch_.cuda.synchronize()
            got = y.read()
        assert np.array_equal(scratch.read(), records), "records overwritten"
        hold(got, p, tag, "merge")
    hip.weights_free(h)
    print("worst error / bound so far:", {k: round(r, 4) for k, r in sorted(WORST.items())})
