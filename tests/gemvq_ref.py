"""CPU model (numpy, float64 / int64) of one k_gemv_q launch, the decode step's GEMV on producer-quantised activations -- test infrastructure.

bitnet-rs_amd/csrc/kernels_gemvq.hip is the specification; the line ranges name what each function restates.  The activation format is
tests/qact_ref.py's (csrc/qact.hpp); codes, code maps, interleave16, gamma(n), Product and the residual / silu * up epilogues are tests/gemm_ref.py's
(the two kernels share those formulas: gsilu_mul there is :460 here, the residual :432).

  weights     make_weights: int8 code values [rows, cols] and one float64 scale per 32-block (None: QK256) -- gemm_ref.Matrix keeps a float64
              scale per COLUMN, which the larger shapes here (8224 x 2304) cannot afford; kinds and code maps are gemm_ref's.
  K ranges    k_ranges (:109-116): K part kp of a row tile covers blocks (kp nblk) >> log2 ks .. ((kp + 1) nblk) >> log2 ks.  (The `kpart = 11 - wave`
              remap at 8 parts (:115) changes which WAVE computes a part, not what the part holds, and the partial sums are stored and added by
              part (:393, :427-430): the model has parts, no waves.)
  product     product (:355-393, :425-430): per 16-column half the exact integer i = sum_k (256 d1 + d0)_k w_k (:369), times the half's group scale;
              the two halves of a 32-block joined by one fmaf (:370-371), the block scale applied by the fma that accumulates (:372-377), the lane
              group's blocks in order, two lane-swap additions (:386-391), the K parts in order (:430).
  LayerNorm   layernorm_after (:399-415, :431): mean and variance from the statistics pairs, applied after the product with g_r = W[r,:] . gamma
              (g_rows: bitnet_hip_weights_bind_ln computes it with k_gemv_mfma, csrc/kernels_mfma.hip :355-375, :385-484).
  epilogues   residual (:432), silu(gate) * up on interleave16 pairs (:437-462): gemm_ref.add_residual / gemm_ref.silu_mul.  The QAct output and its
              statistics (:434, :462) are qact_ref.quantize_qact of the kernel's own f32 output, checked for bits by the GPU file.
  merging     merge_records (:130-175, :229-288, :314-324): the softmax merge of the attention's chunk records in float64 and what f32 may differ
              by; quant_interval (:289-311, :325-337): every QAct the quantiser can make of a value within that distance.
  bounds      a count of f32 roundings x 2^-24 x the magnitudes that enter them, gamma(n) = n u / (1 - n u); the derivations stand at each function.
              Nothing here is fitted to a device's output."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402
from qact_ref import QREC, _slot, quantize_qact  # noqa: E402

U = R.U
KINDS = ("qk256", "i2s32", "i2s32h")  # scale form 0 (none), 1 (f32 per 32-block), 2 (f16 per 32-block)
SCALE_FORM = {"qk256": 0, "i2s32": 1, "i2s32h": 2}
REC_FLOATS = 8 + 4 * 128  # one attention chunk record: (m, l)[4], o[4][128] (csrc/common.hpp kAttnRecFloats)
TINY = 2.0 ** -126        # what a flushed or denormal f32 result may lose


# ---------------------------------------------------------------- weights
class Weights:
    """w int8 [rows, cols] (code values); scale float64 [rows, ceil(cols / block)] or None; block = columns per scale (32, or 256 for the
    256-block scales only k_gemv_mfma takes); upload = the arguments of the upload call"""

    def __init__(self, kind, w, scale, upload, block=32):
        self.kind, self.w, self.scale, self.upload, self.block = kind, w, scale, upload, block
        self.rows, self.cols = w.shape

    def _rows32(self, a, absolute):
        out = np.zeros(self.rows)
        blk = self.block if self.cols % 32 == 0 else 256  # (ragged columns: k_gemv_mfma's shapes, no scales or 256-block ones)
        nb = -(-self.cols // blk)
        for r0 in range(0, self.rows, 1024):  # (the largest shapes hold 19 M weights: no whole-matrix float64 copy)
            w = self.w[r0:r0 + 1024].astype(np.float64)
            t = (np.abs(w) if absolute else w) * a[None, :]
            if nb * blk != self.cols:
                t = np.concatenate([t, np.zeros((t.shape[0], nb * blk - self.cols))], axis=1)
            t = t.reshape(-1, nb, blk).sum(-1)
            if self.scale is not None:
                t = t * (np.abs(self.scale[r0:r0 + 1024]) if absolute else self.scale[r0:r0 + 1024])
            out[r0:r0 + 1024] = t.sum(1)
        return out

    def abs_row_sums(self, a):
        """sum_k |W[r, k]| a_k for a >= 0 [cols] -> [rows] (float64; the block scale included)"""
        return self._rows32(np.asarray(a, np.float64), True)

    def dot(self, a):
        """sum_k W[r, k] a_k in float64"""
        return self._rows32(np.asarray(a, np.float64), False)


def make_weights(kind, rows, cols, seed, scales="float", any_shape=False):
    """scales: "float" = arbitrary block scales (f16 values for i2s32h); "pow2" = two neighbouring powers of two (no f16 values for i2s32: a matrix
    whose 32-block scales all are f16 values takes the f16 scale tiles).  any_shape (k_gemv_mfma): rows of any count, kind "i2s256" (one f32 scale
    per 256-block), and for qk256 columns of any multiple of 4 -- the row keeps whole 64-byte blocks, the codes past `cols` are random and must
    not enter the product."""
    assert kind in KINDS + (("i2s256",) if any_shape else ()) and (any_shape or (cols % 256 == 0 and rows % 16 == 0))
    rng = np.random.default_rng(seed)
    if kind == "qk256":
        assert cols % 4 == 0
        stride = -(-cols // 256) * 64
        qs = rng.integers(0, 256, (rows, stride), dtype=np.uint8)
        return Weights(kind, R.QK256_MAP[R.unpack_codes(qs, cols)].astype(np.int8), None, dict(qs=qs, stride=stride))
    assert cols % 256 == 0  # (a scaled matrix of ragged columns has no QK256-shaped rows: it leaves the MFMA kernel)
    block = 256 if kind == "i2s256" else 32
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(rows, cols), p=[0.5, 0.25, 0.25])
    if scales == "pow2":
        s = np.exp2(-rng.integers(0, 2, (rows, cols // block)).astype(np.float64) - (30.0 if kind == "i2s32" else 0.0)).astype(np.float32)
    else:
        s = rng.uniform(0.05, 2.0, (rows, cols // block)).astype(np.float32)
        if kind == "i2s32h":
            s = s.astype(np.float16).astype(np.float32)
    return Weights(kind, R.I2S_MAP[codes].astype(np.int8), s.astype(np.float64), dict(packed=R.pack_codes(codes), scales=s, block=block), block)


def pair(a, b):
    """the (gate, up) handle of weights_concat(.., interleave16=True)"""
    sc = None if a.scale is None else R.interleave16(a.scale, b.scale)
    return Weights(a.kind, R.interleave16(a.w, b.w), sc, dict(parts=(a, b)), a.block)


# ---------------------------------------------------------------- the activation
def read_qact(rec, n):
    """QAct records -> d0, d1 int64 [n] (the digit planes) and as float64 [n / 16] (the group scales, powers of two)"""
    assert n % 256 == 0
    r = np.asarray(rec, np.uint8)[: n // 256 * QREC].reshape(n // 256, QREC)
    d0 = r[:, :256].copy().view(np.int8).astype(np.int64).reshape(-1)
    d1 = r[:, 256:512].copy().view(np.int8).astype(np.int64).reshape(-1)
    sc = r[:, 512:].copy().view(np.float32).astype(np.float64)
    return d0, d1, sc[:, [_slot(t) for t in range(16)]].reshape(-1)


def dequantised(rec, n):
    d0, d1, as_ = read_qact(rec, n)
    return (256 * d1 + d0) * np.repeat(as_, 16)


# ---------------------------------------------------------------- the product
def k_ranges(nblk, k_split):
    """:109-116 -- [(b0, b1)] per K part"""
    lg = {1: 0, 2: 1, 4: 2, 8: 3}[k_split]
    return [((kp * nblk) >> lg, ((kp + 1) * nblk) >> lg) for kp in range(k_split)]


def block_sums(wts, q, as_, scale=None, rows=slice(None)):
    """-> blk, mag float64 [rows, nblk]: per 256-column block the exact sum_k s w_k q_k as and the sum of the magnitudes |s| |i_h| as_h of its 16
    halves (i_h the exact integer of a half, what enters the roundings).  |i_h| <= 16 * 2 * 2^14 = 2^19: int32 holds it, float64 holds i_h as_h and
    the handful of additions behind it to 2^-53, which is 2^-29 of the bound's unit."""
    scale = wts.scale if scale is None else scale
    w = wts.w[rows]
    n, cols = w.shape
    blk, mag = np.zeros((n, cols // 256)), np.zeros((n, cols // 256))
    q32 = q.astype(np.int32)
    for r0 in range(0, n, 1024):
        i_h = (w[r0:r0 + 1024].astype(np.int32) * q32[None, :]).reshape(-1, cols // 16, 16).sum(-1, dtype=np.int64)
        t16, m16 = i_h * as_[None, :], np.abs(i_h) * as_[None, :]
        t32, m32 = t16.reshape(-1, cols // 32, 2).sum(-1), m16.reshape(-1, cols // 32, 2).sum(-1)
        if scale is not None:
            s = scale[rows][r0:r0 + 1024]
            t32, m32 = t32 * s, m32 * np.abs(s)
        blk[r0:r0 + 1024] = t32.reshape(-1, cols // 256, 8).sum(-1)
        mag[r0:r0 + 1024] = m32.reshape(-1, cols // 256, 8).sum(-1)
    return blk, mag


def product_roundings(nblk, k_split):
    """f32 roundings in sequence on the longest path from a 16-half to the output: the fmaf joining the two halves of a 32-block (1; the first half's
    i_0 as_0 is an integer below 2^19 times a power of two: exact), the accumulating fma or addition of every 32-block of the lane's K range (2 per
    256-block, the block scale inside the fma: one rounding each; the first one adds to 0 but is counted), the two lane-swap additions (2), the K
    parts added to 0 in order (k_split - 1; 0 + part is exact)."""
    longest = max(b1 - b0 for b0, b1 in k_ranges(nblk, k_split))
    return 1 + 2 * longest + 2 + (k_split - 1)


def product(wts, d0, d1, as_, k_split, fault=None, spread=None):
    """k_gemv_q's row sums before the epilogue -> gemm_ref.Product (one token: arrays [1, rows]).

    want = sum over the K parts of their blocks' exact sums.  |error| <= gamma(n) sum |s| |i_h| as_h + n 2^-126, n = product_roundings: recursive
    summation, every term passing through at most n roundings, each relative to a partial sum no larger than the sum of the magnitudes (Higham,
    Accuracy and Stability, 4.2); the last term covers results below the normal range.  Where the partial sums of EVERY order stay below 2^24 units
    of the smallest term's quantum (`units`: power-of-two block scales, equal group scales) nothing rounds: bound 0, exact32 = f32(want).
    spread [cols] >= 0 (the merging form): the activation is only known to lie within `spread` of these digits' value; the output moves by at most
    sum_k |W_k| spread_k, and the magnitudes that enter the roundings grow by as much.
    fault: see FAULTS -- the model's answer under one planted fault."""
    nblk = wts.cols // 256
    q = (128 if fault == "plane_weight" else 256) * d1 + d0
    scale = wts.scale
    if fault == "scale_pair" and scale is not None:  # the two 32-block scales of a lane pair (pp = 0 / 1, :370-375), everywhere
        scale = scale.reshape(wts.rows, -1, 2)[:, :, ::-1].reshape(wts.rows, -1)
    blk, mag = block_sums(wts, q, as_, scale)
    ranges = k_ranges(nblk, k_split)
    parts = np.stack([blk[:, b0:b1].sum(1) for b0, b1 in ranges], axis=1)  # [rows, k_split]
    if fault == "part_dropped":  # the last K part of the first row tile never reaches the sum
        parts[:16, k_split - 1] = 0.0
    elif fault == "parts_swapped":  # part 0 of two neighbouring tiles: the LDS slot of the wrong tile (:393, :427)
        parts[:16, 0], parts[16:32, 0] = parts[16:32, 0].copy(), parts[:16, 0].copy()
    elif fault == "clamped_twice":  # a short range's clamped slot (:213) added instead of skipped (:358)
        longest = max(b1 - b0 for b0, b1 in ranges)
        kp = [i for i, (b0, b1) in enumerate(ranges) if b1 - b0 < longest][0]
        parts[:, kp] += blk[:, ranges[kp][1] - 1]
    want, m = parts.sum(1), mag.sum(1)
    n = product_roundings(nblk, k_split)
    extra = 0.0 if spread is None else wts.abs_row_sums(spread)
    bound = R.gamma(n) * (m + extra) + n * TINY + extra
    # exactness: every term is a multiple of (smallest group scale) x (quantum of the block scales); units = the sum of magnitudes in that quantum
    quantum = as_.min() * (1.0 if wts.scale is None else float(R.quantum(np.abs(wts.scale).reshape(1, -1)).min()))
    units = m / quantum
    exact = (units < R.EXACT_UNITS) & (spread is None)
    return R.Product(want[None, :], np.where(exact, 0.0, bound)[None, :], R._f32_exact(want)[None, :], units[None, :], n, m[None, :])


# ---------------------------------------------------------------- LayerNorm after the product
G_ROUNDINGS = 2 * 2 * 5 + 4 + 7  # see g_rows


def g_rows(wts, ln_gamma, bind_k_split=None):
    """bind_k_split (the K split of the binding launch, where the caller knows it from bitnet_hip_gemv_geometry): the bound of tests/gemv_mfma_ref.py's
    model of that very launch, which knows the digits and counts the roundings of the partition taken; without it the partition-free bound below.

    g_r = W[r, :] . gamma as bitnet_hip_weights_bind_ln leaves it: ONE k_gemv_mfma launch on the f32 vector gamma (kernels_mfma.hip) -> g float64
    [rows] (the exact dot product) and what the device's f32 g_r may differ from it by.

    That kernel holds every element of a wave's K range as q = floor(x 2^(29 - E) + 1/2), E the exponent of the range's maximum (:360-365): off by at
    most 2^(E - 30) <= 2^-30 max|gamma|.  Its digit sums are exact integers.  f32 roundings: with 32-block scales every block and digit plane is
    folded by a multiply and an addition (:406-424; 2 per fold, 2 folds per 256-block, at most 5 blocks per wave), then two additions join the digit
    planes and two the lane groups (:475-479), and up to 7 additions the K parts (:512); without scales the digit sums stay integers up to the four
    joining additions.  The count is taken at its largest over every partition the launcher can choose (the binding launch is not the timed one):
        |g_r - g| <= gamma(31) 1.01 sum_k |W_k| (|gamma_k| + 2^-30 max|gamma|) + 2^-30 max|gamma| sum_k |W_k|
    (1.01: the balanced digits' magnitudes sum_d 256^d |d_d| exceed |q| by at most 128 / 127 per plane).  Exactly g where every gamma_k is one of two
    neighbouring powers of two and the block scales are powers of two: q is 2^29 or 2^28, one digit plane, and every sum stays below 2^24 units."""
    if bind_k_split is not None:
        import gemv_mfma_ref  # (imports this module: resolved at call time)

        return gemv_mfma_ref.g_rows(wts, ln_gamma, bind_k_split)
    gm = np.asarray(ln_gamma, np.float32).astype(np.float64)
    g = wts.dot(gm)
    gmax = np.abs(gm).max()
    mant = np.frexp(gm)[0]
    pow2 = np.all(np.abs(mant) == 0.5) and gmax <= 2.0 * np.abs(gm).min()
    sq = 1.0 if wts.scale is None else float(R.quantum(np.abs(wts.scale).reshape(1, -1)).min())
    if pow2 and (wts.scale is None or np.all(np.abs(np.frexp(wts.scale)[0]) == 0.5)) and wts.abs_row_sums(np.abs(gm)).max() / (np.abs(gm).min() * sq) < R.EXACT_UNITS:
        return g, np.zeros(wts.rows)
    bg = R.gamma(G_ROUNDINGS) * 1.01 * wts.abs_row_sums(np.abs(gm) + 2.0 ** -30 * gmax) + 2.0 ** -30 * gmax * wts.abs_row_sums(np.ones(wts.cols))
    return g, bg


def ln_statistics(stats, cols, eps, depth=None):
    """:399-415 -- the statistics pairs [cols / 16, 2] (f64) -> the f32 mean (as float64) and the denominator sqrtf(f32(var) + eps) (as float64).

    The device adds the pairs in f64 in an order of its own (lane-strided, then across the wave); an order can move either sum by 2^-53 per addition
    of the magnitudes.  A vector on which that decides an f32 rounding (of the mean, or of the variance) is no reproducible input: asserted.
    depth: the additions in sequence on the longest path of the summation, where the caller knows it (default: one per pair, any order at all).
    A column whose entries are all multiples of one power of two and sum to less than 2^53 of them in magnitude is added exactly in any order."""
    st = np.asarray(stats, np.float64).reshape(-1, 2)
    inv = 1.0 / cols
    s1, s2 = st[:, 0].sum(), st[:, 1].sum()
    slack = (len(st) if depth is None else depth) * 2.0 ** -53
    e1, e2 = slack * np.abs(st[:, 0]).sum(), slack * np.abs(st[:, 1]).sum()
    if depth is not None:
        q1, q2 = float(R.quantum(st[:, 0].reshape(1, -1)).min()), float(R.quantum(st[:, 1].reshape(1, -1)).min())
        e1 = 0.0 if np.abs(st[:, 0]).sum() / q1 < 2.0 ** 53 else e1
        e2 = 0.0 if np.abs(st[:, 1]).sum() / q2 < 2.0 ** 53 else e2
    mean_d = s1 * inv
    var_d = s2 * inv - mean_d * mean_d
    f32 = lambda v: np.float32(v)
    var_of = lambda a, b: max(b * inv - (a * inv) * (a * inv), 0.0)
    corners = [var_of(s1 + a, s2 + b) for a in (-e1, e1) for b in (-e2, e2)]
    assert f32((s1 - e1) * inv) == f32((s1 + e1) * inv) == f32(mean_d), "mean ambiguous under the summation order"
    assert all(f32(c) == f32(max(var_d, 0.0)) for c in corners), "variance ambiguous under the summation order"
    denom = np.sqrt(f32(max(var_d, 0.0)) + f32(eps), dtype=np.float32)
    return float(f32(mean_d)), float(denom)


def layernorm_after(p, stats, cols, eps, g, bg, fault=None, depth=None):
    """:431, :455-456 -- v = f32(((double)v - mean g_r) r), r = 1 / denom from v_rcp_f64 and two Newton steps (within 2^-51 of 1 / denom).

    The target is (v* - mean g) / denom with v* the exact product and g the exact W . gamma.  The kernel's v is within p.bound of v*, its g_r within
    bg of g; the f64 operations (one product, one subtraction, one product, the reciprocal) stay within 2^-50 of the magnitudes; ONE f32 rounding:
        |error| <= (b_v + |mean| b_g) / denom + 2^-50 (|v| + |mean g|) / denom + u |want| + 2^-126
    With an exact product and an exact g_r that is the once-rounded value up to the f64 operations: the exact inputs are held to this."""
    mean, denom = ln_statistics(stats, cols, eps, depth)
    if fault == "g_row":
        g = np.roll(g, -16)
    v = np.where(p.bound[0] == 0, p.exact32[0].astype(np.float64), p.want[0])
    want = (v - mean * g) / denom
    bound = (p.bound[0] + abs(mean) * bg) / denom + 2.0 ** -50 * (np.abs(v) + np.abs(mean * g)) / denom + U * np.abs(want) + TINY
    return R.Product(want[None, :], bound[None, :], None, None, p.roundings + 1, None)


def silu_mul(p, fault=None):
    """:437-462 -- gemm_ref.silu_mul: the same formula, gv * rcp(1 + __expf(-gv)) * uv, on the same (gate tile, up tile) pairing; its bound takes
    v_exp_f32 and v_rcp_f32 at 1 ulp each (AMD Instinct CDNA4 ISA reference guide, VOP1 opcode descriptions of V_EXP_F32 and V_RCP_F32: "1ULP
    accuracy"; the kernel's own comment at :458 says the same)."""
    if fault == "silu_on_up":
        sw = lambda a: None if a is None else a.reshape(1, -1, 2, 16)[:, :, ::-1].reshape(1, -1)
        p = R.Product(sw(p.want), sw(p.bound), sw(p.exact32), None, p.roundings, None)
    return R.silu_mul(p)


def add_residual(p, res, fault=None):
    """:432 -- gemm_ref.add_residual; after the LayerNorm epilogue there is no exact f32 value to add to, only a bound"""
    res = np.asarray(res, np.float32)
    if fault == "residual_row":
        res = np.roll(res, 1)
    if p.exact32 is None:
        want = p.want + res
        return R.Product(want, p.bound + U * (np.abs(want) + p.bound), None, None, p.roundings + 1, None)
    return R.add_residual(p, res[None, :])


def launch(wts, rec, k_split, ln=None, silu=False, residual=None, fault=None, spread=None):
    """one launch: QAct records -> product -> [LayerNorm: ln = (stats, eps, gamma)] -> [silu * up] -> [residual] -> Product [1, out rows]"""
    d0, d1, as_ = read_qact(rec, wts.cols)
    p = product(wts, d0, d1, as_, k_split, fault, spread)
    if ln is not None:
        stats, eps, ln_gamma = ln
        g, bg = g_rows(wts, ln_gamma)
        p = layernorm_after(p, stats, wts.cols, eps, g, bg, fault)
    if silu:
        p = silu_mul(p, fault)
    if residual is not None:
        p = add_residual(p, residual, fault)
    return p


def target(p):
    """what the output is held to: the f32 value where the bound is 0, the float64 value elsewhere"""
    return np.where(p.bound == 0, p.exact32.astype(np.float64), p.want) if p.exact32 is not None else p.want


# ---------------------------------------------------------------- the merging prologue
def merge_records(scratch, pos, n_heads, n_kv, chunks_max, nr, fault=None):
    """:130-175, :229-288 -- the attention output [n_heads * 128] from the chunk records of launch_attn_decode(.., combine = false), in float64:
        out = sum_c e^(m_c - M) o_c / sum_c e^(m_c - M) l_c over the live records c < (pos + 64) >> 6, M = max m_c
    record (kv head, chunk c) at (kv chunks_max + c) REC_FLOATS floats: (m, l) of group member j at 2 j, o at 8 + 128 j; records past the buffer are
    read from its last one (:138) and are dead.  -> v float64 [cols], delta float64 [cols]: what the kernel's f32 value may differ from v by.

    delta: x_c = m_c - M rounds once (|x_c| u in the exponent); __expf(x) = v_exp_f32(x L), L = f32(log2 e): the product rounds once (|x_c| u more),
    L is 1.3e-8 off log2 e (0.22 |x_c| u), the instruction is good to 1 ulp (2 u) -- expf, which the 8-record instance takes from 5 live records on
    (:236, :266), is no worse: the weights w_c are within e_w = (2.25 max|x_c| + 2) u, relatively.  Numerator and denominator are NR fused
    multiply-adds each (gamma(NR) of sum_c w_c |o_c|, and of L > 0); 1 / L and the product round once each (a division: once):
        |v_f32 - v| <= (2 e_w + 2 gamma(NR) + 3 u) sum_c w_c |o_c| / L + 2^-126
    (a weight below 2^-126 is flushed: at most 2^-126 |o_c| / L with L >= 1 -- the record that holds M has w = 1, l >= 1 -- inside the last term for
    |o| of order 1, and the test's inputs are)."""
    group = n_heads // n_kv
    m_chunks = (pos + 64) >> 6
    if fault == "live_ignored":
        m_chunks -= 1
    elif fault == "dead_included":
        m_chunks += 1
    assert 1 <= m_chunks <= nr
    s = np.asarray(scratch, np.float32).astype(np.float64)
    v, delta = np.zeros(n_heads * 128), np.zeros(n_heads * 128)
    for h in range(n_heads):
        kv, j = h // group, h % group
        recs = [s[(kv * chunks_max + min(c, chunks_max - 1)) * REC_FLOATS:][:REC_FLOATS] for c in range(m_chunks)]
        m = np.array([r[2 * j] for r in recs])
        l_ = np.array([r[2 * j + 1] for r in recs])
        o = np.stack([r[8 + 128 * j: 8 + 128 * (j + 1)] for r in recs])
        x = m - m.max()
        w = np.exp(x)
        big_l = (w * l_).sum()
        v[128 * h: 128 * (h + 1)] = (w[:, None] * o).sum(0) / big_l
        e_w = (2.25 * np.abs(x).max() + 2.0) * U
        delta[128 * h: 128 * (h + 1)] = (2.0 * e_w + 2.0 * R.gamma(nr) + 3.0 * U) * (w[:, None] * np.abs(o)).sum(0) / big_l + TINY
    return v, delta


def quant_interval(v, delta):
    """:289-311, :325-337 (qact_emit's arithmetic) on a value only known to lie within delta of v -> rec (quantize_qact of f32(v): the model's digits)
    and spread float64 [n]: how far the kernel's dequantised element can lie from the model's.

    Per 16-group: if |v| +- delta cannot move the group maximum's exponent, the scale is known and the element is one of the integers
    floor((v -+ delta) 2^(13 - E) + 1/2) .. : spread = the farther end's distance from the model's digit (0 for most elements: delta is a fraction of
    a step).  If it can, the kernel may have taken the neighbouring scale: spread = delta + one step of the coarser scale."""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    rec = quantize_qact(v32)
    n = v32.size
    d0, d1, as_ = read_qact(rec, n) if n % 256 == 0 else (None, None, None)
    assert d0 is not None
    xq = ((256 * d1 + d0) * np.repeat(as_, 16)).reshape(-1, 16)
    vg, dg = np.asarray(v, np.float64).reshape(-1, 16), np.asarray(delta, np.float64).reshape(-1, 16)
    be = lambda a: np.clip(a.astype(np.float32).view(np.uint32) >> 23, 32, 254).astype(np.int64)
    lo, hi = be(np.maximum(np.abs(vg) - dg, 0.0).max(1)), be((np.abs(vg) + dg).max(1))
    step = np.exp2((hi - 127 - 13).astype(np.float64))[:, None]
    q_lo, q_hi = np.floor((vg - dg) / step + 0.5), np.floor((vg + dg) / step + 0.5)
    known = np.maximum(np.abs(q_lo * step - xq), np.abs(q_hi * step - xq))
    spread = np.where((lo == hi)[:, None], known, dg + step)
    return rec, spread.reshape(-1)


# ---------------------------------------------------------------- inputs
def exact_vector(cols, seed, group_scale=None, log2_unit=-9):
    """small integers times ONE power of two, every 16-group holding one +-8192 (so every group takes the same exponent and q = the integer):
    -> u float32 [cols] (what is quantised).  group_scale [cols / 16] of powers of two: x = u / group_scale is returned too (the un-normalised
    vector of a LayerNorm producer whose gamma is group_scale, repeated).  log2_unit: the power of two (21 brings the products with block scales of
    2^-30 back to order 1, where silu is no straight line)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(-8, 9, cols).astype(np.float64)
    pos = np.arange(0, cols, 16) + rng.integers(0, 16, cols // 16)
    n[pos] = 8192.0 * rng.choice(np.array([-1.0, 1.0]), cols // 16)
    u = (n * 2.0 ** log2_unit).astype(np.float32)
    if group_scale is None:
        return u
    return u, (u.astype(np.float64) / np.repeat(group_scale, 16)).astype(np.float32)


def float_vector(cols, seed, kind="mixed"):
    """mixed: the magnitudes of tests/test_batch_ops_gpu.slot_vector (0.01, 1, 30 per column); tiny: the same with a whole 16-group far below the
    format's smallest scale; mean: a large mean (30 +- 1); zero"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(cols, np.float32)
    if kind == "mean":
        return rng.normal(30.0, 1.0, cols).astype(np.float32)
    x = (rng.normal(0.05, 1, cols) * rng.choice([0.01, 1.0, 30.0], cols)).astype(np.float32)
    if kind == "tiny":
        x[32:48] = 1e-30 * rng.choice([-1.0, 1.0], 16)
    return x


def producer(x, ln_gamma=None):
    """what a producing kernel leaves for a consumer: the QAct records of x [* gamma] and, for a LayerNorm consumer, the statistics pairs of x
    (f32 sums over 16 values, stored as f64: csrc/qact.hpp :52-58)"""
    x = np.asarray(x, np.float32)
    rec = quantize_qact(x, ln_gamma)
    xg = x.reshape(-1, 16)
    with np.errstate(over="ignore"):
        st = np.stack([xg.sum(1, dtype=np.float32), (xg * xg).sum(1, dtype=np.float32)], axis=1).astype(np.float64)
    return rec, st


FAULTS = ["part_dropped", "parts_swapped", "clamped_twice", "scale_pair", "plane_weight", "g_row", "silu_on_up", "residual_row", "live_ignored",
          "dead_included"]
