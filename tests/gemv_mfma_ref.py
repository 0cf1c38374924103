"""CPU model (numpy, float64 / int64) of one k_gemv_mfma launch, the library's public GEMV on f32 activations -- test infrastructure.

bitnet-rs_amd/csrc/kernels_mfma.hip is the specification; the line ranges name what each function restates.  Codes, code maps, interleave16,
gamma(n), Product and the residual / silu * up epilogues are tests/gemm_ref.py's; weights (make_weights(.., any_shape=True)), k_ranges, merge_records,
ln_statistics and layernorm_after are tests/gemvq_ref.py's: the kernels share those formulas.

  K ranges    gemvq_ref.k_ranges (:167-169): K part kp covers blocks (kp nblk) >> log2 ks .. ((kp + 1) nblk) >> log2 ks.  The `kpart = 11 - wave`
              remap at 8 parts (:168) changes which WAVE computes a part, not what it holds; the partial sums are stored and added by part
              (:477, :499, :515-518): the model has parts, no waves.
  quantising  quantise (:341-358): per K range, am = the largest |x| of the range (columns at or beyond `cols` are 0: :343-348), be = max(32, biased
              exponent of am), q_k = floor(x_k 2^(156 - be) + 1/2).  digits (:92-104): the four balanced base-256 digits of q, computed from the
              bytes of (q + 0x00808080) ^ 0x00808080 as the kernel does -- the model never goes from q to the sums directly.
  product     product (:371-442, :463-479, :499): digit sums S_d = sum_k w_k d_dk as exact int64 (checked against int32), per fold: the whole K range
              (no scales), a 256-block (wscale, :428-439), a 32-block per k-group (forms 1 and 2, :384-420); folds in K order in f32, then
              (S0 c0 + S1 c1) + (S2 c2 + S3 c3), c_d = 2^(8 d) 2^(be - 156) (:463-469), the four k-group columns of forms 1 and 2 last (:470-473),
              the K parts in order from 0 (:499).
  LayerNorm   layernorm_prologue (LN 1, :292-340): the normalised row in float64 and how far the kernel's f32 row may lie from it;
              LN 2 (:283-291, :444-461, :484-492, :500): x * gamma in f32, then gemvq_ref.layernorm_after with g_rows below.
  epilogues   residual with the row offset of m > 1 (:145, :502), silu(gate) * up on interleave16 pairs (:506-528), QAct out = quantize_qact of the
              kernel's own f32 output (:503, :526; checked for bits by the GPU file), the merge of chunk records (:205-221, :256-281).
  bounds      a count of f32 roundings x 2^-24 x the magnitudes that enter them; the derivations stand at each function.  Nothing here is fitted
              to a device's output."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402
import gemvq_ref as Q  # noqa: E402

U, TINY = R.U, Q.TINY
KINDS = ("qk256", "i2s256", "i2s32", "i2s32h")  # no scales; wscale (f32 per 256-block); scale form 1 (f32 per 32-block); 2 (f16 per 32-block)
SCALE_FORM = {"qk256": 0, "i2s256": 0, "i2s32": 1, "i2s32h": 2}
FOLD = {"qk256": 0, "i2s256": 256, "i2s32": 32, "i2s32h": 32}  # columns per f32 fold (0: the digit sums of a whole K range stay integers)
MIN_EXACT_QUANTUM = 2.0 ** -100  # an "exact" case keeps every term a normal f32 number


# ---------------------------------------------------------------- quantising
def biased_exponent(am):
    return int(np.float32(am).view(np.uint32) >> 23) & 0xFF


def quantise(xs, fault=None):
    """:341-358 -- one K range (float32, already masked) -> be, q int64.

    sc = 2^(156 - be) and |x| < 2^(be - 126): |x sc| < 2^30, no overflow, and the product by a power of two is exact whenever it is a normal number.
    Where it is not (|x sc| < 2^-126: x a denormal, or far below the range maximum) the f32 product may be a denormal or flushed to 0 -- either way
    below 1/2, and floor(. + 1/2) is 0 as for the exact product.  So q = floor(x 2^(156 - be) + 1/2) in exact arithmetic for EVERY finite input
    (float64 holds x 2^(156 - be) + 1/2 exactly: 24 bits below 2^30 plus a half); infinities and NaN are no inputs of the tests (asserted).
    v_cvt_rpi_i32_f32 is taken at its word, floor(x + 1/2) of the real numbers; fault "rpi_in_f32": the sum x + 1/2 rounded to f32 first, which
    sends every odd |x| in [2^23, 2^24) to the even neighbour (rpi_vector is the input that tells the two apart)."""
    xs = np.asarray(xs, np.float32)
    assert np.all(np.isfinite(xs))
    am = float(np.abs(xs).max()) if xs.size else 0.0
    be = max(32, biased_exponent(am))
    t = xs.astype(np.float64) * 2.0 ** (156 - be) + 0.5
    if fault == "rpi_in_f32":
        t = t.astype(np.float32).astype(np.float64)
    q = np.floor(t).astype(np.int64)
    assert np.abs(q).max(initial=0) <= 1 << 30
    return be, q


def digits(q, fault=None):
    """:92-104 -- q int64 -> d int64 [4, n]: bytes of (q + 0x00808080) ^ 0x00808080 as signed bytes.  The addition makes the three low bytes the
    unsigned d_i + 128 (its carries are the adder's), the top byte is d3 as it is; the flip takes the 128 off again.
    fault "carry": neither the addition nor the flip -- the bytes of q read as signed bytes, no carry into the next digit."""
    t = np.asarray(q, np.int64) & 0xFFFFFFFF
    if fault != "carry":
        t = ((t + 0x00808080) & 0xFFFFFFFF) ^ 0x00808080
    b = np.stack([(t >> (8 * i)) & 0xFF for i in range(4)])
    return np.where(b >= 128, b - 256, b)


# ---------------------------------------------------------------- the product
def product_roundings(kind, nblk, k_split):
    """f32 roundings in sequence on the longest path from a digit sum to the output.  The digit sums and their conversions are exact (|S| <= 128 * 2 *
    1280 < 2^24), so are the products by c_d (powers of two).  Per fold a multiplication by the scale and an addition (2; one if contracted; the f16
    form's v_fma_mix is one), folds of the longest K range in sequence (1 per 256-block with wscale, 2 per 256-block and k-group with 32-block
    scales); two additions join the digit columns; two more the k-group columns (32-block scales); the K parts are added to 0 in order
    (k_split - 1: 0 + part is exact)."""
    longest = max(b1 - b0 for b0, b1 in Q.k_ranges(nblk, k_split))
    folds = {0: 0, 256: longest, 32: 2 * longest}[FOLD[kind]]
    return 2 * folds + 2 + (2 if FOLD[kind] == 32 else 0) + (k_split - 1)


def _tail_codes(wts, nblk):
    """the code values of the columns at or beyond `cols` that the tiles hold (qk256 rows keep whole 64-byte blocks)"""
    return R.QK256_MAP[R.unpack_codes(wts.upload["qs"], nblk * 256)].astype(np.int8)[:, wts.cols:]


def product(wts, x, k_split, fault=None, spread=None):
    """k_gemv_mfma's row sums before the epilogue, for the f32 vector x [cols] the waves quantise -> gemm_ref.Product (arrays [1, rows]).

    want = sum over the K parts, in order, of  2^(be - 156) sum_d 256^d sum_folds s_fold S_d,fold  in float64 (every term an integer below 2^19 times
    a 24-bit scale times a power of two: exact; the handful of float64 additions are 2^-29 of the bound's unit).
    |error| <= gamma(n) sum |s_fold| 256^d |S_d,fold| 2^(be - 156) + n 2^-126, n = product_roundings: recursive summation, every term passing through
    at most n roundings, each relative to a partial sum no larger than the sum of the magnitudes (Higham, Accuracy and Stability, 4.2); the last term
    covers results below the normal range.  Where the partial sums of EVERY order stay below 2^24 units of the smallest term's quantum (`units`;
    power-of-two scales, one digit plane) nothing rounds: bound 0, exact32 = f32(want).
    spread [cols] >= 0: the activation is only known to lie within `spread` of x (the LayerNorm prologue, the merge).  The kernel's dequantised
    element then lies within spread_k + one step 2^(be' - 156) of the model's (half a step each, be' the larger exponent the range maximum can take
    within the spread), the output moves by at most sum_k |W_k| of that, and the magnitudes that enter the roundings grow by as much.
    fault: see FAULTS."""
    rows, cols = wts.rows, wts.cols
    nblk = -(-cols // 256)
    kind = wts.kind
    fold = FOLD[kind]
    ranges = Q.k_ranges(nblk, k_split)
    xp = np.zeros(nblk * 256, np.float32)
    xp[:cols] = np.asarray(x, np.float32)
    sp = np.zeros(nblk * 256)
    if spread is not None:
        sp[:cols] = spread
    w_tail = None
    if fault == "tail_unmasked" and cols % 256:  # the clamped last float4 of the row (:176, :225) instead of 0 (:348)
        xp[cols:] = np.tile(xp[cols - 4:cols], (nblk * 256 - cols) // 4)
        w_tail = _tail_codes(wts, nblk)
    scale = wts.scale
    if scale is not None and fault in ("scale_pair", "scale_half") and fold == 32:  # the two 32-blocks of a lane pair (p = 0 / 1, :399-413)
        scale = scale.reshape(rows, -1, 2)[:, :, ::-1].reshape(rows, -1)
    cw = [1.0, 65536.0 if fault == "plane_weight" else 256.0, 65536.0, 16777216.0]
    longest = max(b1 - b0 for b0, b1 in ranges)
    short = [i for i, (b0, b1) in enumerate(ranges) if 0 < b1 - b0 < longest]
    parts, mag = np.zeros((rows, k_split)), np.zeros(rows)
    step = np.zeros(nblk * 256)
    quanta = []
    for kp, (b0, b1) in enumerate(ranges):
        if b1 == b0:
            continue
        idx = np.arange(256 * b0, 256 * b1)
        if fault == "clamped_twice" and short and kp == short[0]:  # the clamped slot (:241) added instead of skipped (:383): the last block once more
            idx = np.concatenate([idx, np.arange(256 * (b1 - 1), 256 * b1)])
        be, q = quantise(xp[idx], fault)
        inv_s = 2.0 ** (be - 156)
        if spread is not None:
            am_hi = np.nextafter(np.float32((np.abs(xp[idx]).astype(np.float64) + sp[idx]).max()), np.float32(np.inf))
            step[idx] = 2.0 ** (max(32, biased_exponent(am_hi)) - 156)
        d = digits(q, fault)
        if fault in ("plane_dropped_0", "plane_dropped_1", "plane_dropped_2", "plane_dropped_3"):
            d[int(fault[-1])] = 0
        elif fault == "planes_swapped":
            d[[1, 2]] = d[[2, 1]]
        n = len(idx)
        f = fold if fold else n
        sfold = None
        if scale is not None:
            sfold = scale[:, idx[::f] // f]
            if fault == "wscale_block" and fold == 256:  # every fold of the range takes the scale of the range's last block (the clamped index, :432)
                sfold = np.repeat(sfold[:, -1:], sfold.shape[1], axis=1)
        inside = idx < cols
        dT = d.reshape(4, n // f, f).transpose(1, 2, 0).astype(np.float64)  # [fold, k, digit]
        for r0 in range(0, rows, 1024):
            w = np.zeros((min(1024, rows - r0), n))
            w[:, inside] = wts.w[r0:r0 + 1024][:, idx[inside]]
            if w_tail is not None:
                w[:, ~inside] = w_tail[r0:r0 + 1024][:, idx[~inside] - cols]
            # the digit sums per fold as integers: every product is an integer of at most 2 * 128, a sum of 1280 of them stays below 2^19 -- a
            # float64 matrix product holds them exactly in any order; kept as int64 from here
            S = np.matmul(w.reshape(-1, n // f, f).transpose(1, 0, 2), dT).transpose(2, 1, 0).astype(np.int64)  # [digit, row, fold]
            assert np.abs(S).max(initial=0) < 1 << 31, "a digit sum leaves int32"
            t, a = S.astype(np.float64), np.abs(S).astype(np.float64)
            if sfold is not None:
                t, a = t * sfold[None, r0:r0 + 1024], a * np.abs(sfold[None, r0:r0 + 1024])
            for dd in range(4):
                parts[r0:r0 + 1024, kp] += t[dd].sum(1) * cw[dd] * inv_s
                mag[r0:r0 + 1024] += a[dd].sum(1) * cw[dd] * inv_s
        low = int(np.bitwise_or.reduce(np.abs(q))) if q.size else 0  # every digit term 256^d d_d is a multiple of q's lowest set bit
        quanta.append(inv_s * float(low & -low if low else 1 << 30))
    if fault == "part_dropped":  # the last K part of the first row tile never reaches the sum
        parts[:16, k_split - 1] = 0.0
    elif fault == "parts_swapped":  # part 0 of two neighbouring tiles: the LDS slot of the wrong tile (:477, :499)
        parts[:16, 0], parts[16:32, 0] = parts[16:32, 0].copy(), parts[:16, 0].copy()
    want = parts.sum(1)
    n_r = product_roundings(kind, nblk, k_split)
    extra = 0.0
    if spread is not None:
        extra = wts.abs_row_sums(sp[:cols] + step[:cols])
    bound = R.gamma(n_r) * (mag + extra) + n_r * TINY + extra
    sq = 1.0 if wts.scale is None else float(R.quantum(np.abs(wts.scale).reshape(1, -1)).min())
    quantum = (min(quanta) if quanta else 1.0) * sq
    units = mag / quantum
    exact = (units < R.EXACT_UNITS) & (spread is None) & (quantum >= MIN_EXACT_QUANTUM)
    return R.Product(want[None, :], np.where(exact, 0.0, bound)[None, :], R._f32_exact(want)[None, :], units[None, :], n_r, mag[None, :])


# ---------------------------------------------------------------- LayerNorm
STAT_DEPTH = 4 * 4 + 6 + 8  # :297-318 -- per thread at most NV = 4 float4s (16 terms in sequence), six steps across the wave, eight waves in sequence


def element_statistics(x):
    """the (x, x^2) pairs the kernel sums in f64 (:297-318, :448-461, :486-492) in gemvq_ref.ln_statistics' form: one pair per element (the products
    of f32 values are exact in f64); that function allows any order of the additions and asserts that none decides an f32 rounding"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    return np.stack([x64, x64 * x64], axis=1)


def layernorm_prologue(x, ln_gamma, eps, fault=None):
    """LN 1 (:292-340) -> v float32 [cols] (the model's normalised row: the float64 LayerNorm with the kernel's f32 mean and denominator, rounded to
    f32 once) and spread float64 [cols]: what the kernel's f32 row may differ from it by.

    The kernel computes ((x - mean) / denom) * gamma in f32: a subtraction, a division (correctly rounded: hipcc's default for HIP) and a product,
    three roundings in sequence on each element; the model's own rounding to f32 is a fourth half-ulp:  |v_kernel - v| <= gamma(4) |v| + 2^-126.
    fault "mean_kept": no mean subtraction."""
    mean, denom = Q.ln_statistics(element_statistics(x), len(x), eps, STAT_DEPTH)
    if fault == "mean_kept":
        mean = 0.0
    v = (np.asarray(x, np.float32).astype(np.float64) - mean) / denom * np.asarray(ln_gamma, np.float32).astype(np.float64)
    return v.astype(np.float32), R.gamma(4) * np.abs(v) + TINY


def g_rows(wts, ln_gamma, bind_k_split):
    """g_r = W[r, :] . gamma as bitnet_hip_weights_bind_ln leaves it: ONE LN 0 launch of this kernel on the f32 vector gamma, at the K split of the
    unpaired launch (bind_k_split: what bitnet_hip_gemv_geometry reports for flags = 0) -> g float64 [rows] (the exact dot product) and bg: what the
    device's f32 g_r may differ from it by = this model's product bound plus the quantisation itself, half a step 2^(be - 156) per element:
        |g_r - g| <= bound(product) + |product.want - g|     (the second term is computed, not bounded: the model knows the digits)
    Exactly g where the product is exact and the quantisation loses nothing (gamma of two neighbouring powers of two)."""
    gm = np.asarray(ln_gamma, np.float32)
    p = product(wts, gm, bind_k_split)
    g = wts.dot(gm.astype(np.float64))
    held = np.where(p.bound[0] == 0, p.exact32[0].astype(np.float64), p.want[0])
    return g, p.bound[0] + np.abs(held - g)


# ---------------------------------------------------------------- one launch
def launch(wts, x, k_split, ln=None, silu=False, residual=None, fault=None, spread=None):
    """one launch on one activation row: x f32 [cols] -> [LayerNorm: ln = (form 1 | 2, gamma, eps, bind_k_split)] -> product -> [LN 2 epilogue] ->
    [silu * up] -> [residual] -> Product [1, out rows]"""
    x = np.asarray(x, np.float32)
    if ln is None:
        p = product(wts, x, k_split, fault, spread)
    elif ln[0] == 1:
        _, ln_gamma, eps, _ = ln
        v, sp = layernorm_prologue(x, ln_gamma, eps, fault)
        p = product(wts, v, k_split, fault, sp)
    else:
        _, ln_gamma, eps, bind_ks = ln
        y = x * np.asarray(ln_gamma, np.float32)  # :286-291, one f32 product per element (IEEE: the model's is the kernel's)
        p = product(wts, y, k_split, fault, spread)
        g, bg = g_rows(wts, ln_gamma, bind_ks)
        if fault == "g_row" and silu:  # :523 reading ln_g of tile t0 for the up tile
            g = g.reshape(-1, 2, 16)
            g = np.stack([g[:, 0], g[:, 0]], axis=1).reshape(-1)
        p = Q.layernorm_after(p, element_statistics(x), wts.cols, eps, g, bg, depth=STAT_DEPTH)
    if silu:
        p = Q.silu_mul(p, fault)
    if residual is not None:
        p = Q.add_residual(p, residual)
    return p


def launch_rows(wts, xs, k_split, residual=None, fault=None, **kw):
    """m > 1 (:143-146): row i of x with row i of the residual -> [Product].  fault "residual_row": row 0's residual for every row"""
    out = []
    for i, x in enumerate(xs):
        res = None if residual is None else residual[0 if fault == "residual_row" else i]
        out.append(launch(wts, x, k_split, residual=res, fault=fault, **kw))
    return out


target = Q.target


def stored_rows(wts, p, fault=None):
    """what the launch leaves in a buffer of 16 ceil(rows / 16) floats that held NaN: the rows of p, NaN beyond them (:498 stores row < rows only).
    fault "surplus_tile_stored": the last tile's rows at or beyond `rows` are written too (finite values)"""
    n = -(-p.want.shape[1] // 16) * 16
    out = np.full(n, np.nan)
    out[: p.want.shape[1]] = target(p)[0]
    if fault == "surplus_tile_stored":
        out[p.want.shape[1]:] = 0.0
    return out


# ---------------------------------------------------------------- the merging prologue
def merged_row(scratch, pos, n_heads, n_kv, chunks_max, fault=None):
    """:205-221, :256-281 -- gemvq_ref.merge_records at 4 records: the f32 row the waves quantise (the float64 merge, rounded once) and its spread.
    fault "dead_record": a record beyond the live count keeps its m (one more record enters the merge); "record_head": the group index and the KV
    head exchanged in the record address (:212-213; on n_kv == group shapes a permutation of the heads)."""
    v, delta = Q.merge_records(scratch, pos, n_heads, n_kv, chunks_max, 4, "dead_included" if fault == "dead_record" else None)
    if fault == "record_head":
        group = n_heads // n_kv
        assert group == n_kv
        v = v.reshape(n_kv, group, 128).transpose(1, 0, 2).reshape(-1)
    return v.astype(np.float32), delta + U * np.abs(v)


# ---------------------------------------------------------------- inputs
PIN = 2.0 ** 29


def plane_vector(cols, plane, seed, log2_unit=-20):
    """the plane-isolating exact vector of digit plane p: every 256-column block holds the pin pair +2^29 u, -2^29 u in its columns 0 and 1 (the
    test gives the two columns the same code in every row, so they cancel in the integer sums), which fixes every K range's exponent at that of
    2^29 u whatever the partition: q = x / u.  Every other element is n 2^(8 p) u with integer |n| <= 127 (63 for p = 3): plane p alone.
    A ragged last block keeps its pins if it has at least 2 columns (cols % 4 == 0: it has)."""
    rng = np.random.default_rng(seed)
    top = 63 if plane == 3 else 127
    n = rng.integers(-top, top + 1, cols).astype(np.float64) * 256.0 ** plane
    n[0::256] = PIN
    n[1::256] = -PIN
    return (n * 2.0 ** log2_unit).astype(np.float32)


def rpi_vector(cols, seed, log2_unit=-20):
    """plane_vector of plane 0 with, in columns 2 and 3 of every 256-block, +(2^23 + 2^16 + a) u and -(2^23 + 2^16 + b) u, a and b odd below 128:
    odd integers between 2^23 and 2^24, where x + 1/2 is no f32 number.  Their digits are (a, 0, -127, 1) and (-b, 0, 127, -1): with one code in
    both columns planes 2 and 3 cancel in the integer sums and plane 0 keeps w (a - b), so the case stays exact -- and a conversion that rounds
    x + 1/2 to f32 first gives w (a - b + 2)."""
    rng = np.random.default_rng(seed)
    x = plane_vector(cols, 0, seed, log2_unit).astype(np.float64) * 2.0 ** -log2_unit
    nb = len(x[2::256])
    x[2::256] = 2.0 ** 23 + 2.0 ** 16 + 2 * rng.integers(0, 64, nb) + 1
    x[3::256] = -(2.0 ** 23 + 2.0 ** 16 + 2 * rng.integers(0, 64, nb) + 1)
    return (x * 2.0 ** log2_unit).astype(np.float32)


def pin_codes(wts):
    """the same code in columns 0 .. 3 of every 256-block, in place (packed bytes and code values): every 2-bit field of byte 0 := bits 0..1"""
    for c in (1, 2, 3):
        wts.w[:, c::256] = wts.w[:, 0::256]
    key = "qs" if "qs" in wts.upload else "packed"
    wts.upload[key][:, 0::64] = (wts.upload[key][:, 0::64] & 3) * 0x55
    return wts


def float_vector(cols, seed, kind, ranges=None):
    """mixed: per-column magnitudes over 2^+-12; range: K ranges whose maxima differ by 2^20 (ranges = [(c0, c1)] in columns); zero_range: one whole
    K range zero; tiny: maxima below 2^-95 (the exponent clamp at 32); edge: the range maxima exactly 2^e and 2^e (2 - 2^-23), |q| reaches 2^30;
    zero; mean: mean 50 x the deviation"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(cols, np.float32)
    if kind == "mean":
        return rng.normal(50.0, 1.0, cols).astype(np.float32)
    x = rng.normal(0.0, 1.0, cols) * np.exp2(rng.uniform(-12.0, 12.0, cols))
    if kind == "tiny":
        x = rng.normal(0.0, 1.0, cols) * 2.0 ** -100
    ranges = ranges or [(0, cols)]
    if kind == "range":
        for i, (c0, c1) in enumerate(ranges):
            x[c0:c1] *= 2.0 ** (-20 * (i % 2))
    if kind == "zero_range":
        c0, c1 = ranges[len(ranges) // 2]
        x[c0:c1] = 0.0
    if kind == "edge":
        x = rng.normal(0.0, 0.25, cols)
        for i, (c0, c1) in enumerate(ranges):
            if c1 > c0:
                x[c0:c1] = np.clip(x[c0:c1], -0.99, 0.99)
                x[c0 + (7 * i) % (c1 - c0)] = (1.0 if i % 2 == 0 else 2.0 - 2.0 ** -23) * (-1.0) ** (i // 2)
    return x.astype(np.float32)


def column_ranges(cols, k_split):
    nblk = -(-cols // 256)
    return [(min(256 * b0, cols), min(256 * b1, cols)) for b0, b1 in Q.k_ranges(nblk, k_split)]


FAULTS = ["plane_dropped_0", "plane_dropped_1", "plane_dropped_2", "plane_dropped_3", "planes_swapped", "plane_weight", "carry", "part_dropped",
          "parts_swapped", "clamped_twice", "tail_unmasked", "surplus_tile_stored", "scale_pair", "scale_half", "wscale_block", "g_row", "mean_kept",
          "silu_on_up", "residual_row", "dead_record", "record_head", "rpi_in_f32"]
