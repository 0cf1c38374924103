"""CPU model (numpy, float64 / int64) of what every form of the many-row matmul carries into its product -- test infrastructure.

bitnet-rs_amd/csrc/kernels_gemm.hip is the specification; the line ranges name what each function restates.

  weights       dense_qk256 / dense_i2s: the dense integer matrix behind the packed 2-bit codes (code j of a row = bits 2 (j % 4) of byte j / 4;
                QK256 map {-2, -1, 1, 2}, I2_S map {0, 1, 0, -1}) and the block scale of every column (row-major [rows, cols / block]); interleave16
                = bitnet_hip_weights_concat(.., interleave16): 16-row tiles a0, b0, a1, b1, ...
  digit forms   quant_rows (k_quant_rows :93-232, k_quant_rows_w :242-358 without its LayerNorm: denom = 1 there): E = biased exponent of the row
                maximum, at least 32; q = rint(x 2^(S - E)), S = 8 NDIG - 3; inverse scale 2^(E - S).  With the LayerNorm prologue (:115-146): f64
                sums, f32 mean and denom, (x - mean) / denom * g in f32.  digits256 (:217-230) / digits32 (:172-197): the balanced digits of q.
  f16 rows      quant_rows_f16 (k_quant_rows_f16 :828-900): f16(x 2^-E), inverse scale 2^E, E clamped to 32 .. 253; rows_to_f16 (k_rows_to_f16
                :1917-1944): f16(x) or f16(x gamma), clamped at +-65504.
  QB32 rows     quant_qb32 (qb32_pack_unit :945-979): per 32-column unit E_u (biased, 24 .. 240), q = rint(v 2^(13 - E_u)), exponent byte E_u - 10.
  products      Product: the exact float64 product of those integers / f16 values with the dense weights, the magnitudes that enter the f32
                roundings, and the number of units the largest partial sum of ANY summation order can reach (`units`: below 2^24 the f32 result is
                the exact one whatever the order).
  bounds        bound_* : per form, a count of f32 roundings x 2^-24 x the magnitudes that enter them (gamma(n) = n u / (1 - n u), Higham's
                constant for n roundings in sequence); the derivations stand at each function.
  epilogues     residual (:443-446, :1141-1144), silu(gate) * up on interleave16 pairs (gsilu_mul :420, store_wave_tiles :469-478,
                f16_chain_epilogue :1113-1135), the f16 hand-over with its clamp (gclamp_f16 :400-403)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24         # unit roundoff of f32
EXACT_UNITS = 2.0 ** 24  # partial sums of fewer units are exact in f32
LOG2E_F32 = float.fromhex("0x1.715476p+0")  # __expf's multiplier
QK256_MAP = np.array([-2, -1, 1, 2], np.int64)
I2S_MAP = np.array([0, 1, 0, -1], np.int64)
KINDS = ("qk256", "i2s256", "i2s32", "i2s32h")


def gamma(n):
    """n f32 roundings in sequence: |error| <= gamma(n) x the magnitudes (first order n u, the denominator carries the higher orders)"""
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------- weights
def unpack_codes(packed, cols):
    """[rows, bytes] -> uint8 [rows, cols]: code j = bits 2 (j % 4) of byte j / 4"""
    p = np.asarray(packed, np.uint8)
    return np.stack([(p >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(p.shape[0], -1)[:, :cols]


def pack_codes(codes):
    c = np.asarray(codes, np.uint8)
    return (c[:, 0::4] | c[:, 1::4] << 2 | c[:, 2::4] << 4 | c[:, 3::4] << 6).astype(np.uint8)


class Matrix:
    """wint int64 [rows, cols]; scale float64 [rows, cols] (the block scale of every column) or None; upload = the arguments of the upload call"""

    def __init__(self, kind, wint, scale, block, upload):
        self.kind, self.wint, self.scale, self.block, self.upload = kind, wint, scale, block, upload
        self.rows, self.cols = wint.shape

    @property
    def dense(self):
        return self.wint.astype(np.float64) if self.scale is None else self.wint * self.scale

    def head(self, rows):
        """the first `rows` rows as a matrix of their own (the row-tail cases: the same codes and scales, fewer rows)"""
        up = dict(self.upload)
        if self.kind == "qk256":
            up["qs"] = self.upload["qs"][:rows]
        else:
            up["packed"], up["scales"] = self.upload["packed"][:rows], self.upload["scales"][:rows]
        return Matrix(self.kind, self.wint[:rows], None if self.scale is None else self.scale[:rows], self.block, up)


def make_matrix(kind, rows, cols, seed, scales="float"):
    """scales: "float" = arbitrary block scales (f16 values for i2s32h), "pow2" = powers of two within a factor of 8 of each other"""
    rng = np.random.default_rng(seed)
    if kind == "qk256":
        stride = -(-cols // 256) * 64
        qs = rng.integers(0, 256, (rows, stride), dtype=np.uint8)
        return Matrix(kind, QK256_MAP[unpack_codes(qs, cols)], None, 0, dict(qs=qs, stride=stride))
    block = 256 if kind == "i2s256" else 32
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(rows, cols), p=[0.5, 0.25, 0.25])
    nb = -(-cols // block)
    if scales == "pow2":
        # i2s32: powers of two that are NO f16 values (2^-30 .. 2^-33) -- a matrix whose 32-block scales all are takes the f16 scale tiles (i2s32h)
        s = np.exp2(-rng.integers(0, 4, (rows, nb)).astype(np.float64) - (30.0 if kind == "i2s32" else 0.0)).astype(np.float32)
    else:
        s = rng.uniform(0.25, 2.0, (rows, nb)).astype(np.float32)
        if kind == "i2s32h":
            s = s.astype(np.float16).astype(np.float32)
    full = np.repeat(s.astype(np.float64), block, axis=1)[:, :cols]
    return Matrix(kind, I2S_MAP[codes], full, block, dict(packed=pack_codes(codes), scales=s, block=block))


def interleave16(a, b):
    """rows of two equal matrices as 16-row tiles a0, b0, a1, b1, ... (any trailing axes)"""
    assert a.shape == b.shape and a.shape[0] % 16 == 0
    t = np.stack([a.reshape(-1, 16, *a.shape[1:]), b.reshape(-1, 16, *b.shape[1:])], axis=1)
    return t.reshape(2 * a.shape[0], *a.shape[1:])


def pair(ma, mb):
    """the (gate, up) handle of weights_concat(.., interleave16=True) as one Matrix (upload = the two parts)"""
    sc = None if ma.scale is None else interleave16(ma.scale, mb.scale)
    return Matrix(ma.kind, interleave16(ma.wint, mb.wint), sc, ma.block, dict(parts=(ma, mb)))


# ---------------------------------------------------------------- row quantisers
def _biased_exponent(am, lo, hi=255):
    return np.clip((np.asarray(am, np.float32).view(np.uint32) >> 23) & 0xFF, lo, hi).astype(np.int64)


def layernorm_rows(x, g, eps):
    """:115-146 -- f64 sums, f32 mean and denom, (x - mean) / denom * g in f32 (each operation rounds once; IEEE division and square root)"""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    cols = x.shape[1]
    mean_d = x64.sum(1) / cols
    s2 = (x64 * x64).sum(1) / cols
    var_d = s2 - mean_d * mean_d
    # the compiler may contract s2 - mean * mean into one fused operation (one rounding instead of two): rows on which the two disagree once
    # converted to f32 are no reproducible input
    fused = np.array([float(Fraction(float(a)) - Fraction(float(b)) ** 2) for a, b in zip(s2, mean_d)]) if x.shape[0] <= 4096 else var_d
    assert np.array_equal(np.maximum(fused, 0.0).astype(np.float32), np.maximum(var_d, 0.0).astype(np.float32)), "variance ambiguous under contraction"
    mean = mean_d.astype(np.float32)
    denom = np.sqrt(np.maximum(var_d, 0.0).astype(np.float32) + np.float32(eps)).astype(np.float32)
    v = (x - mean[:, None]) / denom[:, None] * np.asarray(g, np.float32)[None, :]
    assert v.dtype == np.float32
    return v


def quant_rows(x, ndig, ln=None):
    """-> q int64 [m, K], inv float64 [m] = 2^(E - S)  (:147-158, :220; ln = (gamma, eps))"""
    v = np.asarray(x, np.float32) if ln is None else layernorm_rows(x, *ln)
    S = 8 * ndig - 3
    be = _biased_exponent(np.abs(v).max(axis=1), 32)
    sc = np.exp2((127 + S - be).astype(np.float64)).astype(np.float32)  # (254 + S - be) << 23
    q = np.rint(v * sc[:, None]).astype(np.int64)
    return q, np.exp2((be - S - 127).astype(np.float64))


def digits256(q, ndig):
    """balanced base-256 digits, the top one unbounded: bytes of (q + B) ^ B (:217-221) -> int64 [ndig, m, K]"""
    out, r = [], np.asarray(q, np.int64)
    for _ in range(ndig - 1):
        d = ((r + 128) & 255) - 128
        out.append(d)
        r = (r - d) >> 8
    out.append(r)
    return np.stack(out)


def digits32(q):
    """balanced base-32 digits of the fp6 form: r1 = rint(q / 32), d0 = q - 32 r1, r2 = rint(r1 / 32), d1 = r1 - 32 r2, d2 = r2 (:192-193)"""
    qf = np.asarray(q, np.float64)
    r1 = np.rint(qf / 32.0)
    r2 = np.rint(r1 / 32.0)
    return np.stack([qf - 32.0 * r1, r1 - 32.0 * r2, r2]).astype(np.int64)


def quant_rows_f16(x, ln=None):
    """-> xh float64 [m, K] (f16 values), inv float64 [m] = 2^E  (:880-899)"""
    v = np.asarray(x, np.float32) if ln is None else layernorm_rows(x, *ln)
    be = _biased_exponent(np.abs(v).max(axis=1), 32, 253)
    sc = np.exp2((127 - be).astype(np.float64)).astype(np.float32)
    with np.errstate(over="ignore"):
        xh = (v * sc[:, None]).astype(np.float16)
    return xh.astype(np.float64), np.exp2((be - 127).astype(np.float64))


def rows_to_f16(x, gamma_=None):
    """:1927-1932 -- f16(x) or f16(x * gamma), clamped at +-65504"""
    v = np.asarray(x, np.float32)
    if gamma_ is not None:
        v = v * np.asarray(gamma_, np.float32)[None, :]
    return np.clip(v, -65504.0, 65504.0).astype(np.float16).astype(np.float64)


def quant_qb32(x, gamma_=None):
    """:945-979 -- -> q int64 [m, K], s int64 [m, K / 32] (the exponent bytes); the value of a column is q 2^(s - 130)"""
    v = np.asarray(x, np.float32)
    if gamma_ is not None:
        v = v * np.asarray(gamma_, np.float32)[None, :]
    m, cols = v.shape
    u = v.reshape(m, cols // 32, 32)
    be = _biased_exponent(np.abs(u).max(axis=2), 24, 240)
    sc = np.exp2((140 - be).astype(np.float64)).astype(np.float32)  # (267 - be) << 23 = 2^(13 - E_u)
    q = np.rint(u * sc[:, :, None]).astype(np.int64).reshape(m, cols)
    return q, be - 10


def qb32_values(q, s):
    return q * np.repeat(np.exp2(s.astype(np.float64) - 130.0), 32, axis=1)


def decode_fp6_records(buf, m, cols, rec):
    """the base-32 digit records the fp6 quantisers write (:88-92, :980-989), read back: per token and 256-block `rec` bytes (576 in the fused entry's
    workspace, 592 = + 8 exponent bytes + 8 of padding in a QB32 buffer) of [lane group g 4][digit 3][MFMA m 2][24 bytes = 32 six-bit sign|magnitude
    codes]; k-slot 8 j + n of unit (g, m) is column 64 g + 32 m + 8 j + 4 (n & 1) + (n >> 1).  -> q int64 [m, cols] (cols = the padded width),
    exponent bytes int64 [m, cols / 32] (None for rec = 576).  The same reading as tests/qb32_ref.decode (tests/test_gemm_ref.py holds the two
    against each other), in byte arithmetic instead of single bits: the instance tests read up to 16384 rows."""
    nblk = cols // 256
    r = np.asarray(buf, np.uint8)[: m * nblk * rec].reshape(m, nblk, rec)
    b = r[:, :, :576].reshape(m, nblk, 4, 3, 2, 8, 3).astype(np.int64)
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    code = np.stack([b0 & 63, (b0 >> 6) | ((b1 & 15) << 2), (b1 >> 4) | ((b2 & 3) << 4), b2 >> 2], axis=-1).reshape(m, nblk, 4, 3, 2, 32)
    val = (code & 31) * np.where(code & 32, -1, 1)
    q = val[:, :, :, 0] + 32 * val[:, :, :, 1] + 1024 * val[:, :, :, 2]  # [m, nblk, g, mm, k-slot]
    j = np.arange(32)
    out = np.zeros((m, nblk, 4, 2, 32), np.int64)
    out[..., 8 * (j // 8) + 4 * (j & 1) + ((j % 8) >> 1)] = q
    exps = r[:, :, 576:584].astype(np.int64).reshape(m, nblk * 8) if rec > 576 else None
    return out.reshape(m, cols), exps


def decode_int8_planes(buf, m, kp, ndig):
    """the int8 digit planes [m_pad / 16][NDIG][16][kp] (:49, :212) -> q int64 [m, kp]"""
    mp = -(-m // 16) * 16
    p = np.asarray(buf, np.uint8)[: mp * ndig * kp].view(np.int8).reshape(mp // 16, ndig, 16, kp).astype(np.int64)
    return sum(p[:, d] << (8 * d) for d in range(ndig)).reshape(mp, kp)[:m]


# ---------------------------------------------------------------- exactness
def quantum(a, axis=1):
    """the largest power of two of which every entry along `axis` is an integer multiple (1 for an all-zero line) -> float64, keepdims"""
    a = np.asarray(a, np.float64)
    mant, e = np.frexp(a)
    mi = np.abs(mant * 2.0 ** 53).astype(np.int64)
    low = np.where(mi == 0, 1, mi & -mi).astype(np.float64)
    lsb = np.where(mi == 0, 4096.0, e - 53 + np.log2(low))
    lo = lsb.min(axis=axis, keepdims=True)
    return np.exp2(np.where(lo == 4096.0, 0.0, lo))


def max_units(a_terms, w):
    """a_terms [m, K] >= 0: the magnitudes of a token's terms per column (all multiples of the row's quantum), w [rows, K] the dense weights ->
    [m, rows]: sum_k |a w| in units of quantum(a) quantum(w) -- every product and every partial sum of any order is an integer number of these units
    and no larger than this, so below 2^24 the f32 accumulator holds each of them exactly"""
    ga, gw = quantum(a_terms), quantum(w)
    return (np.abs(a_terms) / ga) @ (np.abs(w) / gw).T


# ---------------------------------------------------------------- products per form
class Product:
    """want float64 [m, rows]: the exact product, scaled; bound float64 [m, rows]: what f32 may differ by (0 where the result is exact);
    exact32 float32 [m, rows] or None: the value the kernel must give where `bound` is 0; units: see max_units"""

    def __init__(self, want, bound, exact32=None, units=None, roundings=0, mag=None):
        self.want, self.bound, self.exact32, self.units, self.roundings, self.mag = want, bound, exact32, units, roundings, mag


def _f32_exact(want):
    with np.errstate(over="ignore"):
        return np.asarray(want, np.float64).astype(np.float32)


def product_int8(q, inv, mat, ndig):
    """k_gemm_mfma (:507-815) on the int8 digit planes.

    unscaled (WS 0): the digit sums D_d = sum_k d_dk w_k are exact int32 (|D_d| <= 128 * 2 * 8192 = 2^21 < 2^24: their conversions are exact too);
      combine_digits (:370-375) adds them up as ((D0 + 256 D1) + (65536 D2 + 2^24 D3)): NDIG - 1 additions, each rounding once (the products by
      256^d are exact, and a contracted multiply-add rounds the same sum once), then x 2^(E - S), exact.
        2 digits: ONE rounding of the exact integer -- exact32 = f32(sum_k q_k w_k) 2^(E - 13), bound 0.
        3, 4 digits: |error| <= gamma(NDIG - 1) sum_d 256^d |D_d| 2^(E - S); 0 where sum_k |q_k w_k| stays below 2^24 units of q's quantum
        (rows that occupy one digit plane: every term of the additions is a multiple of that quantum).
    scaled (WS 1: one fold per 256-block :783-800; WS 2: per 32-block :765-777; WS 3: per 32-block, combine_digits_i + fma_mix :703-714): a fold
      is cv = combine_digits(block sums) (at most NDIG - 1 roundings of magnitudes sum_d 256^d |D_db|; combine_digits_i's single conversion is no
      more), cv * s (one), + the accumulator (one; as a fused multiply-add the two are one); nf folds in sequence, then x 2^(E - S), exact:
        |error| <= gamma(NDIG + nf) sum_b |s_b| sum_d 256^d |D_db| 2^(E - S)
      (recursive summation of nf terms, each carrying NDIG relative roundings of its own).  Where the partial sums of every order stay below 2^24
      units (`units`; power-of-two scales, bounded rows) nothing rounds: bound 0 and exact32 = f32(want)."""
    m, K = q.shape
    W = mat.wint.astype(np.float64)
    dig = digits256(q, ndig).astype(np.float64)
    if mat.scale is None:
        D = np.stack([dig[d] @ W.T for d in range(ndig)])
        A = sum(D[d] * 256.0 ** d for d in range(ndig))
        mag = sum(np.abs(D[d]) * 256.0 ** d for d in range(ndig)) * inv[:, None]
        want = A * inv[:, None]
        # rows on one digit plane: every D_d 256^d is a multiple of q's quantum, and below 2^24 of them nothing rounds (2 digits: exact as they are)
        units = None if ndig == 2 else max_units(np.abs(q).astype(np.float64), W)
        exact = True if ndig == 2 else units < EXACT_UNITS
        return Product(want, np.where(exact, 0.0, gamma(ndig - 1) * mag), _f32_exact(A) * inv[:, None].astype(np.float32), units, ndig - 1, mag)
    nb = -(-K // mat.block)
    want, mag = np.zeros((m, mat.rows)), np.zeros((m, mat.rows))
    for b in range(nb):
        sl = slice(b * mat.block, min(K, (b + 1) * mat.block))
        s = mat.scale[:, sl.start][None, :]
        Db = [dig[d][:, sl] @ W[:, sl].T for d in range(ndig)]
        want += s * sum(Db[d] * 256.0 ** d for d in range(ndig))
        mag += np.abs(s) * sum(np.abs(Db[d]) * 256.0 ** d for d in range(ndig))
    # one fold per block the KERNEL walks: its 256-blocks hold 8 folds of 32 columns (zero padded past K), or one
    nf = -(-K // 256) * (8 if mat.block == 32 else 1)
    units = max_units(np.abs(q).astype(np.float64), mat.dense)
    exact = units < EXACT_UNITS
    want, mag = want * inv[:, None], mag * inv[:, None]
    return Product(want, np.where(exact, 0.0, gamma(ndig + nf) * mag), _f32_exact(want), units, ndig + nf, mag)


def product_fp6(q, inv, mat):
    """k_gemm_fp6 / k_gemm_fp6w (:1569-1772, :1780-1912): the 2-digit integer as three base-32 digits, every product d w 32^i an exact integer, ONE f32
    accumulator over the 3 K terms of a row in an order the matrix core chooses: |error| <= gamma(3 K) sum_k |w_k| (|d0| + 32 |d1| + 1024 |d2|)
    2^(E - 13) -- and exactly f32(sum_k q_k w_k) 2^(E - 13), the int8 form's value, where that sum of magnitudes stays below 2^24 (any order exact)."""
    W = mat.wint.astype(np.float64)
    d = np.abs(digits32(q)).astype(np.float64)
    terms = d[0] + 32.0 * d[1] + 1024.0 * d[2]
    units = terms @ np.abs(W).T
    A = q.astype(np.float64) @ W.T
    n = 3 * q.shape[1]
    return Product(A * inv[:, None], np.where(units < EXACT_UNITS, 0.0, gamma(n) * units * inv[:, None]), _f32_exact(A) * inv[:, None].astype(np.float32),
                   units, n, units * inv[:, None])


def product_f16(xh, inv, mat):
    """k_gemm_f16a / k_gemm_f16h (:1191-1376, :1399-1523) on f16 rows: the A operand is the code value times the block's f16 scale, exact in f16
    (expand8_f16 :920-931); every product of two f16 values is exact in f32 (22 bits); one f32 accumulator takes the K products of a row in an order
    the matrix core chooses: |error| <= gamma(K) sum_k |xh_k W_k|, then x 2^E, exact (inv = 1 on the chain: the epilogue computes
    (acc * 1 - 0 * g) * 1).  Exact where the partial sums of every order stay below 2^24 units."""
    Wd = mat.dense
    want = (xh @ Wd.T) * inv[:, None]
    mag = (np.abs(xh) @ np.abs(Wd).T) * inv[:, None]
    units = max_units(np.abs(xh), Wd)
    n = xh.shape[1]
    return Product(want, np.where(units < EXACT_UNITS, 0.0, gamma(n) * mag), _f32_exact(want), units, n, mag)


def product_qb32(q, s, mat):
    """k_gemm_fp6<.., EPI = 1> (:1683-1744) on QB32 rows: k_gemm_fp6's products with the unit's own power of two in the scale operand (:1730): terms
    d w 32^i 2^(s_u - 130), one f32 accumulator, no row scale: |error| <= gamma(3 K) sum_k |w_k| (|d0| + 32 |d1| + 1024 |d2|) 2^(s_u - 130); exact where
    the partial sums stay below 2^24 units of the row's smallest 2^(s_u - 130)."""
    W = mat.wint.astype(np.float64)
    d = np.abs(digits32(q)).astype(np.float64)
    lsb = np.repeat(np.exp2(s.astype(np.float64) - 130.0), 32, axis=1)
    terms = (d[0] + 32.0 * d[1] + 1024.0 * d[2]) * lsb
    mag = terms @ np.abs(W).T
    units = mag / lsb.min(axis=1, keepdims=True)
    want = (q * lsb) @ W.T
    n = 3 * q.shape[1]
    return Product(want, np.where(units < EXACT_UNITS, 0.0, gamma(n) * mag), _f32_exact(want), units, n, mag)


# ---------------------------------------------------------------- epilogues
def add_residual(p, res):
    """y = v + r in f32, v within p.bound of p.want: |got - (want + r)| <= bound + u (|want + r| + bound); an exact v gives f32(f32(v) + r)"""
    res = np.asarray(res, np.float32)
    want = p.want + res
    exact32 = None if p.exact32 is None else (p.exact32 + res).astype(np.float32)
    grow = np.where(p.bound > 0, p.bound + U * (np.abs(want) + p.bound), 0.0)
    return Product(want, grow, exact32, p.units, p.roundings + 1, p.mag)


def silu_mul(p):
    """rows of an interleave16 pair: 16-row tiles alternate (gate, up) -> [m, rows / 2] of silu(gate) * up, silu(v) = v / (1 + exp(-v)).

    The kernel computes gv * rcp(1 + __expf(-gv)) * uv (gsilu_mul :420), and __expf(a) is v_exp_f32(L * a) with L = f32(log2 e) = 0x1.715476p+0
    (the compiler's HIP math header): restated here as 2^(L a) with that L -- its distance from log2 e, 1.3e-8 relative, moves e^40 by 9 u and is no
    error of the kernel's.  What is left: the product L a rounds once (|L a| u in the argument = |a| u relative in the value), the instruction is
    good to 1 ulp (2 u); 1 + e rounds once; v_rcp_f32 is good to 1 ulp (2 u); two products round once each.  e / (1 + e) < 1, so the exponential's
    error enters the denominator at most in full:
        |error| <= (|g| + 2 + 1 + 2 + 2) u |silu(g) up| = (|g| + 7) u |want|,
    to which the inputs' own bounds add |d silu / dg| <= 1.1 times the gate's and |silu(g)| / |up| times the rest:
        bound = 1.1 b_g |up| + |silu(g)| b_u + (|g| + 7) u |want| + 2^-119 |up| + 2^-126     (first order)
    The last terms: from g < -126 ln 2 = -87.3 on the denominator passes 2^126, its reciprocal is a denormal, which v_rcp_f32 returns as 0 -- and
    so is the kernel's result where |silu(g)| = |g| e^g < 87.4 * 2^-126 < 2^-119; and a product below 2^-126 may be flushed likewise."""
    m, rows = p.want.shape
    t = p.want.reshape(m, rows // 32, 2, 16)
    b = p.bound.reshape(m, rows // 32, 2, 16)
    g, u_, bg, bu = t[:, :, 0], t[:, :, 1], b[:, :, 0], b[:, :, 1]
    if p.exact32 is not None:  # where the products are exact the kernel's inputs are these f32 values
        e = p.exact32.astype(np.float64).reshape(m, rows // 32, 2, 16)
        g, u_ = np.where(bg == 0, e[:, :, 0], g), np.where(bu == 0, e[:, :, 1], u_)
    with np.errstate(over="ignore"):
        sg = g / (1.0 + np.exp2(-g * LOG2E_F32))
    want = sg * u_
    bound = 1.1 * bg * np.abs(u_) + np.abs(sg) * bu + (np.abs(g) + 7.0) * U * np.abs(want) + 2.0 ** -119 * np.abs(u_) + 2.0 ** -126
    out = Product(want.reshape(m, rows // 2), bound.reshape(m, rows // 2), None, None, p.roundings + 7, None)
    out.source = p
    return out


def to_f16(p, gout=None):
    """the f16 hand-over: f16(clamp(v [* gamma_out])) (:400-403, :1152): one f32 product (u) and one f16 rounding (2^-11 relative, 2^-25 absolute
    below the normal range) of a value within `bound` of `want`"""
    want, bound = p.want, p.bound
    if gout is not None:
        g = np.asarray(gout, np.float64)[None, :]
        want, bound = want * g, bound * np.abs(g) + U * np.abs(want * g)
    want = np.clip(want, -65504.0, 65504.0)
    return Product(want, bound + 2.0 ** -11 * (np.abs(want) + bound) + 2.0 ** -25, None, None, p.roundings + 2, None)


# ---------------------------------------------------------------- inputs
def float_rows(m, K, seed):
    """random f32 rows whose magnitudes differ by row, exp(uniform(-3, 3)) per row; one row all zero"""
    rng = np.random.default_rng(seed)
    x = (rng.normal(0.0, 1.0, (m, K)) * np.exp(rng.uniform(-3.0, 3.0, (m, 1)))).astype(np.float32)
    x[m // 3] = 0.0
    return x


def int_rows(m, K, seed, top=1000, peak=8192, every=None):
    """integer-valued rows times one power of two per row: n in -top .. top, and +-peak in one column of every row (every = None) or of every run of
    `every` columns -- the peak fixes the exponent the quantiser takes, so q = n 2^j for a known j and nothing rounds.  One row all zero."""
    rng = np.random.default_rng(seed)
    n = rng.integers(-top, top + 1, (m, K)).astype(np.float64)
    sign = rng.choice(np.array([-1.0, 1.0]), (m, K))
    if every is None:
        n[np.arange(m), rng.integers(0, K, m)] = peak * sign[:, 0]
    else:
        pos = np.arange(0, K, every)[None, :] + rng.integers(0, every, (m, K // every))
        np.put_along_axis(n, pos, peak * np.take_along_axis(sign, pos, 1), axis=1)
    x = n * np.exp2(rng.integers(-6, 7, (m, 1)).astype(np.float64))
    x[m // 3] = 0.0
    return x.astype(np.float32)
