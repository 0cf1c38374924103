// kernels_head.hip -- the SCREENED greedy head (gfx950): the token k_logits_f16 + k_argmax_final (kernels_decode.hip) would pick, bit for
// bit, from about half their bytes.  A greedy step needs the index of the largest logit, not 128256 logits:
//
//   k_head_screen_build  once per table: every row E_v as int8 codes q_v with one f32 scale s_v = max|E_v| / 127, and one f32 coefficient
//                        c_v that bounds how far s_v * (q_v . y) can lie from the logit the full head computes, per unit of |y|_2
//   k_head_screen        per token: streams the int8 image only; per row ub_v = a_v + c_v * r, per workgroup the maximum of
//                        lb_v = a_v - c_v * r, with a_v = s_v * sum_k q_vk y_k, y = LN(x) * gamma (head_final_norm: the full head's bits)
//                        and r >= |y|_2
//   k_head_rescore       L = max lb; every row for which ub_v < L is NOT provably true is computed from the f16 table with the full head's
//                        own row arithmetic (head.hpp); per-workgroup (best value, lowest index) partials for the unchanged k_argmax_final
//
// ---- the bound (Cauchy-Schwarz plus counted roundings; u = 2^-24, H = hidden, d = H / 64 + 6) ----------------------------------------
// Let y be the f32 activations both heads hold in registers, T = sum_k y_k E_vk in exact arithmetic, F the f32 logit of the full head.
//  (1) F sums the 64 lane chains of H / 64 fused multiply-adds and a 6-step butterfly: every term passes through at most d roundings, so
//      |F - T| <= g(d) sum_k |y_k E_vk| <= g(d) |y| |E_v|, g(n) = n u / (1 - n u)                      [Higham, Accuracy and Stability, 4.2]
//      (were the multiply-add not fused, d + 1: covered by the constant below).
//  (2) With rho_v = |E_v - s_v q_v|_2 and D = sum_k q_vk y_k exact:  |T - s_v D| = |sum_k y_k (E_vk - s_v q_vk)| <= |y| rho_v.
//  (3) The screen computes D^ on the same lane map and butterfly (int8 -> f32 is exact): |D^ - D| <= g(d) |q_v| |y|, and a_v = fl(s_v D^),
//      |a_v - s_v D^| <= u s_v |D^| <= u (1 + g(d)) s_v |q_v| |y|.  s_v |q_v| <= |E_v| + rho_v.
//  Sum:  |F - a_v| <= |y| [ rho_v (1 + e1) + e2 |E_v| ],  e1 = g(d) + u (1 + g(d)) < 2^-10,  e2 = 2 g(d) + u (1 + g(d)) < (2 d + 4) u.
//  Underflow: a rounding in the subnormal range adds at most 2^-126 (flushed or gradual); at most 2 H <= 2^14 of them: < 2^-100 in all.
//  Overflow: |E_vk| < 2^16 and H <= 2^13, so no partial sum exceeds 2^22.5 |y|: none while |y| <= 2^60.  Beyond that (or |y| not finite)
//  the screen uses r = +inf: every ub is +inf or NaN, every lb -inf or NaN, every row is kept.
// The builder stores  c_v = ((1 + 2^-10)^2 rho^ + K u (1 + 2^-10) E^ + 2^-55) (1 + 2^-20),  K = 2 d + 4 = H / 32 + 16,  where rho^, E^ are
// the f32 square roots of f32 sums of squares over the same lane map (<= d + 3 roundings per term: relative error < 2^-17, so one factor
// 1 + 2^-10 makes each an upper bound); squares below 2^-126 may vanish from the sum: their roots total < sqrt(H) 2^-63 < 2^-55.  A row with
// a non-finite entry gets codes 0, scale 0 and c_v = +inf: kept whatever y is.  The trailing 1 + 2^-20 covers the three roundings of the
// expression itself.
// The screen takes  r = sqrt(sum y_k^2) (1 + 2^-10) + 2^-55  (same argument), w = fl(c_v r) (1 + 2^-20) + 2^-100 >= c_v |y| + 2^-100, and
// rounds outwards once more:  ub = t + 2^-22 |t|, t = fl(a_v + w);  lb = t' - 2^-22 |t'|, t' = fl(a_v - w).  Hence lb_v <= F_v <= ub_v for
// every row whose F_v is a number; a row whose F_v is NaN has a non-finite entry or a non-finite y, and is kept.
// A row with ub_v < L has F_v <= ub_v < L <= F_w for the row w that set L: it cannot be the maximum nor tie with it.  Every other row is
// computed exactly as the full head computes it, so the pick -- largest value, lowest index on ties, NaN as -inf -- is the full head's.
#include "common.hpp"
#include "head.hpp"
#include "wave.hpp"

namespace bitnet_hip {

// ---- the image: for the row pair p = v / 2, chunk c (512 columns), lane l: 16 bytes at ((p * H / 512 + c) * 64 + l) * 16 -- codes of row 2 p,
// columns 512 c + 8 l + [0, 8), then the same columns of row 2 p + 1: one 16-byte load per lane feeds two rows on the full head's lane ->
// element map, one wave load is 1 KiB of consecutive bytes.  After the codes, per row, the pair (s_v, c_v).  An odd vocabulary is padded by a
// zero row that no kernel reports. ----
__host__ __device__ static size_t screen_pairs(size_t vocab) { return (vocab + 1) / 2; }
static bool head_screen_supported(int hidden) {
    const int n = hidden / 512;
    return hidden > 0 && hidden % 512 == 0 && (n == 1 || n == 2 || n == 4 || n == 5 || n == 8);
}
size_t head_screen_bytes(size_t hidden, size_t vocab) {
    if (!head_screen_supported((int)hidden) || vocab == 0 || vocab > 0x7fffffffu) return 0;
    return screen_pairs(vocab) * 2 * hidden + screen_pairs(vocab) * 2 * sizeof(float2);
}

// one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void k_head_screen_build(const _Float16 *__restrict__ table, int hidden, int vocab, uint8_t *__restrict__ image,
                                                           float2 *__restrict__ rowdata) {
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nch = hidden >> 9, rows = 2 * (int)screen_pairs((size_t)vocab);
    if (v >= rows) return;
    const bool pad = v >= vocab;
    const _Float16 *e = table + (size_t)(pad ? 0 : v) * hidden + 8 * lane;
    uint8_t *out = image + ((size_t)(v >> 1) * nch * 64 + lane) * 16 + (v & 1) * 8;
    float mx = 0.0f;
    bool bad = false;
    for (int c = 0; c < nch; ++c) {
        const h8 w = *reinterpret_cast<const h8 *>(e + 512 * c);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float a = pad ? 0.0f : fabsf((float)w[i]);
            bad |= !(a <= 65504.0f);
            mx = fmaxf(mx, a);
        }
    }
    bad = __ballot(bad) != 0;
    mx = wave64_max_f_xor(mx);
    const float s = bad ? 0.0f : mx / 127.0f;
    float r2 = 0.0f, e2 = 0.0f;
    for (int c = 0; c < nch; ++c) {
        const h8 w = *reinterpret_cast<const h8 *>(e + 512 * c);
        uint32_t pk[2] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float a = (pad || bad) ? 0.0f : (float)w[i];
            const float q = s > 0.0f ? fminf(fmaxf(rintf(a / s), -127.0f), 127.0f) : 0.0f;
            const float r = fmaf(-s, q, a);
            r2 = fmaf(r, r, r2);
            e2 = fmaf(a, a, e2);
            pk[i >> 2] |= ((uint32_t)(int)q & 0xffu) << (8 * (i & 3));
        }
        *reinterpret_cast<uint2 *>(out + (size_t)c * 64 * 16) = make_uint2(pk[0], pk[1]);
    }
    r2 = wave64_sum_f_xor(r2);
    e2 = wave64_sum_f_xor(e2);
    if (lane == 0) {
        const float up = 1.0f + 0x1p-10f;
        const float rho = sqrtf(r2) * up, ne = sqrtf(e2) * up;
        const float K = (float)(hidden / 32 + 16);
        const float c = (rho * up + K * 0x1p-24f * ne + 0x1p-55f) * (1.0f + 0x1p-20f);
        rowdata[v] = make_float2(s, bad ? INFINITY : c);
    }
}

hipError_t launch_head_screen_build(const void *table, int hidden, int vocab, void *image, hipStream_t stream) {
    if (!head_screen_bytes((size_t)hidden, (size_t)vocab)) return hipErrorInvalidValue;
    const size_t pairs = screen_pairs((size_t)vocab);
    float2 *rowdata = reinterpret_cast<float2 *>(static_cast<uint8_t *>(image) + pairs * 2 * (size_t)hidden);
    hipLaunchKernelGGL(k_head_screen_build, dim3((unsigned)((2 * pairs + 3) / 4)), dim3(256), 0, stream, static_cast<const _Float16 *>(table), hidden, vocab,
                       static_cast<uint8_t *>(image), rowdata);
    return hipGetLastError();
}

// ---- the workspace the two kernels share (floats; HeadScreenWs in common.hpp): [0, vocab) ub | lb maxima, one per screening workgroup | the raw
// head input x [hidden] | four counter words: rows kept by the last launch, launches, rows kept by all launches, unused | [vocab] the rescored logits of the kept rows (other entries untouched) ----
HeadScreenWs head_screen_ws(float *ws, size_t hidden, size_t vocab, size_t n_wg) {
    HeadScreenWs w;
    const size_t v4 = (vocab + 3) / 4 * 4, n4 = (n_wg + 3) / 4 * 4;
    w.ub = ws, w.lb_max = ws + v4, w.x = w.lb_max + n4, w.count = reinterpret_cast<unsigned *>(w.x + hidden), w.rescored = w.x + hidden + 4;
    w.floats = v4 + n4 + hidden + 4 + v4;
    return w;
}

// (float)(int8) of byte B of a dword in ONE instruction (SDWA byte select with sign extension): with the multiply-add, two VALU
// instructions per weight.  Left to the compiler the same conversion is a shift, a bit-field extract and a convert.
template <int B>
__device__ __forceinline__ float cvt_i8(uint32_t w) {
    float r;
    if constexpr (B == 0) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0" : "=v"(r) : "v"(w));
    if constexpr (B == 1) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1" : "=v"(r) : "v"(w));
    if constexpr (B == 2) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2" : "=v"(r) : "v"(w));
    if constexpr (B == 3) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3" : "=v"(r) : "v"(w));
    return r;
}
// four weights of one dword into a row's chain, in element order
__device__ __forceinline__ void screen_dword(const float *xr4, uint32_t w, float &acc) {
    acc += xr4[0] * cvt_i8<0>(w);
    acc += xr4[1] * cvt_i8<1>(w);
    acc += xr4[2] * cvt_i8<2>(w);
    acc += xr4[3] * cvt_i8<3>(w);
}

// a lane's two partials of one row pair from one 16-byte load per chunk: the full head's chunk / element order, one chain per row
template <int NCH>
__device__ __forceinline__ void screen_lane_dot(const float (&xr)[NCH][8], const v4u (&w)[NCH], float &a0, float &a1) {
    a0 = a1 = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            screen_dword(&xr[c][4 * h], w[c][h], a0);
            screen_dword(&xr[c][4 * h], w[c][2 + h], a1);
        }
}

// RP row pairs per wave iteration: RP * 2 * hidden bytes in flight per wave (what k_logits_f16 keeps: R * hidden * 2)
template <int NCH, int RP>
__global__ __launch_bounds__(256) void k_head_screen(const uint8_t *__restrict__ image, const float2 *__restrict__ rowdata, const float *__restrict__ x,
                                                     const float *__restrict__ gamma, float eps, int hidden, int vocab, float *__restrict__ ub,
                                                     float *__restrict__ lb_max, float *__restrict__ x_copy, unsigned *__restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [hidden] normalised activations
    __shared__ float slot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0) {
        for (int i = tid; i < hidden; i += 256) x_copy[i] = x[i];
        if (tid == 0) count[0] = 0u, count[1] += 1u;  // rows kept by this launch; launches
    }
    head_final_norm(x, gamma, eps, hidden, xs, slot);
    float ss = 0.0f;
    for (int i = tid; i < hidden; i += 256) ss = fmaf(xs[i], xs[i], ss);
    const float nrm = sqrtf(block256_sum_f(ss, slot)) * (1.0f + 0x1p-10f) + 0x1p-55f;
    const float r = nrm <= 0x1p60f ? nrm : INFINITY;  // NaN, +inf or beyond the overflow-free range: keep every row
    float xr[NCH][8];
    head_lane_x<NCH, false>(xs, NCH, lane, xr);
    float lbm = -INFINITY;
    const int pairs = (vocab + 1) >> 1, total_waves = gridDim.x * 4;
    for (int p = (blockIdx.x * 4 + wave) * RP; p < pairs; p += total_waves * RP) {
        v4u w[RP][NCH];
#pragma unroll
        for (int j = 0; j < RP; ++j) {
            // pairs past the end re-read the last pair (never stored)
            const uint8_t *e = image + ((size_t)(p + j < pairs ? p + j : pairs - 1) * NCH * 64 + lane) * 16;
#pragma unroll
            for (int c = 0; c < NCH; ++c) w[j][c] = load_nt16v(e + (size_t)c * 64 * 16);
        }
        const int row = 2 * p + lane;  // lane j < 2 RP finishes row 2 p + j
        float2 sc = make_float2(0.0f, 0.0f);
        if (lane < 2 * RP && row < vocab) sc = rowdata[row];
        float acc[2 * RP];
#pragma unroll
        for (int j = 0; j < RP; ++j) screen_lane_dot<NCH>(xr, w[j], acc[2 * j], acc[2 * j + 1]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int j = 0; j < 2 * RP; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
        float d = acc[0];
#pragma unroll
        for (int j = 1; j < 2 * RP; ++j) d = lane == j ? acc[j] : d;
        if (lane < 2 * RP && row < vocab) {
            const float a = sc.x * d;
            const float wd = sc.y * r * (1.0f + 0x1p-20f) + 0x1p-100f;
            const float t = a + wd, t2 = a - wd;
            ub[row] = fmaf(fabsf(t), 0x1p-22f, t);
            const float lb = fmaf(fabsf(t2), -0x1p-22f, t2);
            if (lb > lbm) lbm = lb;  // a NaN never enters
        }
    }
    lbm = block256_max_f(lbm, slot);
    if (tid == 0) lb_max[blockIdx.x] = lbm;
}

// The rows the screen could not exclude, from the f16 table with the full head's row arithmetic; partials for k_argmax_final.
template <int NCH>
__global__ __launch_bounds__(256) void k_head_rescore(const _Float16 *__restrict__ table, const float *__restrict__ x, const float *__restrict__ gamma,
                                                      float eps, int hidden, int vocab, const float *__restrict__ ub, const float *__restrict__ lb_max,
                                                      int n_lb, float *__restrict__ rescored, unsigned *__restrict__ count,
                                                      float *__restrict__ best_val, int *__restrict__ best_idx) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ float slot[4];
    __shared__ float wbv[4];
    __shared__ int wbi[4];
    __shared__ unsigned wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    head_final_norm(x, gamma, eps, hidden, xs, slot);
    float xr[NCH][8];
    head_lane_x<NCH, false>(xs, NCH, lane, xr);
    float m = -INFINITY;
    for (int i = tid; i < n_lb; i += 256) {
        const float v = lb_max[i];
        if (v > m) m = v;
    }
    const float L = block256_max_f(m, slot);
    const int per_wg = (vocab + (int)gridDim.x - 1) / (int)gridDim.x;
    const int begin = (int)blockIdx.x * per_wg, end = begin + per_wg < vocab ? begin + per_wg : vocab;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    unsigned kept = 0;
    for (int base = begin + 64 * wave; base < end; base += 256) {
        const int row = base + lane;
        // keep unless ub < L is PROVEN: a NaN on either side keeps the row
        unsigned long long mask = __ballot(row < end && !(ub[row < end ? row : begin] < L));
        kept += (unsigned)__popcll(mask);
        while (mask) {
            const int rr = base + (int)__builtin_ctzll(mask);
            mask &= mask - 1;
            h8 w[NCH];
            head_lane_row<NCH, false>(table + (size_t)rr * hidden + 8 * lane, NCH, w);
            const float acc = wave64_sum_f_xor(head_lane_dot<NCH>(xr, w));
            if (lane == 0) {
                rescored[rr] = acc;
                const float v = acc != acc ? -INFINITY : acc;  // NaN -> -inf (sampling.rs:45-49)
                if (v > bv || (v == bv && rr < bi)) {
                    bv = v;
                    bi = rr;
                }
            }
        }
    }
    if (lane == 0) {
        wbv[wave] = bv;
        wbi[wave] = bi;
        wcnt[wave] = kept;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w2 = 1; w2 < 4; ++w2)
            if (wbv[w2] > bv || (wbv[w2] == bv && wbi[w2] < bi)) {
                bv = wbv[w2];
                bi = wbi[w2];
            }
        best_val[blockIdx.x] = bv;
        best_idx[blockIdx.x] = bi;
        const unsigned n = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (n) atomicAdd(count, n), atomicAdd(count + 2, n);  // this launch; all launches
    }
}

int head_rescore_wgs(int n_wg) { return n_wg < 128 ? n_wg : 128; }

hipError_t launch_head_screen(const void *table, const float *x, const float *gamma, float eps, int hidden, int vocab, const void *image, float *ws,
                              float *best_val, int *best_idx, int n_wg, hipStream_t stream) {
    if (!head_screen_bytes((size_t)hidden, (size_t)vocab)) return hipErrorInvalidValue;
    const HeadScreenWs w = head_screen_ws(ws, (size_t)hidden, (size_t)vocab, (size_t)n_wg);
    const uint8_t *img = static_cast<const uint8_t *>(image);
    const float2 *rowdata = reinterpret_cast<const float2 *>(img + screen_pairs((size_t)vocab) * 2 * (size_t)hidden);
    const int n_r = head_rescore_wgs(n_wg);
    const size_t lds = (size_t)hidden * sizeof(float);
#define BH_HPICK(NCHv, RPv)                                                                                                                      \
    if (hidden == 512 * NCHv) {                                                                                                                  \
        hipLaunchKernelGGL((k_head_screen<NCHv, RPv>), dim3(n_wg), dim3(256), lds, stream, img, rowdata, x, gamma, eps, hidden, vocab, w.ub,      \
                           w.lb_max, w.x, w.count);                                                                                              \
        hipLaunchKernelGGL((k_head_rescore<NCHv>), dim3(n_r), dim3(256), lds, stream, static_cast<const _Float16 *>(table), x, gamma, eps, hidden, \
                           vocab, w.ub, w.lb_max, n_wg, w.rescored, w.count, best_val, best_idx);                                                \
    }
    BH_HPICK(1, 4) BH_HPICK(2, 4) BH_HPICK(4, 4) BH_HPICK(5, 3) BH_HPICK(8, 2)
#undef BH_HPICK
    return hipGetLastError();
}

}  // namespace bitnet_hip
