// wave.hpp -- the lane-level helpers under every kernel of this library (gfx950, wave64): vector types, DPP / readlane moves, the wave and
// block reductions, the 2-bit code expansion, v_fma_mix, non-temporal loads, the 1-KiB LDS-DMA.  Device code only; this is their ONLY home.
//
// THE ORDER OF ADDITIONS OF EVERY REDUCTION BELOW IS A CONTRACT: tests pin results to the bit (the f64 LayerNorm statistics of the QAct and
// f16 chains, the final norm that k_logits_f16 and the scoring prologue must round alike).  Variants that differ in order or in instructions
// are separate functions side by side -- never merge two, never reorder one.  Everything is __forceinline__ and compiled under the including
// file's own flags (kernels_exact.hip / kernels_sample.hip: -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bitnet_hip {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// ---- DPP controls: the four steps that reduce a row of 16 lanes (lanes 16 t .. 16 t + 15), and the two that carry rows across the wave ----
constexpr int kDppQuad1 = 0xB1;        // quad_perm [1,0,3,2]: lane ^ 1
constexpr int kDppQuad2 = 0x4E;        // quad_perm [2,3,0,1]: lane ^ 2
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror: lane 7 - l of its half row
constexpr int kDppMirror = 0x140;      // row_mirror: lane 15 - l of its row
constexpr int kDppBcast15 = 0x142;     // row_bcast:15: lane 15 of a row into the next row
constexpr int kDppBcast31 = 0x143;     // row_bcast:31: lane 31 into rows 2 and 3

// ---- lane moves: old = 0 and bound_ctrl, every row and bank enabled ----
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {  // two 32-bit halves
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = dpp_u<CTRL>((unsigned)u), hi = dpp_u<CTRL>((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// ---- reductions inside a row of 16 lanes (qact.hpp: one 16-group per row); every lane of the row gets the result ----
// order: v + lane^1, + lane^2, + half mirror, + mirror
__device__ __forceinline__ float row16_sum_f(float v) {  // four v_add_f32 with a DPP operand
    v += dpp_f<kDppQuad1>(v);
    v += dpp_f<kDppQuad2>(v);
    v += dpp_f<kDppHalfMirror>(v);
    v += dpp_f<kDppMirror>(v);
    return v;
}
// order: as row16_sum_f, in f64
__device__ __forceinline__ double row16_sum_d(double v) {
    v += dpp_d<kDppQuad1>(v);
    v += dpp_d<kDppQuad2>(v);
    v += dpp_d<kDppHalfMirror>(v);
    v += dpp_d<kDppMirror>(v);
    return v;
}
// max |v| over the row, on the bit patterns as unsigned integers (non-negative floats order like them); same four steps, order-free
__device__ __forceinline__ float row16_max_abs(float v) {
    uint32_t u = __float_as_uint(v) & 0x7fffffffu, o;
    o = dpp_u<kDppQuad1>(u), u = o > u ? o : u;
    o = dpp_u<kDppQuad2>(u), u = o > u ? o : u;
    o = dpp_u<kDppHalfMirror>(u), u = o > u ? o : u;
    o = dpp_u<kDppMirror>(u), u = o > u ? o : u;
    return __uint_as_float(u);
}

// ---- wave sums, f64 (the LayerNorm statistics of the activation chains) ----
// order: row16_sum_d inside each row, then readlane of lanes 0 / 16 / 32 / 48: (r0 + r1) + (r2 + r3)            [k_gemv_mfma, k_gemv_q]
__device__ __forceinline__ double wave64_sum_d_rows_readlane(double v) {
    v = row16_sum_d(v);
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 16 * i);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 16 * i);
        r[i] = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
    }
    return (r[0] + r[1]) + (r[2] + r[3]);
}
// own + partner row through v_permlane16_swap (rows32 = false) / v_permlane32_swap: with both operands the same register the swap leaves
// (own, partner) in some order in its two results, and their sum is what is wanted
__device__ __forceinline__ double permlane_swap_sum_d(double v, bool rows32) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t l = (uint32_t)u, h = (uint32_t)(u >> 32);
    const auto a = rows32 ? __builtin_amdgcn_permlane32_swap(l, l, false, false) : __builtin_amdgcn_permlane16_swap(l, l, false, false);
    const auto b = rows32 ? __builtin_amdgcn_permlane32_swap(h, h, false, false) : __builtin_amdgcn_permlane16_swap(h, h, false, false);
    return __builtin_bit_cast(double, ((uint64_t)b[0] << 32) | a[0]) + __builtin_bit_cast(double, ((uint64_t)b[1] << 32) | a[1]);
}
// order: row16_sum_d inside each row, then the row pairs (r0, r1), (r2, r3) by permlane16 swap, then the two halves by permlane32 swap -- all
// on the VALU, no ds_bpermute round trips; every lane ends with the same value                                          [k_quant_rows_w]
__device__ __forceinline__ double wave64_sum_d_rows_permlane(double v) {
    v = row16_sum_d(v);
    v = permlane_swap_sum_d(v, false);
    return permlane_swap_sum_d(v, true);
}
// order: xor butterfly 32, 16, 8, 4, 2, 1 over ds_bpermute                                                               [k_quant_rows]
__device__ __forceinline__ double wave64_sum_d_xor(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- wave sums and maxima, f32 ----
// order: xor butterfly 32, 16, 8, 4, 2, 1                                  [k_norm_rows, k_logits_f16, the scoring prologue, k_gemv_valu]
__device__ __forceinline__ float wave64_sum_f_xor(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// fmaxf over the same butterfly
__device__ __forceinline__ float wave64_max_f_xor(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// order: row16_sum_f inside each row, then readlane of lanes 0 / 16 / 32 / 48: (r0 + r1) + (r2 + r3)                    [decode attention]
__device__ __forceinline__ float wave64_sum_f_rows_readlane(float v) {
    v = row16_sum_f(v);
    return (readlane_f(v, 0) + readlane_f(v, 16)) + (readlane_f(v, 32) + readlane_f(v, 48));
}
// fmaxf over the four row steps, then over the same four readlanes                                                    [decode attention]
__device__ __forceinline__ float wave64_max_f_rows_readlane(float v) {
    v = fmaxf(v, dpp_f<kDppQuad1>(v));
    v = fmaxf(v, dpp_f<kDppQuad2>(v));
    v = fmaxf(v, dpp_f<kDppHalfMirror>(v));
    v = fmaxf(v, dpp_f<kDppMirror>(v));
    return fmaxf(fmaxf(readlane_f(v, 0), readlane_f(v, 16)), fmaxf(readlane_f(v, 32), readlane_f(v, 48)));
}
// fmaxf over the four row steps, then xor 16 and xor 32 over ds_bpermute; every lane gets the result                       [k_quant_rows]
__device__ __forceinline__ float wave64_max_f_rows_xor(float v) {
    v = fmaxf(v, dpp_f<kDppQuad1>(v));
    v = fmaxf(v, dpp_f<kDppQuad2>(v));
    v = fmaxf(v, dpp_f<kDppHalfMirror>(v));
    v = fmaxf(v, dpp_f<kDppMirror>(v));
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}
// maximum of a NON-NEGATIVE float: on the bit patterns as unsigned integers (same order, no NaN canonicalisation instructions), the four row
// steps with the lane's own value as `old`, row_bcast 15 / 31 across the rows, read from lane 63                          [k_gemv_mfma]
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_u(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
    return o > v ? o : v;
}
__device__ __forceinline__ float wave64_max_bits_rows_bcast(float v) {
    uint32_t u = __float_as_uint(v);
    u = dpp_max_u<kDppQuad1, 0xf>(u);
    u = dpp_max_u<kDppQuad2, 0xf>(u);
    u = dpp_max_u<kDppHalfMirror, 0xf>(u);
    u = dpp_max_u<kDppMirror, 0xf>(u);
    u = dpp_max_u<kDppBcast15, 0xa>(u);  // into rows 1 and 3
    u = dpp_max_u<kDppBcast31, 0xc>(u);  // into rows 2 and 3
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)u, 63));
}

// ---- 256-thread block reductions through four floats of LDS (`slot`); every thread of the block must call them ----
// order: wave64_sum_f_xor in each wave, then (w0 + w1) + (w2 + w3).  The final norm of k_logits_f16 and the scoring prologue
// (k_score_rows_f16) must round alike: both call THIS function.
__device__ __forceinline__ float block256_sum_f(float v, float *slot) {
    v = wave64_sum_f_xor(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}
__device__ __forceinline__ float block256_max_f(float v, float *slot) {
    v = wave64_max_f_xor(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
}

// ---- 2-bit codes, f16 halves ----
// One dword = 16 codes (already field-transposed, k_retile) -> the A operand of one int8 MFMA: register i, byte b <- LUT[code of element 4 i + b]
__device__ __forceinline__ v4i decode16(uint32_t w, uint32_t lut) {
    v4i a;
    a[0] = (int)__builtin_amdgcn_perm(0u, lut, w & 0x03030303u);
    a[1] = (int)__builtin_amdgcn_perm(0u, lut, (w >> 2) & 0x03030303u);
    a[2] = (int)__builtin_amdgcn_perm(0u, lut, (w >> 4) & 0x03030303u);
    a[3] = (int)__builtin_amdgcn_perm(0u, lut, (w >> 6) & 0x03030303u);
    return a;
}
// a * f16(h[15:0]) + c  /  a * f16(h[31:16]) + c in f32, no conversion instruction
__device__ __forceinline__ float fma_mix_lo(float a, uint32_t h, float c) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(h), "v"(c));
    return r;
}
__device__ __forceinline__ float fma_mix_hi(float a, uint32_t h, float c) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(h), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pack_h2(float lo, float hi) {
    const _Float16 a = (_Float16)lo, b = (_Float16)hi;
    return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
}
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int cvt_rpi(float x) {  // to the nearest integer in ONE instruction: floor(x + 0.5), ties go up (|error| <= 0.5 either way)
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// ---- memory ----
// Weight bytes are read ONCE per launch by ONE CU: non-temporal loads keep them from displacing the activation vectors in L2 / Infinity
// Cache and land sooner (MI355X_MICROARCH.md, nt-weights).
__device__ __forceinline__ v4u load_nt16v(const void *p) { return __builtin_nontemporal_load(reinterpret_cast<const v4u *>(p)); }
__device__ __forceinline__ uint4 load_nt16(const void *p) {
    const v4u v = load_nt16v(p);
    return uint4{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ float4 load_nt16f(const float *p) {
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
    return float4{v[0], v[1], v[2], v[3]};
}
// LDS-DMA: 64 lanes x 16 B from (scalar base + per-lane byte offset) to LDS bytes [lds_dst, lds_dst + 1024), no VGPR staging.  The LDS address
// travels in m0, which hipcc also uses (LDS instructions, readlane indices): it is saved and restored inside the one asm block, with the s_nop
// the m0 write needs ahead of the load.  INVISIBLE TO hipcc's vmcnt BOOKKEEPING (cdna_hip_programming.md 5.7): the calling kernel waits for its
// pieces with an explicit s_waitcnt vmcnt(n) ahead of the barrier that publishes the tile; a counted wait (n > 0) is right only while no
// compiler-emitted vector-memory instruction sits between the DMA and the wait (tests/test_isa_guard.py re-checks that from the ISA);
// hipcc's own waits for the loads it does track only ever over-wait (loads return in order).
__device__ __forceinline__ void lds_dma_1k(unsigned lane_off, const void *sbase, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_off), "s"(sbase), "s"(lds_dst)
                 : "memory");
}

}  // namespace bitnet_hip
