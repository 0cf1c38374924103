// qact.hpp -- "QAct": an activation vector quantised ONCE by the kernel that produces it, in the form the
// streaming I2_S GEMV (kernels_gemvq.hip) feeds straight to the matrix cores.
//
// north_star asks for "2-bit weight unpack x f16 activation dot product".  QAct is the f16-class activation of
// this library: per 16 consecutive elements one power-of-two scale and a 15-bit fixed-point value per element,
//     x_k  ~=  as[k / 16] * (256 * d1[k] + d0[k]),      d0, d1 int8 (balanced base-256 digits),
//     as = 2^(E - 13), E = exponent of the group's absolute maximum  =>  |256 d1 + d0| <= 2^14,
// i.e. every element is held to 2^-15 of its 16-group's maximum (f16 holds 2^-12 of the ELEMENT; for the dot
// products of this path the group-relative bound is what matters, and it is ~8x tighter than an f16 row with one
// shared scale would be).  The digits are int8 planes, so v_mfma_i32_16x16x64_i8 multiplies them with the expanded
// 2-bit weights and every 16-element partial sum is an EXACT integer; scales are applied once per 32 weights.
//
// Why the producer quantises: in round 1 every one of the 1,728 waves of a gate|up launch
// converted its own K range (218 VALU instructions per wave, 96 KB of f32 activation + gamma loads per workgroup
// through the CU's 64 B/clk vector-memory path) -- half of the kernel's issue slots.  A producer workgroup
// owns 16 output rows = one 16-group: it quantises them in its epilogue (~25 instructions on ONE wave).
//
// Layout in HBM, per 256 columns one 576-byte record (a consumer wave copies its K range into LDS with flat 16-byte
// loads):   [0, 256) d0 plane   [256, 512) d1 plane   [512, 576) sixteen f32 group scales
// Scale slot of 16-group t (t = k / 16 inside the record): lane group g = t / 4 of the MFMA's K = 64, MFMA m = t % 4
// of the record's four; m = 2 p + h (p = which 32-block of the lane group, h = which half of it) -> slot 4 g + 2 h + p,
// so the four scales a consumer lane needs for one record are 16 contiguous bytes.
//
// LayerNorm rides along as in round 1 (applied after the product): the producer multiplies by the consumer's gamma
// before quantising and leaves one (sum, sum of squares) pair per 16 rows (f32 sums stored as f64); the consumer adds the
// pairs up in f64.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave.hpp"

namespace bitnet_hip {

constexpr int kQRec = 576;  // bytes per 256-column record

__host__ __device__ inline size_t qact_bytes(size_t cols) { return ((cols + 255) / 256) * (size_t)kQRec; }

// The format, ONCE (qact_emit; k_gemv_q's merging prologue).  Bits of the group's |maximum| -> sc = 2^(13 - E) to multiply with, as = 2^(E - 13) to store
__device__ __forceinline__ void qact_scales(uint32_t max_bits, float &sc, float &as) {
    int be = (int)(max_bits >> 23);  // biased exponent of the group maximum
    be = be < 32 ? 32 : be;          // keeps both scales normal floats; groups below 2^-95 quantise to zero
    be = be > 254 ? 254 : be;        // Inf / NaN input: garbage in, finite scale out
    sc = __uint_as_float((uint32_t)(267 - be) << 23);
    as = __uint_as_float((uint32_t)(be - 13) << 23);
}
// value -> balanced digits: q = floor(u sc + 1/2), |q| <= 2^14; byte 0 of the result = d0, byte 1 = d1
__device__ __forceinline__ uint32_t qact_digits(float u, float sc) { return ((uint32_t)cvt_rpi(u * sc) + 0x80u) ^ 0x80u; }
// 16-group tp of a record -> its scale slot (lane group g = tp / 4, MFMA m = tp % 4 = 2 p + h -> 4 g + 2 h + p, see above)
__device__ __forceinline__ float *qact_scale_slot(uint8_t *rec, int group) {
    const int tp = group & 15, g = tp >> 2, m = tp & 3;
    return reinterpret_cast<float *>(rec + 512) + (4 * g + 2 * (m & 1) + (m >> 1));
}

// One thread per element, the 16 threads of a DPP row = the 16 elements of group `group` (rows 16 group .. + 15 of
// the producing matrix = columns of the consumer), r = element inside the group.  v = the f32 value (what the
// reference holds), u = what the consumer multiplies its weights with (v, or v * gamma for a LayerNorm consumer).
// EVERY lane of the row must call this (DPP reductions).  stats (nullable): [group][2] f64 (sum v, sum v^2).
__device__ __forceinline__ void qact_emit(uint8_t *__restrict__ qout, double *__restrict__ stats, int group, int r, float v, float u) {
    if (stats) {
        // f32 sums over the 16 values (8 instructions on the ONE wave that runs a producer's epilogue; the f64 form was 24
        // with their DPP hazards), widened to f64 for the consumer, which adds the pairs of the whole row up in f64: the
        // statistics stay ~1e-7 accurate, two orders below the activation format itself
        const float s1 = row16_sum_f(v), s2 = row16_sum_f(v * v);
        if (r == 0) *reinterpret_cast<double2 *>(stats + 2 * (size_t)group) = double2{(double)s1, (double)s2};
    }
    float sc, as;
    qact_scales(__float_as_uint(row16_max_abs(u)), sc, as);
    const uint32_t t = qact_digits(u, sc);
    const int rec = group >> 4, tp = group & 15;
    uint8_t *base = qout + (size_t)rec * kQRec;
    base[16 * tp + r] = (uint8_t)t;
    base[256 + 16 * tp + r] = (uint8_t)(t >> 8);
    if (r == 0) *qact_scale_slot(base, group) = as;
}

}  // namespace bitnet_hip
