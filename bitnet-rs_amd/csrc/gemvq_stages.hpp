// gemvq_stages.hpp -- stages of the QAct GEMV written ONCE for k_gemv_q (kernels_gemvq.hip) and k_gemv_q_batch (kernels_batch.hip): "batch-1's
// arithmetic in its order" by construction.  Each compiles to the instructions both kernels held before; the other stages: EXPERIMENTS.md 28.
#pragma once

#include "wave.hpp"

namespace bitnet_hip {
// Ring slot j of a wave's K range b0 .. b1 - 1 -> its 256-column block, clamped: a short range re-reads its last tile
__device__ __forceinline__ int ring_block(int b0, int b1, int j) { return b0 + j < b1 ? b0 + j : b1 - 1; }
// One 32-weight block (pp = 0 / 1 of the lane group's two) behind its MFMA pair: digits recombined, as = its scales (h0 p0, h0 p1, h1 p0, h1 p1)
__device__ __forceinline__ float gemvq_block_value(v4i acc, float4 as, int pp) {
    // acc[2 d + h]: exact sums over the 16 weights of half h with digit plane d; |.| <= 16 * 2 * 128
    const int i0 = (int)(((uint32_t)acc[2] << 8) + (uint32_t)acc[0]), i1 = (int)(((uint32_t)acc[3] << 8) + (uint32_t)acc[1]);
    const float t = (float)i0 * (pp ? as.y : as.x);
    return fmaf((float)i1, pp ? as.w : as.z, t);
}
// The four k-groups of a weight row sit in lanes c, c + 16, c + 32, c + 48: two lane swaps (v_permlane16_swap, v_permlane32_swap) add them
// up in every wave at once -- (g0 + g1) + (g2 + g3) -- instead of 4 LDS reads per K part in the one storing wave
__device__ __forceinline__ float sum_kgroups(float facc) {
    // inline asm with the hazard pad inside (a VALU write needs 2 wait states before v_permlane*_swap reads it):
    // hipcc's __builtin_amdgcn_permlane16_swap folded the two results into one register here (ROCm 7.2)
    float a = facc, b = facc;
    asm volatile("v_nop\n\tv_nop\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    facc = a + b;  // rows (g0 + g1, g0 + g1, g2 + g3, g2 + g3)
    a = facc, b = facc;
    asm volatile("v_nop\n\tv_nop\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}
// A row's (sum, sum of squares) -> the f32 mean the reference subtracts, 1 / sqrt(var + eps) by v_rcp_f64 + two Newton steps; 1/cols from the host [+ k_gemv_mfma]
__device__ __forceinline__ void ln_from_sums(double s1, double s2, double inv_cols, float ln_eps, double *ln_mean, double *ln_rdenom) {
    const double mean_d = s1 * inv_cols;
    const double var_d = s2 * inv_cols - mean_d * mean_d;
    *ln_mean = (double)(float)mean_d;
    const double denom = (double)sqrtf((float)(var_d > 0.0 ? var_d : 0.0) + ln_eps);
    double r = __builtin_amdgcn_rcp(denom);
    r = r * (2.0 - denom * r);
    *ln_rdenom = r * (2.0 - denom * r);
}
// One vector's statistics from its n_stats pairs in LDS, one wave.  k_gemv_q restates the loop (as a call two of its moves change order)
__device__ __forceinline__ void ln_row_stats(const uint8_t *cs, int n_stats, int lane, double inv_cols, float ln_eps, double &ln_mean, double &ln_rdenom) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < n_stats; i += 64) {
        const double2 pr = *reinterpret_cast<const double2 *>(cs + 16 * i);
        s1 += pr.x;
        s2 += pr.y;
    }
    s1 = wave64_sum_d_rows_readlane(s1);
    s2 = wave64_sum_d_rows_readlane(s2);
    ln_from_sums(s1, s2, inv_cols, ln_eps, &ln_mean, &ln_rdenom);
}

}  // namespace bitnet_hip
