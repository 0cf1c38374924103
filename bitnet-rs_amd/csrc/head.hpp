// head.hpp -- the pieces of the batch-1 decode head (k_logits_f16, kernels_decode.hip) that the screened greedy head (kernels_head.hip)
// must repeat BIT FOR BIT: the final norm into LDS, the lane -> element map of the activation slice, a row's loads and a lane's partial
// dot product.  Both files call these; neither restates them.
#pragma once

#include "common.hpp"
#include "wave.hpp"

namespace bitnet_hip {

// final norm (T:1589) of the 256-thread workgroup: xs[0, hidden) = LN(x) * gamma, or x itself without gamma.  Every thread calls it; ends
// with a barrier.
__device__ __forceinline__ void head_final_norm(const float *__restrict__ x, const float *__restrict__ gamma, float eps, int hidden, float *xs,
                                                float *slot) {
    const int tid = threadIdx.x;
    float s = 0.0f;
    for (int i = tid; i < hidden; i += 256) s += x[i];
    const float mean = gamma ? block256_sum_f(s, slot) / (float)hidden : 0.0f;
    float ss = 0.0f;
    for (int i = tid; i < hidden; i += 256) {
        const float d = x[i] - mean;
        ss += d * d;
    }
    const float denom = gamma ? sqrtf(block256_sum_f(ss, slot) / (float)hidden + eps) : 1.0f;
    for (int i = tid; i < hidden; i += 256) xs[i] = gamma ? (x[i] - mean) / denom * gamma[i] : x[i];
    __syncthreads();
}

// a lane's slice of the activations: element i of chunk c is column 512 c + 8 lane + i; chunks past hidden / 512 (GUARD) are zero padding
template <int NCH, bool GUARD>
__device__ __forceinline__ void head_lane_x(const float *xs, int nchunks, int lane, float (&xr)[NCH][8]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) xr[c][i] = (!GUARD || c < nchunks) ? xs[512 * c + 8 * lane + i] : 0.0f;
}

// a lane's slice of one table row (e = the row + 8 lane): the table is read once per token by one wave: non-temporal (MI355X_MICROARCH.md,
// nt-weights)
template <int NCH, bool GUARD>
__device__ __forceinline__ void head_lane_row(const _Float16 *e, int nchunks, h8 (&w)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        // a chunk past hidden / 512 is padding: zeros, not a second read of chunk 0 (0 * Inf of a table entry there would be NaN)
        if (!GUARD || c < nchunks)
            w[c] = __builtin_nontemporal_load(reinterpret_cast<const h8 *>(e + 512 * c));
        else
            w[c] = (h8)(_Float16)0.0f;
    }
}

// a lane's partial of one row: chunks in order, elements in order, one chain (v_fma_mix_f32).  The row's logit is the xor butterfly
// 32 .. 1 over the 64 partials (wave64_sum_f_xor; k_logits_f16 interleaves the same steps over its R rows).
template <int NCH>
__device__ __forceinline__ float head_lane_dot(const float (&xr)[NCH][8], const h8 (&w)[NCH]) {
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += xr[c][i] * (float)w[c][i];
    return acc;
}

}  // namespace bitnet_hip
