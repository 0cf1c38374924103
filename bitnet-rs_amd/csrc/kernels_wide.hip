// kernels_wide.hip -- the two ends of the WIDE decode step (gfx950): up to kWideMax live sequences' current tokens as the dense rows of one
// matrix, so that every weight matrix is read once on the matrix cores (the many-row matmuls of the prompt forward) and all logits rows come
// from one pass over the embedding table (k_score_*).  Between the two ends each row attends over its own sequence's cache
// (k_attn_partial_rows / k_attn_combine_rows, beside the forms they share their bodies with in kernels_attn.hip).
//
//   k_embed_rows   row b of x = embedding of history_ptrs[b][*pos_ptrs[b]]: k_embed_f16's clamp and conversion, so a row's bits are that
//                  kernel's; an idle row (NULL history or position) is zero-filled -- the matmuls read every row and must see finite data;
//   k_pick_rows    the hand-over behind the head: logits row b -> the member's own logits buffer, and the greedy hand-over of
//                  k_argmax_final (token, history at p + 1 unless forced, position) from the head's per-row argmax.
// Per-sequence state is reached through DEVICE pointer tables, as in kernels_batch.hip; a NULL entry is an idle row.
#include <algorithm>

#include "common.hpp"
#include "wave.hpp"

namespace bitnet_hip {

namespace {

// grid (ceil(hidden / 8 / 256), n_seq): a thread converts 8 consecutive elements (hidden % 8 == 0)
__global__ __launch_bounds__(256) void k_embed_rows(const _Float16 *__restrict__ table, const int *const *__restrict__ history_ptrs,
                                                    const int *const *__restrict__ pos_ptrs, int hidden, int vocab, float *__restrict__ x_out) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= (hidden >> 3)) return;
    const int *hist = history_ptrs[b], *pp = pos_ptrs[b];
    float4 *o = reinterpret_cast<float4 *>(x_out + (size_t)b * hidden + 8 * c);
    if (!hist || !pp) {  // idle row (block-uniform)
        o[0] = float4{0.f, 0.f, 0.f, 0.f};
        o[1] = float4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    int tok = hist[*pp];
    tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
    const h8 h = *reinterpret_cast<const h8 *>(table + (size_t)tok * hidden + 8 * c);
    o[0] = float4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    o[1] = float4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
}

// grid (copy blocks, n_seq): the blocks of row b stride over its vocab entries; block 0's first thread then does the hand-over (nothing in
// this launch reads what it writes).  A row without a logits pointer is idle; one with neither a token nor a position pointer gets logits only.
__global__ __launch_bounds__(256) void k_pick_rows(const float *__restrict__ logits, const int *__restrict__ argmax, int vocab,
                                                   float *const *__restrict__ logits_ptrs, int *const *__restrict__ token_ptrs,
                                                   int *const *__restrict__ pos_ptrs, int *const *__restrict__ history_ptrs,
                                                   const int *const *__restrict__ n_forced_ptrs) {
    const int b = blockIdx.y;
    float *dst = logits_ptrs[b];
    if (!dst) return;  // block-uniform
    const float *src = logits + (size_t)b * vocab;
    const int tid = blockIdx.x * 256 + threadIdx.x, nt = gridDim.x * 256;
    if ((vocab & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int i = tid; i < (vocab >> 2); i += nt) d4[i] = s4[i];
    } else {
        for (int i = tid; i < vocab; i += nt) dst[i] = src[i];
    }
    if (tid != 0) return;
    int *token_out = token_ptrs ? token_ptrs[b] : nullptr;
    int *pos_ptr = pos_ptrs ? pos_ptrs[b] : nullptr;
    if (!token_out && !pos_ptr) return;  // a member that samples
    int tok = argmax[b];
    tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
    if (token_out) *token_out = tok;
    if (pos_ptr) {
        const int p = *pos_ptr;
        int *history = history_ptrs ? history_ptrs[b] : nullptr;
        const int *n_forced = n_forced_ptrs ? n_forced_ptrs[b] : nullptr;
        if (history && (!n_forced || p + 1 >= *n_forced)) history[p + 1] = tok;
        *pos_ptr = p + 1;
    }
}

}  // namespace

hipError_t launch_embed_rows(const void *table, const int *const *history_ptrs, const int *const *pos_ptrs, int n_seq, int hidden, int vocab, float *x_out,
                             hipStream_t stream) {
    if (hidden <= 0 || hidden % 8 != 0 || vocab <= 0 || n_seq < 1 || n_seq > kWideMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_embed_rows, dim3((unsigned)div_ceil((size_t)(hidden >> 3), 256), (unsigned)n_seq), dim3(256), 0, stream,
                       static_cast<const _Float16 *>(table), history_ptrs, pos_ptrs, hidden, vocab, x_out);
    return hipGetLastError();
}

hipError_t launch_pick_rows(const float *logits, const int *argmax, int n_seq, int vocab, float *const *logits_ptrs, int *const *token_ptrs, int *const *pos_ptrs,
                            int *const *history_ptrs, const int *const *n_forced_ptrs, hipStream_t stream) {
    if (vocab <= 0 || n_seq < 1 || n_seq > kWideMax) return hipErrorInvalidValue;
    // 4 elements per thread and pass: 16 blocks of 256 threads copy a 128k-entry row in 8 passes (64 rows: 1024 workgroups, four per CU)
    const unsigned blocks = (unsigned)std::min<size_t>(16, div_ceil((size_t)vocab, 1024));
    hipLaunchKernelGGL(k_pick_rows, dim3(blocks, (unsigned)n_seq), dim3(256), 0, stream, logits, argmax, vocab, logits_ptrs, token_ptrs, pos_ptrs, history_ptrs,
                       n_forced_ptrs);
    return hipGetLastError();
}

}  // namespace bitnet_hip
