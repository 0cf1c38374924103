// kernels_score.hip -- teacher-forced scoring of prompt rows (crates/bitnet-cli/src/score.rs:96-119, log_softmax_stable :160-173;
// commands/eval.rs teacher-forced NLL; parity::eval_logits_all_positions): the tied LM head over ALL rows of the prompt forward,
// with a log-sum-exp epilogue so the [n, vocab] logits are never stored unless asked for.
//
//   k_score_rows_f16   a_r = f16(LN(x_r) * gamma): the final norm of k_logits_f16 (kernels_decode.hip) in its f32 op order, rounded once;
//                      zero rows up to the token tile.
//   k_score_head       l = a . E^T on v_mfma_f32_16x16x32_f16, f32 accumulate.  Workgroup tile 128 vocabulary rows x 128 tokens, four
//                      waves of 64 x 64 (2 x 2), K steps of 64 columns staged global -> LDS by LDS-DMA (global_load_lds_dwordx4) into two
//                      buffers.  Both operands are K-contiguous (the B^T form): an LDS row is the 128 bytes of one step of one row, its
//                      16-byte unit u stored at u ^ ((row >> 1) & 7) -- the swizzle is applied to the DMA's SOURCE address, the image stays
//                      lane-linear -- so the sixteen rows a ds_read_b128 service group reads fall on sixteen different bank groups.
//                      Epilogue on the accumulators: per token and 128-row vocabulary block, max and sum exp(l - max) over the finite logits
//                      (non-finite -> -inf, score.rs:106-110), the argmax (NaN = -inf, lowest index on ties: sampling.rs:45-49,189-202), the
//                      target's raw logit, and optionally the raw logits of rows < logits_rows.  The two vocabulary halves of a block are merged
//                      in LDS in a fixed order; one partial (max, sum, best value, best index) per (token, block) goes to the workspace.
//                      Workgroup order: the token tiles of one vocabulary block run back to back on one XCD (the table is read from HBM
//                      about once; the token rows, 21 MB at 4096 x 2560, stay in the MALL).
//   k_score_combine    one workgroup per row merges its partials in a fixed order: lse = M + log(S), nll = lse - l_target, argmax.
// Deterministic: fixed reduction orders everywhere, no float atomics.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "common.hpp"
#include "wave.hpp"

namespace bitnet_hip {
namespace {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;

constexpr int kSV = 128;                // vocabulary rows per workgroup
constexpr int kST = 128;                // tokens per workgroup
constexpr int kSK = 64;                 // columns per K step (128 bytes of a row)
constexpr int kSTile = kSV * kSK * 2;   // bytes of one staged operand tile (16 KiB; kSV == kST)
constexpr int kSLds = 4 * kSTile;       // two buffers x two operands

// (v, i) beats (bv, bi): larger value, or equal value and lower index
__device__ __forceinline__ bool sc_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// (m, s) <- (m, s) (+) (m2, s2): running max and sum exp(l - max); an empty side (max -inf) adds nothing
__device__ __forceinline__ void sc_merge(float &m, float &s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    const float a = m == -INFINITY ? 0.0f : s * expf(m - mm);
    const float b = m2 == -INFINITY ? 0.0f : s2 * expf(m2 - mm);
    m = mm;
    s = a + b;
}

__global__ __launch_bounds__(256) void k_score_rows_f16(const float *__restrict__ x, const float *__restrict__ gamma, float eps, int hidden,
                                                        int n_rows, _Float16 *__restrict__ a) {
    __shared__ float slot[4];
    const int tid = threadIdx.x;
    _Float16 *ar = a + (size_t)blockIdx.x * hidden;
    if ((int)blockIdx.x >= n_rows) {
        for (int i = tid; i < hidden; i += 256) ar[i] = (_Float16)0.0f;
        return;
    }
    const float *xr = x + (size_t)blockIdx.x * hidden;
    float s = 0.0f;
    for (int i = tid; i < hidden; i += 256) s += xr[i];
    const float mean = gamma ? block256_sum_f(s, slot) / (float)hidden : 0.0f;
    float ss = 0.0f;
    for (int i = tid; i < hidden; i += 256) {
        const float d = xr[i] - mean;
        ss += d * d;
    }
    const float denom = gamma ? sqrtf(block256_sum_f(ss, slot) / (float)hidden + eps) : 1.0f;
    for (int i = tid; i < hidden; i += 256) ar[i] = (_Float16)(gamma ? (xr[i] - mean) / denom * gamma[i] : xr[i]);
}

struct ScoreArgs {
    const _Float16 *table;  // [vocab, hidden]
    const _Float16 *a;      // [n_pad, hidden]
    const int32_t *targets;
    float *logits;          // [logits_rows, vocab] or null
    v4f *part;            // [n_pad][vb_count]: (max, sum, best value, best index as bits)
    float *tlog;            // [n_pad]: raw logit of the row's target
    int hidden, vocab, n_rows, logits_rows, vb_count, tb_count;
};

__device__ __forceinline__ void sc_glds(const uint8_t *src, uint8_t *lds_dst) {
    __builtin_amdgcn_global_load_lds((glb_void_t *)src, (lds_void_t *)lds_dst, 16, 0, 0);
}

__global__ __launch_bounds__(256, 2) void k_score_head(ScoreArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSLds];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4, wv = wave & 1, wt = wave >> 1;
    int id = blockIdx.x;
    {  // one XCD works through consecutive logical ids: the token tiles of a vocabulary block
        const int total = gridDim.x;
        if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    }
    const int vb = id / p.tb_count, tb = id - vb * p.tb_count;
    const int v0 = vb * kSV, t0 = tb * kST;
    const size_t row_b = (size_t)p.hidden * 2;
    // staging: a piece is 8 rows x 128 bytes (one DMA instruction, 1 KiB); wave w moves pieces 4 w .. 4 w + 3 of each operand.  Lane l of
    // piece i lands at row 8 i + (l >> 3), slot l & 7, and fetches the unit stored there: (l & 7) ^ ((row >> 1) & 7).
    const uint8_t *esrc[4], *asrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 8 * (4 * wave + i) + (lane >> 3);
        const int q = (lane & 7) ^ ((row >> 1) & 7);
        const int vr = v0 + row < p.vocab ? v0 + row : p.vocab - 1;  // rows past the vocabulary re-read the last one (masked below)
        esrc[i] = reinterpret_cast<const uint8_t *>(p.table) + (size_t)vr * row_b + q * 16;
        asrc[i] = reinterpret_cast<const uint8_t *>(p.a) + (size_t)(t0 + row) * row_b + q * 16;
    }
    auto stage = [&](int ks, int buf) {
        uint8_t *eb = lds + buf * 2 * kSTile, *ab = eb + kSTile;
#pragma unroll
        for (int i = 0; i < 4; ++i) sc_glds(esrc[i] + (size_t)ks * 128, eb + (4 * wave + i) * 1024);
#pragma unroll
        for (int i = 0; i < 4; ++i) sc_glds(asrc[i] + (size_t)ks * 128, ab + (4 * wave + i) * 1024);
    };
    // fragment of lane (c, g) in K half kk: row c of its 16-row tile, unit 4 kk + g (row & 15 == c, so the swizzle is (c >> 1) & 7)
    int off_e[2], off_a[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int u = ((4 * kk + g) ^ ((c >> 1) & 7)) * 16;
        off_e[kk] = (wv * 64 + c) * 128 + u;
        off_a[kk] = (wt * 64 + c) * 128 + u;
    }
    v4f acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = (v4f){0.f, 0.f, 0.f, 0.f};
    const int nk = p.hidden / kSK;
    stage(0, 0);
    for (int ks = 0; ks < nk; ++ks) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of step ks have landed
        __syncthreads();                                  // ... everyone's; and nobody reads the buffer of step ks - 1 any more
        if (ks + 1 < nk) stage(ks + 1, (ks + 1) & 1);
        const uint8_t *eb = lds + (ks & 1) * 2 * kSTile, *ab = eb + kSTile;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            h8 af[4], bf[4];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) af[rt] = *reinterpret_cast<const h8 *>(eb + off_e[kk] + rt * 16 * 128);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bf[ct] = *reinterpret_cast<const h8 *>(ab + off_a[kk] + ct * 16 * 128);
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rt], bf[ct], acc[rt][ct], 0, 0, 0);
        }
    }
    // epilogue: acc[rt][ct][j] = logit of vocabulary row v0 + 64 wv + 16 rt + 4 g + j, token t0 + 64 wt + 16 ct + c
    float pm[4], ps[4], pv[4];
    int pi[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int token = t0 + wt * 64 + ct * 16 + c;
        const int tgt = token < p.n_rows ? p.targets[token] : -1;
        const bool dump = token < p.logits_rows;
        float m = -INFINITY, bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + wv * 64 + rt * 16 + 4 * g + j;
                const float l = acc[rt][ct][j];
                const bool in = v < p.vocab;
                const float e = (in && isfinite(l)) ? l : -INFINITY;
                m = fmaxf(m, e);
                const float av = (!in || l != l) ? -INFINITY : l;
                const int ai = in ? v : 0x7fffffff;
                if (sc_better(av, ai, bv, bi)) bv = av, bi = ai;
                if (v == tgt) p.tlog[token] = l;
                if (dump && in) p.logits[(size_t)token * p.vocab + v] = l;
            }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float s = 0.0f;
        if (m != -INFINITY) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = v0 + wv * 64 + rt * 16 + 4 * g + j;
                    const float l = acc[rt][ct][j];
                    if (v < p.vocab && isfinite(l)) s += expf(l - m);
                }
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (sc_better(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        pm[ct] = m, ps[ct] = s, pv[ct] = bv, pi[ct] = bi;
    }
    // merge the two vocabulary halves of the block (wave column wv = 0 holds the lower indices) and write one partial per token
    __syncthreads();  // every wave is done with the staged tiles
    v4f *xch = reinterpret_cast<v4f *>(lds);  // [wt][64 tokens]
    if (wv == 1 && g == 0) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) xch[wt * 64 + ct * 16 + c] = (v4f){pm[ct], ps[ct], pv[ct], __int_as_float(pi[ct])};
    }
    __syncthreads();
    if (wv == 0 && g == 0) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int token = t0 + wt * 64 + ct * 16 + c;
            if (token >= p.n_rows) continue;
            const v4f o = xch[wt * 64 + ct * 16 + c];
            float m = pm[ct], s = ps[ct], bv = pv[ct];
            int bi = pi[ct];
            sc_merge(m, s, o.x, o.y);
            if (sc_better(o.z, __float_as_int(o.w), bv, bi)) bv = o.z, bi = __float_as_int(o.w);
            p.part[(size_t)token * p.vb_count + vb] = (v4f){m, s, bv, __int_as_float(bi)};
        }
    }
}

__global__ __launch_bounds__(256) void k_score_combine(const v4f *__restrict__ part, const float *__restrict__ tlog,
                                                       const int32_t *__restrict__ targets, int vb_count, int vocab, float *__restrict__ nll,
                                                       int32_t *__restrict__ argmax) {
    __shared__ float sm[256], ss[256], sv[256];
    __shared__ int si[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const v4f *pr = part + (size_t)row * vb_count;
    float m = -INFINITY, s = 0.0f, bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int b = tid; b < vb_count; b += 256) {
        const v4f q = pr[b];
        sc_merge(m, s, q.x, q.y);
        if (sc_better(q.z, __float_as_int(q.w), bv, bi)) bv = q.z, bi = __float_as_int(q.w);
    }
    sm[tid] = m, ss[tid] = s, sv[tid] = bv, si[tid] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            float m1 = sm[tid], s1 = ss[tid];
            sc_merge(m1, s1, sm[tid + off], ss[tid + off]);
            sm[tid] = m1, ss[tid] = s1;
            if (sc_better(sv[tid + off], si[tid + off], sv[tid], si[tid])) sv[tid] = sv[tid + off], si[tid] = si[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int t = targets[row];
        float r;
        if (t < 0)
            r = 0.0f;
        else if (t >= vocab || sm[0] == -INFINITY)  // no such entry / every logit of the row non-finite (log_softmax_stable gives NaN)
            r = NAN;
        else {
            const float lt = tlog[row];
            r = isfinite(lt) ? (sm[0] + logf(ss[0])) - lt : INFINITY;
        }
        nll[row] = r;
        if (argmax) argmax[row] = si[0] == 0x7fffffff ? 0 : si[0];
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: a [n_pad, hidden] f16 | tlog [n_pad] f32 | partials [n_pad][vb_count] x 16 bytes; 0 if any product overflows
size_t score_ws_bytes(size_t n_rows, size_t hidden, size_t vocab) {
    const size_t n_pad = div_ceil(n_rows, kST) * kST, vbc = div_ceil(vocab, kSV);
    size_t a = 0, pt = 0, tot = 0;
    if (__builtin_mul_overflow(n_pad, hidden, &a) || __builtin_mul_overflow(a, (size_t)2, &a)) return 0;
    if (__builtin_mul_overflow(n_pad, vbc, &pt) || __builtin_mul_overflow(pt, (size_t)16, &pt)) return 0;
    if (__builtin_add_overflow(align256(a), align256(n_pad * 4), &tot) || __builtin_add_overflow(tot, pt, &tot)) return 0;
    return tot;
}

}  // namespace
}  // namespace bitnet_hip

using namespace bitnet_hip;

extern "C" {

size_t bitnet_hip_score_workspace_bytes(size_t n_rows, size_t hidden, size_t vocab) {
    if (n_rows == 0 || hidden == 0 || vocab == 0 || n_rows >= (1u << 30) || vocab >= (1u << 30) || hidden >= (1u << 20)) return 0;
    return score_ws_bytes(n_rows, hidden, vocab);
}

int bitnet_hip_score_f16_dev(const void *table_f16_dev, const float *x_dev, const float *gamma_dev, float eps, size_t hidden, size_t vocab,
                             size_t n_rows, const int32_t *targets_dev, float *nll_dev, int32_t *argmax_dev, float *logits_dev,
                             size_t logits_rows, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!table_f16_dev || !x_dev || !targets_dev || !nll_dev || !workspace_dev || (logits_rows && !logits_dev))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to score_f16_dev");
    if (hidden == 0 || hidden % kSK != 0)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "score_f16_dev: hidden must be a positive multiple of 64, got %zu", hidden);
    if (vocab == 0 || n_rows == 0)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "score_f16_dev: dimensions must be > 0: vocab=%zu, n_rows=%zu", vocab, n_rows);
    if (logits_rows > n_rows)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "score_f16_dev: logits_rows %zu > n_rows %zu", logits_rows, n_rows);
    size_t dump = 0;
    const size_t need = bitnet_hip_score_workspace_bytes(n_rows, hidden, vocab);  // 0: a product overflows
    const size_t grid = need ? div_ceil(n_rows, kST) * div_ceil(vocab, kSV) : 0;
    if (need == 0 || __builtin_mul_overflow(logits_rows, vocab, &dump) || __builtin_mul_overflow(dump, (size_t)4, &dump) || grid >= (1u << 31))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "score_f16_dev: dimensions too large for this library (n_rows=%zu, hidden=%zu, vocab=%zu)",
                         n_rows, hidden, vocab);
    if (workspace_bytes < need)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "score_f16_dev: workspace too small: %zu bytes needed, %zu given", need, workspace_bytes);
    const size_t n_pad = div_ceil(n_rows, kST) * kST, vbc = div_ceil(vocab, kSV);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    ScoreArgs a;
    a.table = static_cast<const _Float16 *>(table_f16_dev);
    a.a = reinterpret_cast<const _Float16 *>(ws);
    a.tlog = reinterpret_cast<float *>(ws + align256(n_pad * hidden * 2));
    a.part = reinterpret_cast<v4f *>(ws + align256(n_pad * hidden * 2) + align256(n_pad * 4));
    a.targets = targets_dev;
    a.logits = logits_rows ? logits_dev : nullptr;
    a.hidden = (int)hidden, a.vocab = (int)vocab, a.n_rows = (int)n_rows, a.logits_rows = (int)logits_rows;
    a.vb_count = (int)vbc, a.tb_count = (int)(n_pad / kST);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_score_rows_f16, dim3((unsigned)n_pad), dim3(256), 0, s, x_dev, gamma_dev, eps, (int)hidden, (int)n_rows,
                       reinterpret_cast<_Float16 *>(ws));
    BH_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_score_head, dim3((unsigned)grid), dim3(256), 0, s, a);
    BH_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_score_combine, dim3((unsigned)n_rows), dim3(256), 0, s, a.part, a.tlog, targets_dev, (int)vbc, (int)vocab, nll_dev,
                       argmax_dev);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

}  // extern "C"
