// kernels_batch.hip -- the decode step's kernels for SEVERAL sequences per launch (gfx950): the QAct GEMV, the embedding gather and the
// logits head, each taking n_seq <= kBatchMax vectors (the batched attention lives beside its batch-1 form in kernels_attn.hip).
//
// The reference's forward takes [B, T, H] and its KVCache::new(config, batch_size, ..) carries a batch dimension
// (crates/bitnet-transformer/src/lib.rs:281, :1146-1160, :1215-1245, :1437-1478); this library's decode path had no B.  One decode step is a
// chain of ~155 dependent launches whose cost is the launch, not the bytes (EXPERIMENTS.md 4.1): the way to more tokens per second is to make
// every launch carry more sequences.  Here the weight stream is read ONCE per launch and multiplied with every sequence's vector.
//
// CONTRACT: for each vector the arithmetic is the batch-1 kernel's, operation for operation and in its order (k_gemv_q, k_embed_q,
// k_logits_f16 + k_argmax_final), so every output is BIT-IDENTICAL to the batch-1 entry point called on that vector alone
// (tests/test_batch_ops_gpu.py compares raw bits).  Where hipcc's contraction decided the batch-1 result (the head's dot product and its
// variance sum compile to fused multiply-adds) the fused form is written out here.  The GEMV keeps it BY CONSTRUCTION in the stages both
// kernels call (gemvq_stages.hpp, qact.hpp); its other stages are restated below, named where they stand, and held by that test alone.
#include "common.hpp"
#include "gemvq_stages.hpp"
#include "qact.hpp"
#include "wave.hpp"

namespace bitnet_hip {

namespace {

constexpr int kGemvBatchLdsMax = 160 * 1024;  // gfx950: 160 KiB of LDS per workgroup

struct GemvQBatchArgs : GemvQPrefix {  // tiles .. stats_out as k_gemv_q's (common.hpp), every per-vector buffer [n_seq] of them
    int n_seq, out_rows;
    uint32_t qbytes, qout_bytes;
};
static_assert(sizeof(GemvQBatchArgs) == 152, "the layout k_gemv_q_batch was compiled for: the prefix, then these members");

// k_gemv_q (kernels_gemvq.hip) for NB vectors: 8 waves, the same wave -> (row tile, K range) map, the same block order, lane swaps and K-part
// sum per vector.  Shared functions: ring_block, gemvq_block_value, sum_kgroups, ln_row_stats -> ln_from_sums, qact_emit.  RESTATED (EXPERIMENTS.md 28):
// wave map, epilogue operand rows and dummy loads, scale-tile loads, A-operand lane, weight-scale accumulations, K-part sums with LayerNorm and silu * up.  A wave loads and expands each weight tile ONCE (the B operand of the int8 MFMA) and multiplies it with every vector's digit
// planes (the A operand, from that vector's LDS image).  NB = compile-time vector count (2, 4, 8); slots n_seq .. NB - 1 redo vector
// n_seq - 1 and are never stored.  LDS: RING zero records, then n_seq whole QAct vectors (the down-projection's 6912 columns: 15.5 KB each),
// n_seq statistics blocks (LN), NB x 8 x 16 partial sums -- up to 160 KiB (raise_dynamic_lds).
// The activation copy takes 8 passes of 8 KiB per round: the first round is requested ahead of the weight stream (vmcnt retires in order),
// further rounds (only 8 vectors of more than 4096 columns need one) behind it.
template <int RING, int SC, int LN, int NB>
__global__ __launch_bounds__(512) void k_gemv_q_batch(GemvQBatchArgs p) {
    constexpr int NW = 8, NT = NW * 64, NCP = 8;
    constexpr int ZB = RING * kQRec;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t qtot = (uint32_t)p.n_seq * p.qbytes;         // multiples of 16 (kQRec = 36 * 16)
    const uint32_t stot = (uint32_t)p.n_seq * (uint32_t)p.n_stats * 16u;
    uint8_t *zq = lds;                    // [ZB] zeros the dead A lanes read
    uint8_t *cq = lds + ZB;               // [n_seq][qbytes]
    uint8_t *cs = cq + qtot;              // [n_seq][n_stats][16] (LN)
    float *part = reinterpret_cast<float *>(cs + (LN ? stot : 0u));  // [NB][NW][16]
    if (16 * tid < ZB) *reinterpret_cast<v4u *>(zq + 16 * tid) = v4u{0u, 0u, 0u, 0u};

    // ---- wave -> (row tile, K range): k_gemv_q's map, restated ----
    const int ksplit = 1 << p.ks_log2;
    const int tiles_per_wg = NW >> p.ks_log2;
    const int n_tiles = p.rows >> 4;
    int tile = blockIdx.x * tiles_per_wg + (wave >> p.ks_log2);
    tile = tile < n_tiles ? tile : n_tiles - 1;
    int kpart = wave & (ksplit - 1);
    if (p.ks_log2 == 3 && wave >= 4) kpart = 11 - wave;
    const int b0 = (kpart * p.nblk) >> p.ks_log2, b1 = ((kpart + 1) * p.nblk) >> p.ks_log2;

    // ---- 1. activations (first round), statistics, epilogue operands (k_gemv_q's e_row .. e_gam, restated): all unconditional, clamped ----
    v4u qa[NCP];
#pragma unroll
    for (int i = 0; i < NCP; ++i) qa[i] = *reinterpret_cast<const v4u *>(p.qin + umin32(16u * (uint32_t)(tid + NT * i), qtot - 16u));
    v4u st[LN ? 4 : 1];  // n_seq * n_stats <= 8 * 256 pairs (launcher)
    if (LN) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            st[i] = *reinterpret_cast<const v4u *>(reinterpret_cast<const uint8_t *>(p.stats_in) + umin32(16u * (uint32_t)(tid + NT * i), stot - 16u));
    }
    const int e_tl = tid >> 4, e_r = tid & 15;
    int e_row, e_g0 = 0, e_g1 = 0;
    if (!p.silu_mul) {
        e_row = 16 * (blockIdx.x * tiles_per_wg + e_tl) + e_r;
        e_row = e_row < p.rows ? e_row : p.rows - 1;
        e_g0 = e_row;
    } else {
        const int half_rows = p.rows >> 1;
        const int pg = blockIdx.x * (tiles_per_wg >> 1) + e_tl;
        e_row = 16 * pg + e_r;
        e_row = e_row < half_rows ? e_row : half_rows - 1;
        e_g0 = 32 * (e_row >> 4) + e_r;
        e_g1 = e_g0 + 16;
    }
    float e_lg0 = 0.0f, e_lg1 = 0.0f;
    if (LN) {
        e_lg0 = p.ln_g[e_g0];
        e_lg1 = p.ln_g[e_g1];
    }
    float e_res[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int bb = b < p.n_seq ? b : p.n_seq - 1;
        e_res[b] = (p.residual ? p.residual : reinterpret_cast<const float *>(p.qin))[p.residual ? (size_t)bb * p.out_rows + e_row : 0];
    }
    const float e_gam = (p.gamma_out ? p.gamma_out : reinterpret_cast<const float *>(p.qin))[p.gamma_out ? e_row : 0];
    __builtin_amdgcn_sched_barrier(0);
    // ---- 2. weight tiles (+ scale tiles, k_gemv_q's loads restated): read once by this wave only ----
    const size_t tb0 = (size_t)tile * p.nblk;
    const uint8_t *wbase = p.tiles + (tb0 * 64 + lane) * 16;
    v4u wt[RING];
    uint32_t sh[SC == 2 ? RING : 1];
    float2 sf[SC == 1 ? RING : 1];
#pragma unroll
    for (int j = 0; j < RING; ++j) {
        const int blk = ring_block(b0, b1, j);
        wt[j] = load_nt16v(wbase + (size_t)blk * 1024);
        if (SC == 2) sh[j] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p.stiles) + (tb0 + blk) * 64 + lane);
        if (SC == 1) {
            const float *sp = reinterpret_cast<const float *>(p.stiles) + ((tb0 + blk) * 64 + lane) * 2;
            sf[j] = float2{__builtin_nontemporal_load(sp), __builtin_nontemporal_load(sp + 1)};
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- 3. QAct records and statistics pairs -> LDS, once per workgroup ----
#pragma unroll
    for (int i = 0; i < NCP; ++i) {
        const uint32_t o = 16u * (uint32_t)(tid + NT * i);
        if (o < qtot) *reinterpret_cast<v4u *>(cq + o) = qa[i];
    }
    for (uint32_t base = 16u * NT * NCP; base < qtot; base += 16u * NT * NCP) {
#pragma unroll
        for (int i = 0; i < NCP; ++i) qa[i] = *reinterpret_cast<const v4u *>(p.qin + umin32(base + 16u * (uint32_t)(tid + NT * i), qtot - 16u));
#pragma unroll
        for (int i = 0; i < NCP; ++i) {
            const uint32_t o = base + 16u * (uint32_t)(tid + NT * i);
            if (o < qtot) *reinterpret_cast<v4u *>(cq + o) = qa[i];
        }
    }
    if (LN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t o = 16u * (uint32_t)(tid + NT * i);
            if (o < stot) *reinterpret_cast<v4u *>(cs + o) = st[i];
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // A-operand lane (k-group g, selector row c): k_gemv_q's ba0 / ba1 / sa restated as offsets, one image per vector
    const int g = lane >> 4, c = lane & 15;
    const bool mine = (c >> 2) == g;
    const bool m0 = mine && (c & 1) == 0, m1 = mine && (c & 1) == 1;
    const uint32_t live = (uint32_t)(kQRec * b0 + 256 * ((c >> 1) & 1) + 64 * g);
    const uint32_t sa = (uint32_t)(kQRec * b0 + 512 + 16 * g);
    const uint8_t *pa0[NB], *pa1[NB], *psa[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint8_t *vq = cq + (uint32_t)(b < p.n_seq ? b : p.n_seq - 1) * p.qbytes;
        pa0[b] = m0 ? vq + live : zq;
        pa1[b] = m1 ? vq + live : zq;
        psa[b] = vq + sa;
    }

    float facc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) facc[b] = 0.0f;
#pragma unroll
    for (int j = 0; j < RING; ++j) {
        if (j > 0 && b0 + j >= b1) continue;  // wave-uniform
        const uint32_t wd[4] = {wt[j][0], wt[j][1], wt[j][2], wt[j][3]};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const v4i w0 = decode16(wd[2 * pp], p.lut), w1 = decode16(wd[2 * pp + 1], p.lut);  // expanded once, used by every vector
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float4 as = *reinterpret_cast<const float4 *>(psa[b] + kQRec * j);
                v4i acc = {0, 0, 0, 0};
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i *>(pa0[b] + kQRec * j + 32 * pp), w0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i *>(pa1[b] + kQRec * j + 32 * pp + 16), w1, acc, 0, 0, 0);
                const float t = gemvq_block_value(acc, as, pp);
                if (SC == 2)
                    facc[b] = pp ? fma_mix_hi(t, sh[j], facc[b]) : fma_mix_lo(t, sh[j], facc[b]);
                else if (SC == 1)
                    facc[b] = fmaf(t, pp ? sf[j].y : sf[j].x, facc[b]);
                else
                    facc[b] += t;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float f = sum_kgroups(facc[b]);
        if (lane < 16) part[(b * NW + ((wave >> p.ks_log2) << p.ks_log2) + kpart) * 16 + lane] = f;
    }

    // ---- 4. epilogue: the storing waves, vector after vector (k_gemv_q's K-part sums, LayerNorm, silu and stores, restated) ----
    const bool storing = wave * 64 < tiles_per_wg * 16;
    double ln_mean[LN ? NB : 1], ln_rdenom[LN ? NB : 1];
    if (LN && storing) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            ln_row_stats(cs + (uint32_t)(b < p.n_seq ? b : p.n_seq - 1) * (uint32_t)p.n_stats * 16u, p.n_stats, lane, p.inv_cols, p.ln_eps, ln_mean[b], ln_rdenom[b]);
    }
    __syncthreads();
    if (!storing) return;
    const int tl = e_tl, r = e_r;
    if (!p.silu_mul) {
        if (tl >= tiles_per_wg) return;
        const int t_glob = blockIdx.x * tiles_per_wg + tl;
        if (t_glob >= n_tiles) return;  // whole 16-lane rows leave together
        const int row = 16 * t_glob + r;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= p.n_seq) break;
            const float *pb = part + b * NW * 16;
            float pv[NW];
#pragma unroll
            for (int kp = 0; kp < NW; ++kp) pv[kp] = pb[((tl << p.ks_log2) + (kp < ksplit ? kp : 0)) * 16 + r];
            float v = 0.0f;
#pragma unroll
            for (int kp = 0; kp < NW; ++kp) v += kp < ksplit ? pv[kp] : 0.0f;  // fixed order: K parts 0, 1, ...
            if (LN) v = (float)(((double)v - ln_mean[LN ? b : 0] * (double)e_lg0) * ln_rdenom[LN ? b : 0]);
            if (p.residual) v += e_res[b];
            if (p.y) p.y[(size_t)b * p.out_rows + row] = v;
            if (p.qout)
                qact_emit(p.qout + (size_t)b * p.qout_bytes, p.stats_out ? p.stats_out + (size_t)b * (p.out_rows >> 4) * 2 : nullptr, t_glob, r, v,
                          p.gamma_out ? v * e_gam : v);
        }
    } else {
        const int pairs_per_wg = tiles_per_wg >> 1;
        if (tl >= pairs_per_wg) return;
        const int p_glob = blockIdx.x * pairs_per_wg + tl;
        if (2 * p_glob >= n_tiles) return;
        const int row = 16 * p_glob + r;  // row of silu(gate) * up
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= p.n_seq) break;
            const float *pb = part + b * NW * 16;
            float pg[NW / 2], pu[NW / 2];
#pragma unroll
            for (int kp = 0; kp < NW / 2; ++kp) {
                pg[kp] = pb[(((2 * tl) << p.ks_log2) + (kp < ksplit ? kp : 0)) * 16 + r];
                pu[kp] = pb[(((2 * tl + 1) << p.ks_log2) + (kp < ksplit ? kp : 0)) * 16 + r];
            }
            float gv = 0.0f, uv = 0.0f;
#pragma unroll
            for (int kp = 0; kp < NW / 2; ++kp) {
                gv += kp < ksplit ? pg[kp] : 0.0f;
                uv += kp < ksplit ? pu[kp] : 0.0f;
            }
            if (LN) {
                gv = (float)(((double)gv - ln_mean[LN ? b : 0] * (double)e_lg0) * ln_rdenom[LN ? b : 0]);
                uv = (float)(((double)uv - ln_mean[LN ? b : 0] * (double)e_lg1) * ln_rdenom[LN ? b : 0]);
            }
            const float v = gv * __builtin_amdgcn_rcpf(1.0f + __expf(-gv)) * uv;
            if (p.y) p.y[(size_t)b * p.out_rows + row] = v;
            if (p.qout)
                qact_emit(p.qout + (size_t)b * p.qout_bytes, p.stats_out ? p.stats_out + (size_t)b * (p.out_rows >> 4) * 2 : nullptr, p_glob, r, v,
                          p.gamma_out ? v * e_gam : v);
        }
    }
}

// k_embed_q for n_seq tokens: grid (hidden / 256, n_seq); token = history_ptrs[b][*pos_ptrs[b]], clamped as in batch-1
__global__ __launch_bounds__(256) void k_embed_q_batch(const _Float16 *__restrict__ table, const int *const *__restrict__ history_ptrs,
                                                       const int *const *__restrict__ pos_ptrs, int hidden, int vocab, float *__restrict__ x_out,
                                                       const float *__restrict__ gamma, uint8_t *__restrict__ qout, uint32_t qbytes,
                                                       double *__restrict__ stats) {
    const int b = blockIdx.y;
    const int *hist = history_ptrs[b];
    if (!hist) return;  // idle slot (block-uniform)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hidden) return;
    const int *pp = pos_ptrs[b];
    int tok = hist[pp ? *pp : 0];
    tok = tok < 0 ? 0 : tok >= vocab ? vocab - 1 : tok;
    const float v = (float)table[(size_t)tok * hidden + i];
    x_out[(size_t)b * hidden + i] = v;
    qact_emit(qout + (size_t)b * qbytes, stats ? stats + (size_t)b * (hidden >> 4) * 2 : nullptr, i >> 4, i & 15, v, gamma ? v * gamma[i] : v);
}

// ---- the decode head for n_seq rows: k_logits_f16 (kernels_decode.hip) with the f16 table read ONCE ------------------------------------
// One wave per R vocabulary rows, grid-strided, as batch-1; a wave holds its R table rows in registers and walks the vectors, whose
// normalised activations stay in LDS ([n_seq][hidden]: eight vectors do not fit the registers batch-1 keeps one in).  Per (vector, row):
// lane l takes elements 512 c + 8 l + i in the order c, i as a fused multiply-add chain from 0 (what `acc += x * (float)w` compiles to in
// k_logits_f16: v_fma_mix_f32), then the xor butterfly 32 .. 1 -- the batch-1 bits whatever R and the grid are.  The final norm is batch-1's
// (block256_sum_f; its variance sum compiles to a fused multiply-add, written out here).  GUARD instances (hidden / 512 not an instance of its
// own) also restate batch-1's padding: chunks past hidden / 512 add 0 * 0, which turns an accumulated -0 into +0.
template <int NCH, int R, bool GUARD>
__global__ __launch_bounds__(256) void k_logits_f16_batch(const _Float16 *__restrict__ table, const float *__restrict__ x, const float *__restrict__ gamma,
                                                          float eps, int hidden, int vocab, int n_seq, float *const *__restrict__ logits_ptrs,
                                                          float *__restrict__ best_val, int *__restrict__ best_idx) {
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [n_seq][hidden]
    __shared__ float slot[4];
    __shared__ float wbv[kBatchMax][4];
    __shared__ int wbi[kBatchMax][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = 0; b < n_seq; ++b) {
        const float *xb = x + (size_t)b * hidden;
        float s = 0.0f;
        for (int i = tid; i < hidden; i += 256) s += xb[i];
        const float mean = gamma ? block256_sum_f(s, slot) / (float)hidden : 0.0f;
        float ss = 0.0f;
        for (int i = tid; i < hidden; i += 256) {
            const float d = xb[i] - mean;
            ss = fmaf(d, d, ss);
        }
        const float denom = gamma ? sqrtf(block256_sum_f(ss, slot) / (float)hidden + eps) : 1.0f;
        for (int i = tid; i < hidden; i += 256) xs[(size_t)b * hidden + i] = gamma ? (xb[i] - mean) / denom * gamma[i] : xb[i];
    }
    __syncthreads();
    const int nchunks = hidden >> 9;
    float bv[kBatchMax];
    int bi[kBatchMax];
#pragma unroll
    for (int b = 0; b < kBatchMax; ++b) bv[b] = -INFINITY, bi[b] = 0x7fffffff;
    const int total_waves = gridDim.x * 4;
    for (int row = (blockIdx.x * 4 + wave) * R; row < vocab; row += total_waves * R) {
        h8 w[R][NCH];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const _Float16 *e = table + (size_t)(row + r < vocab ? row + r : vocab - 1) * hidden + 8 * lane;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (!GUARD || c < nchunks)
                    w[r][c] = __builtin_nontemporal_load(reinterpret_cast<const h8 *>(e + 512 * c));
                else
                    w[r][c] = (h8)(_Float16)0.0f;
            }
        }
#pragma unroll
        for (int b = 0; b < kBatchMax; ++b) {
            if (b >= n_seq) break;
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                float xr[8];
                if (!GUARD || c < nchunks) {
                    const float4 lo = *reinterpret_cast<const float4 *>(xs + (size_t)b * hidden + 512 * c + 8 * lane);
                    const float4 hi = *reinterpret_cast<const float4 *>(xs + (size_t)b * hidden + 512 * c + 8 * lane + 4);
                    xr[0] = lo.x, xr[1] = lo.y, xr[2] = lo.z, xr[3] = lo.w, xr[4] = hi.x, xr[5] = hi.y, xr[6] = hi.z, xr[7] = hi.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) xr[i] = 0.0f;
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[r] = fmaf(xr[i], (float)w[r][c][i], acc[r]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
            float *lg = logits_ptrs[b];
            if (lane == 0 && lg) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (row + r < vocab) {
                        lg[row + r] = acc[r];
                        const float v = acc[r] != acc[r] ? -INFINITY : acc[r];  // NaN -> -inf
                        if (v > bv[b] || (v == bv[b] && row + r < bi[b])) {
                            bv[b] = v;
                            bi[b] = row + r;
                        }
                    }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < kBatchMax; ++b) {
            wbv[b][wave] = bv[b];
            wbi[b][wave] = bi[b];
        }
    }
    __syncthreads();
    if (tid < n_seq) {
        float v = wbv[tid][0];
        int ix = wbi[tid][0];
        for (int w2 = 1; w2 < 4; ++w2)
            if (wbv[tid][w2] > v || (wbv[tid][w2] == v && wbi[tid][w2] < ix)) {
                v = wbv[tid][w2];
                ix = wbi[tid][w2];
            }
        best_val[(size_t)tid * gridDim.x + blockIdx.x] = v;
        best_idx[(size_t)tid * gridDim.x + blockIdx.x] = ix;
    }
}

// k_argmax_final per slot (grid = n_seq): the pick, history at p + 1 unless forced, the position.  A slot with neither a token nor a position
// pointer (logits only: it samples) and an idle slot (no logits pointer) are left alone.
__global__ __launch_bounds__(256) void k_argmax_final_batch(const float *__restrict__ best_val, const int *__restrict__ best_idx, int n,
                                                            float *const *__restrict__ logits_ptrs, int *const *__restrict__ token_ptrs,
                                                            int *const *__restrict__ pos_ptrs, int *const *__restrict__ history_ptrs,
                                                            const int *const *__restrict__ n_forced_ptrs) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int b = blockIdx.x;
    int *token_out = token_ptrs ? token_ptrs[b] : nullptr;
    int *pos_ptr = pos_ptrs ? pos_ptrs[b] : nullptr;
    if (!logits_ptrs[b] || (!token_out && !pos_ptr)) return;  // block-uniform
    best_val += (size_t)b * n;
    best_idx += (size_t)b * n;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = best_val[i];
        const int idx = best_idx[i];
        if (v > bv || (v == bv && idx < bi)) {
            bv = v;
            bi = idx;
        }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float v = sv[threadIdx.x + off];
            const int idx = si[threadIdx.x + off];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && idx < si[threadIdx.x])) {
                sv[threadIdx.x] = v;
                si[threadIdx.x] = idx;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int tok = si[0] == 0x7fffffff ? 0 : si[0];
        if (token_out) *token_out = tok;
        if (pos_ptr) {
            const int p = *pos_ptr;
            int *history = history_ptrs ? history_ptrs[b] : nullptr;
            const int *n_forced = n_forced_ptrs ? n_forced_ptrs[b] : nullptr;
            if (history && (!n_forced || p + 1 >= *n_forced)) history[p + 1] = tok;
            *pos_ptr = p + 1;
        }
    }
}

}  // namespace

hipError_t launch_embed_q_batch(const void *table, const int *const *history_ptrs, const int *const *pos_ptrs, int n_seq, int hidden, int vocab,
                                float *x_out, const float *gamma, void *qout, double *stats, hipStream_t stream) {
    if (hidden <= 0 || hidden % 16 != 0 || n_seq < 1 || n_seq > kBatchMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_embed_q_batch, dim3((unsigned)div_ceil((size_t)hidden, 256), (unsigned)n_seq), dim3(256), 0, stream,
                       static_cast<const _Float16 *>(table), history_ptrs, pos_ptrs, hidden, vocab, x_out, gamma, static_cast<uint8_t *>(qout),
                       (uint32_t)qact_bytes((size_t)hidden), stats);
    return hipGetLastError();
}

static int gemv_batch_nb(int n_seq) { return n_seq <= 2 ? 2 : n_seq <= 4 ? 4 : 8; }  // the instantiated vector count NB

size_t gemv_q_batch_lds_bytes(const Weights &w, const GemvGeom &g, bool ln, int n_seq) {
    return (size_t)g.ring_t * kQRec + (size_t)n_seq * kQRec * g.nblk + (ln ? (size_t)n_seq * (w.cols / 16) * 16 : 0) +
           (size_t)gemv_batch_nb(n_seq) * 8 * 16 * sizeof(float);
}

hipError_t launch_gemv_q_batch(const Weights &w, const GemvQIo &io, int n_seq, hipStream_t stream) {
    if (!w.tiles || !gemvq_supported(w) || !io.qin || io.attn_rec || n_seq < 1 || n_seq > kBatchMax) return hipErrorInvalidValue;
    const int nw = 8;
    const GemvGeom g = gemv_geometry(w, io.silu_mul, nw);  // batch-1's K partition
    GemvQBatchArgs a;
    const hipError_t ef = fill_gemv_q_prefix(a, w, io, g);
    if (ef != hipSuccess) return ef;
    a.n_seq = n_seq;
    a.out_rows = (int)(io.silu_mul ? w.rows / 2 : w.rows);
    a.qbytes = (uint32_t)kQRec * (uint32_t)a.nblk;
    a.qout_bytes = (uint32_t)qact_bytes((size_t)a.out_rows);
    const bool ln = io.ln_gamma != nullptr;
    const int ring = g.ring, sc = g.sc, nb = gemv_batch_nb(n_seq);
    if (ring > 5 || (ln && a.n_stats > 256)) return hipErrorInvalidValue;
    const size_t lds = gemv_q_batch_lds_bytes(w, g, ln, n_seq);
    if (lds > (size_t)kGemvBatchLdsMax) return hipErrorInvalidValue;
    void (*kfn)(GemvQBatchArgs) = nullptr;
#define BH_BPICK3(RINGv, NBv)                                                                                                                        \
    if (!kfn && ring <= RINGv && nb == NBv)                                                                                                          \
        kfn = ln ? (sc == 2 ? k_gemv_q_batch<RINGv, 2, 1, NBv> : sc == 1 ? k_gemv_q_batch<RINGv, 1, 1, NBv> : k_gemv_q_batch<RINGv, 0, 1, NBv>)      \
                 : (sc == 2 ? k_gemv_q_batch<RINGv, 2, 0, NBv> : sc == 1 ? k_gemv_q_batch<RINGv, 1, 0, NBv> : k_gemv_q_batch<RINGv, 0, 0, NBv>);
#define BH_BPICK(RINGv) BH_BPICK3(RINGv, 2) BH_BPICK3(RINGv, 4) BH_BPICK3(RINGv, 8)
    BH_BPICK(2) BH_BPICK(3) BH_BPICK(4) BH_BPICK(5)
#undef BH_BPICK
#undef BH_BPICK3
    if (!kfn) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        const hipError_t e = raise_dynamic_lds(kfn, kGemvBatchLdsMax);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kfn, dim3(g.grid), dim3(nw * 64), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_logits_f16_batch(const void *table, const float *x, const float *gamma, float eps, int hidden, int vocab, int n_seq,
                                   float *const *logits_ptrs, float *best_val, int *best_idx, int n_wg, int *const *token_ptrs, int *const *pos_ptrs,
                                   int *const *history_ptrs, const int *const *n_forced_ptrs, hipStream_t stream) {
    if (n_seq < 1 || n_seq > kBatchMax) return hipErrorInvalidValue;
    const LogitsInstance li = logits_instance(hidden, 4);  // launch_logits_f16's instance, hence its padding; R is free: it does not enter a row's arithmetic
    void (*kfn)(const _Float16 *, const float *, const float *, float, int, int, int, float *const *, float *, int *) = nullptr;
#define BH_LBPICK(NCHv, Rv, Gv) \
    if (li.nch == NCHv && li.r == Rv && li.guard == Gv) kfn = k_logits_f16_batch<NCHv, Rv, Gv>;
    BH_LBPICK(1, 4, false) BH_LBPICK(2, 4, false) BH_LBPICK(4, 4, false) BH_LBPICK(5, 4, false) BH_LBPICK(8, 2, false) BH_LBPICK(8, 2, true) BH_LBPICK(16, 1, true)
#undef BH_LBPICK
    if (!kfn) return hipErrorInvalidValue;
    const size_t lds = (size_t)n_seq * hidden * sizeof(float);
    constexpr int kLdsMax = 152 * 1024;  // beside the kernel's static arrays
    if (lds > (size_t)kLdsMax) return hipErrorInvalidValue;  // 8 vectors of more than 4864 columns: take them in two calls
    if (lds > 64 * 1024) {
        const hipError_t e = raise_dynamic_lds(kfn, kLdsMax);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kfn, dim3(n_wg), dim3(256), lds, stream, static_cast<const _Float16 *>(table), x, gamma, eps, hidden, vocab, n_seq, logits_ptrs,
                       best_val, best_idx);
    if (token_ptrs || pos_ptrs)
        hipLaunchKernelGGL(k_argmax_final_batch, dim3(n_seq), dim3(256), 0, stream, best_val, best_idx, n_wg, logits_ptrs, token_ptrs, pos_ptrs, history_ptrs,
                           n_forced_ptrs);
    return hipGetLastError();
}

}  // namespace bitnet_hip
