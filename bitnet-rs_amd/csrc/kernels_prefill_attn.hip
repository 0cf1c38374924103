// kernels_prefill_attn.hip -- causal self-attention over a whole prompt (prefill) on gfx950.
//
// The reference runs the same per-head softmax(Q K^T / sqrt(d) + causal mask) V for a
// [T]-token forward (T:410-533) with RoPE applied to q and k (T:134-163) and k, v appended
// to the cache (T:1171-1202).  Here, for a FRESH sequence (positions 0..T-1):
//
//   k_prefill_prep  grid (T/64, heads + 2*kv_heads): one 64-token x 128-dim slab of q, k or v
//                   through LDS: RoPE (q, k); q -> f16 [head][T][128], pre-multiplied by the softmax
//                   scale and log2(e); k -> f16 [kv][T][128] and the decode cache (f32 transposed
//                   [kv][128][max_pos], or the f16 cache layout); v -> f16 transposed [kv][128][T]
//                   with the keys of every 32-group in MFMA-operand order, and the decode cache.
//                   Every global access is contiguous along the fastest index.
//   k_prefill_attn  4 waves = (heads of one KV head) x (wave columns of 32 queries), two workgroups per
//                   CU: flash attention on v_mfma_f32_16x16x32_f16, f32 accumulation, f32 online
//                   softmax in base 2.  K / V^T tiles arrive by LDS-DMA into unpadded XOR-swizzled
//                   double buffers; operand reads run two chunks ahead through a register ring.
//                   It works on S^T = K Q^T and O^T = V^T P^T so that the probabilities never
//                   leave registers: an S^T accumulator (lane: query c, keys 4g..4g+3) is
//                   already in B-operand form for the second product once the V^T operand
//                   uses the same key -> k-slot map.
//   k_prefill_merge combines the key-split partials of launches too small to fill the chip.
// A LIVE sequence (seq_len new tokens at positions past_len .. over a cache holding 0 .. past_len - 1: the reference's seq_len queries
// over past_len + seq_len keys, T:455-470, T:704-719, append T:1171-1202) runs the same attention kernel behind
//   k_extend_prep   which builds the k / v images from the decode cache (past) and the new rows (appended); see launch_attn_extend.
// q, k, v and the probabilities are rounded to f16 for the matrix cores (relative 2^-11);
// the f32 KV cache the decode steps read afterwards holds the exact f32 values.
#include <cstdlib>

#include "common.hpp"
#include "wave.hpp"

namespace bitnet_hip {

constexpr int kPD = 128;       // head dim
constexpr int kQB = 64;        // keys per tile; query rows come in 64-row blocks (q_block_pos)
constexpr int kQPad = 128;     // query rows are padded to this (the largest workgroup query tile)
constexpr int kKTile = kQB * kPD * 2;   // one K tile in LDS: 64 keys x 256 bytes, unpadded; 16-byte unit u of key r sits at u ^ (r & 15)
constexpr int kVTile = kPD * kQB * 2;   // one V^T tile: 128 dims x 128 bytes (keys in operand order, k_prefill_prep); unit u of dim r sits at u ^ ((r >> 1) & 7)
constexpr int kKVBuf = kKTile + kVTile; // the kernel keeps two (tile t + 1 lands while tile t is multiplied)
constexpr int kTilesPerSplit = 16;  // key split (PrefillArgs::ksplit): key tiles one workgroup walks at least before a block is cut

struct PrefillArgs {
    // element (head h, row t, dim d) of q / k / v sits at base + h * hs + t * ld + d
    const float *q, *k, *v;
    int ld_q, ld_kv;        // row strides (floats)
    int hs_q, hs_kv;        // head strides (floats): 128 for [row][head][dim] rows, rows*128 for [head][row][dim]
    int out_hs, out_ld;     // output element (h, t, d) at out + h * out_hs + t * out_ld + d
    int rope, causal;       // apply RoPE to q and k here / causal mask
    float scale;            // softmax scale (1/sqrt(d) in the transformer)
    const int *q_block_pos;  // absolute position of each 64-query block (null: block b starts at 64 b)
    int nq, nq_pad;          // query rows held here (token-parallel prefill: a subset of the prompt)
    const float *rope_sin, *rope_cos;
    float *kcache, *vcache;
    int n_heads, n_kv, max_pos, T, Tpad;  // T = context tokens (keys)
    _Float16 *qh, *kh, *vt;  // workspace: q [head][nq_pad][128], k [kv][Tpad][128], v^T [kv][128][Tpad]
    float *out;              // [nq, heads * 128]
    // token-parallel prefill: the k|v rows as the all-gather left them, [rank][that rank's two zigzag chunks] -- the row
    // of absolute position t is found here instead of by a scatter pass on the host side.  zz_world == 0: absolute order.
    int zz_world, zz_chunk;  // ranks, tokens per chunk (T = 2 * world * chunk; chunk % 64 == 0)
    int kv_f16;              // the k|v rows travelled as f16 (half the bytes on the wire); k / v then point at _Float16
    int cache_f16;           // the decode caches hold f16 (kernels_attn.hip KV16 layout)
    int head_fast;           // grid = (head groups, query groups): the dispatch order walks ALL heads' longest blocks first (see launch_attn_kernel)
    int out_f16;             // `out` holds _Float16 (same element strides): the o-projection's f16 chain reads it as it is (kernels_gemm.hip k_gemm_f16a)
    // key split: the key tiles of a query block are dealt to `ksplit` workgroups (blockIdx.z), each leaving an un-normalised partial
    // (o, m, l) that k_prefill_merge combines -- for launches whose query blocks alone would not fill the chip (one rank's 1024
    // queries x 8192 keys of the 8-GPU prefill are 160 workgroups with up to 128 key tiles each; a 1024-token prompt likewise)
    int phase;               // 0: prepare q, k, v and attend; 1: the query slabs only (needs no k|v: runs beside the all-gather);
                             // 2: the k / v slabs and the attention (the query slabs were prepared by a phase-1 call on the same workspace)
    int ksplit;
    int split_tiles;         // key tiles one workgroup walks at least before a query block is cut (attn_split_tiles)
    int slot0;               // k_prefill_prep: first slot of its grid (n_heads: the query slabs are prepared by k_prefill_attn itself)
    int q_in_kernel;         // k_prefill_attn reads the f32 query rows itself (RoPE, scale, f16) instead of the f16 image k_prefill_prep left
    float *part_o;           // [ksplit][nq_pad][heads][128]
    float *part_ml;          // [ksplit][nq_pad][heads][2]  (running maximum in base-2 units, sum)
};

// row of absolute position t (a multiple of 64) in the gathered k|v buffer: chunk c = t / chunk belongs to rank c (first
// half of the chunks) or 2 world - 1 - c (second half), as that rank's first or second chunk
__device__ __forceinline__ int zz_row(const PrefillArgs &p, int t) {
    if (p.zz_world == 0) return t;
    const int c = t / p.zz_chunk, off = t - c * p.zz_chunk;
    const bool first = c < p.zz_world;
    const int r = first ? c : 2 * p.zz_world - 1 - c;
    return r * 2 * p.zz_chunk + (first ? 0 : p.zz_chunk) + off;
}

// split-half RoPE (crates/bitnet-rope/src/lib.rs:59-93, T:134-163) of 4 adjacent pairs (j .. j + 3, 64 + j ..) of one row of a staged slab, at position pos
__device__ __forceinline__ void rope_rotate4(float (*tile)[kPD + 4], int tok, int j, const float *rope_sin, const float *rope_cos, int pos) {
    const float4 s = *reinterpret_cast<const float4 *>(rope_sin + (size_t)pos * 64 + j), c = *reinterpret_cast<const float4 *>(rope_cos + (size_t)pos * 64 + j);
    const float4 x0 = *reinterpret_cast<const float4 *>(&tile[tok][j]), x1 = *reinterpret_cast<const float4 *>(&tile[tok][64 + j]);
    *reinterpret_cast<float4 *>(&tile[tok][j]) = float4{x0.x * c.x - x1.x * s.x, x0.y * c.y - x1.y * s.y, x0.z * c.z - x1.z * s.z, x0.w * c.w - x1.w * s.w};
    *reinterpret_cast<float4 *>(&tile[tok][64 + j]) = float4{x0.x * s.x + x1.x * c.x, x0.y * s.y + x1.y * c.y, x0.z * s.z + x1.z * c.z, x0.w * s.w + x1.w * c.w};
}

// grid (max(nq_pad, Tpad) / 64, heads + 2 kv): slot < heads: query head (rows of p.q, positions from
// q_block_pos); then k heads, then v heads (rows of p.kv, position = row).
__global__ __launch_bounds__(256) void k_prefill_prep(PrefillArgs p) {
    // one 64-token x 128-dim slab through LDS; every global access is 16 bytes wide (8 for f16 rows) and contiguous along the
    // fastest index of its tensor (the scalar version of this kernel took 48 us per layer for 115 MB of traffic)
    __shared__ __attribute__((aligned(16))) float tile[kQB][kPD + 4];  // + 4: float4 rows stay 16-byte aligned, columns spread over the banks
    const int slot = blockIdx.y + p.slot0, t0 = blockIdx.x * kQB, tid = threadIdx.x;
    const bool is_q = slot < p.n_heads, is_k = !is_q && slot < p.n_heads + p.n_kv;
    if ((p.phase == 1 && !is_q) || (p.phase == 2 && is_q)) return;
    const int n_rows = is_q ? p.nq : p.T;
    if (t0 >= (is_q ? p.nq_pad : p.Tpad)) return;
    const float *src = is_q ? p.q + (size_t)slot * p.hs_q
                     : is_k ? p.k + (size_t)(slot - p.n_heads) * p.hs_kv : p.v + (size_t)(slot - p.n_heads - p.n_kv) * p.hs_kv;
    const int ld = is_q ? p.ld_q : p.ld_kv;
    // absolute position of row t0 (padding blocks past the last real one hold zeros: any position will do)
    const int pos0 = is_q && p.q_block_pos ? ((int)blockIdx.x < (p.nq + kQB - 1) / kQB ? p.q_block_pos[blockIdx.x] : 0) : t0;
    const int r0 = is_q ? t0 : zz_row(p, t0);  // a 64-row block of positions is 64 consecutive gathered rows (chunk % 64 == 0)
    const bool vec_ok = (ld & 3) == 0 && ((uintptr_t)src & 15) == 0;  // rows 16-byte aligned (always, for the decoder's buffers)
    if (!is_q && p.kv_f16) {
        const _Float16 *sh = reinterpret_cast<const _Float16 *>(p.k) + (size_t)(slot - p.n_heads) * p.hs_kv;  // k heads then v heads
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (t0 + tok < n_rows) {
                const _Float16 *e = sh + (size_t)(r0 + tok) * ld + d;
                v = float4{(float)e[0], (float)e[1], (float)e[2], (float)e[3]};
            }
            *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
        }
    } else {
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (t0 + tok < n_rows) {
                const float *e = src + (size_t)(r0 + tok) * ld + d;
                v = vec_ok ? *reinterpret_cast<const float4 *>(e) : float4{e[0], e[1], e[2], e[3]};
            }
            *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
        }
    }
    __syncthreads();
    if ((is_q || is_k) && p.rope) {
        // split-half RoPE (crates/bitnet-rope/src/lib.rs:59-93, T:134-163): pairs (j, j + 64); a thread takes 4 adjacent pairs
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 4, j = (idx & 15) * 4;
            const int pos = t0 + tok < n_rows ? pos0 + tok : 0;
            rope_rotate4(tile, tok, j, p.rope_sin, p.rope_cos, pos);
        }
        __syncthreads();
    }
    // the softmax scale (and the change to base 2) rides in the f16 image of q: one multiply per query element here instead of
    // one per score in every key tile
    const float qmul = is_q ? 1.4426950408889634f * p.scale : 1.0f;
    auto store_rows_f16 = [&](_Float16 *dst) {  // [64 tokens][128] halves, contiguous: 8 bytes per thread and iteration
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
            const float4 v = *reinterpret_cast<const float4 *>(&tile[tok][d]);
            const h4 h = {(_Float16)(v.x * qmul), (_Float16)(v.y * qmul), (_Float16)(v.z * qmul), (_Float16)(v.w * qmul)};
            *reinterpret_cast<h4 *>(dst + (size_t)tok * kPD + d) = h;
        }
    };
    if (is_q) {
        store_rows_f16(p.qh + ((size_t)slot * p.nq_pad + t0) * kPD);
    } else if (is_k) {
        const int kvh = slot - p.n_heads;
        store_rows_f16(p.kh + ((size_t)kvh * p.Tpad + t0) * kPD);
        // decode cache: K transposed in 64-position tiles [chunk][128][64] (kernels_attn.hip); t0 is a tile start
        const size_t head_floats = (size_t)((p.max_pos + 63) / 64) * 64 * kPD;
        float *kt = p.kcache + (size_t)kvh * head_floats + (size_t)(t0 >> 6) * kPD * 64;
        if (p.cache_f16) {  // [chunk][D / 2][64][2] halves
            _Float16 *k16 = reinterpret_cast<_Float16 *>(p.kcache) + (size_t)kvh * head_floats + (size_t)(t0 >> 6) * kPD * 64;
            for (int i = 0; i < 32 && p.kcache; ++i) {
                const int idx = tid + 256 * i, d = idx >> 6, tok = idx & 63;
                if (t0 + tok < p.T) k16[((size_t)(d >> 1) * 64 + tok) * 2 + (d & 1)] = (_Float16)tile[tok][d];
            }
        } else {
            for (int i = 0; i < 8 && p.kcache; ++i) {  // 4 adjacent positions of one dim: 16 contiguous bytes
                const int idx = tid + 256 * i, d = idx >> 4, tok = (idx & 15) * 4;
                if (t0 + tok + 3 < p.T) {
                    *reinterpret_cast<float4 *>(kt + (size_t)d * 64 + tok) = float4{tile[tok][d], tile[tok + 1][d], tile[tok + 2][d], tile[tok + 3][d]};
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (t0 + tok + e < p.T) kt[(size_t)d * 64 + tok + e] = tile[tok + e][d];
                }
            }
        }
    } else {
        const int kvh = slot - p.n_heads - p.n_kv;
        float *vc = p.vcache + (size_t)kvh * ((size_t)((p.max_pos + 63) / 64) * 64 * kPD);  // [max_pos][128]
        if (p.cache_f16) {
            _Float16 *v16 = reinterpret_cast<_Float16 *>(p.vcache) + (size_t)kvh * ((size_t)((p.max_pos + 63) / 64) * 64 * kPD);
            for (int i = 0; i < 32 && p.vcache; ++i) {
                const int idx = tid + 256 * i, tok = idx >> 7, d = idx & 127;
                if (t0 + tok < p.T) v16[(size_t)(t0 + tok) * kPD + d] = (_Float16)tile[tok][d];
            }
        } else {
            for (int i = 0; i < 8 && p.vcache; ++i) {
                const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
                if (t0 + tok < p.T) *reinterpret_cast<float4 *>(vc + (size_t)(t0 + tok) * kPD + d) = *reinterpret_cast<const float4 *>(&tile[tok][d]);
            }
        }
        // [128][Tpad], the keys of every group of 32 in the order the second product's operand wants them: key 4 a + 16 b + j
        // (a < 4, b < 2, j < 4) at slot 8 a + 4 b + j, so that a lane's 8 k-slots (keys 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3: the
        // S^T accumulator layout) are ONE 16-byte unit.  4 adjacent positions of one dim = 8 contiguous bytes here as well.
        _Float16 *vt = p.vt + (size_t)kvh * kPD * p.Tpad;
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, d = idx >> 4, t4 = idx & 15, tok = t4 * 4;
            const int slot = 32 * (t4 >> 3) + 8 * (t4 & 3) + 4 * ((t4 >> 2) & 1);
            const h4 h = {(_Float16)tile[tok][d], (_Float16)tile[tok + 1][d], (_Float16)tile[tok + 2][d], (_Float16)tile[tok + 3][d]};
            *reinterpret_cast<h4 *>(vt + (size_t)d * p.Tpad + t0 + slot) = h;
        }
    }
}

// NW waves per workgroup = HW query heads of ONE KV head x (NW / HW) wave columns; a wave owns NQ groups of 16 queries of its
// head.  All waves multiply the same K / V^T tiles, staged into LDS once per workgroup.
// Every MFMA takes its A operand (16 keys x 32 dims = 1 KiB per wave) from LDS, and those reads are what bounds this kernel
// (ablation, 4096 tokens: 238 us; without the operand reads 137; without softmax arithmetic 218; without tile staging 205;
// MFMAs alone ~100): with ONE query group per wave the reads need 64 B/clk per SIMD of a CU's 128 B/clk.  NQ = 2 lets two
// query groups share each operand read.  That takes ~240 registers, so the GQA form runs 4-wave workgroups (4 heads x 32
// queries) with a launch bound of two waves per SIMD: TWO workgroups per CU with independent barriers (one in its softmax
// while the other multiplies).  The next key tile is requested into registers one iteration ahead and the LDS operand reads
// are pinned one chunk ahead of their MFMAs (hipcc's own schedule waited for every read right before its MFMAs).

// max of three without the v_max(x, x) canonicalisation hipcc puts in front of every fmaxf of an MFMA result (no NaNs here)
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// max over the four lanes (c, g = 0..3) that hold one query's keys, in every lane, on the VALU: v_permlane16_swap / v_permlane32_swap
// (gfx950) instead of two dependent ds_bpermute round trips through the LDS pipe per query group and key tile.  With both operands
// the same register, permlane16_swap leaves (rows 0, 0, 2, 2) and (rows 1, 1, 3, 3) of 16 lanes, permlane32_swap (low half twice)
// and (high half twice): the maximum of each pair is the xor-16 / xor-32 butterfly step.
__device__ __forceinline__ float max_over_g(float v) {
    const unsigned u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float m1 = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned w = __float_as_uint(m1);
    const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// One body, two kernels: PK = false is k_prefill_attn (one sequence: block positions from q_block_pos, keys 0 .. p.T - 1 of the one image);
// PK = true is k_prefill_attn_packed, whose 64-row query blocks belong to DIFFERENT sequences: block b reads its record q_rec[b] =
// {absolute position of its first row, first key tile of its sequence inside the packed images, key count of its sequence, live rows}
// once, here in the prologue, and everything below the prologue is the same code (see launch_attn_packed).
template <int HW, int NW, int NQ, bool PK>
__device__ __forceinline__ void prefill_attn_body(const PrefillArgs &p, const int4 *q_rec) {
    constexpr int QW = NW / HW, QG = 16 * QW * NQ;  // wave columns per workgroup, queries per workgroup
    static_assert(NW == 4, "tile staging deals 32 pieces to 4 waves");
    extern __shared__ __attribute__((aligned(16))) uint8_t kv_lds[];  // [2][K tile | V^T tile]
    __shared__ int s_last;
    const int qg = p.head_fast ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)gridDim.x - 1 - (int)blockIdx.x;  // long (late) blocks first
    const int hg = p.head_fast ? blockIdx.x : blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 15, g = lane >> 4;
    const int h = hg * HW + wave % HW, kvh = h / (p.n_heads / p.n_kv);  // HW divides the group: one KV head per workgroup
    const int qbase = qg * QG + (wave / HW) * 16 * NQ;            // first query row of this wave (16 NQ rows inside one 64-row block)
    const int blk64 = qbase >> 6;                                 // the 64-row block the wave's rows lie in
    int4 rec = {0, 0, 0, 0};
    if (PK) rec = q_rec[blk64];  // (every block up to nq_pad / 64 has a record)
    const int bpos = (PK ? rec.x : p.q_block_pos ? p.q_block_pos[blk64 < (p.nq + kQB - 1) / kQB ? blk64 : 0] : blk64 * kQB) + (qbase & 63);
    const int T = PK ? __builtin_amdgcn_readfirstlane(rec.z) : p.T;  // keys of this block's sequence
    const int q_live = PK ? __builtin_amdgcn_readfirstlane(rec.w) - (qbase & 63) : 0;  // packed: rows of the wave that belong to a sequence (the rest is padding)
    if (tid == 0) s_last = 0;
    __syncthreads();
    {   // last key tile any query of the workgroup sees
        const int top = bpos + 16 * NQ - 1;
        const int need = p.causal ? (top < T ? top : T - 1) / kQB : (T - 1) / kQB;
        if (lane == 0) atomicMax(&s_last, need);
    }
    __syncthreads();
    int kt_first = 0, kt_last = s_last;
    if (p.ksplit > 1) {
        // this workgroup's share of the key tiles: a query block with n tiles is cut into ceil(n / kTilesPerSplit) parts (at most
        // ksplit), so early blocks (few tiles) stay whole and late ones spread over the chip; surplus workgroups only mark their
        // partial empty (m = -inf), which the merge skips
        const int n_t = kt_last + 1;
        int parts = (n_t + p.split_tiles - 1) / p.split_tiles;
        parts = parts < p.ksplit ? parts : p.ksplit;
        if ((int)blockIdx.z >= parts) {
            if (g == 0) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const size_t ro = ((size_t)blockIdx.z * p.nq_pad + qbase + 16 * q + c) * p.n_heads + h;
                    *reinterpret_cast<float2 *>(p.part_ml + ro * 2) = float2{-INFINITY, 0.0f};
                }
            }
            return;
        }
        const int per = (n_t + parts - 1) / parts;
        kt_first = (int)blockIdx.z * per;
        kt_last = kt_first + per - 1 < kt_last ? kt_first + per - 1 : kt_last;
    }
    int qlim[NQ];  // highest visible key position of this lane's query in group q
#pragma unroll
    for (int q = 0; q < NQ; ++q) qlim[q] = p.causal ? bpos + 16 * q + c : T - 1;
    // Q^T operands: 8 consecutive dims per k-slot group, kept in registers for the whole block (filled below, behind the first tile requests)
    h8 qreg[NQ][4];
    v4f o[NQ][8];
    float m_run[NQ], l_run[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[q][dt] = (v4f){0.f, 0.f, 0.f, 0.f};
        m_run[q] = -INFINITY;
        l_run[q] = 0.0f;
    }
    // softmax in base 2; the scale is already in q (k_prefill_prep)
    const int qmin = __builtin_amdgcn_readfirstlane(p.causal ? bpos : T - 1);  // lowest key limit of any query of this wave
    const size_t koff = PK ? (size_t)__builtin_amdgcn_readfirstlane(rec.y) : 0;  // packed: first key tile of the block's sequence in the images
    const uint8_t *kbase = reinterpret_cast<const uint8_t *>(p.kh + (size_t)kvh * p.Tpad * kPD) + koff * kKTile;
    const uint8_t *vbase = reinterpret_cast<const uint8_t *>(p.vt + (size_t)kvh * kPD * p.Tpad) + koff * (kQB * 2);
    // Tile staging by LDS-DMA: a K tile is 16 pieces of 1 KiB (4 keys), a V^T tile 16 pieces (8 dim rows x 128 B); wave w moves
    // pieces 4 w .. 4 w + 3 of each.  A lane fetches the 16-byte unit that belongs at ITS slot of the piece (the XOR swizzles
    // above), so the unpadded tiles read conflict-free.  Byte offsets from the tile's first byte (scalar base):
    unsigned ksrc[4], vsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = 4 * (4 * wave + i) + (lane >> 4), dim = 8 * (4 * wave + i) + (lane >> 3);
        ksrc[i] = (unsigned)(key * 256 + (((lane & 15) ^ (key & 15)) * 16));
        vsrc[i] = (unsigned)dim * (unsigned)(p.Tpad * 2) + (unsigned)((((lane & 7) ^ ((dim >> 1) & 7))) * 16);
    }
    const unsigned lds0 = (unsigned)(uintptr_t)kv_lds;
    auto stage_k = [&](int kt, int buf) {
        const uint8_t *src = kbase + (size_t)kt * kKTile;
        const unsigned dst = lds0 + (unsigned)buf * kKVBuf + (unsigned)(4 * wave) * 1024u;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma_1k(ksrc[i], src, dst + 1024u * i);
    };
    auto stage_v = [&](int kt, int buf) {
        const uint8_t *src = vbase + (size_t)kt * (kQB * 2);
        const unsigned dst = lds0 + (unsigned)buf * kKVBuf + kKTile + (unsigned)(4 * wave) * 1024u;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma_1k(vsrc[i], src, dst + 1024u * i);
    };
    // operand read offsets inside a tile (+ 4096 i per key tile of 16, + 2048 dt per dim tile of 16: immediates)
    const unsigned kro = (unsigned)(c * 256 + ((g ^ c) * 16));                               // ^ (64 ch): unit 4 ch + g of key c
    const unsigned vro = (unsigned)(c * 128 + ((g ^ (c >> 1)) * 16));                         // ^ (64 u): unit 4 u + g of dim c
    // The MFMA operands of a tile form one stream of 8 chunks (K dims 0-31 .. 96-127, then V^T (keys 0-31, dims 0-63), (0-31, 64-127),
    // (32-63, 0-63), (32-63, 64-127)), 4 operands of 1 KiB per wave each; chunk j's LDS reads are issued TWO chunks ahead of its
    // MFMAs, across the softmax and across the tile boundary (hipcc's own schedule waited for every read right before its MFMAs;
    // one chunk ahead still left the waves waiting: the reads' latency, not LDS bandwidth, was what the kernel stood on).
    h8 ring[4][4];
    auto kread = [&](int slot, int ch, const uint8_t *ks) {
        const uint8_t *kp = ks + (kro ^ (unsigned)(64 * ch));
#pragma unroll
        for (int i = 0; i < 4; ++i) ring[slot][i] = *reinterpret_cast<const h8 *>(kp + 4096 * i);
    };
    auto vread = [&](int slot, int st, const uint8_t *vs) {
        const uint8_t *vp = vs + (vro ^ (unsigned)(64 * (st >> 1))) + 2048 * 4 * (st & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) ring[slot][i] = *reinterpret_cast<const h8 *>(vp + 2048 * i);
    };
    // Staging: K and V^T tiles have separate double buffers and separate schedules, each requested a whole tile ahead of its first
    // read.  Two barriers per tile: B1 (before the K chunk 2 MFMAs = before the first V read of this tile is issued) waits for
    // V(kt) and requests V(kt + 1) into the buffer V(kt - 1) left (every wave is past chunk 1 of tile kt: done with tile kt - 1);
    // B2 (before the V chunk 2 MFMAs = before the first K read of the NEXT tile is issued) waits for K(kt + 1) and requests K(kt + 2)
    // into the buffer K(kt) left (its last read was issued two chunks ago and consumed by K chunk 3).  Loads return in order, so
    // "the 4 pieces requested last may still be in flight" is s_waitcnt vmcnt(4).
    stage_k(kt_first, 0);
    stage_v(kt_first, 0);
    if (kt_first < kt_last) stage_k(kt_first + 1, 1);
    // the query operands, requested BEHIND the first K / V^T tiles so that their round trip (strided f32 rows + the RoPE tables) overlaps the tiles'
    if (p.q_in_kernel) {
        // straight from the f32 rows of the q|k|v projection (round 4: two thirds of k_prefill_prep's traffic were the query slabs): a lane's
        // dims 32 ch + 8 g + i (ch < 4) hold both members of every rotation pair (d, d + 64) = (ch, ch + 2), so the split-half RoPE
        // (crates/bitnet-rope/src/lib.rs:59-93, T:134-163) needs no exchange; the same arithmetic as k_prefill_prep, the softmax scale and the
        // change to base 2 folded into the f16 image.  Rows past the last query are zeros.  Every load is unconditional (clamped row).
        const float qmul = 1.4426950408889634f * p.scale;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int row = qbase + 16 * q + c;
            const bool live = PK ? 16 * q + c < q_live : row < p.nq;
            const float *qp = p.q + (size_t)h * p.hs_q + (size_t)(live ? row : 0) * p.ld_q + 8 * g;
            float x[4][8];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const float4 a = *reinterpret_cast<const float4 *>(qp + 32 * ch), b = *reinterpret_cast<const float4 *>(qp + 32 * ch + 4);
                x[ch][0] = a.x, x[ch][1] = a.y, x[ch][2] = a.z, x[ch][3] = a.w, x[ch][4] = b.x, x[ch][5] = b.y, x[ch][6] = b.z, x[ch][7] = b.w;
            }
            if (p.rope) {
                const int pos = live ? bpos + 16 * q + c : 0;
                const float *sp = p.rope_sin + (size_t)pos * 64 + 8 * g, *cp = p.rope_cos + (size_t)pos * 64 + 8 * g;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const float4 s0 = *reinterpret_cast<const float4 *>(sp + 32 * ch), s1 = *reinterpret_cast<const float4 *>(sp + 32 * ch + 4);
                    const float4 c0 = *reinterpret_cast<const float4 *>(cp + 32 * ch), c1 = *reinterpret_cast<const float4 *>(cp + 32 * ch + 4);
                    const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float x0 = x[ch][i], x1 = x[ch + 2][i];
                        x[ch][i] = x0 * cs[i] - x1 * sn[i];
                        x[ch + 2][i] = x0 * sn[i] + x1 * cs[i];
                    }
                }
            }
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int i = 0; i < 8; ++i) qreg[q][ch][i] = live ? (_Float16)(x[ch][i] * qmul) : (_Float16)0.0f;
        }
    } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const _Float16 *qp = p.qh + ((size_t)h * p.nq_pad + qbase + 16 * q + c) * kPD + 8 * g;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) qreg[q][ch] = *reinterpret_cast<const h8 *>(qp + 32 * ch);
        }
    }
    // the builtin form, so that hipcc's own bookkeeping sees its q loads retired here: left to itself it re-waits for them with
    // s_waitcnt vmcnt(0..7) in front of the MFMAs of EVERY iteration -- which, in hardware, waits for the tile requests it cannot see
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    asm volatile("" ::: "memory");
    __syncthreads();
    kread(0, 0, kv_lds);
    kread(1, 1, kv_lds);

    for (int kt = kt_first; kt <= kt_last; ++kt) {
        const int par = (kt - kt_first) & 1;
        const uint8_t *ks = kv_lds + par * kKVBuf, *vs = ks + kKTile, *ks_next = kv_lds + (par ^ 1) * kKVBuf;
        const bool more = kt < kt_last;  // workgroup-uniform
        // ---- S^T = K Q^T - m: 4 key tiles of 16, reduced over 4 dim chunks of 32; one operand read per NQ MFMAs.  The accumulators
        // start at minus the running reference point, so the common tile (reference unchanged) exponentiates them as they are ----
        v4f s[NQ][4];
        float m_init[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            m_init[q] = m_run[q] < -1.0e30f ? 0.0f : m_run[q];  // no reference yet (first tile, or only masked keys so far)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[q][i] = (v4f){-m_init[q], -m_init[q], -m_init[q], -m_init[q]};
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch == 2) {  // B1
                if (more)
                    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (more) stage_v(kt + 1, par ^ 1);
            }
            if (ch < 2)
                kread((ch + 2) & 3, ch + 2, ks);
            else
                vread((ch + 2) & 3, ch - 2, vs);
            __builtin_amdgcn_sched_barrier(0);  // the reads above stay above these MFMAs
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[ch][i], qreg[q][ch], s[q][i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- online softmax for query column c of each group (keys of this lane: 16 i + 4 g + j) ----
        // Only tiles that reach past some query's limit are masked (the diagonal ones, and the context's last): wave-uniform.
        const bool need_mask = kt * kQB + kQB - 1 > qmin;
        h8 pb[NQ][2];
        // The query groups' softmax chains are independent: each stage below handles ALL groups in one basic block (one branch per
        // stage, not per group), so hipcc interleaves their dependent chains -- maximum, exponentials, sum -- instead of running
        // them one after the other.
        float mt[NQ];
        if (need_mask) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                mt[q] = -INFINITY;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int pos = kt * kQB + 16 * i + 4 * g + j;
                        const float v = pos <= qlim[q] ? s[q][i][j] : -INFINITY;  // causal mask (T:452-470) / end of the context
                        s[q][i][j] = v;
                        mt[q] = fmaxf(mt[q], v);
                    }
            }
        } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {  // two half-chains per group
                const float ma = max3_raw(max3_raw(max3_raw(s[q][0][0], s[q][0][1], s[q][0][2]), s[q][0][3], s[q][1][0]), s[q][1][1], s[q][1][2]);
                const float mb = max3_raw(max3_raw(max3_raw(s[q][2][0], s[q][2][1], s[q][2][2]), s[q][2][3], s[q][3][0]), s[q][3][1], s[q][3][2]);
                mt[q] = max3_raw(max3_raw(ma, mb, s[q][1][3]), s[q][3][3], -INFINITY);
            }
        }
        // mt is relative to the running reference.  The reference only moves when the maximum outgrows it by more than 2^8 (the
        // f16 probabilities then stay <= 256, the sums are f32): most tiles skip both the shift of the scores and the rescaling
        // of the 32 output accumulators.  A tile wholly above a query's limit (a later key split's first tile: its 64-row block
        // spans several query groups) leaves mt = -inf: the clamp keeps 2^(-inf - -inf) out and the reference stays "unset".
        bool unset[NQ], grow[NQ], any_grow = false;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            mt[q] = max_over_g(mt[q]);
            unset[q] = m_run[q] < -1.0e30f;
            grow[q] = mt[q] > 8.0f || unset[q];
            any_grow = any_grow || grow[q];
        }
        if (__any(any_grow)) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float shift = grow[q] ? fmaxf(mt[q], -3.0e38f) : 0.0f;
                const float m_new = unset[q] ? shift : m_run[q] + shift;
                const float alpha = __builtin_amdgcn_exp2f(m_run[q] - m_new);  // (no lane of the group grows: shift 0, alpha 1)
                l_run[q] *= alpha;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) o[q][dt] *= alpha;
                m_run[q] = m_new;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[q][i][j] -= shift;
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float ls[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s[q][i][j] = __builtin_amdgcn_exp2f(s[q][i][j]);
                ls[i] = (s[q][i][0] + s[q][i][1]) + (s[q][i][2] + s[q][i][3]);
            }
            l_run[q] += (ls[0] + ls[1]) + (ls[2] + ls[3]);
            // P^T operand: k-slot (g, j) = key 32u + 4g + j (j < 4), 32u + 16 + 4g + (j - 4)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pb[q][u][j] = (_Float16)s[q][2 * u][j];
                    pb[q][u][4 + j] = (_Float16)s[q][2 * u + 1][j];
                }
        }
        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int st = 0; st < 4; ++st) {  // step = (u, half of the dim tiles)
            const int u = st >> 1, d0 = 4 * (st & 1);
            if (st == 2) {  // B2
                if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                __syncthreads();
                if (kt + 2 <= kt_last) stage_k(kt + 2, par);
            }
            if (st < 2)
                vread(st + 2, st + 2, vs);
            else if (more)
                kread(st - 2, st - 2, ks_next);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < NQ; ++q) o[q][d0 + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[st][i], pb[q][u], o[q][d0 + i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        float l = l_run[q];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const int qrow = qbase + 16 * q + c;
        if (p.ksplit > 1) {  // un-normalised partial; padding rows are written too (the merge never reads them)
            const size_t ro = ((size_t)blockIdx.z * p.nq_pad + qrow) * p.n_heads + h;
            float *op = p.part_o + ro * kPD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<float4 *>(op + 16 * dt) = float4{o[q][dt][0], o[q][dt][1], o[q][dt][2], o[q][dt][3]};
            if (g == 0) *reinterpret_cast<float2 *>(p.part_ml + ro * 2) = float2{m_run[q], l};
            continue;
        }
        if (qrow < p.nq) {
            const float inv = 1.0f / l;
            const size_t oo = (size_t)qrow * p.out_ld + (size_t)h * p.out_hs + 4 * g;
            if (p.out_f16) {
                _Float16 *oh = reinterpret_cast<_Float16 *>(p.out) + oo;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt)
                    *reinterpret_cast<h4 *>(oh + 16 * dt) = (h4){(_Float16)(o[q][dt][0] * inv), (_Float16)(o[q][dt][1] * inv), (_Float16)(o[q][dt][2] * inv), (_Float16)(o[q][dt][3] * inv)};
            } else {
                float *op = p.out + oo;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) {
                    const float4 v = {o[q][dt][0] * inv, o[q][dt][1] * inv, o[q][dt][2] * inv, o[q][dt][3] * inv};
                    *reinterpret_cast<float4 *>(op + 16 * dt) = v;
                }
            }
        }
    }
}

template <int HW, int NW, int NQ>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void k_prefill_attn(PrefillArgs p) {
    prefill_attn_body<HW, NW, NQ, false>(p, nullptr);
}
template <int HW, int NW, int NQ>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void k_prefill_attn_packed(PrefillArgs p, const int4 *q_rec) {
    prefill_attn_body<HW, NW, NQ, true>(p, q_rec);
}

// out[row][head][:] = sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s over the key splits; 32 threads (4 dims each) per (row, head)
__global__ __launch_bounds__(256) void k_prefill_merge(PrefillArgs p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int d4 = (int)(i & 31);
    const size_t rh = i >> 5;  // row * heads + head
    if (rh >= (size_t)p.nq * p.n_heads) return;
    const size_t row = rh / p.n_heads, h = rh - row * p.n_heads;
    const size_t stride = (size_t)p.nq_pad * p.n_heads;
    float M = -INFINITY;
    for (int s = 0; s < p.ksplit; ++s) M = fmaxf(M, p.part_ml[(s * stride + rh) * 2]);  // split 0 always holds key 0: finite
    float L = 0.0f;
    float4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.ksplit; ++s) {
        const float2 ml = *reinterpret_cast<const float2 *>(p.part_ml + (s * stride + rh) * 2);
        if (ml.x == -INFINITY) continue;  // a part this block did not need: nothing but the mark was written
        const float w = __builtin_amdgcn_exp2f(ml.x - M);
        const float4 o = *reinterpret_cast<const float4 *>(p.part_o + (s * stride + rh) * kPD + 4 * d4);
        L += w * ml.y;
        a.x += w * o.x, a.y += w * o.y, a.z += w * o.z, a.w += w * o.w;
    }
    const float inv = 1.0f / L;
    if (p.out_f16) {
        *reinterpret_cast<h4 *>(reinterpret_cast<_Float16 *>(p.out) + row * p.out_ld + h * p.out_hs + 4 * d4) = (h4){(_Float16)(a.x * inv), (_Float16)(a.y * inv), (_Float16)(a.z * inv), (_Float16)(a.w * inv)};
        return;
    }
    *reinterpret_cast<float4 *>(p.out + row * p.out_ld + h * p.out_hs + 4 * d4) = float4{a.x * inv, a.y * inv, a.z * inv, a.w * inv};
}

// Workgroup tile of k_prefill_attn for a head shape: 4 waves = hw query heads of ONE KV head x (4 / hw) wave columns of 32 queries, qg query rows
struct AttnTile {
    int hw, qg;
};
static AttnTile attn_tile(int n_heads, int n_kv) {
    const int group = n_heads / n_kv, hw = group % 4 == 0 ? 4 : group % 2 == 0 ? 2 : 1;
    return {hw, 16 * (4 / hw) * 2};
}

// key splits of a launch (grid.z): only when the query blocks alone leave CUs idle (fewer than two workgroups per CU), as many
// as the longest block has 16-tile parts, at most 8
static int attn_split_tiles() {
    static const int v = [] { const char *e = getenv("BITNET_HIP_ATTN_SPLIT_TILES"); const int x = e ? atoi(e) : kTilesPerSplit; return x < 1 ? 1 : x; }();
    return v;
}
static int attn_key_parts(int T) {
    const int tiles = (T + kQB - 1) / kQB, s = (tiles + attn_split_tiles() - 1) / attn_split_tiles();
    return s < 1 ? 1 : s > 8 ? 8 : s;
}
static int attn_ksplit(int n_heads, int n_kv, int nq_pad, int T) {
    const AttnTile t = attn_tile(n_heads, n_kv);
    const long n_wg = (long)(nq_pad / t.qg) * (n_heads / t.hw);
    return n_wg >= 512 ? 1 : attn_key_parts(T);
}
// k_prefill_attn reads the f32 query rows itself; a launcher adds its own alignment condition (PrefillArgs::q_in_kernel)
static bool attn_q_in_kernel() {
    static const bool v = !(getenv("BITNET_HIP_ATTN_Q_IN_KERNEL") && atoi(getenv("BITNET_HIP_ATTN_Q_IN_KERNEL")) == 0);
    return v;
}

// q_rec: the per-block records of a packed call (launch_attn_packed): the same grid on k_prefill_attn_packed, never key-split
static hipError_t launch_attn_kernel(const PrefillArgs &p, hipStream_t stream, const int4 *q_rec = nullptr) {
    // hw 4: 4 waves = the 4 heads of a KV head x 32 queries each, two such workgroups per CU; 2: 2 heads x 2 wave columns x 32 queries
    const AttnTile t = attn_tile(p.n_heads, p.n_kv);
    void (*ak)(PrefillArgs);
    void (*akp)(PrefillArgs, const int4 *);
    if (t.hw == 4)
        ak = k_prefill_attn<4, 4, 2>, akp = k_prefill_attn_packed<4, 4, 2>;
    else if (t.hw == 2)
        ak = k_prefill_attn<2, 4, 2>, akp = k_prefill_attn_packed<2, 4, 2>;
    else
        ak = k_prefill_attn<1, 4, 2>, akp = k_prefill_attn_packed<1, 4, 2>;
    dim3 grid((unsigned)(p.nq_pad / t.qg), (unsigned)(p.n_heads / t.hw), (unsigned)p.ksplit);
    // Workgroups are dispatched in linear id order (x fastest).  With the query groups in x, head group 0's blocks all start before head
    // group 1's first: on a causal prompt (640 workgroups for 512 slots at 4096 tokens x 20 heads) the LAST head group's longest blocks only
    // start once earlier groups' short ones have finished, and stand alone at the end.  With the head groups in x the order is longest
    // blocks of every head first, shortest last (longest-processing-time order over the whole launch).
    static const bool head_fast = !(getenv("BITNET_HIP_ATTN_HEAD_FAST") && atoi(getenv("BITNET_HIP_ATTN_HEAD_FAST")) == 0);
    PrefillArgs pa = p;
    pa.head_fast = head_fast ? 1 : 0;
    if (head_fast) grid = dim3(grid.y, grid.x, grid.z);
    if (q_rec) {
        if (p.ksplit != 1) return hipErrorInvalidValue;
        const hipError_t er = raise_dynamic_lds(akp, 2 * kKVBuf);
        if (er != hipSuccess) return er;
        hipLaunchKernelGGL(akp, grid, dim3(256), 2 * kKVBuf, stream, pa, q_rec);
        return hipGetLastError();
    }
    const hipError_t er = raise_dynamic_lds(ak, 2 * kKVBuf);  // two tile buffers = 64 KiB of dynamic LDS (+ a static word)
    if (er != hipSuccess) return er;
    hipLaunchKernelGGL(ak, grid, dim3(256), 2 * kKVBuf, stream, pa);
    if (p.ksplit > 1)
        hipLaunchKernelGGL(k_prefill_merge, dim3((unsigned)div_ceil((size_t)p.nq * p.n_heads * 32, 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// The workspace of one call, as byte offsets from its 256-byte aligned base: the f16 images (q [head][qpad][128], k [kv][tpad][128],
// v^T [kv][128][tpad]), the key split's partials, then the launcher's own array (q_block_pos of an extend, q_rec of a packed call), every
// part rounded to 256 bytes.  The size functions return `total`, the launchers carve from the same object.
struct AttnLayout {
    size_t qpad, tpad;        // query rows padded to kQPad, key positions padded to kQB
    int ksplit;               // key splits of the launch (attn_ksplit; 1: the partials are not used)
    size_t qh, kh, vt;        // the f16 images
    size_t part_o, part_ml;   // [ksplit][qpad][heads][128], [ksplit][qpad][heads][2]
    size_t tail;              // int q_block_pos[qpad / 64] (extend) / int4 q_rec[qpad / 64] (packed)
    size_t total;             // + 256: the caller's pointer need not be aligned
};
enum class AttnPartials { kExact, kBound, kNone };  // what is reserved for the key split's partials
// kExact: what this launch's ksplit needs.  kBound (extend): a bound on kExact over all nq' <= nq, T' <= T -- the partials vanish once the query
// blocks alone fill the chip, so the exact size is not monotone; the bound is non-decreasing in both lengths: the most parts T keys have, for
// the most query rows a split launch has (attn_ksplit: n_wg < 512).  kNone (packed): never key-split.
static AttnLayout attn_layout(int n_heads, int n_kv, size_t nq, size_t T, AttnPartials partials, size_t tail_elem_bytes) {
    AttnLayout L;
    L.qpad = div_ceil(nq, kQPad) * kQPad;
    L.tpad = div_ceil(T, kQB) * kQB;
    L.ksplit = partials == AttnPartials::kNone ? 1 : attn_ksplit(n_heads, n_kv, (int)L.qpad, (int)T);
    int parts = L.ksplit;
    size_t part_rows = L.qpad;
    if (partials == AttnPartials::kBound) {
        const AttnTile t = attn_tile(n_heads, n_kv);
        const size_t q_split_max = (size_t)(511 / (n_heads / t.hw)) * t.qg;
        parts = attn_key_parts((int)T);
        part_rows = L.qpad < q_split_max ? L.qpad : q_split_max;
    }
    L.qh = 0;
    L.kh = L.qh + (size_t)n_heads * L.qpad * kPD * sizeof(_Float16);
    L.vt = L.kh + (size_t)n_kv * L.tpad * kPD * sizeof(_Float16);
    L.part_o = div_ceil(L.vt + (size_t)n_kv * kPD * L.tpad * sizeof(_Float16), 256) * 256;
    L.part_ml = L.part_o + (size_t)L.ksplit * L.qpad * n_heads * kPD * sizeof(float);
    L.tail = L.part_o + (parts > 1 ? (size_t)parts * part_rows * n_heads * (kPD + 2) * sizeof(float) : 0);
    L.total = L.tail + div_ceil(L.qpad / kQB * tail_elem_bytes, 256) * 256 + 256;
    return L;
}

size_t attn_prefill_workspace_bytes(int n_heads, int n_kv, int nq, int T) {
    return attn_layout(n_heads, n_kv, (size_t)nq, (size_t)T, AttnPartials::kExact, 0).total;
}

static uint8_t *attn_ws_base(void *workspace) { return reinterpret_cast<uint8_t *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255); }

// What the whole-prompt, extend, packed and generic launchers share: element (head h, row t, dim d) of q / k / v at base + h * 128 + t * ld + d
// ([row][head][dim] rows), the transformer's RoPE, causal mask and 1/sqrt(d), the images and partials of the layout.  flags: bit 0 f16 caches,
// bit 1 f16 output rows.  Everything else is zero: absolute key order, f32 k|v rows, phase 0, q from the f16 image, no q_block_pos.
static PrefillArgs attn_args(const AttnLayout &L, uint8_t *ws, const float *q, int ld_q, const float *k, const float *v, int ld_kv, int nq, int T,
                             const float *rope_sin, const float *rope_cos, void *kcache, void *vcache, int n_heads, int n_kv, int max_pos, void *out,
                             int flags) {
    PrefillArgs p{};
    p.q = q;
    p.k = k;
    p.v = v;
    p.ld_q = ld_q;
    p.ld_kv = ld_kv;
    p.hs_q = p.hs_kv = kPD;
    p.out_hs = kPD;
    p.out_ld = n_heads * kPD;
    p.rope = 1;
    p.causal = 1;
    p.scale = 1.0f / sqrtf((float)kPD);
    p.nq = nq;
    p.nq_pad = (int)L.qpad;
    p.rope_sin = rope_sin;
    p.rope_cos = rope_cos;
    p.kcache = static_cast<float *>(kcache);
    p.vcache = static_cast<float *>(vcache);
    p.n_heads = n_heads;
    p.n_kv = n_kv;
    p.max_pos = max_pos;
    p.T = T;
    p.Tpad = (int)L.tpad;
    p.qh = reinterpret_cast<_Float16 *>(ws + L.qh);
    p.kh = reinterpret_cast<_Float16 *>(ws + L.kh);
    p.vt = reinterpret_cast<_Float16 *>(ws + L.vt);
    p.out = static_cast<float *>(out);
    p.cache_f16 = flags & 1;
    p.out_f16 = (flags >> 1) & 1;  // bit 1 of the flag word: f16 output rows
    p.ksplit = L.ksplit;
    p.split_tiles = attn_split_tiles();
    p.part_o = reinterpret_cast<float *>(ws + L.part_o);
    p.part_ml = reinterpret_cast<float *>(ws + L.part_ml);
    return p;
}

// q: nq query rows (stride ld_q floats) whose 64-row blocks sit at absolute positions q_block_pos
// (null: 64 b); kv: T context rows in absolute order (stride ld_kv: k heads then v heads).
hipError_t launch_attn_prefill(const float *q, int ld_q, const int *q_block_pos, int nq, const float *kv, int ld_kv, int T,
                               const float *rope_sin, const float *rope_cos, float *kcache, float *vcache, int n_heads, int n_kv,
                               int D, int max_pos, void *workspace, size_t workspace_bytes, float *out, hipStream_t stream,
                               int zz_world, int kv_f16, int cache_f16, int phase) {
    if (phase < 0 || phase > 2) return hipErrorInvalidValue;
    if (D != kPD || T <= 0 || nq <= 0 || T > max_pos || n_heads % n_kv != 0) return hipErrorInvalidValue;
    if (zz_world < 0 || (zz_world > 0 && (T % (2 * zz_world * kQB) != 0))) return hipErrorInvalidValue;
    const AttnLayout L = attn_layout(n_heads, n_kv, (size_t)nq, (size_t)T, AttnPartials::kExact, 0);
    if (!workspace || workspace_bytes < L.total) return hipErrorInvalidValue;
    // (f16 rows: the prep kernel indexes k heads then v heads from p.k itself)
    PrefillArgs p = attn_args(L, attn_ws_base(workspace), q, ld_q, kv, kv + (size_t)n_kv * kPD, ld_kv, nq, T, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, max_pos, out, cache_f16);
    p.q_block_pos = q_block_pos;
    p.zz_world = zz_world;
    p.zz_chunk = zz_world > 0 ? T / (2 * zz_world) : 0;
    p.kv_f16 = kv_f16;
    p.phase = phase;
    const unsigned nbq = (unsigned)(p.nq_pad / kQB), nbk = (unsigned)(p.Tpad / kQB);
    // the attention kernel needs 16-byte aligned f32 query rows for its own q path; anything else keeps the f16 image of the prep kernel
    p.q_in_kernel = attn_q_in_kernel() && (ld_q & 3) == 0 && ((uintptr_t)q & 15) == 0 ? 1 : 0;
    if (phase == 1) {  // the query slabs alone (nothing to do when the attention kernel prepares them itself)
        if (!p.q_in_kernel) hipLaunchKernelGGL(k_prefill_prep, dim3(nbq, (unsigned)n_heads), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (p.q_in_kernel) {
        p.slot0 = n_heads;
        hipLaunchKernelGGL(k_prefill_prep, dim3(nbk, (unsigned)(2 * n_kv)), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(k_prefill_prep, dim3(nbq > nbk ? nbq : nbk, (unsigned)(n_heads + 2 * n_kv)), dim3(256), 0, stream, p);
    }
    return launch_attn_kernel(p, stream);
}

// ---- continuing a LIVE sequence: seq new tokens at positions past .. past + seq - 1 over a cache that holds 0 .. past - 1 ----
// The reference's attention takes seq_len queries over past_len + seq_len keys from the cache, its causal mask hiding the keys
// beyond past_len + i from query i (T:455-470, T:704-719; cache append T:1171-1202).  k_prefill_attn already separates queries
// (64-row blocks at q_block_pos[b], here past + 64 b: its mask and RoPE only use block position + row) from keys (the f16 images
// kh / vt over T = past + seq positions), so what a continuation needs is the producer of those images:
//
//   k_extend_prep  grid (Tpad / 64, 2 kv): one 64-position tile of k or v through LDS.  Positions < past come from the decode
//                  cache (any of its four layouts), positions in [past, T) from the new q|k|v rows (k with RoPE at the absolute
//                  position) and go INTO the cache at their unaligned offset, positions >= T are zeros; the whole tile is then
//                  written to kh / vt exactly as k_prefill_prep writes it.  A workgroup reads only past slots and writes only
//                  new ones.  Slots >= past are never read: they may hold what a longer, rewound sequence left there.
//
// A past key goes cache -> f16: the bits k_prefill_prep's f16 of the exact value has, so the attention operands of a continued
// prompt are those of the one-shot prompt.  The re-preparation reads the whole past on every call: O(past) bytes per layer.
struct ExtendPrepArgs {
    const float *k_new, *v_new;  // element (kv head h, new row r, dim d) at base + r * ld + h * 128 + d
    int ld;
    const float *rope_sin, *rope_cos;
    void *kcache, *vcache;
    int n_kv, max_pos, past, T, Tpad, cache_f16;
    _Float16 *kh, *vt;   // [kv][Tpad][128], [kv][128][Tpad]
    int *q_block_pos;    // [n_qblocks]: past + 64 b, filled here so that the call stays asynchronous on its stream
    int n_qblocks;
};

// a staged slab -> [64 tokens][128] halves, contiguous, times mul: 8 bytes per thread and iteration (k_extend_prep, k_packed_qprep;
// k_prefill_prep keeps its own lambda: through this function hipcc hoists its address arithmetic differently)
__device__ __forceinline__ void store_rows_f16(const float (*tile)[kPD + 4], _Float16 *dst, float mul) {
    for (int i = 0; i < 8; ++i) {
        const int tid = threadIdx.x, idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
        const float4 v = *reinterpret_cast<const float4 *>(&tile[tok][d]);
        *reinterpret_cast<h4 *>(dst + (size_t)tok * kPD + d) = (h4){(_Float16)(v.x * mul), (_Float16)(v.y * mul), (_Float16)(v.z * mul), (_Float16)(v.w * mul)};
    }
}

// One 64-position tile of one sequence: t0 = its first position (cache side), img_t0 = its first position inside the f16 images (the same
// for k_extend_prep; a packed image holds several sequences' tiles one after the other, p.Tpad = all of them).
__device__ __forceinline__ void extend_prep_tile(const ExtendPrepArgs &p, float (*tile)[kPD + 4], int t0, int img_t0) {
    // every global access is 16 bytes wide (8 for f16) and contiguous along the fastest index of its tensor, as in k_prefill_prep;
    // only the 4-position (f16: 2-position) groups that straddle `past` or T fall back to single elements
    const int tid = threadIdx.x;
    const bool is_k = (int)blockIdx.y < p.n_kv;
    const int kvh = is_k ? (int)blockIdx.y : (int)blockIdx.y - p.n_kv;
    const int dp = p.past - t0, dl = p.T - t0;
    const int n_past = dp < 0 ? 0 : dp > kQB ? kQB : dp;  // tile rows [0, n_past) come from the cache,
    const int n_live = dl > kQB ? kQB : dl;               // [n_past, n_live) from the new rows, [n_live, 64) are zeros
    const size_t head_elems = (size_t)((p.max_pos + 63) / 64) * 64 * kPD;
    float *c32 = static_cast<float *>(is_k ? p.kcache : p.vcache) + (size_t)kvh * head_elems;
    _Float16 *c16 = static_cast<_Float16 *>(is_k ? p.kcache : p.vcache) + (size_t)kvh * head_elems;
    if (n_past < kQB) {
        const float *src = (is_k ? p.k_new : p.v_new) + (size_t)kvh * kPD;
        const bool vec_ok = (p.ld & 3) == 0 && ((uintptr_t)src & 15) == 0;
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
            if (tok < n_past) continue;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (tok < n_live) {
                const float *e = src + (size_t)(t0 + tok - p.past) * p.ld + d;
                v = vec_ok ? *reinterpret_cast<const float4 *>(e) : float4{e[0], e[1], e[2], e[3]};
            }
            *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
        }
    }
    if (n_past > 0) {
        if (is_k && !p.cache_f16) {  // [chunk][128][64]: 4 adjacent positions of one dim
            const float *kt = c32 + (size_t)(t0 >> 6) * kPD * 64;
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i, d = idx >> 4, tok = (idx & 15) * 4;
                if (tok >= n_past) continue;
                const float4 v = *reinterpret_cast<const float4 *>(kt + (size_t)d * 64 + tok);  // the tile is inside the (chunk-padded) allocation
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (tok + j < n_past) tile[tok + j][d] = e[j];
            }
        } else if (is_k) {  // [chunk][D / 2][64][2]: a dim pair of 2 adjacent positions
            const _Float16 *k16 = c16 + (size_t)(t0 >> 6) * kPD * 64;
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i, d2 = idx >> 5, tok = (idx & 31) * 2;
                if (tok >= n_past) continue;
                const h4 h = *reinterpret_cast<const h4 *>(k16 + ((size_t)d2 * 64 + tok) * 2);
                tile[tok][2 * d2] = (float)h[0];
                tile[tok][2 * d2 + 1] = (float)h[1];
                if (tok + 1 < n_past) {
                    tile[tok + 1][2 * d2] = (float)h[2];
                    tile[tok + 1][2 * d2 + 1] = (float)h[3];
                }
            }
        } else {  // [pos][128]
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
                if (tok >= n_past) continue;
                float4 v;
                if (p.cache_f16) {
                    const h4 h = *reinterpret_cast<const h4 *>(c16 + (size_t)(t0 + tok) * kPD + d);
                    v = float4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                } else {
                    v = *reinterpret_cast<const float4 *>(c32 + (size_t)(t0 + tok) * kPD + d);
                }
                *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
            }
        }
    }
    __syncthreads();
    if (is_k && n_past < n_live) {
        // split-half RoPE of the NEW keys at their absolute positions: the arithmetic of k_prefill_prep (cached keys are rotated already)
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 4, j = (idx & 15) * 4;
            if (tok < n_past || tok >= n_live) continue;
            const int pos = t0 + tok;
            rope_rotate4(tile, tok, j, p.rope_sin, p.rope_cos, pos);
        }
        __syncthreads();
    }
    // ---- append the new positions to the decode cache ----
    if (n_past < n_live) {
        if (is_k && !p.cache_f16) {
            float *kt = c32 + (size_t)(t0 >> 6) * kPD * 64;
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i, d = idx >> 4, tok = (idx & 15) * 4;
                if (tok >= n_past && tok + 3 < n_live) {
                    *reinterpret_cast<float4 *>(kt + (size_t)d * 64 + tok) = float4{tile[tok][d], tile[tok + 1][d], tile[tok + 2][d], tile[tok + 3][d]};
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (tok + e >= n_past && tok + e < n_live) kt[(size_t)d * 64 + tok + e] = tile[tok + e][d];
                }
            }
        } else if (is_k) {
            _Float16 *k16 = c16 + (size_t)(t0 >> 6) * kPD * 64;
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i, d2 = idx >> 5, tok = (idx & 31) * 2;
                const bool lo = tok >= n_past && tok < n_live, hi = tok + 1 >= n_past && tok + 1 < n_live;
                _Float16 *dst = k16 + ((size_t)d2 * 64 + tok) * 2;
                const h2 a = {(_Float16)tile[tok][2 * d2], (_Float16)tile[tok][2 * d2 + 1]}, b = {(_Float16)tile[tok + 1][2 * d2], (_Float16)tile[tok + 1][2 * d2 + 1]};
                if (lo && hi)
                    *reinterpret_cast<h4 *>(dst) = (h4){a[0], a[1], b[0], b[1]};
                else if (lo)
                    *reinterpret_cast<h2 *>(dst) = a;
                else if (hi)
                    *reinterpret_cast<h2 *>(dst + 2) = b;
            }
        } else {
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
                if (tok < n_past || tok >= n_live) continue;
                const float4 v = *reinterpret_cast<const float4 *>(&tile[tok][d]);
                if (p.cache_f16)
                    *reinterpret_cast<h4 *>(c16 + (size_t)(t0 + tok) * kPD + d) = (h4){(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
                else
                    *reinterpret_cast<float4 *>(c32 + (size_t)(t0 + tok) * kPD + d) = v;
            }
        }
    }
    // ---- the f16 images of the whole tile, in k_prefill_prep's order ----
    if (is_k) {
        store_rows_f16(tile, p.kh + ((size_t)kvh * p.Tpad + img_t0) * kPD, 1.0f);
    } else {
        // the V^T key permutation inside each group of 32 (k_prefill_prep): key 4 a + 16 b + j at slot 8 a + 4 b + j
        _Float16 *vt = p.vt + (size_t)kvh * kPD * p.Tpad;
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, d = idx >> 4, t4 = idx & 15, tok = t4 * 4;
            const int slot = 32 * (t4 >> 3) + 8 * (t4 & 3) + 4 * ((t4 >> 2) & 1);
            const h4 h = {(_Float16)tile[tok][d], (_Float16)tile[tok + 1][d], (_Float16)tile[tok + 2][d], (_Float16)tile[tok + 3][d]};
            *reinterpret_cast<h4 *>(vt + (size_t)d * p.Tpad + img_t0 + slot) = h;
        }
    }
}

__global__ __launch_bounds__(256) void k_extend_prep(ExtendPrepArgs p) {
    __shared__ __attribute__((aligned(16))) float tile[kQB][kPD + 4];
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int b = threadIdx.x; b < p.n_qblocks; b += 256) p.q_block_pos[b] = p.past + kQB * b;
    extend_prep_tile(p, tile, blockIdx.x * kQB, blockIdx.x * kQB);
}

// what k_extend_prep / k_packed_prep take from the attention's arguments; q_block_pos: the array k_extend_prep fills (null: packed, records instead)
static ExtendPrepArgs extend_prep_args(const PrefillArgs &p, int past, int *q_block_pos) {
    ExtendPrepArgs e{};
    e.k_new = p.k;
    e.v_new = p.v;
    e.ld = p.ld_kv;
    e.rope_sin = p.rope_sin;
    e.rope_cos = p.rope_cos;
    e.kcache = p.kcache;
    e.vcache = p.vcache;
    e.n_kv = p.n_kv;
    e.max_pos = p.max_pos;
    e.past = past;
    e.T = p.T;
    e.Tpad = p.Tpad;
    e.cache_f16 = p.cache_f16;
    e.kh = p.kh;
    e.vt = p.vt;
    e.q_block_pos = q_block_pos;
    e.n_qblocks = q_block_pos ? p.nq_pad / kQB : 0;
    return e;
}

// the images and (a bound on) the partials of attn_prefill_workspace_bytes, plus the q_block_pos array: non-decreasing in both lengths
static AttnLayout extend_layout(int n_heads, int n_kv, int past, int seq) {
    return attn_layout(n_heads, n_kv, (size_t)seq, (size_t)past + seq, AttnPartials::kBound, sizeof(int));
}
size_t attn_extend_workspace_bytes(int n_heads, int n_kv, int past, int seq) {
    if (n_heads <= 0 || n_kv <= 0 || n_heads % n_kv != 0 || past < 0 || seq <= 0) return 0;
    return extend_layout(n_heads, n_kv, past, seq).total;
}

hipError_t launch_attn_extend(const float *qkv, const float *rope_sin, const float *rope_cos, void *kcache, void *vcache, int n_heads, int n_kv,
                              int D, int max_pos, int past, int seq, void *workspace, size_t workspace_bytes, void *out, int flags, hipStream_t stream) {
    if (D != kPD || past < 0 || seq <= 0 || n_kv <= 0 || n_heads % n_kv != 0 || (size_t)past + seq > (size_t)max_pos) return hipErrorInvalidValue;
    if (!workspace || workspace_bytes < attn_extend_workspace_bytes(n_heads, n_kv, past, seq)) return hipErrorInvalidValue;
    const AttnLayout L = extend_layout(n_heads, n_kv, past, seq);
    const int ld = (n_heads + 2 * n_kv) * kPD;
    const float *k = qkv + (size_t)n_heads * kPD;
    uint8_t *ws = attn_ws_base(workspace);
    PrefillArgs p = attn_args(L, ws, qkv, ld, k, k + (size_t)n_kv * kPD, ld, seq, past + seq, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, max_pos, out, flags);
    int *qbp = reinterpret_cast<int *>(ws + L.tail);
    p.q_block_pos = qbp;
    p.phase = 1;
    p.q_in_kernel = attn_q_in_kernel() && ((uintptr_t)qkv & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(k_extend_prep, dim3((unsigned)(p.Tpad / kQB), (unsigned)(2 * n_kv)), dim3(256), 0, stream, extend_prep_args(p, past, qbp));
    // misaligned query rows: the f16 query image of k_prefill_prep (its query slabs alone), positions from the array filled above
    if (!p.q_in_kernel) hipLaunchKernelGGL(k_prefill_prep, dim3((unsigned)(p.nq_pad / kQB), (unsigned)n_heads), dim3(256), 0, stream, p);
    return launch_attn_kernel(p, stream);
}

// ---- SEVERAL sequences' new tokens in one pair of launches (the prompt side of the batched decode step) ----
// The packed rows [n_rows, (heads + 2 kv) * 128] hold up to kPackMax segments; segment s = one sequence: rows row0[s] .. row0[s] + len[s] - 1
// are its len[s] new tokens at positions past[s] .., over ITS caches.  row0 is a multiple of the attention workgroup's query tile
// (attn_packed_row_align: a workgroup stages ONE set of key tiles for all its waves, so it must lie inside one segment); rows between
// segments are padding.  Per segment the arithmetic is launch_attn_extend's:
//
//   k_packed_prep  grid (all segments' 64-position tiles, 2 kv): workgroup x finds its segment in the table (kernel arguments: the call
//                  stays asynchronous, there is no upload) and runs k_extend_prep's tile body on that segment's caches and rows; the f16
//                  images are ONE pair [kv][sum Tpad_s][128] / [kv][128][sum Tpad_s], segment s's tiles at tile offset sum_{s' < s} Tpad_s' / 64
//                  (table order).  Its first workgroup also writes the per-block records.
//   q_rec[b]       {position of the block's first row, tile offset of its segment, key count past + len of its segment, live rows}, one
//                  int4 per 64-row block up to nq_pad / 64.  A padding block behind a segment's end inside the same workgroup tile (odd
//                  groups: 128-row tiles) carries that segment's offset and 0 live rows; a tile no segment starts in reads tile 0 with one key.
//                  Rows that are not live multiply zeros (finite outputs, no cache traffic).
//   k_prefill_attn_packed  the attention body with position, key count and image offset from q_rec[block] instead of q_block_pos / p.T.
//                  No key split: a packed call exists because it has many query blocks.
constexpr int kPackMax = 64;  // BITNET_HIP_PACK_MAX
struct PackedPrepArgs {
    ExtendPrepArgs e;  // what all segments share (k_new / v_new: packed row 0; Tpad: all segments' tiles); past, T and the caches are per segment
    int4 *q_rec;
    int n_qblocks, n_seq, align_blocks;  // 64-row blocks up to nq_pad, segments, blocks per attention workgroup tile (1 or 2)
    int row0[kPackMax], len[kPackMax], past[kPackMax];
    void *kcache[kPackMax], *vcache[kPackMax];
};

__global__ __launch_bounds__(256) void k_packed_prep(PackedPrepArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kQB][kPD + 4];
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int b = threadIdx.x; b < a.n_qblocks; b += 256) {
            const int g0 = b / a.align_blocks * a.align_blocks;  // first block of the workgroup tile: a segment starts there or the tile is padding
            int4 r = {0, 0, 1, 0};
            int off = 0;
            for (int s = 0; s < a.n_seq; ++s) {
                const int T = a.past[s] + a.len[s], end = a.row0[s] + a.len[s];
                if (g0 * kQB >= a.row0[s] && g0 * kQB < end) {
                    const int live = end - b * kQB;
                    r = int4{a.past[s] + b * kQB - a.row0[s], off, T, live < 0 ? 0 : live > kQB ? kQB : live};
                }
                off += (T + kQB - 1) / kQB;
            }
            a.q_rec[b] = r;
        }
    }
    int s = 0, off = 0;
    for (; s < a.n_seq; ++s) {
        const int nt = (a.past[s] + a.len[s] + kQB - 1) / kQB;
        if ((int)blockIdx.x < off + nt) break;
        off += nt;
    }
    if (s >= a.n_seq) return;  // (the grid is exactly the tiles of the table)
    ExtendPrepArgs e = a.e;
    e.k_new += (size_t)a.row0[s] * e.ld;
    e.v_new += (size_t)a.row0[s] * e.ld;
    e.kcache = a.kcache[s];
    e.vcache = a.vcache[s];
    e.past = a.past[s];
    e.T = a.past[s] + a.len[s];
    extend_prep_tile(e, tile, ((int)blockIdx.x - off) * kQB, (int)blockIdx.x * kQB);
}

// the f16 query image of a packed call whose rows are not 16-byte aligned (k_prefill_prep's query slabs with the block's position and live
// row count from its record): grid (nq_pad / 64, heads)
__global__ __launch_bounds__(256) void k_packed_qprep(PrefillArgs p, const int4 *q_rec) {
    __shared__ __attribute__((aligned(16))) float tile[kQB][kPD + 4];
    const int h = blockIdx.y, t0 = blockIdx.x * kQB, tid = threadIdx.x;
    const int4 r = q_rec[blockIdx.x];
    const float *src = p.q + (size_t)h * p.hs_q;
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (tok < r.w) {
            const float *e = src + (size_t)(t0 + tok) * p.ld_q + d;
            v = float4{e[0], e[1], e[2], e[3]};
        }
        *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
    }
    __syncthreads();
    for (int i = 0; i < 4; ++i) {  // split-half RoPE, the arithmetic of k_prefill_prep
        const int idx = tid + 256 * i, tok = idx >> 4, j = (idx & 15) * 4;
        const int pos = tok < r.w ? r.x + tok : 0;
        rope_rotate4(tile, tok, j, p.rope_sin, p.rope_cos, pos);
    }
    __syncthreads();
    const float qmul = 1.4426950408889634f * p.scale;
    store_rows_f16(tile, p.qh + ((size_t)h * p.nq_pad + t0) * kPD, qmul);
}

int attn_packed_row_align(int n_heads, int n_kv) {
    if (n_heads <= 0 || n_kv <= 0 || n_heads % n_kv != 0) return 0;
    const int qg = attn_tile(n_heads, n_kv).qg;  // the query tile of k_prefill_attn<4,4,2> / <2,4,2> / <1,4,2> (launch_attn_kernel) ...
    return qg < kQB ? kQB : qg;                  // ... in whole 64-row blocks: a block has ONE record
}

// all segments' key tiles, or 0 when a size is out of range (the images' 32-bit byte offsets hold 2^24 positions)
static size_t packed_tiles(int n_seq, const int *past, const int *len) {
    if (n_seq < 1 || n_seq > kPackMax || !past || !len) return 0;
    size_t tiles = 0;
    for (int s = 0; s < n_seq; ++s) {
        if (past[s] < 0 || len[s] < 1 || (size_t)past[s] + (size_t)len[s] >= ((size_t)1 << 24)) return 0;
        tiles += ((size_t)past[s] + (size_t)len[s] + kQB - 1) / kQB;
    }
    return tiles * kQB < ((size_t)1 << 24) ? tiles : 0;
}
// q image + k / v^T images of all tiles + the records: a sum of terms that each grow with past[s] and len[s]
static AttnLayout packed_layout(int n_heads, int n_kv, int n_rows, size_t tiles) {
    return attn_layout(n_heads, n_kv, (size_t)n_rows, tiles * kQB, AttnPartials::kNone, sizeof(int4));
}
size_t attn_packed_workspace_bytes(int n_heads, int n_kv, int n_rows, int n_seq, const int *past, const int *len) {
    const size_t tiles = packed_tiles(n_seq, past, len);
    if (n_heads <= 0 || n_kv <= 0 || n_heads % n_kv != 0 || n_rows < 1 || n_rows >= (1 << 24) || tiles == 0) return 0;
    return packed_layout(n_heads, n_kv, n_rows, tiles).total;
}

hipError_t launch_attn_packed(const float *qkv, int n_rows, const float *rope_sin, const float *rope_cos, int n_seq, const int *row0, const int *len,
                              const int *past, void *const *kcache, void *const *vcache, int n_heads, int n_kv, int D, int max_pos, void *workspace,
                              size_t workspace_bytes, void *out, int flags, hipStream_t stream) {
    const int align = attn_packed_row_align(n_heads, n_kv);
    const size_t need = attn_packed_workspace_bytes(n_heads, n_kv, n_rows, n_seq, past, len);
    if (D != kPD || align == 0 || need == 0 || !row0 || !kcache || !vcache || !workspace || workspace_bytes < need) return hipErrorInvalidValue;
    for (int s = 0; s < n_seq; ++s)  // every write of the two kernels stays inside its segment's rows and cache slots (the ABI also refuses overlaps)
        if (row0[s] < 0 || row0[s] % align != 0 || (size_t)row0[s] + (size_t)len[s] > (size_t)n_rows || (size_t)past[s] + (size_t)len[s] > (size_t)max_pos || !kcache[s] || !vcache[s])
            return hipErrorInvalidValue;
    const int ld = (n_heads + 2 * n_kv) * kPD;
    const size_t tiles = packed_tiles(n_seq, past, len);
    const AttnLayout L = packed_layout(n_heads, n_kv, n_rows, tiles);
    const float *k = qkv + (size_t)n_heads * kPD;
    // T = 0: the key count is per block (q_rec); no caches: they are per segment (PackedPrepArgs)
    uint8_t *ws = attn_ws_base(workspace);
    PrefillArgs p = attn_args(L, ws, qkv, ld, k, k + (size_t)n_kv * kPD, ld, n_rows, 0, rope_sin, rope_cos, nullptr, nullptr, n_heads, n_kv, max_pos, out, flags);
    int4 *q_rec = reinterpret_cast<int4 *>(ws + L.tail);
    p.phase = 1;
    p.q_in_kernel = attn_q_in_kernel() && ((uintptr_t)qkv & 15) == 0 ? 1 : 0;
    PackedPrepArgs a;
    a.e = extend_prep_args(p, 0, nullptr);  // k_new / v_new: packed row 0; past, T and the caches are per segment
    a.q_rec = q_rec;
    a.n_qblocks = p.nq_pad / kQB;
    a.n_seq = n_seq;
    a.align_blocks = align / kQB;
    for (int s = 0; s < kPackMax; ++s) {
        const bool on = s < n_seq;
        a.row0[s] = on ? row0[s] : 0, a.len[s] = on ? len[s] : 0, a.past[s] = on ? past[s] : 0;
        a.kcache[s] = on ? kcache[s] : nullptr, a.vcache[s] = on ? vcache[s] : nullptr;
    }
    hipLaunchKernelGGL(k_packed_prep, dim3((unsigned)tiles, (unsigned)(2 * n_kv)), dim3(256), 0, stream, a);
    if (!p.q_in_kernel) hipLaunchKernelGGL(k_packed_qprep, dim3((unsigned)(p.nq_pad / kQB), (unsigned)n_heads), dim3(256), 0, stream, p, (const int4 *)q_rec);
    return launch_attn_kernel(p, stream, q_rec);
}

// rows x [col0, col0 + ncols) of a row-major f32 matrix -> a compact [rows, ncols] buffer, f32 or f16: the k|v columns of the
// q|k|v projection as one contiguous send buffer for the token-parallel prefill's all-gather
__global__ void k_pack_cols(const float *__restrict__ src, size_t ld, size_t col0, size_t ncols, size_t total, void *__restrict__ dst, int f16) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t r = i / ncols, c = i - r * ncols;
    const float v = src[r * ld + col0 + c];
    if (f16)
        static_cast<_Float16 *>(dst)[i] = (_Float16)v;
    else
        static_cast<float *>(dst)[i] = v;
}
hipError_t launch_pack_cols(const float *src, size_t ld, size_t col0, size_t ncols, size_t rows, void *dst, int f16, hipStream_t stream) {
    const size_t total = rows * ncols;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack_cols, dim3((unsigned)div_ceil(total, 256)), dim3(256), 0, stream, src, ld, col0, ncols, total, dst, f16);
    return hipGetLastError();
}

// Plain multi-head attention over caller tensors [heads][seq][128] (no RoPE, no cache): the shape of
// the reference's fused_attention_hip stub (K/rocm/attention.rs:54-65), one batch element.
hipError_t launch_attn_generic(const float *q, const float *k, const float *v, float *out, int n_heads, int seq, int causal,
                               float scale, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (seq <= 0 || n_heads <= 0 || !workspace) return hipErrorInvalidValue;
    const AttnLayout L = attn_layout(n_heads, n_heads, (size_t)seq, (size_t)seq, AttnPartials::kExact, 0);
    if (workspace_bytes < L.total) return hipErrorInvalidValue;
    PrefillArgs p = attn_args(L, attn_ws_base(workspace), q, kPD, k, v, kPD, seq, seq, nullptr, nullptr, nullptr, nullptr, n_heads, n_heads, seq, out, 0);
    p.hs_q = p.hs_kv = seq * kPD;  // [head][row][dim] tensors, in and out
    p.out_hs = seq * kPD;
    p.out_ld = kPD;
    p.rope = 0;
    p.causal = causal;
    p.scale = scale;
    const unsigned nb = (unsigned)(p.nq_pad / kQB);
    hipLaunchKernelGGL(k_prefill_prep, dim3(nb, (unsigned)(3 * n_heads)), dim3(256), 0, stream, p);
    return launch_attn_kernel(p, stream);
}

}  // namespace bitnet_hip
