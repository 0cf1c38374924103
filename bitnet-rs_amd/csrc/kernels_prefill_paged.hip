// kernels_prefill_paged.hip -- causal prompt attention straight over KV pages (gfx950): several sequences' new tokens in one pair of launches, the keys
// read through page tables and the new keys appended into page slots (include/bitnet_hip_pagedprefill.h).  The semantics are those of
// bitnet_hip_attention_packed_dev with every cache pointer replaced by a page table into ONE K pool and ONE V pool (kv_paged.hpp).
//
//   k_paged_prefill_prep   one pass over the NEW rows only.  grid (max(64-row blocks, new page tiles), heads + 2 kv) x 256 threads:
//       slot < heads   a 64-row query slab through LDS: RoPE at the absolute position, times softmax scale * log2(e), f16 -> workspace [head][row][128]
//                      (k_packed_qprep's arithmetic);
//       k | v slots    ONE page tile that takes new positions (segment s: tiles past / 64 .. (past + len - 1) / 64): its new rows through LDS, RoPE on
//                      k (k_extend_prep's arithmetic), then into slots past % 64 .. of page table[tile]: exact f32, or rounded once to f16.  Slots below
//                      `past` and at or past past + len are not touched;
//       block (0, 0)   also writes the records {position of the block's first row, segment, key count, live rows}, one per 64-row block.
//   k_prefill_attn_paged<HW, KV16>   flash attention on v_mfma_f32_16x16x32_f16, f32 accumulation, f32 online softmax in base 2.  4 waves = HW query
//       heads of ONE KV head x (4 / HW) wave columns of 32 queries; the workgroup walks key tiles 0 .. (its last live position) / 64, every key tile ONE
//       page tile found through the segment's table (ids read and checked up front: one dependent load level).  There is no image of the past.
//
// Where the transposes happen.  A page K tile is [64 dim pairs][64 positions] words, a page V tile [64 positions][128 dims].  The
// kernel computes S^T = K Q^T and O^T = V^T P^T (the probabilities never leave registers: an S^T accumulator is the second product's B operand).
//   K pays NOTHING: the tile goes into LDS in the page's own order, and the A operand of the first product (lane = key c, k-slots = 8 dims) is four
//     WORDS of one position column: rows 16 ch + 4 g + e (e < 4) = dims 32 ch + 8 g .. + 7, the order the query image already has.  Four 4-byte LDS
//     reads a row (256 B) apart instead of one 16-byte read: the same bytes per clock.  Word (row r, position p) sits at column p ^ (((r >> 2) & 3) << 4),
//     so the four row groups g of one read land in four different 16-bank blocks: conflict-free.
//   V is transposed ON THE LDS WRITE from a register staging path: a thread holds word r (dims 2 r, 2 r + 1) of FOUR neighbouring positions, splits
//     the halves and writes two 8-byte runs (4 keys of dim 2 r, 4 keys of dim 2 r + 1) into a [128 dims][64 key slots] tile, keys of every group of 32
//     in the second product's operand order (key 4 a + 16 b + j at slot 8 a + 4 b + j), 16-byte unit u of dim d at u ^ ((d >> 1) & 7): the A-operand
//     reads are single conflict-free 16-byte reads.
// Both tiles are double-buffered (64 KiB) and tile t + 1 is in flight while tile t is multiplied: its V words wait in registers across the first
// product and the softmax, its K words across the second product (where the scores are dead), each written to the other buffer right after; one
// barrier per tile.  f32 pools take the same walk and round to f16 between the registers and LDS: the operands are f16(k), f16(v) for both types.
// Slots at or past a segment's key count enter LDS as zeros; rows that are not live multiply zero queries.  No key split: a short chunk over a
// long past runs on few workgroups (the next step).  Reached from PagedBatch::prefill through Decoder's AttnOp::PagedPack (host/paged_batch.hpp).
#include "common.hpp"
#include "kv_layout.hpp"
#include "kv_paged.hpp"
#include "paged_stage.hpp"
#include "wave.hpp"

namespace bitnet_hip {

namespace {

constexpr int kPpD = kKvDim, kPpT = kKvChunk;
constexpr int kPpMax = BITNET_HIP_PACK_MAX;
constexpr int kPpQPad = 128;                   // query rows are padded to the largest workgroup query tile
constexpr int kPpIdCap = 256;                  // page ids of the walk kept in LDS (16384 positions); beyond: read again from the (checked) table
constexpr int kPpTileBytes = kPgTileBytes, kPpBufBytes = kPgBufBytes;  // paged_stage.hpp: one f16 operand tile; K tile | V^T tile, the kernel keeps two

// the host arrays of a call, as kernel arguments: no upload, the call stays asynchronous
struct PagedSegs {
    int n_seq, align_blocks, n_qblocks;  // segments, 64-row blocks per attention workgroup tile (1 or 2), 64-row blocks up to nq_pad
    int row0[kPpMax], len[kPpMax], past[kPpMax];
    const uint32_t *table[kPpMax];
};

struct PagedPrepArgs {
    const float *qkv;  // [n_rows][(heads + 2 kv) * 128]
    const float *rope_sin, *rope_cos;
    uint32_t *kpool, *vpool;
    _Float16 *qh;  // [head][nq_pad][128]
    int4 *q_rec;   // [nq_pad / 64]
    unsigned n_pages;
    int ld, n_heads, n_kv, nq_pad, cache_f16, n_new_tiles;
    PagedSegs seg;
};

struct PagedAttnArgs {
    const _Float16 *qh;
    const int4 *q_rec;
    const uint32_t *kpool, *vpool;
    void *out;  // [n_rows][heads * 128] f32 or f16
    unsigned n_pages;
    int n_heads, n_kv, nq, nq_pad, out_f16;
    const uint32_t *table[kPpMax];
};

// Entries 0 .. n_entries - 1 of a table against the pool, by the whole workgroup; ids (when given) keeps the first kPpIdCap.  Block-uniform result:
// true = an id outside the pool = the segment is idle for the call.  Both kernels ask this same question of the same entries.
__device__ __forceinline__ bool table_is_bad(const uint32_t *tbl, int n_entries, unsigned n_pages, uint32_t *ids) {
    bool bad = false;
    for (int i = threadIdx.x; i < n_entries; i += 256) {
        const uint32_t pg = tbl[i];
        bad |= pg >= n_pages;
        if (ids && i < kPpIdCap) ids[i] = pg;
    }
    return __syncthreads_or(bad);
}

// split-half RoPE of 4 adjacent pairs (j .. j + 3, 64 + j ..) of one staged row at position pos: the expressions of kernels_prefill_attn.hip's
// rope_rotate4, so that the appended keys carry the bits the contiguous path leaves
__device__ __forceinline__ void paged_rope_rotate4(float (*tile)[kPpD + 4], int tok, int j, const float *rope_sin, const float *rope_cos, int pos) {
    const float4 s = *reinterpret_cast<const float4 *>(rope_sin + (size_t)pos * 64 + j), c = *reinterpret_cast<const float4 *>(rope_cos + (size_t)pos * 64 + j);
    const float4 x0 = *reinterpret_cast<const float4 *>(&tile[tok][j]), x1 = *reinterpret_cast<const float4 *>(&tile[tok][64 + j]);
    *reinterpret_cast<float4 *>(&tile[tok][j]) = float4{x0.x * c.x - x1.x * s.x, x0.y * c.y - x1.y * s.y, x0.z * c.z - x1.z * s.z, x0.w * c.w - x1.w * s.w};
    *reinterpret_cast<float4 *>(&tile[tok][64 + j]) = float4{x0.x * s.x + x1.x * c.x, x0.y * s.y + x1.y * c.y, x0.z * s.z + x1.z * c.z, x0.w * s.w + x1.w * c.w};
}

// the record of 64-row block b: a segment starts at the first block g0 of its workgroup tile, or the tile is padding (segment -1)
__device__ __forceinline__ int4 paged_block_record(const PagedSegs &S, int b) {
    const int g0 = b / S.align_blocks * S.align_blocks;
    int4 r = {0, -1, 1, 0};
    for (int s = 0; s < S.n_seq; ++s) {
        const int end = S.row0[s] + S.len[s];
        if (g0 * kPpT >= S.row0[s] && g0 * kPpT < end) {
            const int live = end - b * kPpT;
            r = int4{S.past[s] + b * kPpT - S.row0[s], s, S.past[s] + S.len[s], live < 0 ? 0 : live > kPpT ? kPpT : live};
        }
    }
    return r;
}

__global__ __launch_bounds__(256) void k_paged_prefill_prep(const PagedPrepArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kPpT][kPpD + 4];
    const PagedSegs &S = a.seg;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int b = tid; b < S.n_qblocks; b += 256) a.q_rec[b] = paged_block_record(S, b);

    if ((int)blockIdx.y < a.n_heads) {
        // ---- a query slab: block b of head h (k_packed_qprep) ----
        const int b = blockIdx.x, h = blockIdx.y, t0 = b * kPpT;
        if (b >= S.n_qblocks) return;
        const int4 r = paged_block_record(S, b);
        const float *src = a.qkv + (size_t)h * kPpD;
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (tok < r.w) {
                const float *e = src + (size_t)(t0 + tok) * a.ld + d;
                v = float4{e[0], e[1], e[2], e[3]};
            }
            *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
        }
        __syncthreads();
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 4, j = (idx & 15) * 4;
            paged_rope_rotate4(tile, tok, j, a.rope_sin, a.rope_cos, tok < r.w ? r.x + tok : 0);
        }
        __syncthreads();
        const float qmul = 1.4426950408889634f * (1.0f / sqrtf((float)kPpD));
        _Float16 *dst = a.qh + ((size_t)h * a.nq_pad + t0) * kPpD;
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
            const float4 v = *reinterpret_cast<const float4 *>(&tile[tok][d]);
            *reinterpret_cast<h4 *>(dst + (size_t)tok * kPpD + d) = (h4){(_Float16)(v.x * qmul), (_Float16)(v.y * qmul), (_Float16)(v.z * qmul), (_Float16)(v.w * qmul)};
        }
        return;
    }

    // ---- one page tile that takes new positions: K (slot < heads + kv) or V of KV head kvh ----
    if ((int)blockIdx.x >= a.n_new_tiles) return;
    const bool is_k = (int)blockIdx.y < a.n_heads + a.n_kv;
    const int kvh = (int)blockIdx.y - a.n_heads - (is_k ? 0 : a.n_kv);
    int s = 0, off = 0;
    for (; s < S.n_seq; ++s) {
        const int nt = (S.past[s] + S.len[s] - 1) / kPpT - S.past[s] / kPpT + 1;
        if ((int)blockIdx.x < off + nt) break;
        off += nt;
    }
    if (s >= S.n_seq) return;  // (the count is exactly the tiles of the table)
    const int past = S.past[s], T = past + S.len[s];
    const uint32_t *tbl = S.table[s];
    if (table_is_bad(tbl, (T - 1) / kPpT + 1, a.n_pages, nullptr)) return;  // idle: nothing of it is written
    const int chunk = past / kPpT + ((int)blockIdx.x - off), t0 = chunk * kPpT;
    const int n_past = past > t0 ? past - t0 : 0;          // tile slots [0, n_past) hold the past and stay as they are,
    const int n_live = T - t0 > kPpT ? kPpT : T - t0;      // [n_past, n_live) take the new rows, [n_live, 64) are not touched
    const uint32_t pg = tbl[chunk];
    const float *src = a.qkv + (size_t)S.row0[s] * a.ld + (size_t)(a.n_heads + (is_k ? 0 : a.n_kv) + kvh) * kPpD;
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + 256 * i, tok = idx >> 5, d = (idx & 31) * 4;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (tok >= n_past && tok < n_live) {
            const float *e = src + (size_t)(t0 + tok - past) * a.ld + d;
            v = float4{e[0], e[1], e[2], e[3]};
        }
        *reinterpret_cast<float4 *>(&tile[tok][d]) = v;
    }
    __syncthreads();
    if (is_k) {
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, tok = idx >> 4, j = (idx & 15) * 4;
            if (tok < n_past || tok >= n_live) continue;
            paged_rope_rotate4(tile, tok, j, a.rope_sin, a.rope_cos, t0 + tok);
        }
        __syncthreads();
    }
    const unsigned R = kv_rows(a.cache_f16 != 0);
    uint32_t *page = (is_k ? a.kpool : a.vpool) + kv_page_tile_words(pg, kvh, a.n_kv, R);
    // whole words, position by position: K word (row, slot) at row * 64 + slot, V word (slot, row) at slot * R + row
    for (unsigned idx = tid; idx < R * kPpT; idx += 256) {
        const int tok = is_k ? (int)(idx & 63) : (int)(idx / R), row = is_k ? (int)(idx >> 6) : (int)(idx % R);
        if (tok < n_past || tok >= n_live) continue;
        page[idx] = a.cache_f16 ? pack_h2(tile[tok][2 * row], tile[tok][2 * row + 1]) : __float_as_uint(tile[tok][row]);
    }
}

template <int HW, bool KV16>
// One workgroup per CU: at two the f16 instance spilled (148 bytes of scratch per lane at the 256-register budget); the staging registers of the
// next tile live beside 64 output and 32 score accumulators.  Bringing it back to two workgroups is tuning left open.
__global__ __launch_bounds__(256) void k_prefill_attn_paged(const PagedAttnArgs p) {
    constexpr int NQ = 2, QG = 32 * (4 / HW);  // query groups of 16 per wave, query rows per workgroup
    constexpr int R = KV16 ? kPpD / 2 : kPpD;  // pool words per position and head
    extern __shared__ __attribute__((aligned(16))) uint8_t kv_lds[];  // [2][K tile | V^T tile]
    __shared__ uint32_t ids[kPpIdCap];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 15, g = lane >> 4;
    const int qgi = (int)gridDim.y - 1 - (int)blockIdx.y;  // late (long) tiles first
    const int h = (int)blockIdx.x * HW + wave % HW, kvh = ((int)blockIdx.x * HW) / (p.n_heads / p.n_kv);
    const int row_wg = qgi * QG, qbase = row_wg + (wave / HW) * 16 * NQ;
    const int4 rec0 = p.q_rec[row_wg >> 6], rec = p.q_rec[qbase >> 6];
    const int seg = __builtin_amdgcn_readfirstlane(rec0.y), T = __builtin_amdgcn_readfirstlane(rec0.z);

    // rows of an idle segment and padding tiles: zeros, and no pool address is formed
    auto write_rows = [&](const v4f (&o)[NQ][8], const float (&inv)[NQ]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int qrow = qbase + 16 * q + c;
            if (qrow >= p.nq) continue;
            const size_t oo = (size_t)qrow * p.n_heads * kPpD + (size_t)h * kPpD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const float4 v = {o[q][dt][0] * inv[q], o[q][dt][1] * inv[q], o[q][dt][2] * inv[q], o[q][dt][3] * inv[q]};
                if (p.out_f16)
                    *reinterpret_cast<h4 *>(static_cast<_Float16 *>(p.out) + oo + 16 * dt) = (h4){(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
                else
                    *reinterpret_cast<float4 *>(static_cast<float *>(p.out) + oo + 16 * dt) = v;
            }
        }
    };
    v4f o[NQ][8];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[q][dt] = (v4f){0.f, 0.f, 0.f, 0.f};
    const float zero_inv[NQ] = {0.0f, 0.0f};
    if (seg < 0) {  // block-uniform: no segment starts in this tile
        write_rows(o, zero_inv);
        return;
    }
    const uint32_t *tbl = p.table[seg];
    if (table_is_bad(tbl, (T - 1) / kPpT + 1, p.n_pages, ids)) {  // block-uniform, and k_paged_prefill_prep's verdict
        write_rows(o, zero_inv);
        return;
    }
    const int wg_pos0 = rec0.x + (row_wg & 63);
    const int kt_last = (wg_pos0 + QG - 1 < T ? wg_pos0 + QG - 1 : T - 1) >> 6;  // last key tile any row of the workgroup sees
    const int bpos = rec.x + (qbase & 63);
    int qlim[NQ];  // highest visible key of this lane's query in group q; rows past the segment's end see all of its keys
#pragma unroll
    for (int q = 0; q < NQ; ++q) qlim[q] = bpos + 16 * q + c < T ? bpos + 16 * q + c : T - 1;
    const int qmin = __builtin_amdgcn_readfirstlane(bpos < T ? bpos : T - 1);

    // ---- tile staging (paged_stage.hpp): page -> registers (requested a tile ahead), registers -> LDS (behind the arithmetic of the tile before).
    //      n_live = T - kt * 64: positions of the tile below the key count (>= 1) ----
    PagedTileStage<KV16> st;
    auto page_of = [&](int kt) -> uint32_t { return kt < kPpIdCap ? ids[kt] : tbl[kt]; };  // (every id passed the check above)
    auto fetch_k = [&](int kt) __attribute__((always_inline)) { st.fetch_k(p.kpool + kv_page_tile_words(page_of(kt), kvh, p.n_kv, R), T - kt * kPpT, tid); };
    auto fetch_v = [&](int kt) __attribute__((always_inline)) { st.fetch_v(p.vpool + kv_page_tile_words(page_of(kt), kvh, p.n_kv, R), T - kt * kPpT, wave, lane); };
    auto commit_k = [&](int kt, int buf) __attribute__((always_inline)) { st.commit_k(kv_lds + buf * kPpBufBytes, T - kt * kPpT, tid); };
    auto commit_v = [&](int buf) __attribute__((always_inline)) { st.commit_v(kv_lds + buf * kPpBufBytes + kPpTileBytes, wave, lane); };

    fetch_k(0);
    fetch_v(0);
    // Q^T operands: 8 consecutive dims per k-slot group, in registers for the whole walk
    h8 qreg[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const _Float16 *qp = p.qh + ((size_t)h * p.nq_pad + qbase + 16 * q + c) * kPpD + 8 * g;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) qreg[q][ch] = *reinterpret_cast<const h8 *>(qp + 32 * ch);
    }
    float m_run[NQ], l_run[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) m_run[q] = -INFINITY, l_run[q] = 0.0f;
    commit_k(0, 0);
    commit_v(0);
    __syncthreads();

    for (int kt = 0; kt <= kt_last; ++kt) {
        const int par = kt & 1;
        const bool more = kt < kt_last;  // workgroup-uniform
        if (more) fetch_v(kt + 1);  // in registers across the first product and the softmax
        const uint32_t *kw = reinterpret_cast<const uint32_t *>(kv_lds + par * kPpBufBytes);
        const uint8_t *vs = kv_lds + par * kPpBufBytes + kPpTileBytes;
        // ---- S^T = K Q^T: 4 key tiles of 16, reduced over 4 dim chunks of 32; the A operand is 4 words of position column 16 i + c ----
        v4f s[NQ][4];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[q][i] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t *kp = kw + (16 * ch + 4 * g) * 64 + (16 * (i ^ g) + c);
                const u32x4 w = {kp[0], kp[64], kp[128], kp[192]};
                const h8 a = __builtin_bit_cast(h8, w);
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qreg[q][ch], s[q][i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);  // one chunk's operand reads in flight at a time: hoisting them all cost registers
        }
        // ---- online softmax for query column c of each group (keys of this lane: 16 i + 4 g + j).  Only tiles that reach past some query's
        //      limit are masked (wave-uniform); key 0 is visible to every row, so the running maximum is finite from the first tile on ----
        const bool need_mask = kt * kPpT + kPpT - 1 > qmin;
        h8 pb[NQ][2];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float mt = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (need_mask) s[q][i][j] = kt * kPpT + 16 * i + 4 * g + j <= qlim[q] ? s[q][i][j] : -INFINITY;
                    mt = fmaxf(mt, s[q][i][j]);
                }
            const float m_new = fmaxf(m_run[q], paged_max_over_g(mt));
            const float alpha = __builtin_amdgcn_exp2f(m_run[q] - m_new);  // the first tile: 2^-inf = 0
            m_run[q] = m_new;
            float ls[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s[q][i][j] = __builtin_amdgcn_exp2f(s[q][i][j] - m_new);
                ls[i] = (s[q][i][0] + s[q][i][1]) + (s[q][i][2] + s[q][i][3]);
            }
            l_run[q] = fmaf(l_run[q], alpha, (ls[0] + ls[1]) + (ls[2] + ls[3]));
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) o[q][dt] *= alpha;
            // P^T operand: k-slot (g, j) = key 32 u + 4 g + j (j < 4), 32 u + 16 + 4 g + (j - 4)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pb[q][u][j] = (_Float16)s[q][2 * u][j];
                    pb[q][u][4 + j] = (_Float16)s[q][2 * u + 1][j];
                }
        }
        if (more) {  // the buffer tile kt - 1 left: every wave passed the barrier below since it read it
            commit_v(par ^ 1);
            fetch_k(kt + 1);  // in registers across the second product, where the scores are dead
        }
        // ---- O^T += V^T P^T: unit 4 u + g of dim 16 dt + c ----
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int d0 = 0; d0 < 8; d0 += 4) {
#pragma unroll
                for (int dt = d0; dt < d0 + 4; ++dt) {
                    const h8 a = *reinterpret_cast<const h8 *>(vs + (16 * dt + c) * 128 + (((4 * u + g) ^ (c >> 1)) * 16));
#pragma unroll
                    for (int q = 0; q < NQ; ++q) o[q][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb[q][u], o[q][dt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        if (more) commit_k(kt + 1, par ^ 1);
        __syncthreads();
    }
    float inv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        float l = l_run[q];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        inv[q] = 1.0f / l;
    }
    write_rows(o, inv);
}

struct PagedLayout {
    size_t qpad, qh, rec, total;
};
PagedLayout paged_layout(size_t n_heads, size_t n_rows) {
    PagedLayout L;
    L.qpad = div_ceil(n_rows, (size_t)kPpQPad) * kPpQPad;
    L.qh = 0;
    L.rec = n_heads * L.qpad * kPpD * sizeof(_Float16);  // a multiple of 256
    L.total = L.rec + div_ceil(L.qpad / kPpT * sizeof(int4), (size_t)256) * 256 + 256;  // + 256: the caller's pointer need not be aligned
    return L;
}

template <bool KV16>
hipError_t launch_paged_attn(int hw, dim3 grid, hipStream_t stream, const PagedAttnArgs &a) {
    void (*k)(PagedAttnArgs) = hw == 4 ? k_prefill_attn_paged<4, KV16> : hw == 2 ? k_prefill_attn_paged<2, KV16> : k_prefill_attn_paged<1, KV16>;
    const hipError_t er = raise_dynamic_lds(k, 2 * kPpBufBytes);  // 64 KiB of dynamic LDS beside the static id list
    if (er != hipSuccess) return er;
    hipLaunchKernelGGL(k, grid, dim3(256), 2 * kPpBufBytes, stream, a);
    return hipGetLastError();
}

}  // namespace

}  // namespace bitnet_hip

using namespace bitnet_hip;

extern "C" {

size_t bitnet_hip_attention_paged_prefill_workspace_bytes(size_t n_heads, size_t n_kv_heads, size_t n_rows) {
    const size_t lim = (size_t)1 << 24;
    if (n_heads == 0 || n_kv_heads == 0 || n_heads >= lim || n_heads % n_kv_heads != 0 || n_heads / n_kv_heads > 4 || n_rows == 0 || n_rows >= lim) return 0;
    return paged_layout(n_heads, n_rows).total;
}

int bitnet_hip_attention_paged_prefill_dev(const float *qkv, size_t n_rows, const float *rope_sin, const float *rope_cos, size_t n_seq, const int32_t *row0,
                                           const int32_t *len, const int32_t *past, const uint32_t *const *tables, void *kpool, void *vpool, size_t n_pages,
                                           size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos, void *workspace, size_t workspace_bytes, void *out,
                                           int flags, void *stream) {
    const char *entry = "attention_paged_prefill_dev";
    // every refusal comes before anything launches: the two kernels write wherever the tables send them
    if (n_seq == 0 || n_seq > BITNET_HIP_PACK_MAX) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_seq %zu outside 1..%d", entry, n_seq, BITNET_HIP_PACK_MAX);
    if (!qkv || !rope_sin || !rope_cos || !row0 || !len || !past || !tables || !kpool || !vpool || !workspace || !out)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to %s", entry);
    if (n_kv_heads == 0 || n_heads == 0 || n_heads % n_kv_heads != 0)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "num_heads %zu must be divisible by num_key_value_heads %zu", n_heads, n_kv_heads);
    if (head_dim != 128) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: head_dim %zu unsupported (128)", entry, head_dim);
    if (n_heads / n_kv_heads > 4) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: group %zu unsupported (1..4)", entry, n_heads / n_kv_heads);
    if (flags & ~(BITNET_HIP_ATTN_CACHE_F16 | BITNET_HIP_ATTN_OUT_F16)) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", entry, flags);
    const bool f16 = (flags & BITNET_HIP_ATTN_CACHE_F16) != 0;
    if (n_pages == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_pages 0", entry);
    if (!bitnet_hip_kv_pool_bytes(n_pages, n_kv_heads, head_dim, f16))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_pages %zu, n_kv_heads %zu)", entry, n_pages, n_kv_heads);
    const size_t align = bitnet_hip_attention_packed_row_align(n_heads, n_kv_heads);
    if (align == 0 || n_rows == 0 || max_pos == 0 || max_pos > ((size_t)1 << 24) || n_heads + 2 * n_kv_heads > 65535)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: sizes out of range", entry);
    size_t new_tiles = 0;
    for (size_t s = 0; s < n_seq; ++s) {
        if (!tables[s]) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segment %zu has a null table", entry, s);
        if (len[s] < 1) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segment %zu: len must be at least 1", entry, s);
        if (past[s] < 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segment %zu: negative past", entry, s);
        if ((size_t)past[s] + (size_t)len[s] > max_pos)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "KV cache overflow: segment %zu, past %d, len %d, max_pos %zu", s, past[s], len[s], max_pos);
        if (row0[s] < 0 || (size_t)row0[s] % align != 0)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segment %zu: row0 %d is not a multiple of the row alignment %zu", entry, s, row0[s], align);
        if ((size_t)row0[s] + (size_t)len[s] > n_rows) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segment %zu ends beyond n_rows %zu", entry, s, n_rows);
        for (size_t t = 0; t < s; ++t) {
            if (row0[s] < row0[t] + len[t] && row0[t] < row0[s] + len[s])
                return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segments %zu and %zu overlap", entry, t, s);
            if (tables[s] == tables[t]) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: segments %zu and %zu share a table", entry, t, s);
        }
        new_tiles += ((size_t)past[s] + (size_t)len[s] - 1) / 64 - (size_t)past[s] / 64 + 1;
    }
    const size_t need = bitnet_hip_attention_paged_prefill_workspace_bytes(n_heads, n_kv_heads, n_rows);
    if (need == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: sizes out of range", entry);
    if (workspace_bytes < need) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "workspace too small: expected %zu, got %zu", need, workspace_bytes);

    const PagedLayout L = paged_layout(n_heads, n_rows);
    uint8_t *ws = reinterpret_cast<uint8_t *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int group = (int)(n_heads / n_kv_heads), hw = group % 4 == 0 ? 4 : group % 2 == 0 ? 2 : 1, qg = 32 * (4 / hw);
    PagedPrepArgs a{};
    a.qkv = qkv, a.rope_sin = rope_sin, a.rope_cos = rope_cos;
    a.kpool = static_cast<uint32_t *>(kpool), a.vpool = static_cast<uint32_t *>(vpool);
    a.qh = reinterpret_cast<_Float16 *>(ws + L.qh), a.q_rec = reinterpret_cast<int4 *>(ws + L.rec);
    a.n_pages = (unsigned)n_pages, a.ld = (int)((n_heads + 2 * n_kv_heads) * 128), a.n_heads = (int)n_heads, a.n_kv = (int)n_kv_heads;
    a.nq_pad = (int)L.qpad, a.cache_f16 = f16, a.n_new_tiles = (int)new_tiles;
    a.seg.n_seq = (int)n_seq, a.seg.align_blocks = (int)(align / 64), a.seg.n_qblocks = (int)(L.qpad / 64);
    PagedAttnArgs b{};
    b.qh = a.qh, b.q_rec = a.q_rec, b.kpool = a.kpool, b.vpool = a.vpool, b.out = out, b.n_pages = a.n_pages;
    b.n_heads = a.n_heads, b.n_kv = a.n_kv, b.nq = (int)n_rows, b.nq_pad = a.nq_pad, b.out_f16 = (flags & BITNET_HIP_ATTN_OUT_F16) != 0;
    for (size_t s = 0; s < (size_t)kPpMax; ++s) {
        const bool on = s < n_seq;
        a.seg.row0[s] = on ? row0[s] : 0, a.seg.len[s] = on ? len[s] : 0, a.seg.past[s] = on ? past[s] : 0;
        a.seg.table[s] = b.table[s] = on ? tables[s] : nullptr;
    }
    const unsigned gx = (unsigned)(new_tiles > L.qpad / 64 ? new_tiles : L.qpad / 64);
    hipLaunchKernelGGL(k_paged_prefill_prep, dim3(gx, (unsigned)(n_heads + 2 * n_kv_heads)), dim3(256), 0, (hipStream_t)stream, a);
    BH_HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)(n_heads / hw), (unsigned)(L.qpad / qg));
    BH_HIP_TRY(f16 ? launch_paged_attn<true>(hw, grid, (hipStream_t)stream, b) : launch_paged_attn<false>(hw, grid, (hipStream_t)stream, b));
    return BITNET_HIP_OK;
}

}  // extern "C"
