// kernels_pagedshared.hip -- the paged decode attention for fork groups (gfx950): the pages a group of sequences shares are read ONCE per group, as one
// matrix product, and each member's private pages by the paged attention itself (include/bitnet_hip_pagedshared.h).
//
//   k_attn_paged_shared<KV16>  grid (n_kv, n_shared_splits, n_groups) x 256 threads.  Workgroup (kvh, s, z) serves the group led by row gleader[z]:
//       members    rows b with leader[b] == the leader and a run S > 0.  A member is LIVE by the paged attention's own rules (table and position
//                  pointers, 0 <= *pos < key_bound, every page id of ITS context < n_pages: k_attn_paged reaches the same verdict on the same words);
//                  the live members are compacted in row order.  The run's S ids are read through the table of the first live member, ALL of them
//                  checked by every workgroup before the first tile address is formed; this workgroup keeps its own (s, s + n_shared_splits, ...);
//       query      4 (or `group`) heads per live member, RoPE at the member's own position, times 1/sqrt(128) log2(e), f16, into an LDS image of
//                  rows x 128, rows padded to 16 with zeros; 16-byte unit u of row r at u ^ (r & 15), so the 16 rows of an operand read spread
//                  over all banks;
//       tiles      paged_stage.hpp: each page tile staged once for all four waves, K in the page's order, V transposed on the write, f32 pools
//                  rounded to f16; double buffer, tile t + 1 in flight while tile t is multiplied, one barrier per tile;
//       products   S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16 (k_prefill_attn_paged's operand orders), f32 accumulation, f32 online
//                  softmax in base 2, P rounded to f16.  No mask: every shared key is visible to every member.  With nt row tiles of 16:
//                    nt >= 4   wave w owns row tiles w, w + 4, w + 8, w + 12 and all 64 keys of a page;
//                    nt < 4    the spare waves split the page's keys: nt = 1 -> 4 waves x 16 keys, nt = 2 -> 2 x 2 waves x 32 keys (nt = 3: one
//                              wave rests); their (m, l, o) meet in LDS after the walk and are merged in wave order;
//       records    per (member, KV head, shared split) one record of k_attn_paged's format (natural-log m, un-normalised l and o) into the shared
//                  region of the scratch.  A split without a page leaves (m, l, o) = (-inf, 0, 0).
//   The suffix pass is k_attn_paged's body (kernels_kvpaged.hip, attn_paged_launch with an AttnPagedLead): the second launch of the stream.
// LDS: 64 KiB of tiles + 256 B per query row (64 KiB at 256 rows) dynamic, 2 KiB static: above the default limit, raised by raise_dynamic_lds.
#include "common.hpp"
#include "kv_layout.hpp"
#include "kv_paged.hpp"
#include "paged_attn.hpp"
#include "paged_shared_splits.hpp"
#include "paged_stage.hpp"
#include "wave.hpp"

namespace bitnet_hip {

namespace {

constexpr int kShIdCap = 256;   // own page ids kept in LDS; beyond: read again from the (checked) table
constexpr int kShNQ = 4;        // row tiles of 16 per wave: 4 waves x 4 x 16 = 256 rows
constexpr int kShMergeLd = 132; // floats per query of a wave's partial in the key-split merge: o[128], m, l, padded to 16 bytes

struct AttnSharedArgs {
    const float *qkv, *rope_sin, *rope_cos;
    const uint32_t *kpool, *vpool;
    const uint32_t *const *tables;
    const int *const *pos_ptrs;
    float *records;  // [n_seq][n_kv][n_shared_splits][kPgRec]
    unsigned n_pages;
    int n_seq, n_heads, n_kv, group, key_bound, n_shared_splits;
    int gleader[kWideMax], leader[kWideMax], shared[kWideMax];
};

template <bool KV16>
__global__ __launch_bounds__(256) void k_attn_paged_shared(const AttnSharedArgs a) {
    constexpr int R = KV16 ? kPgD / 2 : kPgD;
    extern __shared__ __attribute__((aligned(16))) uint8_t sh_lds[];  // [2][K tile | V^T tile], then the query image
    __shared__ uint32_t ids[kShIdCap];
    __shared__ int cand_pos[kWideMax], cand_bad[kWideMax], m_row[kWideMax], m_pos[kWideMax];
    __shared__ int n_live_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, ss = blockIdx.y, L = a.gleader[blockIdx.z];
    const int S = a.shared[L], nss = a.n_shared_splits, group = a.group, n_kv = a.n_kv;

    // ---- members: the pointer and position rules, then every page id of each candidate's own context (k_attn_paged's verdict) ----
    if (tid < kWideMax) {
        int p = -1;
        if (tid < a.n_seq && a.leader[tid] == L && a.shared[tid] > 0) {
            const uint32_t *tb = a.tables[tid];
            const int *pp = a.pos_ptrs[tid];
            if (tb && pp) {
                const int v = *pp;
                if (v >= 0 && v < a.key_bound) p = v;
            }
        }
        cand_pos[tid] = p;
        cand_bad[tid] = 0;
    }
    __syncthreads();
    for (int b = 0; b < a.n_seq; ++b) {
        const int p = cand_pos[b];
        if (p < 0) continue;  // block-uniform
        const uint32_t *tb = a.tables[b];
        for (int i = tid; i <= (p >> 6); i += 256)
            if (tb[i] >= a.n_pages) cand_bad[b] = 1;
    }
    __syncthreads();
    if (wave == 0) {
        const bool live = cand_pos[lane] >= 0 && !cand_bad[lane];
        const unsigned long long mask = __ballot(live);
        const int idx = __popcll(mask & ((1ull << lane) - 1ull));
        if (live) m_row[idx] = lane, m_pos[idx] = cand_pos[lane];
        if (lane == 0) n_live_s = __popcll(mask);
    }
    __syncthreads();
    const int n_live = n_live_s;
    if (n_live == 0) return;  // block-uniform: nobody to serve
    // a run longer than some live member's full pages is a broken promise: no table word behind a member's own context is read (the paged
    // attention reads entries 0 .. pos / 64 only), the group gets no record and its rows come out wrong, never out of bounds
    int min_full = m_pos[0] >> 6;
    for (int i = 1; i < n_live; ++i) min_full = min(min_full, m_pos[i] >> 6);
    if (S > min_full) return;  // block-uniform

    // ---- the run's page ids, through the first live member's table: all S checked, this workgroup's share kept ----
    const uint32_t *tbl = a.tables[m_row[0]];
    bool bad = false;
    for (int i = tid; i < S; i += 256) {
        const uint32_t pg = tbl[i];
        bad |= pg >= a.n_pages;
        const int own = i - ss;
        if (own >= 0 && own % nss == 0 && own / nss < kShIdCap) ids[own / nss] = pg;
    }
    if (__syncthreads_or(bad)) return;  // block-uniform, the same in every workgroup of the group (a broken promise: the members' own checks passed)

    const int rows = n_live * group, nt = (rows + 15) >> 4;  // query rows, row tiles of 16
    const int n_own = ss < S ? (S - ss + nss - 1) / nss : 0;
    auto rec_of = [&](int row) -> float * {  // the record of query row `row` = (member row / group, head row % group)
        const int b = m_row[row / group];
        return a.records + (((size_t)b * n_kv + kvh) * nss + ss) * kPgRec;
    };
    if (n_own == 0) {  // block-uniform: a split without a page
        for (int idx = tid; idx < rows * (kPgD / 4); idx += 256) {
            const int row = idx >> 5, d4 = (idx & 31) * 4;
            float *rec = rec_of(row);
            *reinterpret_cast<float4 *>(rec + 2 * kPgMaxGroup + (row % group) * kPgD + d4) = float4{0.f, 0.f, 0.f, 0.f};
            if (d4 == 0) rec[2 * (row % group)] = -INFINITY, rec[2 * (row % group) + 1] = 0.0f;
        }
        return;
    }

    // ---- the query image ----
    uint8_t *qimg = sh_lds + 2 * kPgBufBytes;
    {
        const float qmul = 1.4426950408889634f * (1.0f / sqrtf((float)kPgD));
        const int ld = (a.n_heads + 2 * n_kv) * kPgD, hd = kPgD / 2;
        for (int idx = tid; idx < nt * 16 * hd; idx += 256) {
            const int row = idx >> 6, j = idx & 63;
            float qa = 0.0f, qb = 0.0f;
            if (row < rows) {
                const int mi = row / group, b = m_row[mi], pos = m_pos[mi];
                const float *q_raw = a.qkv + (size_t)b * ld + (size_t)(kvh * group + row % group) * kPgD;
                const float rs = a.rope_sin[(size_t)pos * hd + j], rc = a.rope_cos[(size_t)pos * hd + j], q0 = q_raw[j], q1 = q_raw[hd + j];
                qa = (q0 * rc - q1 * rs) * qmul;
                qb = (q0 * rs + q1 * rc) * qmul;
            }
            uint8_t *qr = qimg + row * 256;
            *reinterpret_cast<_Float16 *>(qr + (((j >> 3) ^ (row & 15)) * 16) + (j & 7) * 2) = (_Float16)qa;
            *reinterpret_cast<_Float16 *>(qr + ((((hd + j) >> 3) ^ (row & 15)) * 16) + (j & 7) * 2) = (_Float16)qb;
        }
    }

    // ---- who multiplies what (wave-uniform): row tiles tq[q] < nt, key tiles of 16 in kmask ----
    const int ks = nt >= 4 ? 1 : nt == 1 ? 4 : nt == 2 ? 2 : 1, kpart = wave % ks;
    const unsigned kmask = ks == 4 ? 1u << kpart : ks == 2 ? 3u << (2 * kpart) : 0xfu;
    int tq[kShNQ];
    bool act[kShNQ];
#pragma unroll
    for (int q = 0; q < kShNQ; ++q) {
        tq[q] = nt >= 4 ? wave + 4 * q : q == 0 ? wave / ks : nt;
        act[q] = tq[q] < nt;
    }

    PagedTileStage<KV16> st;
    auto page_of = [&](int it) -> uint32_t { return it < kShIdCap ? ids[it] : tbl[ss + it * nss]; };  // (every id passed the check above)
    auto tile_of = [&](const uint32_t *pool, int it) -> const uint32_t * { return pool + kv_page_tile_words(page_of(it), kvh, n_kv, R); };
    st.fetch_k(tile_of(a.kpool, 0), kKvChunk, tid);  // shared pages are full: all 64 positions live
    st.fetch_v(tile_of(a.vpool, 0), kKvChunk, wave, lane);
    v4f o[kShNQ][8];
    float m_run[kShNQ], l_run[kShNQ];
#pragma unroll
    for (int q = 0; q < kShNQ; ++q) {
        m_run[q] = -INFINITY, l_run[q] = 0.0f;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[q][dt] = (v4f){0.f, 0.f, 0.f, 0.f};
    }
    st.commit_k(sh_lds, kKvChunk, tid);
    st.commit_v(sh_lds + kPgTileBytes, wave, lane);
    __syncthreads();  // tile 0 and the query image

    for (int it = 0; it < n_own; ++it) {
        const int par = it & 1;
        const bool more = it + 1 < n_own;  // block-uniform
        if (more) st.fetch_v(tile_of(a.vpool, it + 1), kKvChunk, wave, lane);  // in registers across the first product and the softmax
        const uint32_t *kw = reinterpret_cast<const uint32_t *>(sh_lds + par * kPgBufBytes);
        const uint8_t *vs = sh_lds + par * kPgBufBytes + kPgTileBytes;
        // ---- S^T = K Q^T: this wave's key tiles, reduced over 4 dim chunks of 32; A = 4 words of position column 16 i + c, B = the image ----
        v4f s[kShNQ][4];
#pragma unroll
        for (int q = 0; q < kShNQ; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[q][i] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            h8 qb[kShNQ];
#pragma unroll
            for (int q = 0; q < kShNQ; ++q)
                qb[q] = act[q] ? *reinterpret_cast<const h8 *>(qimg + (16 * tq[q] + c) * 256 + (((4 * ch + g) ^ c) * 16)) : (h8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!((kmask >> i) & 1u)) continue;
                const uint32_t *kp = kw + (16 * ch + 4 * g) * 64 + (16 * (i ^ g) + c);
                const u32x4 w = {kp[0], kp[64], kp[128], kp[192]};
                const h8 ka = __builtin_bit_cast(h8, w);
#pragma unroll
                for (int q = 0; q < kShNQ; ++q)
                    if (act[q]) s[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, qb[q], s[q][i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- online softmax for query column c of each row tile (keys of this lane: 16 i + 4 g + j); key tiles of other waves weigh nothing ----
        h8 pb[kShNQ][2];
#pragma unroll
        for (int q = 0; q < kShNQ; ++q) {
            if (!act[q]) continue;
            float mt = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!((kmask >> i) & 1u)) s[q][i][j] = -INFINITY;
                    mt = fmaxf(mt, s[q][i][j]);
                }
            const float m_new = fmaxf(m_run[q], paged_max_over_g(mt));  // finite: every wave owns 16 visible keys of every page
            const float alpha = __builtin_amdgcn_exp2f(m_run[q] - m_new);  // the first tile: 2^-inf = 0
            m_run[q] = m_new;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) o[q][dt] *= alpha;
            // P^T operand: k-slot (g, j) = key 32 u + 4 g + j (j < 4), 32 u + 16 + 4 g + (j - 4).  l sums the ROUNDED weights, the ones o is built
            // from: the f16 rounding of p then moves the row by 2^-11 sum_j p_j |v_j - out|, not by 2^-11 sum_j p_j |v_j|
            float ls[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pb[q][u][j] = (_Float16)__builtin_amdgcn_exp2f(s[q][2 * u][j] - m_new);
                    pb[q][u][4 + j] = (_Float16)__builtin_amdgcn_exp2f(s[q][2 * u + 1][j] - m_new);
                }
                ls[u] = (((float)pb[q][u][0] + (float)pb[q][u][1]) + ((float)pb[q][u][2] + (float)pb[q][u][3])) +
                        (((float)pb[q][u][4] + (float)pb[q][u][5]) + ((float)pb[q][u][6] + (float)pb[q][u][7]));
            }
            l_run[q] = fmaf(l_run[q], alpha, ls[0] + ls[1]);
        }
        if (more) {  // the buffer tile it - 1 left: every wave passed the barrier below since it read it
            st.commit_v(sh_lds + (par ^ 1) * kPgBufBytes + kPgTileBytes, wave, lane);
            st.fetch_k(tile_of(a.kpool, it + 1), kKvChunk, tid);  // in registers across the second product, where the scores are dead
        }
        // ---- O^T += V^T P^T: unit 4 u + g of dim 16 dt + c, the 32-key halves this wave has keys in ----
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!((kmask >> (2 * u)) & 3u)) continue;
#pragma unroll
            for (int d0 = 0; d0 < 8; d0 += 4) {
#pragma unroll
                for (int dt = d0; dt < d0 + 4; ++dt) {
                    const h8 va = *reinterpret_cast<const h8 *>(vs + (16 * dt + c) * 128 + (((4 * u + g) ^ (c >> 1)) * 16));
#pragma unroll
                    for (int q = 0; q < kShNQ; ++q)
                        if (act[q]) o[q][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb[q][u], o[q][dt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) st.commit_k(sh_lds + (par ^ 1) * kPgBufBytes, kKvChunk, tid);
        __syncthreads();
    }

    // l over the four lanes of a query (m is already the same in all four)
#pragma unroll
    for (int q = 0; q < kShNQ; ++q) {
        l_run[q] += __shfl_xor(l_run[q], 16);
        l_run[q] += __shfl_xor(l_run[q], 32);
    }
    // ---- key split: the partials of waves kpart > 0 meet in the tile buffers (every wave is past the walk's last barrier) and the wave with
    //      kpart 0 merges them in wave order.  Only row tile slot 0 is in use when ks > 1 ----
    if (ks > 1) {  // block-uniform
        float *area = reinterpret_cast<float *>(sh_lds);
        if (kpart > 0 && act[0]) {
            float *pr = area + ((size_t)wave * 16 + c) * kShMergeLd;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<float4 *>(pr + 16 * dt + 4 * g) = float4{o[0][dt][0], o[0][dt][1], o[0][dt][2], o[0][dt][3]};
            if (g == 0) pr[kPgD] = m_run[0], pr[kPgD + 1] = l_run[0];
        }
        __syncthreads();
        if (kpart == 0 && act[0]) {
            for (int k = 1; k < ks; ++k) {
                const float *pr = area + ((size_t)(wave + k) * 16 + c) * kShMergeLd;
                const float mp = pr[kPgD], lp = pr[kPgD + 1];
                const float m_new = fmaxf(m_run[0], mp);
                const float s_old = __builtin_amdgcn_exp2f(m_run[0] - m_new), s_c = __builtin_amdgcn_exp2f(mp - m_new);
                l_run[0] = fmaf(l_run[0], s_old, lp * s_c);
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) {
                    const float4 op = *reinterpret_cast<const float4 *>(pr + 16 * dt + 4 * g);
                    o[0][dt] = (v4f){fmaf(o[0][dt][0], s_old, op.x * s_c), fmaf(o[0][dt][1], s_old, op.y * s_c), fmaf(o[0][dt][2], s_old, op.z * s_c),
                                     fmaf(o[0][dt][3], s_old, op.w * s_c)};
                }
                m_run[0] = m_new;
            }
        }
    }
    // ---- records: lane (c, g) holds dims 16 dt + 4 g .. + 3 of query row 16 tq + c ----
    if (kpart == 0) {
#pragma unroll
        for (int q = 0; q < kShNQ; ++q) {
            const int row = 16 * tq[q] + c;
            if (!act[q] || row >= rows) continue;
            float *rec = rec_of(row);
            const int gh = row % group;
            if (g == 0) rec[2 * gh] = m_run[q] * 0.6931471805599453f, rec[2 * gh + 1] = l_run[q];  // base 2 -> the records' natural-log maximum
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                *reinterpret_cast<float4 *>(rec + 2 * kPgMaxGroup + gh * kPgD + 16 * dt + 4 * g) = float4{o[q][dt][0], o[q][dt][1], o[q][dt][2], o[q][dt][3]};
        }
    }
}

}  // namespace

}  // namespace bitnet_hip

using namespace bitnet_hip;

extern "C" {

size_t bitnet_hip_attention_paged_shared_splits(size_t n_groups, size_t n_kv_heads, size_t shared_pages) {
    return attn_paged_shared_auto_splits(n_groups, n_kv_heads, shared_pages);
}

size_t bitnet_hip_attention_paged_shared_scratch_bytes(size_t n_seq, size_t n_kv_heads, size_t n_splits, size_t n_shared_splits) {
    const size_t base = bitnet_hip_attention_paged_scratch_bytes(n_seq, n_kv_heads, n_splits);
    size_t recs = 0;
    if (!base || __builtin_mul_overflow(n_seq * n_kv_heads, n_shared_splits, &recs) || __builtin_mul_overflow(recs, (size_t)kPgRec * sizeof(float), &recs) ||
        __builtin_add_overflow(base, recs, &recs))
        return 0;
    return recs;
}

int bitnet_hip_attention_decode_paged_shared_dev(const float *qkv, const float *rope_sin, const float *rope_cos, void *kpool, void *vpool, size_t n_pages,
                                                 const uint32_t *const *table_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq, size_t n_heads,
                                                 size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t key_bound, size_t n_splits, void *scratch, int flags,
                                                 void *out, const int32_t *leader, const int32_t *shared_pages, size_t n_shared_splits, void *stream) {
    const char *entry = "attention_decode_paged_shared_dev";
    AttnPagedArgs p;
    if (int rc = attn_paged_front(entry, qkv, rope_sin, rope_cos, kpool, vpool, n_pages, table_ptrs_dev, pos_ptrs_dev, n_seq, n_heads, n_kv_heads, head_dim, max_pos,
                                  key_bound, &n_splits, scratch, flags, out, &p))
        return rc;
    if (!leader || !shared_pages) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to %s", entry);
    const size_t run_max = div_ceil(key_bound, (size_t)64) - 1;
    AttnSharedArgs a{};
    AttnPagedLead lead{};
    size_t s_max = 0, n_groups = 0, members_max = 0;
    for (size_t b = 0; b < n_seq; ++b) {
        const int32_t l = leader[b];
        if (l < 0 || (size_t)l >= n_seq || leader[l] != l)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: leader[%zu] = %d is no leader row of the %zu", entry, b, l, n_seq);
        if (shared_pages[b] < 0 || shared_pages[b] != shared_pages[l] || (size_t)shared_pages[b] > run_max)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: shared_pages[%zu] = %d (its leader's: %d, at most %zu under key_bound %zu)", entry, b, shared_pages[b],
                             shared_pages[l], run_max, key_bound);
        a.leader[b] = l, a.shared[b] = lead.first[b] = shared_pages[b];
        if ((size_t)shared_pages[b] > s_max) s_max = (size_t)shared_pages[b];
    }
    if (n_shared_splits > s_max || n_shared_splits > 65535)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_shared_splits %zu above the longest shared run of %zu pages", entry, n_shared_splits, s_max);
    const bool f16 = (flags & BITNET_HIP_ATTN_CACHE_F16) != 0;
    if (s_max == 0) {  // nothing shared: the paged entry's launch
        BH_HIP_TRY(attn_paged_launch(f16, p, nullptr, n_seq, (hipStream_t)stream));
        return BITNET_HIP_OK;
    }
    for (size_t b = 0; b < n_seq; ++b) {
        if (leader[b] != (int32_t)b || shared_pages[b] == 0) continue;
        size_t members = 0;
        for (size_t m = 0; m < n_seq; ++m) members += leader[m] == (int32_t)b;
        if (members > members_max) members_max = members;
        a.gleader[n_groups++] = (int)b;
    }
    if (n_shared_splits == 0) n_shared_splits = attn_paged_shared_auto_splits(n_groups, n_kv_heads, s_max);
    if (!bitnet_hip_attention_paged_shared_scratch_bytes(n_seq, n_kv_heads, n_splits, n_shared_splits))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_shared_splits %zu)", entry, n_shared_splits);
    a.qkv = qkv, a.rope_sin = rope_sin, a.rope_cos = rope_cos, a.kpool = p.kpool, a.vpool = p.vpool, a.tables = p.tables, a.pos_ptrs = p.pos_ptrs;
    a.records = p.records + n_seq * n_kv_heads * n_splits * (size_t)kPgRec;  // behind the paged entry's own records
    a.n_pages = p.n_pages, a.n_seq = (int)n_seq, a.n_heads = p.n_heads, a.n_kv = p.n_kv, a.group = p.group, a.key_bound = p.key_bound;
    a.n_shared_splits = (int)n_shared_splits;
    lead.records = a.records, lead.n_lead = (int)n_shared_splits;
    const int q_rows = (int)div_ceil(members_max * (size_t)p.group, (size_t)16) * 16;
    const int lds = 2 * kPgBufBytes + q_rows * 256;
    void (*k)(AttnSharedArgs) = f16 ? k_attn_paged_shared<true> : k_attn_paged_shared<false>;
    BH_HIP_TRY(raise_dynamic_lds(k, lds));  // before anything launches
    hipLaunchKernelGGL(k, dim3((unsigned)n_kv_heads, (unsigned)n_shared_splits, (unsigned)n_groups), dim3(256), lds, (hipStream_t)stream, a);
    BH_HIP_TRY(hipGetLastError());
    BH_HIP_TRY(attn_paged_launch(f16, p, &lead, n_seq, (hipStream_t)stream));
    return BITNET_HIP_OK;
}

}  // extern "C"
