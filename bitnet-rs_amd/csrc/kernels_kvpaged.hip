// kernels_kvpaged.hip -- the paged KV cache (gfx950): the one-token attention over page tables, the movers between a page pool and the contiguous
// caches, the page copy of a diverging fork, and their entry points (include/bitnet_hip_paged.h).  The layout is kv_paged.hpp's.
//
//   k_attn_paged<KV16>  grid (n_kv, n_splits, n_seq) x 256 threads, ONE launch.  Workgroup (kvh, s, b) walks pages s, s + n_splits, ... of sequence b
//                       up to the page of its position and keeps a running (m, l, o) for the whole query group of its KV head:
//       page ids   every workgroup of a sequence reads ALL ids of the context (one strided pass, one dependent load level) -- each must reach the
//                  same verdict on a page id >= n_pages, or the arrival count below would not add up -- and keeps its own in LDS;
//       stream     the K and V tiles of page i + 1 are requested before the arithmetic of page i: a register double buffer (16 + 16 dwords per
//                  page and thread for f16, 32 + 32 for f32).  Lane mappings are the layout's: scores lane = position, wave = 32-dim slice (16 dim
//                  pairs in f16) reduced through LDS; P.V lane = dim (or dim pair), the thread's position class through LDS at the end;
//       softmax    online: per page a fresh partial sum, then ONE fused rescale per accumulator, acc = fma(acc, e^(m_old - m_new), page_sum);
//       append     the workgroup whose share holds the page of position p rotates k and writes k and v into slot p % 64 after its last page
//                  (its loads of that tile are long consumed); it attends to the new token from LDS, as attn_partial_body does;
//       merge      each workgroup leaves one (m, l, o) record; the last to arrive (a vector atomic on a per-(sequence, KV head) counter, agent-scope
//                  fences: select.hpp's last_arriver) merges the n_splits records in SPLIT order -- the bits do not depend on arrival order --
//                  writes the output row and re-arms the counter.
//     The query group has at most 4 rows: a 16- or 32-row MFMA tile would run three-quarters empty, and the kernel is a memory stream whose VALU
//     dot products hide under the loads.
//   k_attn_paged_suffix<KV16>  the same body (attn_paged_body) behind the shared-page pass of kernels_pagedshared.hip: sequence b starts at its first
//                       private chunk and its merge takes the shared pass's records first (paged_attn.hpp: AttnPagedLead).
//   k_kv_page_move      one workgroup per (layer, KV head, K | V, chunk) tile, 16-byte integer loads and stores, both directions.
//   k_kv_page_copy      one workgroup per (layer, KV head, K | V, pair) tile.
#include "common.hpp"
#include "kv_guard.hpp"
#include "kv_layout.hpp"
#include "kv_paged.hpp"
#include "paged_attn.hpp"
#include "paged_splits.hpp"
#include "select.hpp"
#include "wave.hpp"

namespace bitnet_hip {

namespace {

// own page ids kept in LDS: 16384 positions per split.  A workgroup that owns more reads the id of page >= kPgIdCap again from the table -- a
// line the validation pass of this same workgroup has just read (it walks the whole table), so a cache hit, not a second trip to memory;
// the library's own split rule reaches it only beyond 32768 positions
constexpr int kPgIdCap = 256;

// The ONE body of the paged decode attention.  LEAD = false is k_attn_paged as the head comment has it.  LEAD = true is the suffix pass of the shared
// entry (kernels_pagedshared.hip): the walk starts at the sequence's first private chunk and the merge takes the shared pass's records first.
template <bool KV16, bool LEAD>
__device__ __forceinline__ void attn_paged_body(const AttnPagedArgs &a, const AttnPagedLead *ld) {
    constexpr int R = KV16 ? kPgD / 2 : kPgD;  // words per position and head
    constexpr int NL = KV16 ? 16 : 32;         // K dwords, and V dwords, per thread and page
    constexpr int NPQ = KV16 ? 4 : 2;          // position classes of the P.V pass
    const int kvh = blockIdx.x, sp = blockIdx.y, b = blockIdx.z;
    const uint32_t *tbl = a.tables[b];
    const int *pp = a.pos_ptrs[b];
    if (!tbl || !pp) return;  // block-uniform: an idle slot
    const int pos = *pp;
    if (pos < 0 || pos >= a.key_bound) return;  // block-uniform: beyond the caller's bound = idle
    const int t_k = pos + 1, last_chunk = pos >> 6, n_chunks = last_chunk + 1, n_splits = a.n_splits;
    const int first = LEAD ? (ld->first[b] < last_chunk ? ld->first[b] : last_chunk) : 0;  // the first chunk of the walk; the page of pos is always walked
    const int n_lead = LEAD && ld->first[b] > 0 ? ld->n_lead : 0;

    __shared__ uint32_t ids[kPgIdCap];
    __shared__ __attribute__((aligned(16))) float qs[kPgMaxGroup * kPgD];
    __shared__ __attribute__((aligned(16))) float kn[kPgD];
    __shared__ __attribute__((aligned(16))) float vn[kPgD];
    __shared__ float partial[4][kKvChunk][kPgMaxGroup];
    __shared__ __attribute__((aligned(16))) float sc[kPgMaxGroup][NPQ][kKvChunk / NPQ];
    __shared__ __attribute__((aligned(16))) float enew[kPgMaxGroup];
    __shared__ __attribute__((aligned(16))) float alpha_s[kPgMaxGroup];
    __shared__ float red[NPQ * kPgMaxGroup * kPgD];
    __shared__ uint32_t arrived;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hd = kPgD / 2, group = a.group;

    // ---- page ids: all of the context are checked, this workgroup's share goes to LDS; the RoPE operands travel with them ----
    bool bad = false;
    for (int i = tid; i < n_chunks; i += 256) {
        const uint32_t pg = tbl[i];
        bad |= pg >= a.n_pages;
        const int own = i - first - sp;
        if (own >= 0 && own % n_splits == 0 && own / n_splits < kPgIdCap) ids[own / n_splits] = pg;
    }
    {
        const float *row = a.qkv + (size_t)b * (size_t)(a.n_heads + 2 * a.n_kv) * kPgD;
        const float *sr = a.rope_sin + (size_t)pos * hd, *cr = a.rope_cos + (size_t)pos * hd;
        const int rg = wave, rj = lane;  // RoPE on q: 4 heads x 64 rotation pairs
        const float *q_raw = row + (size_t)(kvh * group + (rg < group ? rg : group - 1)) * kPgD;
        const float *k_raw = row + (size_t)a.n_heads * kPgD + (size_t)kvh * kPgD;
        const float rs = sr[rj], rc = cr[rj], rq0 = q_raw[rj], rq1 = q_raw[hd + rj], rk0 = k_raw[rj], rk1 = k_raw[hd + rj];
        const float rv = row[(size_t)(a.n_heads + a.n_kv) * kPgD + (size_t)kvh * kPgD + (tid & 127)];
        float qa = 0.0f, qb = 0.0f;
        if (rg < group) {
            qa = rq0 * rc - rq1 * rs;
            qb = rq0 * rs + rq1 * rc;
        }
        qs[rg * kPgD + rj] = qa;
        qs[rg * kPgD + hd + rj] = qb;
        if (wave == 0) {
            kn[rj] = rk0 * rc - rk1 * rs;
            kn[hd + rj] = rk0 * rs + rk1 * rc;
        }
        if (tid < kPgD) vn[tid] = rv;
    }
    if (__syncthreads_or(bad)) return;  // block-uniform, and the same in every workgroup of the sequence: a page id outside the pool = idle

    const int n_own = first + sp < n_chunks ? (n_chunks - first - sp + n_splits - 1) / n_splits : 0;
    const uint32_t *kpool = a.kpool, *vpool = a.vpool;
    const int n_kv = a.n_kv;
    auto page_of = [&](int it) -> uint32_t { return it < kPgIdCap ? ids[it] : tbl[first + sp + it * n_splits]; };  // (every id passed the check above)
    auto load = [&](uint32_t pg, uint32_t(&k)[NL], uint32_t(&v)[NL]) __attribute__((always_inline)) {
        const size_t tile = kv_page_tile_words(pg, kvh, n_kv, R);
        const uint32_t *kp = kpool + tile + (size_t)(NL * wave) * 64 + lane;  // word (row NL * wave + i, position lane)
#pragma unroll
        for (int i = 0; i < NL; ++i) k[i] = kp[i * 64];
        const uint32_t *vp = vpool + tile + tid;  // f16: (position tid / 64 + 4 i, dim pair tid % 64); f32: (position tid / 128 + 2 i, dim tid % 128)
#pragma unroll
        for (int i = 0; i < NL; ++i) v[i] = vp[i * 256];
    };

    const float scale = 1.0f / sqrtf((float)kPgD);
    float m_run = -INFINITY, l_run = 0.0f;  // of head `wave`, the same in every lane
    float run0[kPgMaxGroup] = {0.0f, 0.0f, 0.0f, 0.0f}, run1[kPgMaxGroup] = {0.0f, 0.0f, 0.0f, 0.0f};  // f32 caches use run0 only

    // one page: the next page's loads first, then scores -> softmax pieces -> P.V on the tiles in k / v
    auto step = [&](int it, uint32_t(&k)[NL], uint32_t(&v)[NL], uint32_t(&kx)[NL], uint32_t(&vx)[NL]) __attribute__((always_inline)) {
        if (it + 1 < n_own) load(page_of(it + 1), kx, vx);
        const int chunk = first + sp + it * n_splits, j0 = chunk * kKvChunk;
        const bool last = chunk == last_chunk;  // the page of the new token, the only partial one (block-uniform)
        // ---- scores: lane = position, wave = 32-dim slice
        if (KV16) {
            if (last) {  // the new token's key comes from LDS, rounded as the page will hold it
                const bool isnew = j0 + lane == pos;
#pragma unroll
                for (int i = 0; i < NL; i += 2) {
                    const float4 k4 = *reinterpret_cast<const float4 *>(kn + 32 * wave + 2 * i);
                    const uint32_t p0 = pack_h2(k4.x, k4.y), p1 = pack_h2(k4.z, k4.w);
                    k[i] = isnew ? p0 : k[i];
                    k[i + 1] = isnew ? p1 : k[i + 1];
                }
            }
            float acc[kPgMaxGroup] = {0.0f, 0.0f, 0.0f, 0.0f}, acc2[kPgMaxGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < NL; i += 2) {
#pragma unroll
                for (int g = 0; g < kPgMaxGroup; ++g) {
                    const float4 q4 = *reinterpret_cast<const float4 *>(qs + g * kPgD + 32 * wave + 2 * i);
                    acc[g] = fma_mix_lo(q4.x, k[i], acc[g]);
                    acc2[g] = fma_mix_hi(q4.y, k[i], acc2[g]);
                    acc[g] = fma_mix_lo(q4.z, k[i + 1], acc[g]);
                    acc2[g] = fma_mix_hi(q4.w, k[i + 1], acc2[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < kPgMaxGroup; ++g) partial[wave][lane][g] = acc[g] + acc2[g];
        } else {
            if (last) {
                const bool isnew = j0 + lane == pos;
#pragma unroll
                for (int i = 0; i < NL; i += 4) {
                    const float4 k4 = *reinterpret_cast<const float4 *>(kn + 32 * wave + i);
                    k[i] = isnew ? __float_as_uint(k4.x) : k[i];
                    k[i + 1] = isnew ? __float_as_uint(k4.y) : k[i + 1];
                    k[i + 2] = isnew ? __float_as_uint(k4.z) : k[i + 2];
                    k[i + 3] = isnew ? __float_as_uint(k4.w) : k[i + 3];
                }
            }
            v2f acc[kPgMaxGroup] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
            for (int i = 0; i < NL; i += 4) {
                const v2f k01 = {__uint_as_float(k[i]), __uint_as_float(k[i + 1])}, k23 = {__uint_as_float(k[i + 2]), __uint_as_float(k[i + 3])};
#pragma unroll
                for (int g = 0; g < kPgMaxGroup; ++g) {
                    const float4 q4 = *reinterpret_cast<const float4 *>(qs + g * kPgD + 32 * wave + i);
                    acc[g] = __builtin_elementwise_fma((v2f){q4.x, q4.y}, k01, acc[g]);
                    acc[g] = __builtin_elementwise_fma((v2f){q4.z, q4.w}, k23, acc[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < kPgMaxGroup; ++g) partial[wave][lane][g] = acc[g][0] + acc[g][1];
        }
        __syncthreads();
        // ---- softmax pieces against the RUNNING maximum: wave g owns head g, lane = position.  Slots at or past the new token hold stale
        //      bytes: whatever their scores are, they are replaced here.  Every page of the walk has a live position, so m_new is finite.
        {
            const int g = wave, j = j0 + lane;
            float s = ((partial[0][lane][g] + partial[1][lane][g]) + partial[2][lane][g]) + partial[3][lane][g];
            s = j < t_k ? s * scale : -INFINITY;
            const float m_new = fmaxf(m_run, wave64_max_f_rows_readlane(s));
            const float e = j < t_k ? expf(s - m_new) : 0.0f;
            const float l_c = wave64_sum_f_rows_readlane(e);
            const float al = expf(m_run - m_new);  // the first page: e^(-inf) = 0
            l_run = fmaf(l_run, al, l_c);
            m_run = m_new;
            // the new token's value is not in the tile registers: its weight goes aside and its slot gets 0
            sc[g][lane % NPQ][lane / NPQ] = j == pos ? 0.0f : e;
            if (j == pos) enew[g] = e;
            if (lane == 0) alpha_s[g] = al;
        }
        __syncthreads();
        // ---- un-normalised P.V of this page from zero, then ONE fused rescale of the running sum.  Stale slots carry exact zero weights
        //      and finite bytes (the pool is zero-filled before first use): no masking.
        const float4 al4 = *reinterpret_cast<const float4 *>(alpha_s);
        const float alg[kPgMaxGroup] = {al4.x, al4.y, al4.z, al4.w};
        if (KV16) {
            const int dp = tid & 63, pq = tid >> 6;
            float a0[kPgMaxGroup] = {0.0f, 0.0f, 0.0f, 0.0f}, a1[kPgMaxGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < NL; i += 4) {
#pragma unroll
                for (int g = 0; g < kPgMaxGroup; ++g) {
                    const float4 w = *reinterpret_cast<const float4 *>(&sc[g][pq][i]);
                    a0[g] = fma_mix_lo(w.x, v[i], a0[g]);
                    a1[g] = fma_mix_hi(w.x, v[i], a1[g]);
                    a0[g] = fma_mix_lo(w.y, v[i + 1], a0[g]);
                    a1[g] = fma_mix_hi(w.y, v[i + 1], a1[g]);
                    a0[g] = fma_mix_lo(w.z, v[i + 2], a0[g]);
                    a1[g] = fma_mix_hi(w.z, v[i + 2], a1[g]);
                    a0[g] = fma_mix_lo(w.w, v[i + 3], a0[g]);
                    a1[g] = fma_mix_hi(w.w, v[i + 3], a1[g]);
                }
            }
            if (last && pq == 0) {  // the new token: value from LDS (rounded as the page will hold it), weight from enew
                const float v0 = (float)(_Float16)vn[2 * dp], v1 = (float)(_Float16)vn[2 * dp + 1];
                const float4 en = *reinterpret_cast<const float4 *>(enew);
                const float eg[kPgMaxGroup] = {en.x, en.y, en.z, en.w};
#pragma unroll
                for (int g = 0; g < kPgMaxGroup; ++g) a0[g] += eg[g] * v0, a1[g] += eg[g] * v1;
            }
#pragma unroll
            for (int g = 0; g < kPgMaxGroup; ++g) run0[g] = fmaf(run0[g], alg[g], a0[g]), run1[g] = fmaf(run1[g], alg[g], a1[g]);
        } else {
            const int d = tid & 127, hp = tid >> 7;
            v2f a2[kPgMaxGroup] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
            for (int i = 0; i < NL; i += 4) {
                const v2f v01 = {__uint_as_float(v[i]), __uint_as_float(v[i + 1])}, v23 = {__uint_as_float(v[i + 2]), __uint_as_float(v[i + 3])};
#pragma unroll
                for (int g = 0; g < kPgMaxGroup; ++g) {
                    const float4 w = *reinterpret_cast<const float4 *>(&sc[g][hp][i]);
                    a2[g] = __builtin_elementwise_fma((v2f){w.x, w.y}, v01, a2[g]);
                    a2[g] = __builtin_elementwise_fma((v2f){w.z, w.w}, v23, a2[g]);
                }
            }
            float ar[kPgMaxGroup];
#pragma unroll
            for (int g = 0; g < kPgMaxGroup; ++g) ar[g] = a2[g][0] + a2[g][1];
            if (last && hp == 0) {
                const float vnd = vn[d];
                const float4 en = *reinterpret_cast<const float4 *>(enew);
                ar[0] += en.x * vnd, ar[1] += en.y * vnd, ar[2] += en.z * vnd, ar[3] += en.w * vnd;
            }
#pragma unroll
            for (int g = 0; g < kPgMaxGroup; ++g) run0[g] = fmaf(run0[g], alg[g], ar[g]);
        }
    };

    {
        uint32_t ka[NL], va[NL], kb[NL], vb[NL];
        if (n_own > 0) load(page_of(0), ka, va);
        for (int it = 0; it < n_own; it += 2) {
            step(it, ka, va, kb, vb);
            if (it + 1 < n_own) step(it + 1, kb, vb, ka, va);
        }
    }

    // ---- append: the share that holds the new token's page, after its last page (whole words: f16 pairs packed by one thread) ----
    if (n_own > 0 && first + sp + (n_own - 1) * n_splits == last_chunk) {
        const size_t tile = kv_page_tile_words(page_of(n_own - 1), kvh, n_kv, R);
        const int slot = pos & 63;
        if (KV16) {
            if (tid < 64) a.kpool[tile + (size_t)tid * 64 + slot] = pack_h2(kn[2 * tid], kn[2 * tid + 1]);
            else if (tid < 128) a.vpool[tile + (size_t)slot * R + (tid - 64)] = pack_h2(vn[2 * (tid - 64)], vn[2 * (tid - 64) + 1]);
        } else {
            if (tid < 128) a.kpool[tile + (size_t)tid * 64 + slot] = __float_as_uint(kn[tid]);
            else a.vpool[tile + (size_t)slot * R + (tid - 128)] = __float_as_uint(vn[tid - 128]);
        }
    }

    // ---- this workgroup's record: the position classes meet through LDS (a share without a page leaves m = -inf, l = 0, o = 0) ----
    float *rec = a.records + (((size_t)b * n_kv + kvh) * n_splits + sp) * kPgRec;
    if (KV16) {
        const int dp = tid & 63, pq = tid >> 6;
#pragma unroll
        for (int g = 0; g < kPgMaxGroup; ++g) {
            red[(pq * kPgMaxGroup + g) * kPgD + 2 * dp] = run0[g];
            red[(pq * kPgMaxGroup + g) * kPgD + 2 * dp + 1] = run1[g];
        }
    } else {
        const int d = tid & 127, hp = tid >> 7;
#pragma unroll
        for (int g = 0; g < kPgMaxGroup; ++g) red[(hp * kPgMaxGroup + g) * kPgD + d] = run0[g];
    }
    __syncthreads();
    {
        const int d = tid & 127, hp = tid >> 7;
#pragma unroll
        for (int g = 2 * hp; g < 2 * hp + 2; ++g) {
            float o = red[g * kPgD + d] + red[(kPgMaxGroup + g) * kPgD + d];
            if (KV16) o = o + (red[(2 * kPgMaxGroup + g) * kPgD + d] + red[(3 * kPgMaxGroup + g) * kPgD + d]);
            rec[2 * kPgMaxGroup + g * kPgD + d] = o;
        }
        if (lane == 0) {
            rec[2 * wave] = m_run;
            rec[2 * wave + 1] = l_run;
        }
    }

    // ---- hand-over: the last workgroup of this (sequence, KV head) to arrive merges the records in split order ----
    if (n_splits > 1) {
        if (!last_arriver(a.tickets + (size_t)b * n_kv + kvh, n_splits, &arrived)) return;
    } else {
        __syncthreads();
    }
    {
        const int g = tid >> 6, d2 = 2 * lane;  // head g, dims d2 and d2 + 1
        float m = -INFINITY, l = 0.0f;
        float2 o = {0.0f, 0.0f};
        auto merge_run = [&](const float *base, int n) __attribute__((always_inline)) {
            for (int s0 = 0; s0 < n; s0 += 4) {
                float mc[4], lc[4];
                float2 oc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float *r = base + (size_t)(s0 + u < n ? s0 + u : s0) * kPgRec;  // past the end: this trip's first record again, dropped below
                    mc[u] = r[2 * g];
                    lc[u] = r[2 * g + 1];
                    oc[u] = *reinterpret_cast<const float2 *>(r + 2 * kPgMaxGroup + g * kPgD + d2);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (s0 + u < n) {  // the first record holds page 0 (or, in a suffix pass, a shared page): m is finite from the first step on; an empty share has e^(-inf) = 0
                        const float m_new = fmaxf(m, mc[u]);
                        const float s_old = expf(m - m_new), s_c = expf(mc[u] - m_new);
                        l = fmaf(l, s_old, lc[u] * s_c);
                        o.x = fmaf(o.x, s_old, oc[u].x * s_c);
                        o.y = fmaf(o.y, s_old, oc[u].y * s_c);
                        m = m_new;
                    }
                }
            }
        };
        if (LEAD) merge_run(ld->records + ((size_t)b * n_kv + kvh) * ld->n_lead * kPgRec, n_lead);  // shared records first, in shared-split order
        merge_run(a.records + ((size_t)b * n_kv + kvh) * n_splits * kPgRec, n_splits);
        if (g < group) {
            const size_t col = (size_t)b * a.n_heads * kPgD + (size_t)(kvh * group + g) * kPgD + d2;
            const float x = o.x / l, y = o.y / l;
            if (a.out) {
                *reinterpret_cast<float2 *>(a.out + col) = make_float2(x, y);
            } else {  // one rounding to nearest-even, the matmuls' f16 row format
                a.out_h[col] = (_Float16)x;
                a.out_h[col + 1] = (_Float16)y;
            }
        }
    }
}

template <bool KV16>
__global__ __launch_bounds__(256) void k_attn_paged(const AttnPagedArgs a) {
    attn_paged_body<KV16, false>(a, nullptr);
}

template <bool KV16>
__global__ __launch_bounds__(256) void k_attn_paged_suffix(const AttnPagedArgs a, const AttnPagedLead ld) {
    attn_paged_body<KV16, true>(a, &ld);
}

// ---- the movers -----------------------------------------------------------------------------------------------------------------------------
struct KvPageMoveArgs {
    const void *const *cache_k, *const *cache_v;  // [n_layers] contiguous caches
    const void *const *pool_k, *const *pool_v;    // [n_layers] pools
    const uint32_t *table;
    unsigned n_pages, n_kv, rows, n_chunks;  // n_chunks = ceil(n / 64) = workgroups per segment
    unsigned to_pages;                       // 1: caches -> pages, 0: pages -> caches
    size_t head_words, n;
};

// Workgroup = one (layer, KV head, K | V, chunk) tile: rows * 16 vectors.  Whole chunks and V rows go as 16-byte vectors; of the partial last
// chunk K moves the first n % 64 words of each row (dword accesses), V its first n % 64 rows.
__global__ __launch_bounds__(kKvCopyThreads) void k_kv_page_move(const KvPageMoveArgs a) {
    const KvSegment s = kv_segment(blockIdx.x, a.n_chunks, a.n_kv);
    const unsigned chunk = s.part;
    const uint32_t pg = a.table[chunk];
    if (pg >= a.n_pages) return;  // block-uniform: a page id outside the pool moves nothing
    g_u32 *cache = as_global((s.is_v ? a.cache_v : a.cache_k)[s.layer]) + s.base(a.head_words) + kv_chunk_words(chunk, a.rows);
    g_u32 *page = as_global((s.is_v ? a.pool_v : a.pool_k)[s.layer]) + kv_page_tile_words(pg, s.kv, a.n_kv, a.rows);
    const g_u32 *src = a.to_pages ? cache : page;
    g_u32 *dst = a.to_pages ? page : cache;
    const size_t live = a.n - (size_t)chunk * 64 < 64 ? a.n - (size_t)chunk * 64 : 64;  // positions of this chunk below n (>= 1)
    const unsigned run4 = s.is_v ? (unsigned)live * (a.rows / 4) : (live == 64 ? a.rows * 16 : 0);
    const g_u32x4 *s4 = reinterpret_cast<const g_u32x4 *>(src);
    g_u32x4 *d4 = reinterpret_cast<g_u32x4 *>(dst);
    unsigned i = threadIdx.x;
    for (; i + (kKvCopyUnroll - 1) * kKvCopyThreads < run4; i += kKvCopyUnroll * kKvCopyThreads) {
        u32x4 v[kKvCopyUnroll];
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; ++u) v[u] = s4[i + u * kKvCopyThreads];
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; ++u) d4[i + u * kKvCopyThreads] = v[u];
    }
    for (; i < run4; i += kKvCopyThreads) d4[i] = s4[i];
    if (!s.is_v && live < 64) {
        const unsigned words = a.rows * 64;
        for (unsigned j = threadIdx.x; j < words; j += kKvCopyThreads)
            if ((j & 63u) < (unsigned)live) dst[j] = src[j];
    }
}

constexpr int kPageCopyMax = 64;

struct KvPageCopyArgs {
    void *const *pool_k, *const *pool_v;  // [n_layers]
    unsigned n_kv, rows, n_pairs;
    uint32_t src[kPageCopyMax], dst[kPageCopyMax];
};

// Workgroup = one (layer, KV head, K | V, pair) tile of rows * 16 vectors.
__global__ __launch_bounds__(kKvCopyThreads) void k_kv_page_copy(const KvPageCopyArgs a) {
    const KvSegment s = kv_segment(blockIdx.x, a.n_pairs, a.n_kv);
    g_u32 *pool = as_global((s.is_v ? a.pool_v : a.pool_k)[s.layer]);
    const g_u32x4 *s4 = reinterpret_cast<const g_u32x4 *>(pool + kv_page_tile_words(a.src[s.part], s.kv, a.n_kv, a.rows));
    g_u32x4 *d4 = reinterpret_cast<g_u32x4 *>(pool + kv_page_tile_words(a.dst[s.part], s.kv, a.n_kv, a.rows));
    const unsigned run4 = a.rows * 16;  // a multiple of kKvCopyUnroll * kKvCopyThreads
    for (unsigned i = threadIdx.x; i < run4; i += kKvCopyUnroll * kKvCopyThreads) {
        u32x4 v[kKvCopyUnroll];
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; ++u) v[u] = s4[i + u * kKvCopyThreads];
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; ++u) d4[i + u * kKvCopyThreads] = v[u];
    }
}
static_assert((kKvDim / 2) * 16 % (kKvCopyUnroll * kKvCopyThreads) == 0, "k_kv_page_copy's loop has no tail");

// ---- the refusals the entries share ----
// bytes of one pool, or 0: a geometry the launches refuse or a product that wraps (page ids stay below 2^31)
size_t pool_bytes(size_t n_pages, size_t n_kv_heads, size_t head_dim, bool f16) {
    size_t bytes = 0;
    if (n_pages == 0 || n_pages >= ((size_t)1 << 31) || n_kv_heads == 0 || head_dim != 128) return 0;
    if (__builtin_mul_overflow(n_pages, n_kv_heads, &bytes) || __builtin_mul_overflow(bytes, (size_t)kv_rows(f16) * kKvChunk * sizeof(uint32_t), &bytes)) return 0;
    return bytes;
}

int check_pool(const char *entry, size_t n_pages, size_t n_kv_heads, size_t head_dim, bool f16) {
    if (n_pages == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_pages 0", entry);
    if (!pool_bytes(n_pages, n_kv_heads, head_dim, f16))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_pages %zu, n_kv_heads %zu)", entry, n_pages, n_kv_heads);
    return BITNET_HIP_OK;
}

int page_move(const char *entry, bool to_pages, const void *const *k_ptrs, const void *const *v_ptrs, const void *const *kpool_ptrs, const void *const *vpool_ptrs,
              const uint32_t *table, size_t n_pages, size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t n_positions, int flags,
              void *stream) {
    if (!k_ptrs || !v_ptrs || !kpool_ptrs || !vpool_ptrs || !table) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to %s", entry);
    if (int rc = kv_guard_shape(entry, n_layers, n_kv_heads, head_dim, flags)) return rc;
    if (n_positions > max_pos)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "KV cache overflow: n_positions %zu, max_pos %zu", n_positions, max_pos);
    KvGeometry g;
    if (int rc = kv_guard_sizes(entry, n_layers, 1, n_kv_heads, head_dim, max_pos, (size_t)0x7fffffff - 63, flags, &g)) return rc;
    if (int rc = check_pool(entry, n_pages, n_kv_heads, head_dim, (flags & BITNET_HIP_ATTN_KV_F16) != 0)) return rc;
    if (n_positions == 0) return BITNET_HIP_OK;  // valid, and nothing to launch
    const size_t n_chunks = div_ceil(n_positions, (size_t)64);
    size_t blocks = 0;
    if (__builtin_mul_overflow(g.segments, n_chunks, &blocks) || blocks > (size_t)0x7fffffff)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: %zu segments of %zu chunks)", entry, g.segments, n_chunks);
    KvPageMoveArgs a;
    a.cache_k = k_ptrs, a.cache_v = v_ptrs, a.pool_k = kpool_ptrs, a.pool_v = vpool_ptrs, a.table = table;
    a.n_pages = (unsigned)n_pages, a.n_kv = (unsigned)n_kv_heads, a.rows = (unsigned)g.rows, a.n_chunks = (unsigned)n_chunks, a.to_pages = to_pages;
    a.head_words = g.head_words, a.n = n_positions;
    hipLaunchKernelGGL(k_kv_page_move, dim3((unsigned)blocks), dim3(kKvCopyThreads), 0, (hipStream_t)stream, a);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

}  // namespace

// ---- the front and the launch kernels_pagedshared.hip borrows (paged_attn.hpp) ----
int attn_paged_front(const char *entry, const float *qkv, const float *rope_sin, const float *rope_cos, void *kpool, void *vpool, size_t n_pages,
                     const uint32_t *const *table_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq, size_t n_heads, size_t n_kv_heads, size_t head_dim,
                     size_t max_pos, size_t key_bound, size_t *n_splits, void *scratch, int flags, void *out, AttnPagedArgs *a) {
    if (n_seq == 0 || n_seq > BITNET_HIP_WIDE_MAX)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_seq %zu must be 1..%d", entry, n_seq, BITNET_HIP_WIDE_MAX);
    if (!qkv || !rope_sin || !rope_cos || !kpool || !vpool || !table_ptrs_dev || !pos_ptrs_dev || !scratch || !out)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to %s", entry);
    if (flags & ~(BITNET_HIP_ATTN_CACHE_F16 | BITNET_HIP_ATTN_OUT_F16))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x (BITNET_HIP_ATTN_CACHE_F16 | BITNET_HIP_ATTN_OUT_F16)", entry, flags);
    if (n_kv_heads == 0 || n_heads % n_kv_heads != 0)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "num_heads %zu must be divisible by num_key_value_heads %zu", n_heads, n_kv_heads);
    if (head_dim != 128 || n_heads / n_kv_heads > 4 || n_heads == 0)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: head_dim %zu / group %zu unsupported (head_dim 128, group 1..4)", entry, head_dim, n_heads / n_kv_heads);
    const bool f16 = (flags & BITNET_HIP_ATTN_CACHE_F16) != 0;
    if (int rc = check_pool(entry, n_pages, n_kv_heads, head_dim, f16)) return rc;
    // positions are ints in the kernel, the grid's x takes the KV heads
    if (max_pos == 0 || max_pos > ((size_t)1 << 24) || n_heads > 65535)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_heads %zu, max_pos %zu)", entry, n_heads, max_pos);
    if (key_bound == 0 || key_bound > max_pos)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: key_bound %zu must be 1..max_pos %zu", entry, key_bound, max_pos);
    const size_t pages = div_ceil(key_bound, (size_t)64);
    if (*n_splits > pages || *n_splits > 65535)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_splits %zu above the %zu pages of key_bound %zu", entry, *n_splits, pages, key_bound);
    if (*n_splits == 0) *n_splits = attn_paged_auto_splits(n_seq, n_kv_heads, key_bound);
    if (!bitnet_hip_attention_paged_scratch_bytes(n_seq, n_kv_heads, *n_splits))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_seq %zu, n_kv_heads %zu, n_splits %zu)", entry, n_seq, n_kv_heads,
                         *n_splits);
    a->qkv = qkv, a->rope_sin = rope_sin, a->rope_cos = rope_cos;
    a->kpool = static_cast<uint32_t *>(kpool), a->vpool = static_cast<uint32_t *>(vpool);
    a->tables = table_ptrs_dev, a->pos_ptrs = reinterpret_cast<const int *const *>(pos_ptrs_dev);
    a->tickets = static_cast<uint32_t *>(scratch);
    a->records = reinterpret_cast<float *>(a->tickets + kPgTicketWords * n_kv_heads);
    a->out = (flags & BITNET_HIP_ATTN_OUT_F16) ? nullptr : static_cast<float *>(out);
    a->out_h = (flags & BITNET_HIP_ATTN_OUT_F16) ? static_cast<_Float16 *>(out) : nullptr;
    a->n_pages = (unsigned)n_pages, a->n_heads = (int)n_heads, a->n_kv = (int)n_kv_heads, a->group = (int)(n_heads / n_kv_heads);
    a->key_bound = (int)key_bound, a->n_splits = (int)*n_splits;
    return BITNET_HIP_OK;
}

hipError_t attn_paged_launch(bool f16, const AttnPagedArgs &a, const AttnPagedLead *lead, size_t n_seq, hipStream_t stream) {
    const dim3 grid((unsigned)a.n_kv, (unsigned)a.n_splits, (unsigned)n_seq);
    if (lead) hipLaunchKernelGGL(f16 ? k_attn_paged_suffix<true> : k_attn_paged_suffix<false>, grid, dim3(256), 0, stream, a, *lead);
    else hipLaunchKernelGGL(f16 ? k_attn_paged<true> : k_attn_paged<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace bitnet_hip

using namespace bitnet_hip;

extern "C" {

size_t bitnet_hip_kv_pool_bytes(size_t n_pages, size_t n_kv_heads, size_t head_dim, int f16) { return pool_bytes(n_pages, n_kv_heads, head_dim, f16 != 0); }

size_t bitnet_hip_attention_paged_splits(size_t n_seq, size_t n_kv_heads, size_t key_bound) { return attn_paged_auto_splits(n_seq, n_kv_heads, key_bound); }

size_t bitnet_hip_attention_paged_scratch_bytes(size_t n_seq, size_t n_kv_heads, size_t n_splits) {
    size_t recs = 0, tickets = 0;
    if (n_seq == 0 || n_seq > (size_t)kWideMax || n_kv_heads == 0 || n_splits == 0) return 0;
    if (__builtin_mul_overflow(n_seq, n_splits, &recs) || __builtin_mul_overflow(recs, n_kv_heads, &recs) || __builtin_mul_overflow(recs, (size_t)kPgRec * sizeof(float), &recs) ||
        __builtin_mul_overflow(kPgTicketWords * sizeof(uint32_t), n_kv_heads, &tickets) || __builtin_add_overflow(recs, tickets, &recs))
        return 0;
    return recs;
}

int bitnet_hip_attention_decode_paged_dev(const float *qkv, const float *rope_sin, const float *rope_cos, void *kpool, void *vpool, size_t n_pages,
                                          const uint32_t *const *table_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq, size_t n_heads,
                                          size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t key_bound, size_t n_splits, void *scratch, int flags,
                                          void *out, void *stream) {
    const char *entry = "attention_decode_paged_dev";
    AttnPagedArgs a;
    if (int rc = attn_paged_front(entry, qkv, rope_sin, rope_cos, kpool, vpool, n_pages, table_ptrs_dev, pos_ptrs_dev, n_seq, n_heads, n_kv_heads, head_dim, max_pos,
                                  key_bound, &n_splits, scratch, flags, out, &a))
        return rc;
    BH_HIP_TRY(attn_paged_launch((flags & BITNET_HIP_ATTN_CACHE_F16) != 0, a, nullptr, n_seq, (hipStream_t)stream));
    return BITNET_HIP_OK;
}

int bitnet_hip_kv_page_in_dev(const void *const *k_ptrs_dev, const void *const *v_ptrs_dev, void *const *kpool_ptrs_dev, void *const *vpool_ptrs_dev,
                              const uint32_t *table_dev, size_t n_pages, size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t n_positions,
                              int flags, void *stream) {
    return page_move("kv_page_in_dev", true, k_ptrs_dev, v_ptrs_dev, kpool_ptrs_dev, vpool_ptrs_dev, table_dev, n_pages, n_layers, n_kv_heads, head_dim, max_pos,
                     n_positions, flags, stream);
}

int bitnet_hip_kv_page_out_dev(const void *const *kpool_ptrs_dev, const void *const *vpool_ptrs_dev, const uint32_t *table_dev, size_t n_pages,
                               void *const *k_ptrs_dev, void *const *v_ptrs_dev, size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                               size_t n_positions, int flags, void *stream) {
    return page_move("kv_page_out_dev", false, k_ptrs_dev, v_ptrs_dev, kpool_ptrs_dev, vpool_ptrs_dev, table_dev, n_pages, n_layers, n_kv_heads, head_dim, max_pos,
                     n_positions, flags, stream);
}

int bitnet_hip_kv_page_copy_dev(void *const *kpool_ptrs_dev, void *const *vpool_ptrs_dev, size_t n_pages, const uint32_t *pairs, size_t n_pairs, size_t n_layers,
                                size_t n_kv_heads, size_t head_dim, int flags, void *stream) {
    const char *entry = "kv_page_copy_dev";
    if (!kpool_ptrs_dev || !vpool_ptrs_dev || !pairs) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to %s", entry);
    if (int rc = kv_guard_shape(entry, n_layers, n_kv_heads, head_dim, flags)) return rc;
    if (n_pairs == 0 || n_pairs > (size_t)kPageCopyMax)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_pairs %zu must be 1..%d", entry, n_pairs, kPageCopyMax);
    if (int rc = check_pool(entry, n_pages, n_kv_heads, head_dim, (flags & BITNET_HIP_ATTN_KV_F16) != 0)) return rc;
    size_t segments = 0;
    if (!kv_segments_fit(n_layers, n_kv_heads, &segments))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_layers %zu, n_kv_heads %zu)", entry, n_layers, n_kv_heads);
    KvPageCopyArgs a;
    for (size_t i = 0; i < n_pairs; ++i) {
        a.src[i] = pairs[2 * i], a.dst[i] = pairs[2 * i + 1];
        if (a.src[i] >= n_pages || a.dst[i] >= n_pages)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: pair %zu (%u -> %u) names a page outside the pool of %zu", entry, i, a.src[i], a.dst[i], n_pages);
        for (size_t j = 0; j <= i; ++j)  // a destination is no source of the call (its own included) and no other destination
            if (a.dst[i] == a.src[j] || a.src[i] == a.dst[j] || (j < i && a.dst[i] == a.dst[j]))
                return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: pair %zu (%u -> %u) overlaps pair %zu", entry, i, a.src[i], a.dst[i], j);
    }
    a.pool_k = kpool_ptrs_dev, a.pool_v = vpool_ptrs_dev;
    a.n_kv = (unsigned)n_kv_heads, a.rows = (unsigned)kv_rows((flags & BITNET_HIP_ATTN_KV_F16) != 0), a.n_pairs = (unsigned)n_pairs;
    hipLaunchKernelGGL(k_kv_page_copy, dim3((unsigned)(segments * n_pairs)), dim3(kKvCopyThreads), 0, (hipStream_t)stream, a);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

}  // extern "C"
