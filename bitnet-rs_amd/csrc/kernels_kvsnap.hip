// kernels_kvsnap.hip -- compact snapshots of a live sequence's KV state (gfx950): SAVE packs cache slots [0, n) of every layer's K and V of one
// sequence into a caller-owned buffer with no max_pos in it, RESTORE unpacks the first n positions of such a buffer into the caches of up to
// kBatchMax destinations, each by ONE launch, bit for bit.
//
// The reference's prefix cache (crates/bitnet-inference/src/prefix_cache.rs) holds one opaque `cached_state` byte vector per cached prefix
// (:64-77); the snapshot is that vector on the device.  k_kv_fork copies between caches of equal max_pos; a snapshot costs what its positions
// cost (2 * n_layers * n_kv * S * 128 elements), so a few hundred prefixes stay resident where a few live decoders would.
//
// The snapshot, PUBLIC (include/bitnet_hip_kvsnap.h), position-major, in the cache's element type, no padding to 64:
//   K [n_layers][n_kv][S][128]  then  V [n_layers][n_kv][S][128]
// The caches, private (kernels_kvfork.hip, kernels_attn.hip), per KV head padded to C = ceil(max_pos / 64) chunks, in 32-bit WORDS, R = 128 words
// per position for f32 and 64 for f16:
//   K  [kv][C][R][64]     position-fastest inside a chunk
//   V  [kv][C * 64][R]    dimension-fastest: the snapshot's own order
// In words the snapshot is [S][R] per (layer, KV head) for both: an f16 K word of the cache is the (d even, d odd) pair of one position, which is
// also the word a position-major f16 row holds.  So V is fork's contiguous run copy with another head stride on the snapshot side, and K is a
// [R][64] <-> [64][R] transpose of 32-bit words per chunk, the same code for both types.
//
// The K transpose goes through LDS in 64 x 64 word tiles (one chunk is R / 64 tiles), so that BOTH global sides move whole 16-byte vectors, 16
// lanes on each 256-byte row: a tile row of the source is read as 16 vectors, written to LDS as 64 single words down a column, and the transposed
// row comes back out of LDS as 16 vectors.  LDS holds the tile in the DESTINATION's order, [q][r] with q the destination row, rows of 64 words
// and NO padding; the 4-word slot s = r / 4 of row q is stored at slot s ^ (q / 4) (mod 16).  The bank argument (MI355X LDS: ds_write_b32 is
// served in two 32-lane groups over 32 banks, and 2 addresses on one bank cost it nothing because the store's data transfer takes longer than
// two array cycles; ds_read_b128 is served in four 16-lane groups over 64 banks):
//   - store: lane l of a 32-lane group holds source row r = r0 + l / 16 (r0 even, so both rows share r / 4 and differ in r % 4) and source words
//     4 v + j, v = l % 16; store j goes to row q = 4 v + j, bank (((r / 4) ^ v) % 8) * 4 + r % 4.  Over v = 0..15 the XOR takes every value mod 8
//     twice; the two source rows use different banks.  Exactly 2 addresses on each of 16 banks: free.  Without the XOR all 16 lanes of a row
//     would share ONE bank (row stride 64 = 0 mod 32).
//   - load: a wave reads rows q0 .. q0 + 3 with q0 % 4 == 0, lane l the slot l % 16 of row q0 + l / 16.  All four rows share q / 4, so every
//     16-lane group (which mixes lanes of two rows, but never the same l % 16 twice) reads 16 different slots = all 64 banks once: conflict-free.
//   - padding instead of the XOR cannot do this: 16-byte LDS vectors need a row stride T with T % 4 == 0, and the stores walk down a column in
//     steps of 4 rows, 4 T = 0 or 16 mod 32 -- two banks for 16 lanes, 8-way.
// (The compiler pairs the word stores of rows q, q + 1 into ds_write2st64_b32 -- the two are 64 words apart in one slot.  The argument above is
// made for single word stores; how the paired form is served was not measured.  Measured: restore runs at k_kv_fork's rate, EXPERIMENTS.md 38.)
// Integer loads and stores throughout: NaN payloads and denormals pass.  Nothing outside the named slots is written: save writes S = n positions;
// restore writes slots < n only -- in a partial last chunk of K the first n % 64 words of each row, by dword stores as k_kv_fork does.  Cache
// reads stay inside the padded cache, snapshot reads below position n.
#include "common.hpp"

namespace bitnet_hip {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// the cache pointers come out of pointer tables: typed as GLOBAL memory here, or the copy compiles to flat loads and stores
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
__device__ __forceinline__ g_u32 *as_global(const void *p) { return reinterpret_cast<g_u32 *>(reinterpret_cast<uintptr_t>(p)); }

struct KvSnapArgs {
    const void *const *cache_k, *const *cache_v;  // save: [n_layers]; restore: [n_dst][n_layers]
    const void *snap;                             // K [n_layers][n_kv][S][R] words, then V the same
    unsigned n_layers, n_dst, n_kv, rows;         // rows = R above; n_dst = 1 for save
    unsigned parts;                               // workgroups per (layer, KV head, K | V) segment
    size_t head_words;                            // C * 64 * R
    size_t n, S;                                  // positions to move (>= 1), positions the snapshot holds (>= n; save: == n)
};

constexpr int kSnapThreads = 256;
constexpr int kSnapUnroll = 4;  // 16-byte loads in flight per lane before the first store (V), tile rows per lane (K)
constexpr int kTile = 64;       // the K tile: 64 x 64 words, 16 KB of LDS

// LDS word index of element (destination row q, destination word r) of the tile
__device__ __forceinline__ unsigned tile_at(unsigned q, unsigned r) { return q * kTile + ((((r >> 2) ^ (q >> 2)) & 15u) << 2) + (r & 3u); }

// One 64 x 64 word tile, transposed: dst[d][dst_at + q * dst_stride + r] = src[r * src_stride + q] for q < q_valid (destination rows that exist)
// and r < r_valid (source rows that exist), d < n_dst.  Strides and dst_at in words, multiples of 4; all pointers 16-byte aligned.  With kWords only the named
// words are stored, one by one (a partial chunk of K on the cache side); else whole vectors.
template <bool kWords>
__device__ __forceinline__ void transpose_tile(unsigned *tile, const g_u32 *src, size_t src_stride, unsigned r_valid, g_u32 *const *dst, unsigned n_dst,
                                               size_t dst_at, size_t dst_stride, unsigned q_valid) {
    const unsigned row = threadIdx.x / 16, v = threadIdx.x % 16;
    u32x4 x[kSnapUnroll];
#pragma unroll
    for (int k = 0; k < kSnapUnroll; ++k) {
        const unsigned r = k * 16 + row;
        x[k] = r < r_valid ? *reinterpret_cast<const g_u32x4 *>(src + r * src_stride + v * 4) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < kSnapUnroll; ++k) {
        const unsigned r = k * 16 + row;
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[tile_at(v * 4 + j, r)] = x[k][j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSnapUnroll; ++k) x[k] = *reinterpret_cast<const u32x4 *>(&tile[tile_at(k * 16 + row, v * 4)]);
    __syncthreads();  // the tile may be refilled by the caller's next round
#pragma unroll
    for (int k = 0; k < kSnapUnroll; ++k) {
        const unsigned q = k * 16 + row;
        if (q >= q_valid) continue;
        const size_t at = dst_at + q * dst_stride + v * 4;
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < n_dst) {
                if (!kWords) {
                    *reinterpret_cast<g_u32x4 *>(dst[d] + at) = x[k];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (v * 4 + j < r_valid) dst[d][at + j] = x[k][j];
                }
            }
    }
}

// a contiguous run of run4 16-byte vectors, every vector loaded once and stored n_dst times (k_kv_fork's loop)
__device__ __forceinline__ void copy_run(const g_u32 *src, g_u32 *const *dst, unsigned n_dst, size_t run4, unsigned part, unsigned parts) {
    const size_t stride = (size_t)parts * kSnapThreads;
    const g_u32x4 *s4 = reinterpret_cast<const g_u32x4 *>(src);
    size_t i = (size_t)part * kSnapThreads + threadIdx.x;
    for (; i + (kSnapUnroll - 1) * stride < run4; i += kSnapUnroll * stride) {
        u32x4 x[kSnapUnroll];
#pragma unroll
        for (int u = 0; u < kSnapUnroll; ++u) x[u] = s4[i + u * stride];
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < n_dst) {
#pragma unroll
                for (int u = 0; u < kSnapUnroll; ++u) reinterpret_cast<g_u32x4 *>(dst[d])[i + u * stride] = x[u];
            }
    }
    for (; i < run4; i += stride) {
        const u32x4 x = s4[i];
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < n_dst) reinterpret_cast<g_u32x4 *>(dst[d])[i] = x;
    }
}

template <bool kRestore>
__global__ __launch_bounds__(kSnapThreads) void k_kv_snap(const KvSnapArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned tile[kTile * kTile];
    const unsigned seg = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
    const unsigned is_v = seg & 1u, kv = (seg >> 1) % a.n_kv, layer = (seg >> 1) / a.n_kv;
    const size_t base = (size_t)kv * a.head_words;
    // this segment's [S][R] words of the snapshot, and its head in every cache of the call
    g_u32 *snap = as_global(a.snap) + (((size_t)is_v * a.n_layers + layer) * a.n_kv + kv) * a.S * a.rows;
    g_u32 *cache[kBatchMax];
#pragma unroll
    for (int d = 0; d < kBatchMax; ++d)
        cache[d] = (unsigned)d < a.n_dst ? as_global((is_v ? a.cache_v : a.cache_k)[(size_t)d * a.n_layers + layer]) + base : nullptr;
    g_u32 *const one[kBatchMax] = {snap, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    static_assert(kBatchMax == 8, "the single-destination table above");

    if (is_v) {
        const size_t run4 = a.n * (a.rows / 4);
        if (kRestore) copy_run(snap, cache, a.n_dst, run4, part, a.parts);
        else copy_run(cache[0], one, 1, run4, part, a.parts);
        return;
    }
    // K: tile t = (chunk t / per, cache rows 64 * (t % per) ..) <-> (snapshot positions 64 * chunk .., words 64 * (t % per) ..)
    const unsigned per = a.rows / kTile;
    const size_t tiles = (a.n + 63) / 64 * per;
    for (size_t t = part; t < tiles; t += a.parts) {  // uniform over the workgroup: the barriers inside are reached by all
        const size_t chunk = t / per, sub = t % per;
        const size_t left = a.n - chunk * 64;
        const unsigned valid = left < 64 ? (unsigned)left : 64u;  // positions of this chunk that move
        const size_t c_at = (chunk * a.rows + sub * kTile) * 64;   // 64 cache rows of 64 positions
        const size_t s_at = chunk * 64 * a.rows + sub * kTile;     // 64 snapshot rows (positions), 64 of their R words
        if (!kRestore) {
            transpose_tile<false>(tile, cache[0] + c_at, 64, kTile, one, 1, s_at, a.rows, valid);
        } else if (valid == 64) {
            transpose_tile<false>(tile, snap + s_at, a.rows, kTile, cache, a.n_dst, c_at, 64, kTile);
        } else {
            transpose_tile<true>(tile, snap + s_at, a.rows, valid, cache, a.n_dst, c_at, 64, kTile);
        }
    }
}

template <bool kRestore>
hipError_t launch(const void *const *cache_k, const void *const *cache_v, const void *snap, size_t n_layers, size_t n_dst, size_t n_kv, size_t rows,
                  size_t head_words, size_t n, size_t S, hipStream_t stream) {
    KvSnapArgs a;
    a.cache_k = cache_k, a.cache_v = cache_v, a.snap = snap;
    a.n_layers = (unsigned)n_layers, a.n_dst = (unsigned)n_dst, a.n_kv = (unsigned)n_kv, a.rows = (unsigned)rows;
    a.head_words = head_words, a.n = n, a.S = S;
    // memory-bound, as k_kv_fork: about 2048 workgroups in all, a segment's rest is strided.  One round of a workgroup moves 16 KB on either
    // side (a K tile, or kSnapUnroll vectors per lane of V); no more parts than V has workgroup-wide vector rows, and at least one.
    const size_t segments = 2 * n_layers * n_kv;
    const size_t want = segments >= 2048 ? 1 : 2048 / segments;
    const size_t have = div_ceil(n * (rows / 4), (size_t)kSnapThreads);  // V's vectors in workgroup-wide rows; K's tiles are strided over the same parts
    a.parts = (unsigned)(want < have ? want : have);
    hipLaunchKernelGGL(k_kv_snap<kRestore>, dim3((unsigned)(segments * a.parts)), dim3(kSnapThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

// The callers hold the guards: rows in {64, 128}, n >= 1, n <= max_pos, head_words = ceil(max_pos / 64) * 64 * rows, 2 * n_layers * n_kv < 2^24,
// the snapshot 16-byte aligned and of 2 * n_layers * n_kv * S * rows words; restore: 1 <= n_dst <= kBatchMax, n <= S.
hipError_t launch_kv_save(const void *const *src_k, const void *const *src_v, size_t n_layers, size_t n_kv, size_t rows, size_t head_words, size_t n,
                          void *snap, hipStream_t stream) {
    return launch<false>(src_k, src_v, snap, n_layers, 1, n_kv, rows, head_words, n, n, stream);
}

hipError_t launch_kv_restore(const void *snap, size_t S, void *const *dst_k, void *const *dst_v, size_t n_layers, size_t n_dst, size_t n_kv,
                             size_t rows, size_t head_words, size_t n, hipStream_t stream) {
    return launch<true>(dst_k, dst_v, snap, n_layers, n_dst, n_kv, rows, head_words, n, S, stream);
}

}  // namespace bitnet_hip
