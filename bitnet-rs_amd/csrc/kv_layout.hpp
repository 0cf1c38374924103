// kv_layout.hpp -- the KV cache layout, private to this library, and what every kernel that touches a cache shares: the index arithmetic, the
// global-memory pointer types, the segment map of the state movers and their fan-out run copy.  Integer arithmetic only: no float operation
// lives here, so a translation unit's floating-point flags cannot matter to it.
//
// One cache = one layer's K or V of one sequence, n_kv heads of D = 128 dims, room for max_pos positions.  A head is padded to
// C = ceil(max_pos / 64) CHUNKS of 64 positions, so a whole chunk can always be read: positions at or past the context hold stale bytes that
// the readers discard.  Stated in 32-bit WORDS, R per position and head: an f32 cache holds one dim per word (R = 128), an f16 cache two
// (R = 64), and one code serves both types:
//   K  [kv][C][R][64]    position-fastest inside a chunk: word (row r, position p) of a head at ((p / 64) * R + r) * 64 + p % 64.  One chunk's
//                        keys are R * 256 contiguous bytes (a plain [D][max_pos] transpose scatters them over 128 runs of 256 B, which HBM
//                        serves badly at long contexts), and the score pass reads positions contiguously (lane = position).
//   V  [kv][C * 64][R]   dimension-fastest: position p is row p, words p * R ..; the P.V pass reads dims contiguously (lane = dim).
// f32: row r is dim r.  f16: a K word is the dim pair (2 r, 2 r + 1) of ONE position, low half first -- element (d, p) is half d % 2 of word
// (d / 2, p) -- and a V word is the neighbouring dims (2 r, 2 r + 1) of its position; values are rounded once, from the exact f32 k / v, when
// they are appended.  K is cached AFTER RoPE, which pairs dims (i, i + 64): rows i and i + 64 of an f32 cache; in an f16 cache dims
// (2 r, 2 r + 1) of row r pair with dims (2 r + 64, 2 r + 65) of row r + 32.
// Every row and every chunk starts 16-byte aligned (R is 64 or 128).  A cache is zero-filled before its first use (include/bitnet_hip.h): the
// readers multiply the stale bytes by zero weights, so they must be finite bit patterns.  A cache is f16 or f32 for its whole life.
#pragma once

#include "common.hpp"

namespace bitnet_hip {

constexpr int kKvChunk = 64;  // positions per chunk
constexpr int kKvDim = 128;   // D

// R: words per position and head
__host__ __device__ constexpr unsigned kv_rows(bool f16) { return f16 ? kKvDim / 2 : kKvDim; }
// words before chunk `chunk` of a head
__host__ __device__ constexpr size_t kv_chunk_words(size_t chunk, size_t rows) { return chunk * rows * kKvChunk; }
// words of one head
__host__ __device__ constexpr size_t kv_head_words(size_t max_pos, size_t rows) { return kv_chunk_words((max_pos + kKvChunk - 1) / kKvChunk, rows); }
// ELEMENTS of one head, either type (an f32 cache's words)
__host__ __device__ __forceinline__ size_t kv_head_floats(int max_pos) { return kv_chunk_words((size_t)((max_pos + 63) / 64), kKvDim); }
// elements before the chunk that holds position pos, either type
__host__ __device__ __forceinline__ size_t kv_chunk_floats(int pos) { return kv_chunk_words((size_t)(pos >> 6), kKvDim); }
// K: word (row, pos) of a head
__host__ __device__ __forceinline__ size_t kv_k_word(int row, int pos, int rows) { return ((size_t)(pos >> 6) * rows + row) * 64 + (pos & 63); }
// K, f32: element (dim d, pos) of a head
__host__ __device__ __forceinline__ size_t kidx(int d, int pos) { return kv_k_word(d, pos, kKvDim); }
// K, f16: element (dim d, pos) of a head, in halves
__host__ __device__ __forceinline__ size_t kidx16(int d, int pos) { return kv_k_word(d >> 1, pos, kKvDim / 2) * 2 + (d & 1); }

// ---- the state movers (kernels_kvfork / kvsnap / kvshift .hip, k_kv_permute) ----

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// the cache pointers come out of pointer tables: typed as GLOBAL memory, or a copy compiles to flat loads and stores
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
__device__ __forceinline__ g_u32 *as_global(const void *p) { return reinterpret_cast<g_u32 *>(reinterpret_cast<uintptr_t>(p)); }
__device__ __forceinline__ g_u32x4 *as_global4(const void *p) { return reinterpret_cast<g_u32x4 *>(reinterpret_cast<uintptr_t>(p)); }

// The movers cut their grid into 2 * n_layers * n_kv SEGMENTS, one per (layer, KV head, K | V), of `parts` workgroups each.  Segments never
// share a word.  base() = the head's first word in its cache: computed where the kernel asks for it, so that each kernel keeps the instruction
// order it had when it spelt the map out.
struct KvSegment {
    unsigned is_v, kv, layer, part;
    __device__ __forceinline__ size_t base(size_t head_words) const { return (size_t)kv * head_words; }
};
__device__ __forceinline__ KvSegment kv_segment(unsigned block, unsigned parts, unsigned n_kv) {
    const unsigned seg = block / parts, part = block % parts;
    const unsigned is_v = seg & 1u, kv = (seg >> 1) % n_kv, layer = (seg >> 1) / n_kv;
    return {is_v, kv, layer, part};
}

// Workgroups per segment of a memory-bound mover: about 2048 (8 per CU) in all, the rest of a segment is strided; never more than the segment
// `have` units of work for, and at least one.
inline unsigned kv_parts(size_t segments, size_t have) {
    const size_t want = segments >= 2048 ? 1 : 2048 / segments;
    return (unsigned)(want < have ? want : have);
}

constexpr int kKvCopyThreads = 256;  // the workgroup of kv_copy_run's callers
constexpr int kKvCopyUnroll = 4;     // 16-byte loads in flight per lane before the first store

// A contiguous run of run4 16-byte vectors, strided over the `parts` workgroups of a segment: every vector is loaded ONCE and stored n_dst
// times (dst holds kBatchMax entries; those at and past n_dst are not touched).  Integer loads and stores: NaN payloads and denormals pass through unchanged.
__device__ __forceinline__ void kv_copy_run(const g_u32 *src, g_u32 *const *dst, unsigned n_dst, size_t run4, unsigned part, unsigned parts) {
    const size_t stride = (size_t)parts * kKvCopyThreads;
    const g_u32x4 *s4 = reinterpret_cast<const g_u32x4 *>(src);
    size_t i = (size_t)part * kKvCopyThreads + threadIdx.x;
    for (; i + (kKvCopyUnroll - 1) * stride < run4; i += kKvCopyUnroll * stride) {
        u32x4 v[kKvCopyUnroll];
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; ++u) v[u] = s4[i + u * stride];
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < n_dst) {
#pragma unroll
                for (int u = 0; u < kKvCopyUnroll; ++u) reinterpret_cast<g_u32x4 *>(dst[d])[i + u * stride] = v[u];
            }
    }
    for (; i < run4; i += stride) {
        const u32x4 v = s4[i];
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < n_dst) reinterpret_cast<g_u32x4 *>(dst[d])[i] = v;
    }
}

}  // namespace bitnet_hip
