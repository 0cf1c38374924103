// kernels_kvfork.hip -- fork of a live sequence's KV state (gfx950): the first n positions of every layer's K and V cache of ONE source are copied,
// bit for bit, into the caches of up to kBatchMax destinations by ONE launch.
//
// The reference keeps a cached prompt prefix as a host structure (crates/bitnet-inference/src/prefix_cache.rs: lookup :173 returns the longest cached
// prefix and its opaque cached_state bytes, insert :212 stores one).  Here the state stays on the device, and a prefix hit is a device-to-device copy
// of cache slots: eight conversations over one system prompt, or eight samples of one prompt, pay one prompt forward.
//
// Layouts (kernels_attn.hip), per KV head padded to C = ceil(max_pos / 64) chunks, in 32-bit WORDS (an f16 K word is the (d even, d odd) pair of one
// position, an f16 V word two neighbouring dims), R = D words-rows per chunk for f32 and D / 2 for f16 -- so one code serves both types:
//   K  [kv][C][R][64]     chunks below n / 64 are one contiguous run of (n / 64) * R * 64 words; in the partial chunk the first n % 64 words of each
//                         of its R rows
//   V  [kv][C * 64][R]    the first n rows: one contiguous run of n * R words
// Both runs are whole 16-byte vectors from a 16-byte aligned start (R is 64 or 128).  A workgroup owns a part of one (layer, KV head, K | V) segment;
// every source vector is loaded ONCE and stored n_dst times -- the fan-out is why this is a kernel and not 2 * n_layers hipMemcpy2DAsync calls per
// destination.  Integer loads and stores: NaN payloads and denormals pass through unchanged.  Nothing outside the copied slots is written.
#include "common.hpp"

namespace bitnet_hip {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// the cache pointers come out of pointer tables: typed as GLOBAL memory here, or the copy compiles to flat loads and stores
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
__device__ __forceinline__ g_u32 *as_global(const void *p) { return reinterpret_cast<g_u32 *>(reinterpret_cast<uintptr_t>(p)); }

struct KvForkArgs {
    const void *const *src_k, *const *src_v;  // [n_layers]
    void *const *dst_k, *const *dst_v;        // [n_dst][n_layers]
    unsigned n_layers, n_dst, n_kv, rows;     // rows = R above
    unsigned parts;                           // workgroups per segment
    size_t head_words;                        // C * 64 * R
    size_t n;                                 // positions to copy (>= 1)
};

constexpr int kForkThreads = 256;
constexpr int kForkUnroll = 4;  // 16-byte loads in flight per lane before the first store

__global__ __launch_bounds__(kForkThreads) void k_kv_fork(const KvForkArgs a) {
    const unsigned seg = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
    const unsigned is_v = seg & 1u, kv = (seg >> 1) % a.n_kv, layer = (seg >> 1) / a.n_kv;
    const size_t base = (size_t)kv * a.head_words;
    const g_u32 *src = as_global((is_v ? a.src_v : a.src_k)[layer]) + base;
    g_u32 *dst[kBatchMax];
#pragma unroll
    for (int d = 0; d < kBatchMax; ++d)
        dst[d] = (unsigned)d < a.n_dst ? as_global((is_v ? a.dst_v : a.dst_k)[(size_t)d * a.n_layers + layer]) + base : nullptr;

    // the contiguous run, in 16-byte vectors
    const size_t whole = a.n / 64;
    const size_t run4 = is_v ? a.n * (a.rows / 4) : whole * 16 * a.rows;
    const size_t stride = (size_t)a.parts * kForkThreads;
    const g_u32x4 *s4 = reinterpret_cast<const g_u32x4 *>(src);
    size_t i = (size_t)part * kForkThreads + threadIdx.x;
    for (; i + (kForkUnroll - 1) * stride < run4; i += kForkUnroll * stride) {
        u32x4 v[kForkUnroll];
#pragma unroll
        for (int u = 0; u < kForkUnroll; ++u) v[u] = s4[i + u * stride];
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < a.n_dst) {
#pragma unroll
                for (int u = 0; u < kForkUnroll; ++u) reinterpret_cast<g_u32x4 *>(dst[d])[i + u * stride] = v[u];
            }
    }
    for (; i < run4; i += stride) {
        const u32x4 v = s4[i];
#pragma unroll
        for (int d = 0; d < kBatchMax; ++d)
            if ((unsigned)d < a.n_dst) reinterpret_cast<g_u32x4 *>(dst[d])[i] = v;
    }

    // K only: the partial chunk, the first n % 64 words of each of its R rows (dword accesses: at most 63 * R words per head)
    const unsigned tail = (unsigned)(a.n % 64);
    if (!is_v && tail) {
        const size_t chunk0 = whole * 64 * a.rows;
        const unsigned words = a.rows * 64;
        for (unsigned j = part * kForkThreads + threadIdx.x; j < words; j += a.parts * kForkThreads) {
            if ((j & 63u) >= tail) continue;
            const unsigned w = src[chunk0 + j];
#pragma unroll
            for (int d = 0; d < kBatchMax; ++d)
                if ((unsigned)d < a.n_dst) dst[d][chunk0 + j] = w;
        }
    }
}

}  // namespace

// The callers hold the guards: 1 <= n_dst <= kBatchMax, rows in {64, 128}, n >= 1, n <= max_pos, head_words = ceil(max_pos / 64) * 64 * rows,
// 2 * n_layers * n_kv < 2^24.
hipError_t launch_kv_fork(const void *const *src_k, const void *const *src_v, void *const *dst_k, void *const *dst_v, size_t n_layers, size_t n_dst,
                          size_t n_kv, size_t rows, size_t head_words, size_t n, hipStream_t stream) {
    KvForkArgs a;
    a.src_k = src_k, a.src_v = src_v, a.dst_k = dst_k, a.dst_v = dst_v;
    a.n_layers = (unsigned)n_layers, a.n_dst = (unsigned)n_dst, a.n_kv = (unsigned)n_kv, a.rows = (unsigned)rows;
    a.head_words = head_words, a.n = n;
    // memory-bound: about 2048 workgroups (8 per CU) in all, the rest of a segment is strided; no more parts than the longest run (V's) has
    // workgroup-wide vectors, and at least one (the partial K chunk is strided by the same parts)
    const size_t segments = 2 * n_layers * n_kv;
    const size_t want = segments >= 2048 ? 1 : 2048 / segments;
    const size_t have = div_ceil(n * (rows / 4), (size_t)kForkThreads);
    a.parts = (unsigned)(want < have ? want : have);
    // plain loads and stores: the non-temporal forms measured 3-6 % faster at one destination x 4096 positions, slower at seven destinations and
    // at short prefixes (EXPERIMENTS.md 17)
    hipLaunchKernelGGL(k_kv_fork, dim3((unsigned)(segments * a.parts)), dim3(kForkThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace bitnet_hip
