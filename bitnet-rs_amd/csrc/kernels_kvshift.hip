// kernels_kvshift.hip -- context shift of a live sequence's KV state (gfx950): in every layer and KV head, cache slot j takes slot j + discard for
// every j in [keep, n - discard) -- V bit for bit, K turned back by the RoPE angle between the two positions -- in place, by ONE launch.
//
// The reference keeps the pieces on the host: KvCacheBuffer::rotate_kv / truncate (crates/bitnet-kernels/src/cuda/kv_cache.rs:305-348) and
// WindowedKVCache (crates/bitnet-gpu-hal/src/sliding_window.rs:161-235).  Here the state lives on the device in private layouts (kernels_attn.hip,
// kernels_kvfork.hip), per KV head padded to C = ceil(max_pos / 64) chunks, in 32-bit WORDS (an f16 K word is the (d even, d odd) pair of one
// position, an f16 V word two neighbouring dims), R = D word-rows per chunk for f32 and D / 2 for f16:
//   K  [kv][C][R][64]     word (row, position % 64) of chunk position / 64
//   V  [kv][C * 64][R]    row j = position j: the move is one contiguous run shifted down by discard * R words (whole 16-byte vectors)
//
// K is cached AFTER RoPE.  The key of slot j + discard was rotated by table row j + discard (sa, ca) and has to look as if rotated by row j (sb, cb).
// Per RoPE pair (x0, x1) = dims (i, i + 64), in f32, unfused (this file is built with -ffp-contract=off) and in this order:
//   c = ca*cb + sa*sb,  s = sa*cb - ca*sb,  x0' = x0*c + x1*s,  x1' = x1*c - x0*s
// The two table rows actually involved, NOT row `discard`: the tables hold sinf / cosf of the f32 product position * inv_freq, and row j + discard is
// not row j composed with row discard to f32 accuracy.  An f16 word is widened exactly and rounded once, to nearest-even.
// In an f32 cache the pair is rows i and i + 64; in an f16 cache dims (2r, 2r + 1) of row r pair with dims (2r + 64, 2r + 65) of row r + 32.
//
// ORDERING: why no slot is read after it was overwritten.  The move is in place and sources [keep + discard, n) overlap destinations
// [keep, n - discard) whenever more than `discard` positions move.
//   (a) A (layer, KV head, K | V) SEGMENT touches only its own words: segments never share a word, so only hazards inside a segment exist.
//   (b) When the ranges overlap, ONE workgroup owns a whole segment (parts == 1) and walks its destination TILES in ascending order; a K tile is
//       one 64-position chunk [64 t, 64 t + 64) cut to the destination range, a V tile 2048 consecutive 16-byte vectors.  Every tile runs
//       load all sources into registers -> __syncthreads() -> store all destinations.
//   (c) Inside a tile: every load of every thread has returned its data before the barrier releases the first store (tile_barrier waits for
//       vmcnt(0) in front of s_barrier), so a store of thread A cannot overtake a load of thread B of the same tile.
//   (d) Across tiles: the sources of tile t' > t lie at or above (start of tile t') + discard, which is above every destination of tile t because
//       discard >= 1 -- a store of tile t never touches a word a LATER tile reads.  The sources of tile t' < t were loaded before the barrier of
//       tile t' that this thread has passed, and a thread reaches the stores of tile t only through the barrier of tile t, which every thread
//       enters after its loads of tiles <= t: nothing EARLIER is still to be read either.
//   (e) When the ranges are disjoint (moved <= discard, the usual "discard half" call) no store touches any source at all, and each segment is
//       split over `parts` workgroups that take every parts-th tile, as k_kv_fork splits its runs.
// The table reads are of constant memory and carry no hazard.  Nothing outside slots [keep, n - discard) is written: slots < keep, the stale slots
// >= n - discard and the padding of the last chunk keep their bytes.
#include "common.hpp"

namespace bitnet_hip {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// the cache pointers come out of pointer tables: typed as GLOBAL memory here, or the move compiles to flat loads and stores
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) const f32x4 g_cf32x4;
__device__ __forceinline__ g_u32 *as_global(const void *p) { return reinterpret_cast<g_u32 *>(reinterpret_cast<uintptr_t>(p)); }
__device__ __forceinline__ g_cf32x4 *as_global4(const float *p) { return reinterpret_cast<g_cf32x4 *>(reinterpret_cast<uintptr_t>(p)); }

struct KvShiftArgs {
    void *const *k, *const *v;   // [n_layers]
    const float *sn, *cs;        // [max_pos][64]
    unsigned n_kv, parts;        // workgroups per segment
    unsigned keep, discard, end; // destinations are slots [keep, end), end = n - discard > keep
    size_t head_words;           // C * 64 * R
};

constexpr int kShiftThreads = 256;
constexpr int kShiftUnroll = 8;  // 16-byte vectors per lane and V tile: 32 words in registers, as a K tile of an f32 cache

// Between a tile's loads and its stores.  The workgroup barrier alone does not wait for outstanding vector loads on gfx950 (the compiler puts no
// s_waitcnt in front of it: the memory model orders a workgroup's accesses in its CU's L1); the wait is spelt out, so that every lane's source
// words ARE in registers before any lane passes the barrier.  The asm holds no load or store of its own; "memory" keeps the tile's loads in front.
__device__ __forceinline__ void tile_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ void rotate(float x0, float x1, float c, float s, float &y0, float &y1) {
    y0 = x0 * c + x1 * s;
    y1 = x1 * c - x0 * s;
}

// One segment of K.  Lane l of wave w holds position 64 * chunk + l and the 16 RoPE pairs i = 16 w .. 16 w + 15 of it: 32 words of an f32 cache
// (rows i and i + 64), 16 words of an f16 cache (rows i / 2 and i / 2 + 32).  A row's 64 lanes read and write 64 consecutive words.
template <bool kF16>
__device__ __forceinline__ void shift_k(g_u32 *base, const KvShiftArgs &a, unsigned part) {
    constexpr unsigned R = kF16 ? 64 : 128;
    constexpr int P = kF16 ? 8 : 16;  // word pairs per thread
    const unsigned l = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned row0 = (unsigned)P * w;
    const unsigned c_last = (a.end - 1) / 64;
    for (unsigned c = a.keep / 64 + part; c <= c_last; c += a.parts) {  // the trip count is the workgroup's: every thread meets every barrier
        const unsigned j = c * 64 + l, js = j + a.discard;
        const bool live = j >= a.keep && j < a.end;
        unsigned lo[P], hi[P];
        float cc[16], ss[16];
        if (live) {
            const g_u32 *src = base + (size_t)(js >> 6) * (R * 64) + (js & 63u);
#pragma unroll
            for (int q = 0; q < P; ++q) lo[q] = src[(row0 + q) * 64], hi[q] = src[(row0 + q + R / 2) * 64];
            g_cf32x4 *sa4 = as_global4(a.sn + (size_t)js * 64 + 16 * w), *ca4 = as_global4(a.cs + (size_t)js * 64 + 16 * w);
            g_cf32x4 *sb4 = as_global4(a.sn + (size_t)j * 64 + 16 * w), *cb4 = as_global4(a.cs + (size_t)j * 64 + 16 * w);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 sa = sa4[g], ca = ca4[g], sb = sb4[g], cb = cb4[g];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cc[4 * g + e] = ca[e] * cb[e] + sa[e] * sb[e];
                    ss[4 * g + e] = sa[e] * cb[e] - ca[e] * sb[e];
                }
            }
        }
        tile_barrier();
        if (live) {
            g_u32 *dst = base + (size_t)c * (R * 64) + l;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                unsigned out_lo, out_hi;
                if constexpr (kF16) {
                    const f16x2 x0 = __builtin_bit_cast(f16x2, lo[q]), x1 = __builtin_bit_cast(f16x2, hi[q]);
                    f16x2 y0, y1;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float r0, r1;
                        rotate((float)x0[h], (float)x1[h], cc[2 * q + h], ss[2 * q + h], r0, r1);
                        y0[h] = (_Float16)r0, y1[h] = (_Float16)r1;
                    }
                    out_lo = __builtin_bit_cast(unsigned, y0), out_hi = __builtin_bit_cast(unsigned, y1);
                } else {
                    float r0, r1;
                    rotate(__builtin_bit_cast(float, lo[q]), __builtin_bit_cast(float, hi[q]), cc[q], ss[q], r0, r1);
                    out_lo = __builtin_bit_cast(unsigned, r0), out_hi = __builtin_bit_cast(unsigned, r1);
                }
                dst[(row0 + q) * 64] = out_lo, dst[(row0 + q + R / 2) * 64] = out_hi;
            }
        }
    }
}

// One segment of V: rows [keep, end) take rows [keep + discard, end + discard), a run of whole 16-byte vectors moved down by discard * R / 4 vectors.
__device__ __forceinline__ void shift_v(g_u32 *base, const KvShiftArgs &a, unsigned rows, unsigned part) {
    constexpr size_t kTile = (size_t)kShiftThreads * kShiftUnroll;
    const size_t lo = (size_t)a.keep * (rows / 4), hi = (size_t)a.end * (rows / 4), sh = (size_t)a.discard * (rows / 4);
    g_u32x4 *p4 = reinterpret_cast<g_u32x4 *>(base);
    for (size_t t0 = lo + (size_t)part * kTile; t0 < hi; t0 += (size_t)a.parts * kTile) {  // workgroup-uniform, as above
        u32x4 v[kShiftUnroll];
#pragma unroll
        for (int u = 0; u < kShiftUnroll; ++u) {
            const size_t i = t0 + (size_t)u * kShiftThreads + threadIdx.x;
            if (i < hi) v[u] = p4[i + sh];
        }
        tile_barrier();
#pragma unroll
        for (int u = 0; u < kShiftUnroll; ++u) {
            const size_t i = t0 + (size_t)u * kShiftThreads + threadIdx.x;
            if (i < hi) p4[i] = v[u];
        }
    }
}

template <bool kF16>
__global__ __launch_bounds__(kShiftThreads) void k_kv_shift(const KvShiftArgs a) {
    const unsigned seg = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
    const unsigned is_v = seg & 1u, kv = (seg >> 1) % a.n_kv, layer = (seg >> 1) / a.n_kv;
    g_u32 *base = as_global((is_v ? a.v : a.k)[layer]) + (size_t)kv * a.head_words;
    if (is_v)
        shift_v(base, a, kF16 ? 64u : 128u, part);
    else
        shift_k<kF16>(base, a, part);
}

}  // namespace

// The callers hold the guards: rows in {64, 128}, discard >= 1, keep + discard < n <= max_pos < 2^31, head_words = ceil(max_pos / 64) * 64 * rows,
// 2 * n_layers * n_kv < 2^24, tables of max_pos rows.
hipError_t launch_kv_shift(void *const *k_ptrs, void *const *v_ptrs, const float *rope_sin, const float *rope_cos, size_t n_layers, size_t n_kv, size_t rows,
                           size_t head_words, size_t keep, size_t discard, size_t n, hipStream_t stream) {
    KvShiftArgs a;
    a.k = k_ptrs, a.v = v_ptrs, a.sn = rope_sin, a.cs = rope_cos;
    a.n_kv = (unsigned)n_kv, a.keep = (unsigned)keep, a.discard = (unsigned)discard, a.end = (unsigned)(n - discard);
    a.head_words = head_words;
    const size_t moved = n - discard - keep;
    const size_t segments = 2 * n_layers * n_kv;
    // overlapping ranges: one workgroup per segment (ORDERING above).  Disjoint ranges: about 2048 workgroups in all, no more per segment than K
    // has chunks to write (a V tile is 64 rows of an f32 cache, 128 of an f16 one: a V part beyond its last tile leaves at once)
    a.parts = 1;
    if (moved <= discard) {
        const size_t want = segments >= 2048 ? 1 : 2048 / segments;
        const size_t have = (a.end - 1) / 64 - keep / 64 + 1;
        a.parts = (unsigned)(want < have ? want : have);
    }
    const dim3 grid((unsigned)(segments * a.parts)), block(kShiftThreads);
    if (rows == 64)
        hipLaunchKernelGGL(k_kv_shift<true>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(k_kv_shift<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace bitnet_hip
