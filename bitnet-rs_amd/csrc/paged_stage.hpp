// paged_stage.hpp -- how one (KV head, 64-position) page tile travels from a pool into the LDS operand tiles of v_mfma_f32_16x16x32_f16, stated once
// for the kernels that multiply whole page tiles: k_prefill_attn_paged (kernels_prefill_paged.hip, whose head comment and DESIGN.md 4.1i explain the
// two layouts and their swizzles) and k_attn_paged_shared (kernels_pagedshared.hip).  256 threads; every function is called by the whole workgroup.
//
//   fetch_k / fetch_v    page -> registers.  K: 16-byte unit idx = tid + 256 i = (dim pair row idx >> 4, positions 4 (idx & 15) ..); f32 pools: the two
//                        dims' rows, paired on the way in.  V: step i takes positions 4 (wave + 4 i) .. + 3 of word `lane` (f32 pools: the float2 of
//                        dims 2 lane, 2 lane + 1).  Units and positions at or past n_live are not read and enter as zeros.
//   commit_k / commit_v  registers -> LDS.  K keeps the page's order, word (row r, position p) at column p ^ (((r >> 2) & 3) << 4).  V is transposed on
//                        the write into [128 dims][64 key slots], key 4 a + 16 b + j of every group of 32 at slot 8 a + 4 b + j, 16-byte unit u of dim
//                        d at u ^ ((d >> 1) & 7).  f32 pools are rounded to f16 here: the operands are f16(k), f16(v) for both pool types.
// Between a fetch and its commit the words wait in the registers of this object, so a tile can be in flight while the one before it is multiplied.
#pragma once

#include "common.hpp"
#include "kv_layout.hpp"
#include "wave.hpp"

namespace bitnet_hip {

constexpr int kPgTileBytes = kKvChunk * kKvDim * 2;  // one f16 operand tile in LDS
constexpr int kPgBufBytes = 2 * kPgTileBytes;        // K tile | V^T tile; the kernels keep two

template <bool KV16>
struct PagedTileStage {
    static constexpr int R = KV16 ? kKvDim / 2 : kKvDim;  // pool words per position and head
    u32x4 kraw[KV16 ? 4 : 8];
    uint32_t vraw[KV16 ? 16 : 32];

    // kp / vp: the tile's first word in the K / V pool; n_live: positions of the tile that hold keys (>= 1)
    __device__ __forceinline__ void fetch_k(const uint32_t *kp, int n_live, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, r = idx >> 4, u = idx & 15;
            const bool on = 4 * u < n_live;
            if (KV16) {
                kraw[i] = on ? *reinterpret_cast<const u32x4 *>(kp + r * 64 + 4 * u) : (u32x4){0u, 0u, 0u, 0u};
            } else {
                kraw[2 * i] = on ? *reinterpret_cast<const u32x4 *>(kp + (2 * r) * 64 + 4 * u) : (u32x4){0u, 0u, 0u, 0u};
                kraw[2 * i + 1] = on ? *reinterpret_cast<const u32x4 *>(kp + (2 * r + 1) * 64 + 4 * u) : (u32x4){0u, 0u, 0u, 0u};
            }
        }
    }
    __device__ __forceinline__ void fetch_v(const uint32_t *vp, int n_live, int wave, int lane) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pos = 4 * (wave + 4 * i) + e;
                if (KV16) {
                    vraw[4 * i + e] = pos < n_live ? vp[pos * R + lane] : 0u;
                } else {
                    const uint2 w = pos < n_live ? *reinterpret_cast<const uint2 *>(vp + pos * R + 2 * lane) : uint2{0u, 0u};
                    vraw[8 * i + 2 * e] = w.x, vraw[8 * i + 2 * e + 1] = w.y;
                }
            }
    }
    // ks / vs: the K tile / V^T tile of the LDS buffer that takes the fetched words
    __device__ __forceinline__ void commit_k(uint8_t *ks, int n_live, int tid) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, r = idx >> 4, u = idx & 15;
            u32x4 w;
            if (KV16) {
                w = kraw[i];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = pack_h2(__uint_as_float(kraw[2 * i][e]), __uint_as_float(kraw[2 * i + 1][e]));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = 4 * u + e < n_live ? w[e] : 0u;  // a unit that straddles the key count
            *reinterpret_cast<u32x4 *>(ks + (r * 64 + ((4 * u) ^ (((r >> 2) & 3) << 4))) * 4) = w;
        }
    }
    __device__ __forceinline__ void commit_v(uint8_t *vs, int wave, int lane) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t4 = wave + 4 * i, slot = 32 * (t4 >> 3) + 8 * (t4 & 3) + 4 * ((t4 >> 2) & 1);
            uint32_t lo[2], hi[2];  // 4 keys of dim 2 lane, 4 keys of dim 2 lane + 1
            if (KV16) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint32_t w0 = vraw[4 * i + 2 * e], w1 = vraw[4 * i + 2 * e + 1];
                    lo[e] = (w0 & 0xffffu) | (w1 << 16);
                    hi[e] = (w0 >> 16) | (w1 & 0xffff0000u);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    lo[e] = pack_h2(__uint_as_float(vraw[8 * i + 4 * e]), __uint_as_float(vraw[8 * i + 4 * e + 2]));
                    hi[e] = pack_h2(__uint_as_float(vraw[8 * i + 4 * e + 1]), __uint_as_float(vraw[8 * i + 4 * e + 3]));
                }
            }
            const int off = (((slot >> 3) ^ (lane & 7)) * 16) + (slot & 7) * 2;
            *reinterpret_cast<uint2 *>(vs + (2 * lane) * 128 + off) = uint2{lo[0], lo[1]};
            *reinterpret_cast<uint2 *>(vs + (2 * lane + 1) * 128 + off) = uint2{hi[0], hi[1]};
        }
    }
};

// max over the four lanes (c, g = 0..3) that hold one query's keys, in every lane (kernels_prefill_attn.hip: the VALU swaps of gfx950)
__device__ __forceinline__ float paged_max_over_g(float v) {
    const unsigned u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float m1 = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned w = __float_as_uint(m1);
    const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

}  // namespace bitnet_hip
