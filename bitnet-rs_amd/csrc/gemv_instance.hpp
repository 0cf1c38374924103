// gemv_instance.hpp -- which decode GEMV instance a launch takes: the K partition (mfma_pick_ksplit, gemv_geometry_of) the three decode GEMV
// launchers share, and the k_gemv_mfma template instance on top of it (gemv_mfma_instance).  Plain host C++ on a shape description, no HIP and no
// device handle: kernels_mfma.hip picks its kernel from these functions, bitnet_hip_gemv_geometry reports them, and tests/host/gemv_instance_sweep.cpp
// runs them on the CPU against the selection as it stood before it moved here.
#pragma once

#include <cstddef>

namespace bitnet_hip {

constexpr int kGemvRing = 5;   // weight tiles (1 KiB each) a wave keeps in flight
constexpr int kGemvNVMax = 4;  // float4 LayerNorm-statistics vectors per thread (512 threads): K <= 8192

inline size_t gemv_div_ceil(size_t a, size_t b) { return (a + b - 1) / b; }

inline int mfma_pick_ksplit(size_t rows, size_t cols, bool paired, int nw) {
    const size_t n_tiles = gemv_div_ceil(rows, 16), nblk = gemv_div_ceil(cols, 256);
    const int ks_max = paired ? 4 : 8;  // K ranges per row tile (<= waves per workgroup)
    // One round of identical workgroups: the largest K split whose grid still fits the 256 CUs with
    // one workgroup each (a second workgroup on some CUs makes those the tail: 432 workgroups
    // for gate|up took 7.4 us against 5.9 us for 216), K range per wave <= kGemvRing blocks.
    for (int ks = ks_max; ks >= 1; ks >>= 1) {
        if ((size_t)ks > nblk || gemv_div_ceil(nblk, (size_t)ks) > (size_t)kGemvRing) continue;
        if (gemv_div_ceil(n_tiles * ks, (size_t)nw) <= 256) return ks;
    }
    // larger matrices need several rounds anyway: spread over the CUs without leaving a wave
    // fewer than ~2 tiles
    int ks = 1;
    while (ks < ks_max && (n_tiles * ks < 8 * 256 || gemv_div_ceil(nblk, ks) > (size_t)kGemvRing) && (size_t)ks * 2 <= nblk) ks *= 2;
    return ks;
}

// The K partition of one decode GEMV launch: launch_gemv_mfma, launch_gemv_q and launch_gemv_q_batch take every one of these numbers from here,
// so the batched launch cannot choose another partition than batch-1 (its per-vector bit identity).
struct GemvGeom {
    int ksplit, ks_log2;  // K ranges per row tile = waves sharing a tile (1, 2, 4 or 8)
    int nblk;             // 256-column blocks per row
    int ring, ring_t;     // blocks per wave, and the instantiated RING that holds them (LDS plane stride)
    int tiles_per_wg;
    unsigned grid;
    int sc;               // 32-block weight scales: 0 none, 1 f32 tiles, 2 f16 tiles
};

// What the selection reads of a matrix
struct GemvShape {
    size_t rows, cols;
    int sc;       // 32-block weight scales: 0 none, 1 f32 tiles, 2 f16 tiles
    bool wscale;  // one f32 scale per (row, 256-block)
};

// Everything the three decode GEMV launchers derive from the K split.  nblk and the grid round up: k_gemv_mfma alone takes ragged shapes
// (the QAct kernels' cols % 256 == 0, rows % 16 == 0 make the rounding a no-op for them).
inline GemvGeom gemv_geometry_of(const GemvShape &s, bool silu_mul, int n_waves) {
    GemvGeom g;
    g.ksplit = mfma_pick_ksplit(s.rows, s.cols, silu_mul, n_waves);
    g.ks_log2 = g.ksplit == 8 ? 3 : g.ksplit == 4 ? 2 : g.ksplit == 2 ? 1 : 0;
    g.nblk = (int)gemv_div_ceil(s.cols, 256);
    g.ring = (int)gemv_div_ceil((size_t)g.nblk, (size_t)g.ksplit);
    g.ring_t = g.ring <= 2 ? 2 : g.ring;
    g.tiles_per_wg = n_waves / g.ksplit;
    g.grid = (unsigned)gemv_div_ceil(gemv_div_ceil(s.rows, 16), (size_t)g.tiles_per_wg);
    g.sc = s.sc;
    return g;
}

// The k_gemv_mfma<8, RING, NV, LN, BS32, MERGE> instance of one launch (kernels_mfma.hip): launch_gemv_mfma picks its kernel from this,
// bitnet_hip_gemv_geometry reports it.
struct GemvMfmaInstance {
    GemvGeom g;
    int nw;          // waves per workgroup
    int ring_inst;   // template RING: the first of 2..5 that holds g.ring blocks
    int nv_inst;     // template NV: 1 without LayerNorm, else the first of 2, 4 that holds the row's float4s over 512 threads
    int ln;          // template LN: 0 none, 1 prologue, 2 after the product (the bound gamma)
    int merge;       // template MERGE
    int wscale;      // the runtime 256-block scale fold
    size_t lds;      // dynamic LDS bytes
    bool raise_lds;  // above the default 64 KiB: hipFuncAttributeMaxDynamicSharedMemorySize is raised first
};

// ln: a LayerNorm weight is passed; ln_bound: it is the one bitnet_hip_weights_bind_ln bound (LN 2).  false: no instance takes the launch.
inline bool gemv_mfma_instance(const GemvShape &s, bool silu_mul, bool ln, bool ln_bound, bool merge, size_t m, GemvMfmaInstance &q) {
    q.nw = 8;  // (16-wave workgroups were a round-1 tuning knob that never paid: removed)
    q.g = gemv_geometry_of(s, silu_mul, q.nw);
    const int nv = ln ? (int)gemv_div_ceil(s.cols / 4, (size_t)q.nw * 64) : 1;
    if (q.g.ring > kGemvRing || nv > kGemvNVMax) return false;
    q.ring_inst = q.g.ring_t;
    q.ln = !ln ? 0 : ln_bound ? 2 : 1;
    q.nv_inst = !ln ? 1 : nv <= 2 ? 2 : 4;
    q.merge = merge ? 1 : 0;
    q.wscale = s.wscale ? 1 : 0;
    if (merge) {  // x merged from the decode attention's chunk records: the o-projection shape only
        if (ln || m != 1 || q.g.ring > 2 || s.cols % 128 != 0) return false;
        q.ring_inst = 2;
    }
    q.lds = (size_t)q.nw * (q.g.sc ? 5 : 4) * (q.g.ring_t * 256 + 16) + 2 * q.nw * sizeof(double) + q.nw * 16 * sizeof(float) +
            (q.ln == 1 ? s.cols * sizeof(float) : 0);
    q.raise_lds = q.lds > 64 * 1024;
    return true;
}

}  // namespace bitnet_hip
