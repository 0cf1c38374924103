// kv_guard.hpp -- the refusals the KV state movers' entry points share (kv_fork_dev, kv_save_dev, kv_restore_dev, kv_shift_dev in abi.hip,
// kv_permute_dev in kernels_beam.hip), host side.  An entry calls kv_guard_shape, makes the refusals that are its own (its position bound, its
// counts, its snapshot), then calls kv_guard_sizes: every refusal names an argument, and the first that applies is the one reported.
#pragma once

#include "common.hpp"

namespace bitnet_hip {

// rows = 32-bit words per position and KV head, head_words per KV head (kv_layout.hpp: kv_rows, kv_head_words); segments = the
// (layer, KV head, K | V) triples a mover's grid is cut into
struct KvGeometry {
    size_t rows = 0, head_words = 0, segments = 0;
};

// The model's shape.  An entry that moves into several caches hands in their count (1..kBatchMax) under the name it gives it: n_dst, n_beams.
inline int kv_guard_shape(const char *entry, size_t n_layers, size_t n_kv_heads, size_t head_dim, int flags, const char *count_name = "", size_t count = 1) {
    if (n_layers == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: n_layers 0", entry);
    if (count == 0 || count > (size_t)kBatchMax)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: %s %zu must be 1..%d", entry, count_name, count, kBatchMax);
    if (head_dim != 128) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: head_dim %zu unsupported (128)", entry, head_dim);
    if (n_kv_heads == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: num_key_value_heads 0", entry);
    if (flags & ~BITNET_HIP_ATTN_KV_F16) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: flags 0x%x (0 or BITNET_HIP_ATTN_KV_F16)", entry, flags);
    return BITNET_HIP_OK;
}

// kv_head_words with every product checked, and the bytes of one cache with it; false: one of them wraps size_t.  After kv_guard_shape.
inline bool kv_cache_fits(size_t n_kv_heads, size_t head_dim, size_t max_pos, int flags, KvGeometry *g) {
    size_t slots = 0, cache_bytes = 0;
    g->rows = (flags & BITNET_HIP_ATTN_KV_F16) ? head_dim / 2 : head_dim;
    return !(__builtin_add_overflow(max_pos, (size_t)63, &slots) || __builtin_mul_overflow(slots / 64 * 64, g->rows, &g->head_words) ||
             __builtin_mul_overflow(g->head_words, n_kv_heads, &cache_bytes) || __builtin_mul_overflow(cache_bytes, sizeof(uint32_t), &cache_bytes));
}

// the segment count; false: it wraps, or is more than a grid's x dimension takes with room for the parts of a segment
inline bool kv_segments_fit(size_t n_layers, size_t n_kv_heads, size_t *segments) {
    return !(__builtin_mul_overflow(n_layers, n_kv_heads, segments) || __builtin_mul_overflow(*segments, (size_t)2, segments) || *segments >= ((size_t)1 << 24));
}

// The sizes: fills g, or refuses a geometry whose products wrap.  max_pos_limit = the largest max_pos the entry's kernel can index (SIZE_MAX:
// any); tables = the caches a pointer table of the call names per layer (the table's n_layers * tables entries must be countable).
inline int kv_guard_sizes(const char *entry, size_t n_layers, size_t tables, size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t max_pos_limit, int flags,
                          KvGeometry *g) {
    size_t entries = 0;
    if (max_pos > max_pos_limit || !kv_cache_fits(n_kv_heads, head_dim, max_pos, flags, g) || !kv_segments_fit(n_layers, n_kv_heads, &g->segments) ||
        __builtin_mul_overflow(n_layers, tables, &entries))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (%s: n_layers %zu, n_kv_heads %zu, max_pos %zu)", entry, n_layers,
                         n_kv_heads, max_pos);
    return BITNET_HIP_OK;
}

}  // namespace bitnet_hip
