/* bitnet_hip_paged.h -- the PAGED KV cache: a page pool shared by many sequences, the one-token attention that reads through page tables, and
 * the movers between a pool and the contiguous caches.  Part of the C ABI of include/bitnet_hip.h, which includes this file; include that
 * header, not this one. */
#ifndef BITNET_HIP_PAGED_H
#define BITNET_HIP_PAGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the paged KV cache ---------------------------------------------------------------------------------------------------------------
 * The reference states the memory model in crates/bitnet-inference/src/kv_cache_optimized.rs (PagedKvCache: pages, a page table, resolve) as
 * a host-side simulation; here it is device memory and kernels.
 *
 * A POOL is one layer's K or V storage for every sequence: n_pages pages of 64 positions, caller-owned, 16-byte aligned, finite bit
 * patterns before first use (zero-filled), f32 or f16 for its whole life.  A page id selects the same 64 positions in every layer's K pool
 * and V pool.  Inside a page the (KV head, 64-position) tile is byte for byte the tile of the contiguous caches the other entries take
 * (K [n_kv][R][64], V [n_kv][64][R] in 32-bit words, R = 128 for f32 and 64 for f16).  bitnet_hip_kv_pool_bytes gives the bytes of ONE
 * layer's K pool (its V pool has as many), or 0 for a geometry the launches refuse.
 * A SEQUENCE is a DEVICE array uint32_t table[ceil(max_pos / 64)] of page ids plus its position: position p lives in slot p % 64 of page
 * table[p / 64].  Sequences may name the same page (a fork): each reads it, only the memory is shared; a page that takes an append must be
 * private to its sequence.
 *
 *   - bitnet_hip_attention_decode_paged_dev: bitnet_hip_attention_decode_rows_dev over page tables, ONE launch.  Row b of qkv_dev
 *     ([n_seq, (n_heads + 2 n_kv) * 128] f32) is sequence b's token at position p = *pos_ptrs_dev[b]: RoPE, its key and value appended to slot
 *     p % 64 of page table_ptrs_dev[b][p / 64] in kpool / vpool (exact f32, or rounded once to f16 under BITNET_HIP_ATTN_CACHE_F16), attention
 *     over keys 0..p.  out_dev: [n_seq, n_heads * 128] f32, or f16 rows under BITNET_HIP_ATTN_OUT_F16.  n_splits workgroups share one (sequence,
 *     KV head): workgroup s streams pages s, s + n_splits, ... with an online softmax, and the last to finish merges the n_splits partial
 *     results IN SPLIT ORDER, so the output bits do not depend on which workgroup finished last.  n_splits = 0: the library chooses,
 *     bitnet_hip_attention_paged_splits(n_seq, n_kv_heads, key_bound) reports the choice (a pure host function); 1..ceil(key_bound / 64) is
 *     honoured.  The caller promises *pos < key_bound <= max_pos.
 *     A sequence is IDLE for the launch -- no page, no scratch word and no output row of it is read or written -- when its table pointer or
 *     position pointer is NULL, when *pos >= key_bound (or negative), or when its table names a page id >= n_pages in entries 0 .. p / 64.
 *     scratch: bitnet_hip_attention_paged_scratch_bytes(n_seq, n_kv_heads, n_splits) bytes (n_splits the resolved count, not 0), 16-byte
 *     aligned, ZERO-FILLED ONCE before first use: its first 64 * n_kv_heads words are the arrival counters, which every launch leaves at 0, so
 *     one scratch serves launches of any n_seq and n_splits it is large enough for, and a captured graph may replay the launch.
 *   - bitnet_hip_kv_page_in_dev: positions 0 .. n_positions - 1 of ONE sequence's contiguous caches (every layer; k_ptrs_dev / v_ptrs_dev:
 *     DEVICE arrays of n_layers cache pointers, as bitnet_hip_kv_fork_dev takes a source) go into the pages table_dev names, in the pools
 *     kpool_ptrs_dev / vpool_ptrs_dev (DEVICE arrays of n_layers pool pointers), BIT FOR BIT, one launch.  Of a partial last page only the live
 *     positions move.  bitnet_hip_kv_page_out_dev is the way back: every cache byte outside positions 0 .. n_positions - 1 keeps its value.
 *     A table entry >= n_pages is skipped (nothing of that chunk moves).  flags: 0 or BITNET_HIP_ATTN_KV_F16, as the other movers.
 *   - bitnet_hip_kv_page_copy_dev: n_pairs = 1..64 whole pages copied src -> dst in every layer's K and V pool, one launch: the
 *     copy-on-write step of a fork that diverges.  pairs: a HOST array [n_pairs][2] of (src, dst) page ids, read before the call returns; no
 *     dst may be a src or another dst of the call.
 *   - all asynchronous and capture-safe: no allocation, no synchronisation.  BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches: n_seq
 *     outside 1..BITNET_HIP_WIDE_MAX, head_dim != 128, n_heads % n_kv_heads != 0 or a group above 4, unknown flag bits, a NULL required
 *     pointer, n_pages 0 or not below 2^31, n_layers 0, n_pairs outside 1..64, a pair that names a page >= n_pages or breaks the rule above,
 *     key_bound outside 1..max_pos, n_positions > max_pos ("KV cache overflow"), n_splits above ceil(key_bound / 64), sizes whose products
 *     wrap.  n_positions == 0 is valid and launches nothing. */
size_t bitnet_hip_kv_pool_bytes(size_t n_pages, size_t n_kv_heads, size_t head_dim, int f16);
size_t bitnet_hip_attention_paged_splits(size_t n_seq, size_t n_kv_heads, size_t key_bound);
size_t bitnet_hip_attention_paged_scratch_bytes(size_t n_seq, size_t n_kv_heads, size_t n_splits);
int bitnet_hip_attention_decode_paged_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev, void *kpool_dev, void *vpool_dev,
                                          size_t n_pages, const uint32_t *const *table_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq,
                                          size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t key_bound, size_t n_splits,
                                          void *scratch_dev, int flags, void *out_dev, void *stream);
int bitnet_hip_kv_page_in_dev(const void *const *k_ptrs_dev, const void *const *v_ptrs_dev, void *const *kpool_ptrs_dev, void *const *vpool_ptrs_dev,
                              const uint32_t *table_dev, size_t n_pages, size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                              size_t n_positions, int flags, void *stream);
int bitnet_hip_kv_page_out_dev(const void *const *kpool_ptrs_dev, const void *const *vpool_ptrs_dev, const uint32_t *table_dev, size_t n_pages,
                               void *const *k_ptrs_dev, void *const *v_ptrs_dev, size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                               size_t n_positions, int flags, void *stream);
int bitnet_hip_kv_page_copy_dev(void *const *kpool_ptrs_dev, void *const *vpool_ptrs_dev, size_t n_pages, const uint32_t *pairs, size_t n_pairs,
                                size_t n_layers, size_t n_kv_heads, size_t head_dim, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_PAGED_H */
