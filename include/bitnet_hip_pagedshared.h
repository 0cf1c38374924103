/* bitnet_hip_pagedshared.h -- the paged decode attention for FORK GROUPS: sequences whose page tables start with the same pages read those pages
 * once per group instead of once per sequence.  Part of the C ABI of include/bitnet_hip.h, which includes this file; include that header, not
 * this one. */
#ifndef BITNET_HIP_PAGEDSHARED_H
#define BITNET_HIP_PAGEDSHARED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- shared pages read once -------------------------------------------------------------------------------------------------------------
 *   - bitnet_hip_attention_decode_paged_shared_dev: bitnet_hip_attention_decode_paged_dev (every argument, every idle rule, the same append
 *     bit for bit) plus the fork groups of the launch, in two launches in stream order:
 *       shared pass   one workgroup set per (KV head, shared split, group).  The queries of every live member (its group of 1..4 heads, RoPE at
 *                     the member's OWN position, times 1/sqrt(128) log2(e), rounded to f16) form one matrix of up to 256 rows; each shared
 *                     page tile is staged once in LDS (f32 pools rounded to f16 on the way) and multiplied on v_mfma_f32_16x16x32_f16 with f32
 *                     accumulation and an f32 online softmax; the probabilities are rounded to f16 for the second product.  Per (member, KV
 *                     head, shared split) it leaves one record in the paged attention's format.
 *       suffix pass   the paged attention itself, each member walking only the pages behind its shared run; its merge takes the shared records
 *                     first, in shared-split order, then its own in split order: the output bits do not depend on arrival order.
 *     leader / shared_pages: HOST arrays [n_seq], read before the call returns.  leader[b] is the row whose table names row b's shared run
 *     (leader[b] == b for a leader or an ungrouped row); shared_pages[b] = S is the length of that run in pages, the same for every row of a
 *     group, 0 for an ungrouped row.  THE CALLER PROMISES that the rows of a group agree with their leader in table entries 0 .. S - 1 and
 *     that S <= *pos >> 6 for each of them (the page that takes the append is never in the run).  A broken promise gives wrong numbers; it
 *     never leaves the pools, the scratch or the output rows, and no table entry behind p / 64 of a live row is read (a group whose run is
 *     longer than some live member's full pages gets no shared record).  An idle member contributes no query row and gets no record; the run is read
 *     through the table of the group's first live row.
 *     Precision: on the shared keys q, p and (f32 pools) k, v are rounded to f16, each a relative 2^-11; the private keys and the new token are
 *     computed as bitnet_hip_attention_decode_paged_dev computes them.
 *     n_shared_splits = 0: the library chooses, bitnet_hip_attention_paged_shared_splits(n_groups, n_kv_heads, largest S) reports the choice
 *     (a pure host function: min(S, 16, ceil(512 / (n_groups * n_kv_heads))), n_groups = the groups with S > 0).
 *     scratch: bitnet_hip_attention_paged_shared_scratch_bytes(n_seq, n_kv_heads, n_splits, n_shared_splits) bytes, both counts resolved;
 *     the layout starts with the paged entry's scratch (counters, ZERO-FILLED ONCE, then its records) and ends with the shared records.
 *     If every shared_pages[b] is 0 the call IS bitnet_hip_attention_decode_paged_dev: the same launch, bit for bit.
 *   - BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches: everything the paged entry refuses; NULL leader or shared_pages; leader[b]
 *     outside [0, n_seq) or leader[leader[b]] != leader[b]; shared_pages[b] negative, differing inside a group or above
 *     ceil(key_bound / 64) - 1; n_shared_splits above the largest S.  BITNET_HIP_ERR_GPU when the device refuses the 128 KiB of LDS. */
size_t bitnet_hip_attention_paged_shared_splits(size_t n_groups, size_t n_kv_heads, size_t shared_pages);
size_t bitnet_hip_attention_paged_shared_scratch_bytes(size_t n_seq, size_t n_kv_heads, size_t n_splits, size_t n_shared_splits);
int bitnet_hip_attention_decode_paged_shared_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev, void *kpool_dev, void *vpool_dev,
                                                 size_t n_pages, const uint32_t *const *table_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq,
                                                 size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t key_bound, size_t n_splits,
                                                 void *scratch_dev, int flags, void *out_dev, const int32_t *leader, const int32_t *shared_pages,
                                                 size_t n_shared_splits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_PAGEDSHARED_H */
