/* bitnet_hip_pagedprefill.h -- PROMPT attention over the paged KV cache: several sequences' new tokens attend through their page tables and
 * are appended straight into pages.  Part of the C ABI of include/bitnet_hip.h, which includes this file; include that header, not this one. */
#ifndef BITNET_HIP_PAGEDPREFILL_H
#define BITNET_HIP_PAGEDPREFILL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bitnet_hip_attention_packed_dev with every cache pointer replaced by a page table into ONE K pool and ONE V pool (bitnet_hip_paged.h: pools,
 * pages, tables).  qkv_dev: [n_rows, n_heads*D + 2*n_kv*D], the raw projections.  Segment s = one sequence owns rows row0[s] .. row0[s] +
 * len[s] - 1; its new tokens sit at positions past[s] ..: RoPE of q and k at those positions, k / v appended into slot p % 64 of page
 * tables[s][p / 64] (exact f32, or rounded once to f16 under BITNET_HIP_ATTN_CACHE_F16: bit for bit what the packed call on contiguous caches
 * followed by bitnet_hip_kv_page_in_dev leaves there), causal GQA attention of each new query over keys 0 .. its own position OF ITS OWN
 * SEQUENCE on the f16 matrix cores.  One prep launch over the new rows and one attention launch; the keys of the past are read from their
 * pages as they are multiplied, so the workspace holds the query image and one record per 64 rows and its size does not depend on any past[s].
 *   - slots below past[s] are read and never written; slots at or past past[s] + len[s], and pages the tables do not name in entries
 *     0 .. (past[s] + len[s] - 1) / 64, take no part in the result and are never written.
 *   - row0[s] is a multiple of bitnet_hip_attention_packed_row_align(n_heads, n_kv_heads); segments do not overlap, their order is free; rows of
 *     no segment are padding (not read, finite unspecified output rows).
 *   - row0, len, past, tables are HOST arrays of n_seq = 1..BITNET_HIP_PACK_MAX entries (tables[s] is a DEVICE pointer to uint32_t page ids);
 *     they travel as kernel arguments: no upload, no allocation, no synchronisation, capture-safe, reusable as soon as the call returns.
 *   - page ids are device data.  A segment whose table names an id >= n_pages in entries 0 .. (past + len - 1) / 64 is IDLE for the call: no
 *     page of it is read or written, its output rows are finite and unspecified.
 *   - segments may name the same pages BELOW their past (a fork: each reads them).  The pages that take a segment's appends must be private to
 *     it: the host cannot see page ids, so this is the caller's promise, as it is for bitnet_hip_attention_decode_paged_dev's appends.
 *   - out_dev: [n_rows, n_heads*D] f32, or f16 rows under BITNET_HIP_ATTN_OUT_F16.
 *   - BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches: everything bitnet_hip_attention_packed_dev refuses (past + len > max_pos: "KV
 *     cache overflow"), n_heads / n_kv_heads above 4, n_pages 0 or not below 2^31, a NULL table, one table pointer in two segments.
 * The workspace size is 0 for invalid sizes. */
size_t bitnet_hip_attention_paged_prefill_workspace_bytes(size_t n_heads, size_t n_kv_heads, size_t n_rows);
int bitnet_hip_attention_paged_prefill_dev(const float *qkv_dev, size_t n_rows, const float *rope_sin_dev, const float *rope_cos_dev, size_t n_seq,
                                           const int32_t *row0, const int32_t *len, const int32_t *past, const uint32_t *const *tables, void *kpool_dev,
                                           void *vpool_dev, size_t n_pages, size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                                           void *workspace_dev, size_t workspace_bytes, void *out_dev, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_PAGEDPREFILL_H */
