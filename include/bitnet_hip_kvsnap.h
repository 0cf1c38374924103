/* bitnet_hip_kvsnap.h -- compact snapshots of a live sequence's KV state.  Part of the C ABI of include/bitnet_hip.h, which includes this file
 * (the entries stand beside bitnet_hip_kv_fork_dev in that header's order of topics); include that header, not this one. */
#ifndef BITNET_HIP_KVSNAP_H
#define BITNET_HIP_KVSNAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- compact snapshots of a live sequence: the KV state of a prompt prefix without the cache around it ------------------
 * The reference's prefix cache keeps, per cached prefix, an opaque `cached_state` byte vector and its size (CacheEntry,
 * crates/bitnet-inference/src/prefix_cache.rs:64-77).  A SNAPSHOT is the device form of those bytes: a caller-owned device buffer that holds
 * the first S positions of every layer's K and V of one sequence and nothing else -- S positions cost S * 2 * n_layers * n_kv_heads * 128
 * elements, where a cache (and so a fork destination) costs max_pos of them.  The layout is PUBLIC; a host may copy a snapshot out and read it:
 *     K [n_layers][n_kv_heads][S][128]   then   V [n_layers][n_kv_heads][S][128]
 * position-major, in the cache's own element type (f32, or f16 with BITNET_HIP_ATTN_KV_F16), no padding to 64 positions, K after RoPE as the
 * cache holds it.  bitnet_hip_kv_snapshot_bytes gives the size of one of n_positions, or 0 for a geometry the launches refuse.
 *   - bitnet_hip_kv_save_dev: cache slots 0 .. n_positions - 1 of every layer and KV head of ONE sequence become a snapshot with
 *     S = n_positions, BIT FOR BIT (integer loads and stores), in ONE launch.  The caches are only read.  k_ptrs_dev / v_ptrs_dev: DEVICE
 *     arrays of n_layers cache pointers.
 *   - bitnet_hip_kv_restore_dev: positions 0 .. n_positions - 1 of a snapshot of snapshot_positions (n_positions <= snapshot_positions) become
 *     cache slots 0 .. n_positions - 1 of every layer and KV head of n_dst = 1..BITNET_HIP_BATCH_MAX destinations, in ONE launch that loads
 *     every snapshot vector once and stores it n_dst times.  Every other byte of every destination cache keeps its value (slots >=
 *     n_positions, the padding slots of the last chunk); the snapshot is only read.  dst_k_ptrs_dev / dst_v_ptrs_dev: DEVICE arrays
 *     [n_dst][n_layers], as bitnet_hip_kv_fork_dev takes them.  restore(save(src, n), n) leaves what fork(src, n) leaves.
 *   - flags: 0 (f32 caches) or BITNET_HIP_ATTN_KV_F16; every cache of one call has the same type (there is no conversion), the same max_pos
 *     and n_kv_heads, head_dim 128, and is 16-byte aligned, as is the snapshot; the snapshot is DISTINCT from every cache of the call, and
 *     no two destination caches overlap;
 *   - asynchronous and capture-safe: no allocation, no synchronisation, no workspace.  n_positions == 0 is valid and launches nothing.  A
 *     NULL table or snapshot, n_layers == 0, n_kv_heads == 0, head_dim != 128, n_dst outside 1..BITNET_HIP_BATCH_MAX, n_positions > max_pos
 *     ("KV cache overflow"), n_positions > snapshot_positions, unknown flag bits, a snapshot that is not 16-byte aligned and sizes that
 *     overflow return BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches. */
size_t bitnet_hip_kv_snapshot_bytes(size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t n_positions, int flags);
int bitnet_hip_kv_save_dev(const void *const *k_ptrs_dev, const void *const *v_ptrs_dev, size_t n_layers, size_t n_kv_heads,
                           size_t head_dim, size_t max_pos, size_t n_positions, int flags, void *snapshot_dev, void *stream);
int bitnet_hip_kv_restore_dev(const void *snapshot_dev, size_t snapshot_positions, void *const *dst_k_ptrs_dev,
                              void *const *dst_v_ptrs_dev, size_t n_layers, size_t n_dst, size_t n_kv_heads, size_t head_dim,
                              size_t max_pos, size_t n_positions, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_KVSNAP_H */
