/* bitnet_hip_widetail.h -- the tail of the WIDE decode step: the sampler table and the logits-tap table at BITNET_HIP_WIDE_MAX entries.  Part of
 * the C ABI of include/bitnet_hip.h, which includes this file (the entries stand beside bitnet_hip_sample_batch_* and
 * bitnet_hip_logprob_batch_dev in that header's order of topics); include that header, not this one. */
#ifndef BITNET_HIP_WIDETAIL_H
#define BITNET_HIP_WIDETAIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the wide step's tail: one sampling launch and one tap launch for up to 64 members -----------------------------------
 * bitnet_hip_sample_batch_create and bitnet_hip_logprob_batch_dev take n_slots = 1..BITNET_HIP_BATCH_MAX (8), the slots of a batched decode
 * step, and keep doing so.  The wide step (bitnet_hip_*_rows_dev) carries up to BITNET_HIP_WIDE_MAX (64) sequences; these two entries are the
 * same tables at that width.  Nothing else differs: one kernel body per table serves the single launch, the 8-slot launch and these, so per
 * bound slot the token, history entry, position, sampler state and record are bit for bit those of bitnet_hip_sample_dev /
 * bitnet_hip_logprob_dev on that entry alone.  No workgroup waits for another (per slot the last workgroup to arrive finishes), so the grid
 * (workgroups per slot, n_slots) -- 64 x 64 workgroups at a 128256-entry vocabulary -- need not be co-resident.
 *   - bitnet_hip_sample_batch_create_wide: bitnet_hip_sample_batch_create with n_slots in 1..BITNET_HIP_WIDE_MAX.  The table is the same
 *     type: bitnet_hip_sample_batch_set / _dev / _destroy serve it unchanged, and _dev is still exactly one launch.  INVALID_ARGUMENT before
 *     the GPU is touched: a NULL out, vocab outside 1..2^20, n_slots 0 or above BITNET_HIP_WIDE_MAX.
 *   - bitnet_hip_logprob_rows_dev: bitnet_hip_logprob_batch_dev with n_slots in 1..BITNET_HIP_WIDE_MAX: table_dev is a DEVICE table of n_slots
 *     bitnet_hip_logprob_args, an entry with records_dev == NULL is empty, exactly one launch, asynchronous and capture-safe.
 *     INVALID_ARGUMENT before anything launches: a NULL table_dev, vocab 0 or > 2^20, n_slots 0 or above BITNET_HIP_WIDE_MAX.
 * The stop criteria need no counterpart: bitnet_hip_stop_batch_* takes BITNET_HIP_STOP_BATCH_MAX (64) entries already. */
int bitnet_hip_sample_batch_create_wide(size_t vocab, size_t n_slots, bitnet_hip_sample_batch **out);
int bitnet_hip_logprob_rows_dev(const bitnet_hip_logprob_args *table_dev, size_t n_slots, size_t vocab, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_WIDETAIL_H */
