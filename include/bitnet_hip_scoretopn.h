/* bitnet_hip_scoretopn.h -- prompt log-probabilities: the scoring head with an exact top-N per row.  Part of the C ABI of include/bitnet_hip.h,
 * which includes this file beside bitnet_hip_score_f16_dev; include that header, not this one. */
#ifndef BITNET_HIP_SCORETOPN_H
#define BITNET_HIP_SCORETOPN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prompt top-N: bitnet_hip_score_f16_dev's pass with the exact top-N of every row and no [n_rows, vocab] buffer ----------------
 * records_dev[r] (n_rows bitnet_hip_logprob_record of include/bitnet_hip.h) gets
 *   token = targets_dev[r] (-1 for any negative target), logit = its raw logit (NaN where the target is outside [0, vocab)),
 *   lse = the log-sum-exp nll_dev[r] was formed from (non-finite logits carry no mass; NaN where every logit of the row is non-finite),
 *   n_top = min(top_n, vocab), top_id / top_logit = the n_top best entries by larger logit first, lower id on equal logits, NaN read as -inf
 *   and -0.0 as +0.0 -- top_logit is the logit as that order reads it; places j >= n_top are (-1, 0).
 * The head leaves each 128-entry vocabulary block's 4 best entries and the value of its 5th; a row whose selection some block's 5th value
 * could still displace recomputes those blocks with the head's own instruction sequence: the list is exact, and its logits have the bits
 * bitnet_hip_score_f16_dev's logits_dev would hold.  nll_dev and argmax_dev are bit for bit bitnet_hip_score_f16_dev's.  The workspace is the
 * score workspace plus 36 bytes per (padded row, vocabulary block).  Asynchronous and capture-safe (no allocation, no synchronisation).
 * Refusals: bitnet_hip_score_f16_dev's, a NULL records_dev, top_n outside 1..BITNET_HIP_LOGPROB_TOP_MAX. */
size_t bitnet_hip_score_topn_workspace_bytes(size_t n_rows, size_t hidden, size_t vocab);
int bitnet_hip_score_topn_f16_dev(const void *table_f16_dev, const float *x_dev, const float *gamma_dev, float eps, size_t hidden, size_t vocab,
                                  size_t n_rows, const int32_t *targets_dev, float *nll_dev, int32_t *argmax_dev, void *records_dev,
                                  size_t top_n, void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_SCORETOPN_H */
