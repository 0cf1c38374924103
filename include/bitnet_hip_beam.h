/* bitnet_hip_beam.h -- beam search on the device: the rule that picks the next beams, and the in-place reorder of the beams' KV caches.  Part of
 * the C ABI of include/bitnet_hip.h, which includes this file; include that header, not this one. */
#ifndef BITNET_HIP_BEAM_H
#define BITNET_HIP_BEAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- beam search: n hypotheses ranked by cumulative log-probability, length penalty, EOS handling ---------------------------------------
 * Replaces nothing in the reference (its generation follows one hypothesis per request); the rule is the well-known early-stopping beam
 * search.  B = n_beams = 1..BITNET_HIP_BEAM_MAX beams are B members of a batched decode step (bitnet_hip_*_batch_dev) whose logits tap runs
 * with top_n = 2 B.  Two launches follow a step, in this order:
 *   bitnet_hip_beam_select_dev   one workgroup: reads each beam's tap record of the position just scored, runs the rule below, rewrites the
 *                                beams' histories and leaves parent[], from[] and n_slots in the state;
 *   bitnet_hip_kv_permute_dev    for every beam b with parent[b] != b, slots [from[b], n_slots) of every layer's K and V of cache b take the
 *                                bits of cache parent[b], IN PLACE, with no scratch copy.
 *
 * THE RULE (csrc/beam_rule.hpp is its only statement in code; tests/beam_ref.py restates it in numpy).  Before the step every beam stands at
 * position p + 1 (the step filled cache slot p and picked history[p + 1]), p = prompt_pos + gen_len; record p + 1 of beam b holds lse and
 * top_id / top_logit [0, 2 B).
 *   candidates: (b, j) scores s = score[b] + (top_logit[j] - lse), both operations in f32 in that order; NaN and -inf read as -inf.  Order:
 *     descending s, then ascending b, then ascending j (so the -inf candidates come last in (b, j) order).  The first 2 B are walked.
 *   walk: a candidate whose token is eos (eos >= 0) at walk index < B joins the pool with len = gen_len + 1 and key = s * len_weight[len]
 *     (f32; a NaN key reads as -inf); at walk index >= B it is skipped.  Any other candidate becomes the next free beam until B are filled:
 *     score, parent = b, token = top_id[j].  Fewer than B such candidates (a row that repeats eos: no tap writes one) fills the rest with
 *     parent = itself, score -inf, token -1 (its history entry stays) and sets BITNET_HIP_BEAM_ERR_SHORT.
 *   pool: at most B hypotheses.  A full pool replaces its worst entry -- the lowest key, among equal keys the latest inserted -- when the new
 *     key is strictly greater.  pool_src / pool_last: per pool slot the beam (before the step) whose tokens the entry written in THIS step
 *     continues and its last token, -1 for a slot this step did not write.
 *   from[b] = div[b][parent[b]] (div BEFORE the step); then div[b][c] = parent[b] == parent[c] ? p + 1 : div_before[parent[b]][parent[c]].
 *     div[b][c] is the first cache slot at which beams b and c may differ; a reset sets every entry to prompt_pos.
 *   gen_len += 1; n_slots = p + 1.  done: BITNET_HIP_BEAM_DONE_POOL when the pool holds B; otherwise, when gen_len == max_new_tokens, the B
 *     new beams join the pool by the same rule in beam order (len = gen_len, src = parent[b], last = token[b]) and
 *     BITNET_HIP_BEAM_DONE_BUDGET is set.
 *   first step: reset leaves score = {0, -inf, ...}: all beams are copies of the prompt and only beam 0 counts.
 * select_dev, beyond the rule: members_dev[b] names beam b's records, position word, history and `capacity` (entries of records and history).
 *   - done != 0 at entry (a FROZEN step): every *pos_dev >= 1 goes back by one, stepped = 0, frozen_steps += 1, nothing else changes: the next
 *     queued step re-consumes the same token and rewrites the same cache slot with the same bytes.  History entries beyond the position are
 *     unspecified after a frozen step.
 *   - range checks before any use: the B positions must be equal, p + 1 inside [1, capacity) of every member and p == prompt_pos + gen_len;
 *     otherwise BITNET_HIP_BEAM_ERR_RANGE is set in done, stepped = 0 and nothing else is read or written (the search is frozen from then on).
 *   - otherwise: the rule; the tokens of every pool entry written in this step are copied from its source beam's history (entries
 *     prompt_pos + 1 .. p, then pool_last); then history[b][from[b] .. p] takes history[parent[b]][..] for every b with parent[b] != b -- one
 *     thread owns an index in ALL B histories, loads every value it needs and only then stores -- and history[b][p + 1] = token[b]
 *     (token -1: left alone); stepped = 1.
 * kv_permute_dev: k_ptrs_dev / v_ptrs_dev are DEVICE arrays [n_beams][n_layers] of cache pointers (beam b, layer l at b * n_layers + l); all
 *   caches share max_pos, n_kv_heads, head_dim 128 and the type (flags: 0 for f32, BITNET_HIP_ATTN_KV_F16), are 16-byte aligned and distinct.
 *   The caller promises n_slots <= key_bound <= max_pos; the grid is sized from key_bound and workgroups beyond n_slots leave.  parent, from,
 *   n_slots and stepped are read from the state on the device: a parent outside [0, n_beams) reads as identity, from is clamped into
 *   [0, n_slots], n_slots into [0, key_bound].  stepped == 0 (a frozen step, a range error, a fresh reset) and identity parents write
 *   nothing.  Everything outside slots [from[b], n_slots) of a moved beam keeps its bits.
 * create / destroy / reset / read manage the state object.  create copies len_weight[0 .. max_new_tokens] (the caller's length weights:
 *   len^-alpha for the usual penalty) and resets at prompt position 0; reset(prompt_pos) is synchronous and starts a new search; read
 *   synchronises the device and copies the state (and, if pool_tokens is not NULL, the pool's tokens [BITNET_HIP_BEAM_MAX][max_new_tokens],
 *   of which the first pool_len[i] of slot i < pool_n are specified).  None of the three is capture-safe.
 * select_dev and kv_permute_dev are exactly one kernel launch each, asynchronous and capture-safe: no allocation, copy or synchronisation.
 * INVALID_ARGUMENT before the GPU is touched: a NULL state, table or output; n_beams outside 1..BITNET_HIP_BEAM_MAX or, for the launches,
 *   another n_beams than the state was created for; eos < -1; max_new_tokens outside 1..2^20; a NULL len_weight; prompt_pos < 0;
 *   n_layers == 0; n_kv_heads == 0; head_dim != 128; key_bound > max_pos; unknown flag bits; sizes that overflow. */
#define BITNET_HIP_BEAM_MAX 8              /* = BITNET_HIP_BATCH_MAX; 2 * 8 <= BITNET_HIP_LOGPROB_TOP_MAX */
#define BITNET_HIP_BEAM_DONE_POOL 1        /* bits of `done` */
#define BITNET_HIP_BEAM_DONE_BUDGET 2
#define BITNET_HIP_BEAM_ERR_RANGE 0x100
#define BITNET_HIP_BEAM_ERR_SHORT 0x200
typedef struct bitnet_hip_beam_state {
    int32_t n_beams, eos, max_new_tokens, prompt_pos;
    int32_t gen_len, done, stepped, n_slots;
    int32_t pool_n, pool_seq, frozen_steps, reserved;
    float   score[BITNET_HIP_BEAM_MAX];
    int32_t parent[BITNET_HIP_BEAM_MAX], from[BITNET_HIP_BEAM_MAX], token[BITNET_HIP_BEAM_MAX];
    int32_t div[BITNET_HIP_BEAM_MAX][BITNET_HIP_BEAM_MAX];
    float   pool_score[BITNET_HIP_BEAM_MAX], pool_key[BITNET_HIP_BEAM_MAX];
    int32_t pool_len[BITNET_HIP_BEAM_MAX], pool_order[BITNET_HIP_BEAM_MAX];   /* pool_order: insertion sequence number */
    int32_t pool_src[BITNET_HIP_BEAM_MAX], pool_last[BITNET_HIP_BEAM_MAX];
} bitnet_hip_beam_state;
typedef struct bitnet_hip_beam_member {
    const void *records_dev;      /* bitnet_hip_logprob_record [capacity] */
    int32_t *pos_dev;
    int32_t *history_dev;         /* [capacity] */
    uint32_t capacity, reserved;
} bitnet_hip_beam_member;
typedef struct bitnet_hip_beam bitnet_hip_beam;
int bitnet_hip_beam_create(size_t n_beams, int32_t eos, size_t max_new_tokens, const float *len_weight, bitnet_hip_beam **out);
void bitnet_hip_beam_destroy(bitnet_hip_beam *beam);
int bitnet_hip_beam_reset(bitnet_hip_beam *beam, int32_t prompt_pos);
int bitnet_hip_beam_read(bitnet_hip_beam *beam, bitnet_hip_beam_state *out, int32_t *pool_tokens);
int bitnet_hip_beam_done_dev(bitnet_hip_beam *beam, const int32_t **done_dev);   /* the device address of `done`, for a 4-byte read */
int bitnet_hip_beam_select_dev(bitnet_hip_beam *beam, const bitnet_hip_beam_member *members_dev, size_t n_beams, void *stream);
int bitnet_hip_kv_permute_dev(void *const *k_ptrs_dev, void *const *v_ptrs_dev, bitnet_hip_beam *beam, size_t n_layers, size_t n_beams,
                              size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t key_bound, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_BEAM_H */
