/* bitnet_hip_grammar.h -- grammar-constrained decoding: the token automaton stage of the sampler.  Part of the C ABI of include/bitnet_hip.h,
 * which includes this file behind the sampler's declarations; include that header, not this one. */
#ifndef BITNET_HIP_GRAMMAR_H
#define BITNET_HIP_GRAMMAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Grammar-constrained decoding: a token-level deterministic automaton whose allowed set moves with every chosen token -- a choice from a
 * fixed list, a tagged record, anything a finite automaton over the tokens describes.  Replaces nothing in the reference (it has no grammar,
 * response-format or logits-processor code under crates/).  A stage GRAMMAR beside CONSTRAINTS, inside the same single launch:
 *   counts; CONSTRAINTS; GRAMMAR; additive penalties; repetition penalty; NaN -> -inf; then the rest of the chain, or Mirostat, unchanged.
 * The automaton is class-compressed and compiled by the caller: token t has class token_class[t] < n_classes, and next[s][c] is the state
 * after a token of class c in state s, or -1: the class is not allowed in s.  Token t is allowed in state s iff next[s][token_class[t]] >= 0.
 * EOS is no special case: a class with transitions only out of accepting states.
 *   mask: with s the sampler's state word (device memory), entry i becomes -inf iff i is not allowed in s.  A ban wins exactly as the
 *     constraints' bans do (+inf with a ban is caught by NaN -> -inf); with both stages on the bans add up.
 *   update: a launch at a position that is neither forced nor frozen by the stop criteria, with t the chosen token and
 *     n = next[s][token_class[t]]: n >= 0: state = n, steps += 1; otherwise violations += 1 and the state stays -- which happens only when
 *     every entry was banned; the pick is then what a row of -inf gives on the path at hand.  A state word outside [0, n_states) (a caller's
 *     stray write) bans every entry and counts a violation; nothing is read outside a table.
 * create: copies both tables to the device (and derives per-state class bitmaps there); the caller's arrays are not kept.  Not capture-safe.
 *   INVALID_ARGUMENT, the field named, before the GPU is touched: a NULL pointer; vocab outside 1..2^20; n_states outside
 *   1..BITNET_HIP_GRAMMAR_MAX_STATES; n_classes outside 1..BITNET_HIP_GRAMMAR_MAX_CLASSES; n_states * n_classes > 2^24; a class id >= n_classes;
 *   a next entry outside [-1, n_states).
 * One handle serves any number of samplers and counts its bindings: destroy on a bound handle takes effect when the last sampler unbinds or
 *   is destroyed.
 * walk: host only (no GPU is touched; works on a machine without one).  From `state` it takes tokens while they are allowed and stops in
 *   front of the first that is not, or that lies outside [0, vocab); *state_out = the state reached, *n_taken = the tokens taken.  Validates the
 *   descriptor as create does, and refuses a state outside [0, n_states).
 * set_grammar: binds the handle (NULL: off), sets the state word to start_state and zeroes both counters.  Synchronous and not capture-safe;
 *   graphs captured before it stay valid and follow it (the mode bit, the table addresses and the state live in device memory).  Refused, with
 *   nothing changed: a start state outside [0, n_states); a grammar made for another vocabulary than the sampler's.
 * set_grammar_state: overwrites the state word (same range check) and leaves the counters: what a host calls after it rewound a sequence,
 *   with the state bitnet_hip_grammar_walk gives for the tokens that remain.
 * grammar_state: the state word and the two counters (any pointer may be NULL); with no grammar bound: -1, 0, 0.  Synchronous.
 * bitnet_hip_sampler_reset puts the state back to the bound start state and zeroes the counters; configure[_ex], set_mirostat and
 *   set_constraints leave all of it alone.
 * bitnet_hip_sample_host: the mask is that of walk(start_state, the call's list) -- list-defined, like that path's counts; the device state
 *   word and the counters are not touched.  bitnet_hip_sample_batch_dev shares the kernel body: per slot bit for bit bitnet_hip_sample_dev's;
 *   slots may share one grammar at different states. */
#define BITNET_HIP_GRAMMAR_MAX_STATES  65536
#define BITNET_HIP_GRAMMAR_MAX_CLASSES 16384
typedef struct bitnet_hip_grammar_desc {
    const uint16_t *token_class; size_t vocab;        /* class of every token id, each < n_classes */
    const int32_t  *next; size_t n_states, n_classes; /* [n_states][n_classes]: the next state, or -1: the class is not allowed in this state */
} bitnet_hip_grammar_desc;
typedef struct bitnet_hip_grammar bitnet_hip_grammar;
int  bitnet_hip_grammar_create(const bitnet_hip_grammar_desc *desc, bitnet_hip_grammar **out);
void bitnet_hip_grammar_destroy(bitnet_hip_grammar *g);
int  bitnet_hip_grammar_walk(const bitnet_hip_grammar_desc *desc, int32_t state, const int32_t *tokens, size_t n,
                             int32_t *state_out, size_t *n_taken);
int  bitnet_hip_sampler_set_grammar(bitnet_hip_sampler *s, bitnet_hip_grammar *g /* NULL: off */, int32_t start_state);
int  bitnet_hip_sampler_set_grammar_state(bitnet_hip_sampler *s, int32_t state);
int  bitnet_hip_sampler_grammar_state(bitnet_hip_sampler *s, int32_t *state, uint64_t *steps, uint64_t *violations);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_GRAMMAR_H */
