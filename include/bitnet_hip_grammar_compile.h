/* bitnet_hip_grammar_compile.h -- the grammar compiler on the device: a byte-level DFA and the vocabulary's byte strings in, the token automaton
 * the sampler's GRAMMAR stage takes out.  Part of the C ABI of include/bitnet_hip.h, which includes this file behind bitnet_hip_grammar.h;
 * include that header, not this one. */
#ifndef BITNET_HIP_GRAMMAR_COMPILE_H
#define BITNET_HIP_GRAMMAR_COMPILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces nothing in the reference (it has no grammar code under crates/).  What bitnet_hip_grammar_create takes ready-made -- token_class[vocab]
 * and next[n_states][n_classes] -- is built here on the device from a deterministic automaton over BYTES, so a front end (a regular expression, a
 * JSON schema) hands over its DFA and never holds a [vocab, states] array.
 *   vocab_create: uploads the vocabulary's byte strings once; token t is bytes[offsets[t] .. offsets[t + 1]) (offsets has vocab + 1 entries).  One
 *     handle serves any number of compiles and is only read by them.  INVALID_ARGUMENT, the field named, before the GPU is touched: a NULL
 *     pointer; vocab outside 1..2^20; offsets[0] != 0; offsets that decrease; a total (offsets[vocab]) above 2^31 - 1.
 *   grammar_compile: the DFA has n_states states, next[n_states][256] with -1 for "no transition", a start state and accepting[s] != 0 for the
 *     states in which the text may end.  The token automaton has n_states + 1 states: the DFA's and an end state, n_states.
 *       - a token's column says where its bytes lead from each DFA state; -1 is absorbing; a token with no bytes is never allowed;
 *       - with eos_id >= 0 that token's column is -1 everywhere except n_states out of every accepting state, and it keeps the end state; every
 *         other token is -1 in the end state (with eos_id = -1 nothing is allowed there);
 *       - tokens with equal columns share a class.
 *     These are bitnet-rs_amd/grammar.py token_automaton's semantics, with ONE deliberate difference: classes are numbered in increasing order of
 *     their smallest token id (numpy numbers them in lexicographic column order).  That numbering is deterministic, independent of any race
 *     between lanes and needs no column sort; the two compilers agree in n_classes and in the expanded function
 *     (state, token) -> next[state][token_class[token]].  The start state of the result is the DFA's.
 *     Returns an ordinary bitnet_hip_grammar: sampler_set_grammar, the batch tables, destroy and the binding count take it unchanged.  Its tables
 *     are built in device memory and never visit the host (bitnet_hip_sample_host fetches a host copy the first time it walks such a handle).
 *     Synchronous on return; not capture-safe.  INVALID_ARGUMENT, the field named, before the GPU is touched: a NULL pointer; n_states outside
 *     1..BITNET_HIP_GRAMMAR_MAX_STATES - 1; a next entry outside [-1, n_states); start outside [0, n_states); eos_id outside [-1, vocab).
 *     INVALID_ARGUMENT after the device passes, with the counts in the message and nothing leaked: more than BITNET_HIP_GRAMMAR_MAX_CLASSES
 *     classes; (n_states + 1) * n_classes > 2^24.  ERR_GPU: a HIP error, or a lane that found no slot in the class table (cannot happen while
 *     the table has 2 * vocab slots; it is checked, not assumed).
 *   grammar_info / grammar_read: the sizes and the two tables of ANY grammar handle, one made by bitnet_hip_grammar_create included; any out
 *     pointer may be NULL.  read copies token_class[vocab] and next[n_states][n_classes] from device memory: what a host needs for
 *     bitnet_hip_grammar_walk after it rewound a sequence.  Synchronous. */
typedef struct bitnet_hip_dfa_desc {
    const int32_t *next; size_t n_states; /* [n_states][256]: the state after a byte, or -1 */
    int32_t start;
    const uint8_t *accepting;             /* one byte per state, non-zero: the text may end here */
} bitnet_hip_dfa_desc;
typedef struct bitnet_hip_vocab bitnet_hip_vocab;
int  bitnet_hip_vocab_create(const uint8_t *bytes, const uint64_t *offsets, size_t vocab, bitnet_hip_vocab **out);
void bitnet_hip_vocab_destroy(bitnet_hip_vocab *v);
int  bitnet_hip_grammar_compile(const bitnet_hip_vocab *v, const bitnet_hip_dfa_desc *dfa, int32_t eos_id /* -1: none */, bitnet_hip_grammar **out);
int  bitnet_hip_grammar_info(const bitnet_hip_grammar *g, size_t *vocab, size_t *n_states, size_t *n_classes);
int  bitnet_hip_grammar_read(const bitnet_hip_grammar *g, uint16_t *token_class, int32_t *next);

#ifdef __cplusplus
}
#endif

#endif /* BITNET_HIP_GRAMMAR_COMPILE_H */
