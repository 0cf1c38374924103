// grammar_desc.hpp -- the host half of the token automaton (bitnet_hip_grammar_desc): the descriptor's validation, which bitnet_hip_grammar_create
// and bitnet_hip_grammar_walk share, and the walk itself.  Plain host C++ on the caller's arrays, no HIP and no device handle: kernels_sample.hip
// calls these functions, and tests/host/grammar_desc_check.cpp runs them stand-alone under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "bitnet_hip.h"

namespace bitnet_hip {

constexpr size_t kGrammarMaxVocab = (size_t)1 << 20;  // the largest vocabulary a sampler takes
constexpr size_t kGrammarMaxCells = (size_t)1 << 24;  // n_states * n_classes

// false, with the field named in msg, for a descriptor create / walk refuse; reads nothing outside the arrays' stated sizes
inline bool grammar_desc_ok(const bitnet_hip_grammar_desc *d, char *msg, size_t cap) {
    if (!d) return snprintf(msg, cap, "desc is NULL"), false;
    if (!d->token_class) return snprintf(msg, cap, "token_class is NULL"), false;
    if (!d->next) return snprintf(msg, cap, "next is NULL"), false;
    if (d->vocab < 1 || d->vocab > kGrammarMaxVocab) return snprintf(msg, cap, "vocab must be in 1..%zu, got %zu", kGrammarMaxVocab, d->vocab), false;
    if (d->n_states < 1 || d->n_states > (size_t)BITNET_HIP_GRAMMAR_MAX_STATES)
        return snprintf(msg, cap, "n_states must be in 1..%d, got %zu", BITNET_HIP_GRAMMAR_MAX_STATES, d->n_states), false;
    if (d->n_classes < 1 || d->n_classes > (size_t)BITNET_HIP_GRAMMAR_MAX_CLASSES)
        return snprintf(msg, cap, "n_classes must be in 1..%d, got %zu", BITNET_HIP_GRAMMAR_MAX_CLASSES, d->n_classes), false;
    if (d->n_states * d->n_classes > kGrammarMaxCells)  // both factors are bounded above: the product cannot wrap
        return snprintf(msg, cap, "n_states * n_classes must be <= %zu, got %zu * %zu", kGrammarMaxCells, d->n_states, d->n_classes), false;
    for (size_t t = 0; t < d->vocab; ++t)
        if ((size_t)d->token_class[t] >= d->n_classes)
            return snprintf(msg, cap, "token_class[%zu] is %u, outside [0, n_classes = %zu)", t, (unsigned)d->token_class[t], d->n_classes), false;
    const size_t cells = d->n_states * d->n_classes;
    for (size_t i = 0; i < cells; ++i)
        if (d->next[i] < -1 || d->next[i] >= (int32_t)d->n_states)
            return snprintf(msg, cap, "next[%zu][%zu] is %d, outside [-1, n_states = %zu)", i / d->n_classes, i % d->n_classes, d->next[i], d->n_states),
                   false;
    return true;
}

// next[state][token_class[token]], or -1 for a token outside [0, vocab); state must be inside [0, n_states)
inline int32_t grammar_step(const bitnet_hip_grammar_desc *d, int32_t state, int32_t token) {
    if (token < 0 || (size_t)token >= d->vocab) return -1;
    return d->next[(size_t)state * d->n_classes + d->token_class[token]];
}

// From `state`, takes tokens while they are allowed and stops in front of the first that is not.  A valid descriptor and state are the caller's.
inline void grammar_walk(const bitnet_hip_grammar_desc *d, int32_t state, const int32_t *tokens, size_t n, int32_t *state_out, size_t *n_taken) {
    size_t k = 0;
    for (; k < n; ++k) {
        const int32_t nx = grammar_step(d, state, tokens[k]);
        if (nx < 0) break;
        state = nx;
    }
    *state_out = state;
    *n_taken = k;
}

}  // namespace bitnet_hip
