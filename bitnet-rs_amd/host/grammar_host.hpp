// grammar_host.hpp -- the C exports of the decoder's grammar control (Decoder::set_grammar, set_grammar_state, grammar_state in decoder.hpp),
// defined in decoder.cpp's extern "C" tail beside bitnet_host_set_constraints.  d: a decoder from bitnet_host_create / _create_shared.
#pragma once

#include <cstdint>

#include "bitnet_hip.h"

extern "C" {
int bitnet_host_set_grammar(void *d, bitnet_hip_grammar *g, int start_state);  // NULL = off
int bitnet_host_set_grammar_state(void *d, int state);
int bitnet_host_grammar_state(void *d, int32_t *state, uint64_t *steps, uint64_t *violations);  // -1 / 0 / 0 without a sampler or a grammar
}
