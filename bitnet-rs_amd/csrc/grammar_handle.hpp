// grammar_handle.hpp -- what stands behind a bitnet_hip_grammar: the automaton's device tables and its binding count.  kernels_sample.hip owns
// the handle's life (create, bind, destroy); kernels_gramc.hip fills one on the device (bitnet_hip_grammar_compile) and reads one back
// (bitnet_hip_grammar_info / _read).  Both derive the per-state class bitmaps with the one launch declared at the end.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace bitnet_hip {

// One automaton on the device, shared by any number of samplers.  `bindings` and `doomed` are guarded by kernels_sample.hip's g_grammar_mu:
// destroy on a bound handle only marks it, and the last sampler to unbind frees it.
struct Grammar {
    int vocab = 0, n_states = 0, n_classes = 0;
    uint16_t *cls = nullptr;   // device [vocab]
    int32_t *next = nullptr;   // device [n_states][n_classes]
    uint32_t *allow = nullptr;  // device [n_states][(n_classes + 31) / 32]
    std::vector<uint16_t> h_cls;  // the host copy sample_host walks; a compiled handle fills it on that path's first use
    std::vector<int32_t> h_next;
    int bindings = 0;
    bool doomed = false;
};

inline void free_grammar(Grammar *g) {
    for (void *p : {(void *)g->cls, (void *)g->next, (void *)g->allow})
        if (p) (void)hipFree(p);
    delete g;
}

// allow[s][w] bit b = next[s][32 w + b] >= 0, every word of allow written (kernels_gramc.hip k_gramc_allow); both tables in device memory.
// Asynchronous on the null stream; returns hipGetLastError().
hipError_t grammar_derive_allow(const int32_t *next_dev, size_t n_states, size_t n_classes, uint32_t *allow_dev);

}  // namespace bitnet_hip

struct bitnet_hip_grammar {
    bitnet_hip::Grammar *g;
};
