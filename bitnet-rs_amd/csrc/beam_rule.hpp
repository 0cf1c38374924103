// beam_rule.hpp -- the beam search rule (include/bitnet_hip_beam.h states it in words), as plain C++ that the host and the device compile alike:
// k_beam_select (kernels_beam.hip) runs beam_cand / beam_rank across its threads and beam_walk in one, tests/host/beam_rule_check.cpp runs
// beam_step -- the same functions composed serially -- stand-alone under the address and undefined-behaviour sanitizers, against
// tests/beam_ref.py.  No HIP type in the host build.  Every float operation is a single f32 operation (no a * b + c to contract).
#pragma once

#include <cstdint>

#include "bitnet_hip_beam.h"

#if defined(__HIPCC__)
#define BH_BEAM_HD __host__ __device__
#else
#define BH_BEAM_HD
#endif

namespace bitnet_hip {

constexpr int kBeamMax = BITNET_HIP_BEAM_MAX;
constexpr int kBeamCands = 2 * kBeamMax * kBeamMax;  // candidates of one step, at most

BH_BEAM_HD inline float beam_neg_inf() { return -__builtin_inff(); }

// score of candidate (b, j): score[b] + (top_logit[j] - lse), NaN and -inf read as -inf
BH_BEAM_HD inline float beam_cand(float score, float logit, float lse) {
    const float lp = logit - lse;
    const float v = score + lp;
    return (v != v || v == beam_neg_inf()) ? beam_neg_inf() : v;
}

// the order of the candidates: descending score, then ascending index i = b * 2B + j (ascending b, then ascending j)
BH_BEAM_HD inline bool beam_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// how many of the n candidates stand before candidate i: its place in the order (the order is total, so the places are 0 .. n - 1)
BH_BEAM_HD inline int beam_rank(const float *cs, int n, int i) {
    const float s = cs[i];
    int r = 0;
    for (int k = 0; k < n; ++k) r += beam_before(cs[k], k, s, i) ? 1 : 0;
    return r;
}

// one hypothesis into the pool: written, or dropped by a full pool whose worst entry is no worse
BH_BEAM_HD inline void beam_pool_add(bitnet_hip_beam_state &s, const float *len_weight, float score, int len, int src, int last) {
    const int B = s.n_beams;
    float key = score * len_weight[len];
    if (key != key) key = beam_neg_inf();
    int slot;
    if (s.pool_n < B) {
        slot = s.pool_n++;
    } else {
        slot = 0;  // the worst: the lowest key, among equal keys the latest inserted
        for (int i = 1; i < B; ++i)
            if (s.pool_key[i] < s.pool_key[slot] || (s.pool_key[i] == s.pool_key[slot] && s.pool_order[i] > s.pool_order[slot])) slot = i;
        if (!(key > s.pool_key[slot])) return;
    }
    s.pool_score[slot] = score, s.pool_key[slot] = key, s.pool_len[slot] = len, s.pool_order[slot] = s.pool_seq++;
    s.pool_src[slot] = src, s.pool_last[slot] = last;
}

// what beam_walk keeps beside the state while it runs: the caller's memory (LDS on the device: indexed arrays on a thread's stack would be scratch)
struct BeamWalkTmp {
    float nscore[kBeamMax];
    int nparent[kBeamMax], ntoken[kBeamMax];
    int ndiv[kBeamMax][kBeamMax];
};

// The walk over the first 2B candidates in order -- ws / wi / wt: score, index b * 2B + j and token of walk index r -- and everything behind it:
// from, div, the counters and the termination.  p: the cache slot the step filled.
BH_BEAM_HD inline void beam_walk(bitnet_hip_beam_state &s, const float *len_weight, const float *ws, const int *wi, const int *wt, int p, BeamWalkTmp &tmp) {
    const int B = s.n_beams;
    float *nscore = tmp.nscore;
    int *nparent = tmp.nparent, *ntoken = tmp.ntoken;
    int(*ndiv)[kBeamMax] = tmp.ndiv;
    for (int i = 0; i < kBeamMax; ++i) s.pool_src[i] = -1, s.pool_last[i] = -1;
    int nb = 0;
    for (int r = 0; r < 2 * B; ++r) {
        const int b = wi[r] / (2 * B);
        if (s.eos >= 0 && wt[r] == s.eos) {
            if (r < B) beam_pool_add(s, len_weight, ws[r], s.gen_len + 1, b, wt[r]);
            continue;
        }
        if (nb < B) nscore[nb] = ws[r], nparent[nb] = b, ntoken[nb] = wt[r], ++nb;
    }
    for (; nb < B; ++nb) nscore[nb] = beam_neg_inf(), nparent[nb] = nb, ntoken[nb] = -1, s.done |= BITNET_HIP_BEAM_ERR_SHORT;
    for (int b = 0; b < B; ++b) {
        s.from[b] = s.div[b][nparent[b]];
        for (int c = 0; c < B; ++c) ndiv[b][c] = nparent[b] == nparent[c] ? p + 1 : s.div[nparent[b]][nparent[c]];
    }
    for (int b = 0; b < B; ++b) {
        s.score[b] = nscore[b], s.parent[b] = nparent[b], s.token[b] = ntoken[b];
        for (int c = 0; c < B; ++c) s.div[b][c] = ndiv[b][c];
    }
    s.gen_len += 1;
    s.n_slots = p + 1;
    s.stepped = 1;
    if (s.pool_n >= B) {
        s.done |= BITNET_HIP_BEAM_DONE_POOL;
    } else if (s.gen_len >= s.max_new_tokens) {
        for (int b = 0; b < B; ++b) beam_pool_add(s, len_weight, s.score[b], s.gen_len, s.parent[b], s.token[b]);
        s.done |= BITNET_HIP_BEAM_DONE_BUDGET;
    }
}

// a fresh search at prompt position P (n_beams, eos and max_new_tokens stay)
BH_BEAM_HD inline void beam_reset(bitnet_hip_beam_state &s, int P) {
    s.prompt_pos = P, s.gen_len = 0, s.done = 0, s.stepped = 0, s.n_slots = P;
    s.pool_n = 0, s.pool_seq = 0, s.frozen_steps = 0, s.reserved = 0;
    for (int b = 0; b < kBeamMax; ++b) {
        s.score[b] = b == 0 ? 0.0f : beam_neg_inf();
        s.parent[b] = b, s.from[b] = P, s.token[b] = -1;
        for (int c = 0; c < kBeamMax; ++c) s.div[b][c] = P;
        s.pool_score[b] = 0.0f, s.pool_key[b] = 0.0f, s.pool_len[b] = 0, s.pool_order[b] = 0, s.pool_src[b] = -1, s.pool_last[b] = -1;
    }
}

// One whole step, serially: lse[b], top_id / top_logit [b][0 .. 2B) with row stride `ld`.  What the kernel does across its threads.
BH_BEAM_HD inline void beam_step(bitnet_hip_beam_state &s, const float *len_weight, const float *lse, const int32_t *top_id, const float *top_logit, int ld,
                                 int p) {
    const int B = s.n_beams, n = 2 * B * B;
    float cs[kBeamCands];
    for (int i = 0; i < n; ++i) {
        const int b = i / (2 * B), j = i % (2 * B);
        cs[i] = beam_cand(s.score[b], top_logit[b * ld + j], lse[b]);
    }
    float ws[2 * kBeamMax];
    int wi[2 * kBeamMax], wt[2 * kBeamMax];
    for (int i = 0; i < n; ++i) {
        const int r = beam_rank(cs, n, i);
        if (r < 2 * B) ws[r] = cs[i], wi[r] = i, wt[r] = top_id[(i / (2 * B)) * ld + i % (2 * B)];
    }
    BeamWalkTmp tmp;
    beam_walk(s, len_weight, ws, wi, wt, p, tmp);
}

}  // namespace bitnet_hip
