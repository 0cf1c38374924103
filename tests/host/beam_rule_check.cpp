// beam_rule_check.cpp -- csrc/beam_rule.hpp stand-alone: the code k_beam_select runs, on the host, under the address and undefined-behaviour
// sanitizers.  Reads searches from the file named by argv[1] (integers; floats as their bits):
//     n_searches
//     per search:  B eos max_new P   then len_weight[max_new + 1]   then per step (max_new of them) and beam: lse, top_id[2B], top_logit[2B]
// runs beam_step until done, and prints per step one line: every word of bitnet_hip_beam_state in the struct's order, then for every pool slot
// its tokens.  tests/test_beam_ref.py holds the lines EQUAL to tests/beam_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "beam_rule.hpp"

using namespace bitnet_hip;

static long long next_int(FILE *f) {
    long long v = 0;
    if (fscanf(f, "%lld", &v) != 1) {
        fprintf(stderr, "beam_rule_check: short input\n");
        exit(2);
    }
    return v;
}
static float next_float(FILE *f) {
    const uint32_t u = (uint32_t)next_int(f);
    float v;
    memcpy(&v, &u, 4);
    return v;
}
static unsigned fbits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char **argv) {
    if (argc < 2) return fprintf(stderr, "usage: beam_rule_check INPUT\n"), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return fprintf(stderr, "beam_rule_check: cannot open %s\n", argv[1]), 2;
    static_assert(sizeof(bitnet_hip_beam_state) == 4 * (12 + 4 * 8 + 64 + 6 * 8), "state layout: no padding");
    const int n_searches = (int)next_int(f);
    for (int q = 0; q < n_searches; ++q) {
        bitnet_hip_beam_state s;
        memset(&s, 0, sizeof(s));
        s.n_beams = (int)next_int(f), s.eos = (int)next_int(f), s.max_new_tokens = (int)next_int(f);
        const int P = (int)next_int(f), B = s.n_beams;
        if (B < 1 || B > kBeamMax || s.max_new_tokens < 1) return fprintf(stderr, "beam_rule_check: bad search header\n"), 2;
        std::vector<float> lw((size_t)s.max_new_tokens + 1);
        for (float &w : lw) w = next_float(f);
        beam_reset(s, P);
        std::vector<std::vector<int>> beam(B), pool(B);
        for (int step = 0; step < s.max_new_tokens; ++step) {
            std::vector<float> lse(B), logit((size_t)B * 2 * B);
            std::vector<int32_t> id((size_t)B * 2 * B);
            for (int b = 0; b < B; ++b) {
                lse[b] = next_float(f);
                for (int j = 0; j < 2 * B; ++j) id[(size_t)b * 2 * B + j] = (int32_t)next_int(f);
                for (int j = 0; j < 2 * B; ++j) logit[(size_t)b * 2 * B + j] = next_float(f);
            }
            if (s.done) continue;  // the rest of the input is read and dropped
            const int p = P + s.gen_len;
            beam_step(s, lw.data(), lse.data(), id.data(), logit.data(), 2 * B, p);
            // the tokens: every pool slot written in this step continues its source beam; then the beams follow their parents
            for (int i = 0; i < s.pool_n; ++i)
                if (s.pool_src[i] >= 0) {
                    pool[i] = beam[s.pool_src[i]];
                    pool[i].push_back(s.pool_last[i]);
                }
            std::vector<std::vector<int>> nb(B);
            for (int b = 0; b < B; ++b) {
                nb[b] = beam[s.parent[b]];
                nb[b].push_back(s.token[b]);
            }
            beam = nb;
            const int32_t *w = reinterpret_cast<const int32_t *>(&s);
            for (size_t i = 0; i < sizeof(s) / 4; ++i) {
                const bool is_float = (i >= 12 && i < 20) || (i >= 12 + 32 + 64 && i < 12 + 32 + 64 + 16);
                if (is_float) {
                    float v;
                    memcpy(&v, w + i, 4);
                    printf("%u ", fbits(v));
                } else {
                    printf("%d ", w[i]);
                }
            }
            for (int i = 0; i < s.pool_n; ++i) {
                printf("| ");
                for (int t : pool[i]) printf("%d ", t);
            }
            printf("\n");
        }
    }
    fclose(f);
    printf("beam_rule_check: ok\n");
    return 0;
}
