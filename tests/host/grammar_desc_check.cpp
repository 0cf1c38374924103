// grammar_desc_check.cpp -- csrc/grammar_desc.hpp (the descriptor validation bitnet_hip_grammar_create and bitnet_hip_grammar_walk share, and the
// walk) as a stand-alone program: built by the host compiler under the address and undefined-behaviour sanitizers and run by
// tests/test_grammar_abi.py.  Every array is a heap block of exactly the stated size, so a read past a table is a sanitizer report.  Valid
// descriptors, every invalid one, and walks checked against a loop written out here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "grammar_desc.hpp"

using namespace bitnet_hip;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Owned {  // exact-size heap copies: the sanitizer sees every byte past them
    std::unique_ptr<uint16_t[]> tc;
    std::unique_ptr<int32_t[]> nx;
    bitnet_hip_grammar_desc d{};
};

static Owned make(const std::vector<uint16_t> &tc, const std::vector<int32_t> &nx, size_t S, size_t C) {
    Owned o;
    o.tc.reset(new uint16_t[tc.size() ? tc.size() : 1]);
    o.nx.reset(new int32_t[nx.size() ? nx.size() : 1]);
    if (!tc.empty()) std::memcpy(o.tc.get(), tc.data(), tc.size() * sizeof(uint16_t));
    if (!nx.empty()) std::memcpy(o.nx.get(), nx.data(), nx.size() * sizeof(int32_t));
    o.d = bitnet_hip_grammar_desc{o.tc.get(), tc.size(), o.nx.get(), S, C};
    return o;
}

static void refused(const bitnet_hip_grammar_desc *d, const char *field) {
    char msg[200] = "";
    const bool ok = grammar_desc_ok(d, msg, sizeof(msg));
    if (ok || !std::strstr(msg, field)) {
        std::printf("FAILED: expected a refusal naming '%s', got ok=%d '%s'\n", field, (int)ok, msg);
        ++failures;
    }
}

int main() {
    char msg[200];
    // ---- every invalid descriptor: refused with the field named, nothing read past a table
    refused(nullptr, "desc");
    {
        Owned o = make({0, 1, 0}, {0, -1, 1, 1}, 2, 2);
        CHECK(grammar_desc_ok(&o.d, msg, sizeof(msg)));
        bitnet_hip_grammar_desc d = o.d;
        d.token_class = nullptr;
        refused(&d, "token_class");
        d = o.d, d.next = nullptr;
        refused(&d, "next");
        d = o.d, d.vocab = 0;
        refused(&d, "vocab");
        d = o.d, d.vocab = ((size_t)1 << 20) + 1;  // refused before token_class is read
        refused(&d, "vocab");
        d = o.d, d.n_states = 0;
        refused(&d, "n_states");
        d = o.d, d.n_states = BITNET_HIP_GRAMMAR_MAX_STATES + 1;
        refused(&d, "n_states");
        d = o.d, d.n_classes = 0;
        refused(&d, "n_classes");
        d = o.d, d.n_classes = BITNET_HIP_GRAMMAR_MAX_CLASSES + 1;
        refused(&d, "n_classes");
        d = o.d, d.n_states = 65536, d.n_classes = 257;  // 65536 * 257 > 2^24: refused before next is read
        refused(&d, "n_states * n_classes");
        d = o.d, d.n_states = (size_t)-1;  // a count that would wrap a product
        refused(&d, "n_states");
    }
    {
        Owned o = make({0, 2, 0}, {0, -1, 1, 1}, 2, 2);  // class 2 of 2
        refused(&o.d, "token_class[1]");
        Owned p = make({0, 1, 0}, {0, -1, 2, 1}, 2, 2);  // next state 2 of 2
        refused(&p.d, "next[1][0]");
        Owned q = make({0, 1, 0}, {0, -2, 1, 1}, 2, 2);  // below -1
        refused(&q.d, "next[0][1]");
    }
    // ---- the limits themselves are valid: 65536 states of 256 classes, and one state of 16384 classes over the largest vocabulary
    {
        std::vector<int32_t> nx((size_t)65536 * 256, -1);
        nx.back() = 65535;
        Owned o = make({255}, nx, 65536, 256);
        CHECK(grammar_desc_ok(&o.d, msg, sizeof(msg)));
        std::vector<uint16_t> tc((size_t)1 << 20, 16383);
        Owned p = make(tc, std::vector<int32_t>(16384, 0), 1, 16384);
        CHECK(grammar_desc_ok(&p.d, msg, sizeof(msg)));
    }
    // ---- walks on random automata against a loop written out here; tokens outside the vocabulary stop the walk
    std::mt19937 rng(5);
    for (int it = 0; it < 200; ++it) {
        const size_t S = 1 + rng() % 9, C = 1 + rng() % 40, V = 1 + rng() % 300;
        std::vector<uint16_t> tc(V);
        for (auto &c : tc) c = (uint16_t)(rng() % C);
        std::vector<int32_t> nx(S * C);
        for (auto &n : nx) n = rng() % 4 == 0 ? -1 : (int32_t)(rng() % S);
        Owned o = make(tc, nx, S, C);
        CHECK(grammar_desc_ok(&o.d, msg, sizeof(msg)));
        const size_t n = rng() % 20;
        std::unique_ptr<int32_t[]> toks(new int32_t[n ? n : 1]);
        for (size_t i = 0; i < n; ++i) {
            const unsigned r = rng() % 16;
            toks[i] = r == 0 ? -1 : r == 1 ? (int32_t)V : r == 2 ? INT32_MAX : r == 3 ? INT32_MIN : (int32_t)(rng() % V);
        }
        const int32_t s0 = (int32_t)(rng() % S);
        int32_t want = s0;
        size_t k = 0;
        for (; k < n; ++k) {
            if (toks[k] < 0 || (size_t)toks[k] >= V) break;
            const int32_t nxt = nx[(size_t)want * C + tc[(size_t)toks[k]]];
            if (nxt < 0) break;
            want = nxt;
        }
        int32_t got = -7;
        size_t taken = 99;
        grammar_walk(&o.d, s0, toks.get(), n, &got, &taken);
        CHECK(got == want && taken == k);
        got = -7, taken = 99;
        grammar_walk(&o.d, s0, nullptr, 0, &got, &taken);  // no tokens: the state stays
        CHECK(got == s0 && taken == 0);
    }
    if (failures) {
        std::printf("grammar_desc_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("grammar_desc_check: ok\n");
    return 0;
}
