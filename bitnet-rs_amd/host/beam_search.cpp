// beam_search.cpp -- see beam_search.hpp.  Owns the beam state object and two small device tables; every launch is a bitnet_hip_* entry point.
#include "beam_search.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace bitnet_host {

#define HCHK(expr)                                                                                                  \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) {                                                                                     \
            char _b[256];                                                                                           \
            snprintf(_b, sizeof(_b), "HIP error %s at %s:%d (%s)", hipGetErrorName(_e), __FILE__, __LINE__, #expr); \
            err_ = _b;                                                                                              \
            return BITNET_HIP_ERR_GPU;                                                                              \
        }                                                                                                           \
    } while (0)
#define BCHK(expr)                        \
    do {                                  \
        int _rc = (expr);                 \
        if (_rc != 0) return fail(#expr); \
    } while (0)

int BeamSearch::fail(const char *what) {
    const char *e = bitnet_hip_get_last_error();
    err_ = std::string(what) + ": " + (e ? e : "error");
    return BITNET_HIP_ERR_EXECUTION;
}

int BeamSearch::fail_arg(const std::string &what) {
    err_ = what;
    return BITNET_HIP_ERR_INVALID_ARGUMENT;
}

BeamSearch::BeamSearch(BatchDecoder &batch, int n_beams, int eos, int max_new_tokens, float alpha) : batch_(batch) {
    dead_ = bind(n_beams, eos, max_new_tokens, alpha) != 0;
}

int BeamSearch::bind(int n_beams, int eos, int max_new_tokens, float alpha) {
    BatchDecoder &batch = batch_;
    // every refusal first: nothing is modified until all of them have passed
    if (batch.dead()) return fail_arg("beam search: the batch is dead");
    if (n_beams < 1 || n_beams > BITNET_HIP_BEAM_MAX || n_beams > batch.n_slots())
        return fail_arg("beam search: n_beams must be 1.." + std::to_string(BITNET_HIP_BEAM_MAX) + " and at most the batch's slots");
    if (eos < -1) return fail_arg("beam search: eos must be a token id or -1 (none)");
    if (max_new_tokens < 1 || max_new_tokens > (1 << 20)) return fail_arg("beam search: max_new_tokens must be 1..2^20");
    if (!std::isfinite(alpha)) return fail_arg("beam search: alpha must be finite");
    for (int b = 0; b < n_beams; ++b) {
        Decoder *d = batch.member(b);
        if (!d) return fail_arg("beam search: slot " + std::to_string(b) + " is empty (the first n_beams slots hold the beams)");
        if (d->sampling()) return fail_arg("beam search: member " + std::to_string(b) + " samples (beams are plain greedy members: no sampler, grammar or constraints)");
        if (d->stop_on()) return fail_arg("beam search: member " + std::to_string(b) + " carries stop criteria (the search has its own EOS and budget)");
        if (d->config().vocab < 2 * n_beams) return fail_arg("beam search: the vocabulary is smaller than 2 * n_beams");
    }
    B_ = n_beams, eos_ = eos, max_new_ = max_new_tokens;
    len_weight_.resize((size_t)max_new_ + 1);
    for (int len = 0; len <= max_new_; ++len) len_weight_[(size_t)len] = len ? (float)std::pow((double)len, -(double)alpha) : 1.0f;
    if (bitnet_hip_beam_create((size_t)B_, eos_, (size_t)max_new_, len_weight_.data(), &beam_) != 0) return fail("bitnet_hip_beam_create");
    const Config &c = batch.member(0)->config();
    const size_t nl = (size_t)c.n_layers;
    std::vector<bitnet_hip_beam_member> members((size_t)B_);
    std::vector<void *> kv(2 * (size_t)B_ * nl);
    for (int b = 0; b < B_; ++b) {
        Decoder *d = batch.member(b);
        if (d->set_logprobs(2 * B_) != 0) return fail_arg("beam search: set_logprobs on member " + std::to_string(b) + ": " + d->error());
        bitnet_hip_logprob_args lp;
        d->logprob_entry(&lp);
        void *g[7];
        d->global_objects(g);
        members[(size_t)b] = bitnet_hip_beam_member{lp.records_dev, static_cast<int32_t *>(g[5]), static_cast<int32_t *>(g[4]), lp.capacity, 0};
        for (size_t l = 0; l < nl; ++l) {
            uint64_t h[4];
            void *p[4] = {};
            d->layer_objects((int)l, h, p);
            kv[(size_t)b * nl + l] = p[2];
            kv[((size_t)B_ + (size_t)b) * nl + l] = p[3];
        }
    }
    if (members_.alloc((size_t)B_) != hipSuccess || kv_tables_.alloc(kv.size()) != hipSuccess ||
        hipMemcpy(members_, members.data(), members.size() * sizeof(members[0]), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(kv_tables_, kv.data(), kv.size() * sizeof(void *), hipMemcpyHostToDevice) != hipSuccess)
        return fail_arg("beam search: device tables");
    return 0;
}

BeamSearch::~BeamSearch() {
    if (beam_) {
        (void)hipDeviceSynchronize();  // not the batch's stream: the batch may be gone already
        bitnet_hip_beam_destroy(beam_);
    }
}

int BeamSearch::start() {
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    const int P = batch_.member(0) ? batch_.member(0)->position() : -1;
    if (P < 0) return fail_arg("beam search: member 0 left its slot, or its position cannot be read");
    std::vector<int32_t> first((size_t)P + 1), other((size_t)P + 1);
    for (int b = 0; b < B_; ++b) {
        Decoder *d = batch_.member(b);
        if (!d) return fail_arg("beam search: slot " + std::to_string(b) + " is empty");
        if (d->sampling() || d->stop_on() || d->logprob_top_n() != 2 * B_)
            return fail_arg("beam search: member " + std::to_string(b) + " changed its sampler, stop criteria or tap since the search was bound");
        if (d->position() != P) return fail_arg("beam search: the members stand at different positions (prefill one, fork into the others)");
        if (d->history(b ? other.data() : first.data(), P + 1) != 0) return fail_arg("beam search: history of member " + std::to_string(b) + ": " + d->error());
        if (b && other != first) return fail_arg("beam search: the members' prefixes differ (prefill one, fork into the others)");
    }
    BCHK(bitnet_hip_beam_reset(beam_, P));
    prompt_pos_ = P, queued_ = 0, done_ = 0, started_ = true;
    return 0;
}

int BeamSearch::run(int chunk, int *steps, float *elapsed_ms) {
    if (steps) *steps = 0;
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (!started_) return fail_arg("beam search: start() first");
    if (chunk < 1) return fail_arg("beam search: run takes chunk >= 1");
    for (int b = 0; b < B_; ++b)
        if (!batch_.member(b)) return fail_arg("beam search: slot " + std::to_string(b) + " is empty");
    const Config &c = batch_.member(0)->config();
    if (prompt_pos_ + max_new_ > c.max_pos - 1) return fail_arg("KV cache overflow");  // the whole budget, before the first launch
    const int32_t *done_dev = nullptr;
    BCHK(bitnet_hip_beam_done_dev(beam_, &done_dev));
    void *s = batch_.stream();
    const size_t nl = (size_t)c.n_layers;
    float total = 0.f;
    int queued = 0;
    while (!done_ && queued_ < max_new_) {
        const int n = std::min(chunk, max_new_ - queued_);  // never past the budget: a frozen step still needs its cache slot
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            if (int rc = batch_.step(1, true, &ms)) {
                err_ = "beam search: step: " + batch_.error();
                return rc;
            }
            total += ms;
            BCHK(bitnet_hip_beam_select_dev(beam_, members_, (size_t)B_, s));
            // after this step the beams hold prompt_pos + queued + 1 slots at the most
            BCHK(bitnet_hip_kv_permute_dev(kv_tables_, kv_tables_ + (size_t)B_ * nl, beam_, nl, (size_t)B_, (size_t)c.n_kv_heads, (size_t)c.head_dim,
                                           (size_t)c.max_pos, (size_t)(prompt_pos_ + queued_ + 1), batch_.member(0)->kv_f16() ? BITNET_HIP_ATTN_KV_F16 : 0, s));
            ++queued_, ++queued;
        }
        int32_t done = 0;
        HCHK(hipMemcpyAsync(&done, done_dev, sizeof(done), hipMemcpyDeviceToHost, (hipStream_t)s));
        HCHK(hipStreamSynchronize((hipStream_t)s));
        done_ = done;
    }
    if (steps) *steps = queued;
    if (elapsed_ms) *elapsed_ms = total;
    return 0;
}

int BeamSearch::state(bitnet_hip_beam_state *out) {
    if (dead_ || !out) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    BCHK(bitnet_hip_beam_read(beam_, out, nullptr));
    return 0;
}

int BeamSearch::hypotheses(std::vector<Hypothesis> *out) {
    if (dead_ || !out) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    out->clear();
    bitnet_hip_beam_state st;
    std::vector<int32_t> tok((size_t)BITNET_HIP_BEAM_MAX * (size_t)max_new_);
    BCHK(bitnet_hip_beam_read(beam_, &st, tok.data()));
    const int n = std::min(std::max(st.pool_n, 0), B_);
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        return st.pool_key[a] > st.pool_key[b] || (st.pool_key[a] == st.pool_key[b] && st.pool_order[a] < st.pool_order[b]);
    });
    for (int i : order) {
        const int len = std::min(std::max(st.pool_len[i], 0), max_new_);
        Hypothesis h;
        h.tokens.assign(tok.begin() + (size_t)i * (size_t)max_new_, tok.begin() + (size_t)i * (size_t)max_new_ + len);
        h.score = st.pool_score[i], h.key = st.pool_key[i];
        out->push_back(std::move(h));
    }
    return 0;
}

}  // namespace bitnet_host

using bitnet_host::BatchDecoder;
using bitnet_host::BeamSearch;

extern "C" {
void *bitnet_host_beam_create(void *batch, int n_beams, int eos, int max_new_tokens, float alpha) {
    if (!batch) return nullptr;
    try {
        return new BeamSearch(*static_cast<BatchDecoder *>(batch), n_beams, eos, max_new_tokens, alpha);
    } catch (...) {
        return nullptr;
    }
}
void bitnet_host_beam_destroy(void *s) { delete static_cast<BeamSearch *>(s); }
const char *bitnet_host_beam_error(void *s) { return s ? static_cast<BeamSearch *>(s)->error().c_str() : "null beam search"; }
int bitnet_host_beam_start(void *s) { return s ? static_cast<BeamSearch *>(s)->start() : BITNET_HIP_ERR_INVALID_ARGUMENT; }
int bitnet_host_beam_run(void *s, int chunk, int *steps, float *elapsed_ms) {
    return s ? static_cast<BeamSearch *>(s)->run(chunk, steps, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_beam_state(void *s, bitnet_hip_beam_state *out) { return s ? static_cast<BeamSearch *>(s)->state(out) : BITNET_HIP_ERR_INVALID_ARGUMENT; }
int bitnet_host_beam_hypotheses(void *s, int *n, int32_t *lens, int32_t *tokens, float *scores, float *keys) {
    if (!s || !n || !lens || !tokens || !scores || !keys) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    BeamSearch *bs = static_cast<BeamSearch *>(s);
    std::vector<BeamSearch::Hypothesis> h;
    if (int rc = bs->hypotheses(&h)) return rc;
    *n = (int)h.size();
    for (size_t i = 0; i < h.size(); ++i) {
        lens[i] = (int32_t)h[i].tokens.size(), scores[i] = h[i].score, keys[i] = h[i].key;
        std::copy(h[i].tokens.begin(), h[i].tokens.end(), tokens + i * (size_t)bs->max_new_tokens());
    }
    return 0;
}
int bitnet_host_beam_len_weights(void *s, float *out, int n) {
    if (!s || !out || n < 0) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    const std::vector<float> &w = static_cast<BeamSearch *>(s)->len_weights();
    if ((size_t)n > w.size()) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    std::copy(w.begin(), w.begin() + n, out);
    return 0;
}
}
