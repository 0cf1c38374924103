// wide_batch.cpp -- see wide_batch.hpp.  Owns the slots and the device tables; the forward is Decoder::wide_forward on the members' root.
#include "wide_batch.hpp"

#include <hip/hip_runtime.h>

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

int WideBatch::fail(const char *what) {
    const char *e = bitnet_hip_get_last_error();
    err_ = std::string(what) + ": " + (e ? e : "error");
    return BITNET_HIP_ERR_EXECUTION;
}

int WideBatch::fail_arg(const std::string &what) {
    err_ = what;
    return BITNET_HIP_ERR_INVALID_ARGUMENT;
}

WideBatch::WideBatch(int n_slots) : n_(n_slots) {
    if (n_slots < 1 || n_slots > BITNET_HIP_WIDE_MAX) {
        err_ = "wide batch: 1.." + std::to_string(BITNET_HIP_WIDE_MAX) + " slots";
        n_ = 0;
        dead_ = true;
        return;
    }
    sig_.assign((size_t)n_, Sig{});
    tap_dev_.assign((size_t)n_, bitnet_hip_logprob_args{});
}

// the three tail tables go before the members (their samplers and stop objects) are let go: the stop table takes its live pointer back from
// every object it holds
void WideBatch::drop_tables() {
    if (sample_tab_) bitnet_hip_sample_batch_destroy(sample_tab_);
    if (stop_tab_) bitnet_hip_stop_batch_destroy(stop_tab_);
    sample_tab_ = nullptr, stop_tab_ = nullptr;
    release_all(tables_, tap_tab_);
    sig_.assign((size_t)n_, Sig{});
    tap_dev_.assign((size_t)n_, bitnet_hip_logprob_args{});
    built_ = false;
}

WideBatch::~WideBatch() {
    drop_tables();
    for (int b = 0; b < n_; ++b)
        if (slot_[b]) bitnet_host_release(slot_[b]);
    if (root_) bitnet_host_release(root_);
}

// the tables of a batch on root_'s model, every entry empty; allocated at the first step
int WideBatch::ensure_tables() {
    if (tables_ && tap_tab_ && sample_tab_ && stop_tab_) return 0;
    drop_tables();  // all four or none: a call that failed between two of them is made good by the next
    const Config &c = root_->config();
    const size_t rows = 2 * (size_t)c.n_layers + 6;
    int rc = 0;
    hipError_t e = tables_.alloc_zeroed(rows * BITNET_HIP_WIDE_MAX);
    if (e == hipSuccess) e = tap_tab_.alloc_zeroed((size_t)n_);
    if (e == hipSuccess) rc = bitnet_hip_sample_batch_create_wide((size_t)c.vocab, (size_t)n_, &sample_tab_);
    if (e == hipSuccess && !rc) rc = bitnet_hip_stop_batch_create((size_t)n_, &stop_tab_);
    if (e != hipSuccess || rc) {
        if (rc) fail("wide batch: creating the tail tables");
        drop_tables();
        HCHK(e);
        return BITNET_HIP_ERR_EXECUTION;
    }
    return 0;
}

void WideBatch::signature(std::vector<Sig> &out) const {
    out.assign((size_t)n_, Sig{});
    for (int b = 0; b < n_; ++b) {
        Decoder *d = slot_[b];
        if (!d || parked_[b]) continue;
        Sig &s = out[(size_t)b];
        s.d = d;
        s.kcache0 = d->layers_.empty() ? nullptr : d->layers_[0].kcache.get();
        s.sampler = d->sampling_ ? d->sampler_ : nullptr;
        d->logprob_entry(&s.tap);
        s.stop = d->stop_object();
    }
}

// The device tables follow `want`.  The pointer tables are dense (row i = the i-th slot of `want` that holds a member); the tail tables are
// indexed by slot -- an entry's kernel work depends on nothing but the entry, so their order is free -- and hold an empty entry for an empty
// or parked slot.  A sampler and a stop object sit in one entry at a time: first every entry whose object goes, then the new ones.
int WideBatch::rebuild(const std::vector<Sig> &want) {
    const size_t NL = (size_t)root_->config().n_layers, W = BITNET_HIP_WIDE_MAX;
    std::vector<void *> t((2 * NL + 6) * W, nullptr);
    size_t i = 0;
    for (int b = 0; b < n_; ++b) {
        Decoder *d = want[(size_t)b].d;
        if (!d) continue;
        for (size_t l = 0; l < NL; ++l) t[(2 * l) * W + i] = d->layers_[l].kcache, t[(2 * l + 1) * W + i] = d->layers_[l].vcache;
        void **g = t.data() + 2 * NL * W;
        g[0 * W + i] = d->pos_, g[1 * W + i] = d->history_, g[2 * W + i] = d->n_forced_, g[3 * W + i] = d->logits_;
        g[4 * W + i] = d->sampling_ ? nullptr : d->token_.get(), g[5 * W + i] = d->sampling_ ? nullptr : d->pos_.get();
        ++i;
    }
    HCHK(hipMemcpy(tables_, t.data(), t.size() * sizeof(void *), hipMemcpyHostToDevice));
    ++table_writes_;
    for (int b = 0; b < n_; ++b) {
        Sig &have = sig_[(size_t)b];
        const Sig &w = want[(size_t)b];
        if (have.sampler && have.sampler != w.sampler) {
            BCHK(bitnet_hip_sample_batch_set(sample_tab_, (size_t)b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
            have.sampler = nullptr, ++table_writes_;
        }
        if (have.stop && have.stop != w.stop) {
            BCHK(bitnet_hip_stop_batch_set(stop_tab_, (size_t)b, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
            have.stop = nullptr, ++table_writes_;
        }
    }
    std::vector<bitnet_hip_logprob_args> taps((size_t)n_);
    for (int b = 0; b < n_; ++b) {
        Sig &have = sig_[(size_t)b];
        const Sig &w = want[(size_t)b];
        Decoder *d = w.d;
        if (w.sampler && have.sampler != w.sampler) {
            BCHK(bitnet_hip_sample_batch_set(sample_tab_, (size_t)b, (bitnet_hip_sampler *)w.sampler, d->logits_, d->token_, d->pos_, d->history_, d->n_forced_));
            have.sampler = w.sampler, ++table_writes_;
        }
        if (w.stop && have.stop != w.stop) {
            BCHK(bitnet_hip_stop_batch_set(stop_tab_, (size_t)b, w.stop, d->pos_, d->history_, (size_t)d->c_.max_pos, d->n_forced_, d->token_));
            have.stop = w.stop, ++table_writes_;
        }
        taps[(size_t)b] = w.tap;
    }
    if (memcmp(taps.data(), tap_dev_.data(), taps.size() * sizeof(taps[0])) != 0) {  // against what the DEVICE holds: a member that left is still there
        HCHK(hipMemcpy(tap_tab_, taps.data(), taps.size() * sizeof(taps[0]), hipMemcpyHostToDevice));
        tap_dev_ = taps;
        ++table_writes_;
    }
    sig_ = want;
    built_ = true;
    return 0;
}

int WideBatch::set_slot(int b, Decoder *d) {
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (b < 0 || b >= n_) return fail_arg("wide batch: slot index out of range");
    bool others = false;
    Decoder *peer = nullptr;
    for (int i = 0; i < n_; ++i)
        if (slot_[i] && i != b) others = true, peer = slot_[i];
    if (d) {
        if (d->dead_) return fail_arg("wide batch: dead member");
        for (int i = 0; i < n_; ++i)
            if (slot_[i] == d && i != b) return fail_arg("wide batch: a member is repeated (this decoder sits in slot " + std::to_string(i) + ")");
        if (others && d->root() != peer->root()) return fail_arg("wide batch: all members must run on the same weights (an owner and its borrowers)");
        if (others && d->kv_f16_ != peer->kv_f16_) return fail_arg("wide batch: mixed KV cache types");
        if (slot_[b] == d) {  // the same member into its own slot: only the parked mark goes
            parked_[b] = false;
            return 0;
        }
    }
    if (!d && !slot_[b]) return 0;  // an empty slot cleared again: nothing changes, nothing is written again
    if (Decoder *old = slot_[b]) {
        // its sampler and its stop object leave the tables before the member can be destroyed
        Sig &have = sig_[(size_t)b];
        if (have.sampler) {
            BCHK(bitnet_hip_sample_batch_set(sample_tab_, (size_t)b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
            ++table_writes_;
        }
        if (have.stop) {
            BCHK(bitnet_hip_stop_batch_set(stop_tab_, (size_t)b, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
            ++table_writes_;
        }
        have = Sig{};
        slot_[b] = nullptr;
        bitnet_host_release(old);
    }
    parked_[b] = false;
    built_ = false;  // the pointer tables name the dense list: whatever the signature says, the next step writes them again
    if (d) {
        if (d->root() != root_) {  // the first member, or an emptied batch taking members of another model: tables for that model
            drop_tables();
            if (root_) bitnet_host_release(root_);
            root_ = d->root();
            root_->refs_++;
        }
        d->refs_++;
        slot_[b] = d;
    } else if (!others && root_) {  // the last member left: the owner and its weights are let go with it (the tables were made for its model)
        drop_tables();
        bitnet_host_release(root_);
        root_ = nullptr;
    }
    return 0;
}

int WideBatch::step(int n, int digits, float *elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    // every refusal comes before the first write
    if (n < 1) return fail_arg("wide batch: n_steps must be at least 1");
    std::vector<Sig> want;
    signature(want);
    Decoder *dense[BITNET_HIP_WIDE_MAX];
    int M = 0, max_p = 0;
    for (int b = 0; b < n_; ++b)
        if (want[(size_t)b].d) dense[M++] = want[(size_t)b].d;
    if (!M) return fail_arg("wide batch: no member to step (every slot is empty or parked)");
    for (int i = 0; i < M; ++i) {
        if (!dense[i]->embed_) return fail_arg("model globals not set");
        if (dense[i]->kv_f16_ != dense[0]->kv_f16_) return fail_arg("wide batch: mixed KV cache types");  // (a member switched in its slot)
    }
    for (int i = 0; i < M; ++i) {
        Decoder *d = dense[i];
        const int p = d->position();
        if (p < 0) {
            err_ = d->err_;
            return BITNET_HIP_ERR_GPU;
        }
        if (const char *e = d->overflow_problem(p, n)) return fail_arg(e);
        max_p = p > max_p ? p : max_p;
    }
    for (int i = 0; i < M; ++i)  // a logits row that waits for its lazy recomputation is brought up to date: the pick writes it from now on
        if (dense[i]->refresh_logits()) {
            err_ = dense[i]->err_;
            return BITNET_HIP_ERR_EXECUTION;
        }
    if (int rc = ensure_tables()) return rc;
    bool same = built_;
    for (int b = 0; same && b < n_; ++b) same = memcmp(&want[(size_t)b], &sig_[(size_t)b], sizeof(Sig)) == 0;
    if (!same)
        if (int rc = rebuild(want)) return rc;
    WideTail tail;
    tail.tables = tables_.get();
    for (int b = 0; b < n_; ++b) {
        const Sig &s = sig_[(size_t)b];
        if (s.sampler) tail.sample = sample_tab_;
        if (s.tap.records_dev) tail.taps = tap_tab_.get(), tail.n_taps = (size_t)n_;
        if (s.stop) tail.stop = stop_tab_;
    }
    const int rc = root_->wide_forward(dense, M, n, max_p, digits, elapsed_ms, &tail);
    memcpy(tail_, tail.launches, sizeof(tail_));
    if (rc) err_ = root_->err_;
    return rc;
}

void WideBatch::tail_launches(int out[3]) const { memcpy(out, tail_, sizeof(tail_)); }

// The stop states of the un-parked members with criteria: *live counts those that have not stopped; park marks the others.  While the stop table
// holds exactly these members (the tables are current), its live counter answers in ONE 4-byte read: as long as it equals their number nobody
// has stopped.  Only when it does not -- somebody stopped, or the tables are behind the slots -- each member's 24-byte state is read to learn who.
int WideBatch::read_stops(bool park, int *live) {
    *live = 0;
    if (built_ && stop_tab_) {
        int with = 0;
        bool current = true;
        for (int b = 0; b < n_; ++b) {
            bitnet_hip_stop *so = slot_[b] && !parked_[b] ? slot_[b]->stop_object() : nullptr;
            current &= sig_[(size_t)b].stop == so;
            with += so != nullptr;
        }
        if (current) {
            int32_t n = 0;
            if (root_) HCHK(hipStreamSynchronize((hipStream_t)root_->stream()));
            BCHK(bitnet_hip_stop_batch_live(stop_tab_, &n));
            if (n == with) {
                *live = with;
                return 0;
            }
        }
    }
    for (int b = 0; b < n_; ++b) {
        Decoder *d = slot_[b];
        if (!d || parked_[b] || !d->stop_object()) continue;
        bitnet_hip_stop_state st;
        if (int rc = d->stop_state(&st)) {
            err_ = d->err_;
            return rc;
        }
        if (st.reason == BITNET_HIP_STOP_NONE)
            ++*live;
        else if (park)
            parked_[b] = true;
    }
    return 0;
}

int WideBatch::live(int *out) {
    if (dead_ || !out) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    return read_stops(false, out);
}

int WideBatch::step_until(int max_steps, int chunk, int digits, int *steps, float *elapsed_ms) {
    if (steps) *steps = 0;
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (max_steps < 0 || chunk < 1) return fail_arg("wide batch: step_until takes max_steps >= 0 and chunk >= 1");
    bool any = false;
    for (int b = 0; b < n_; ++b) any |= slot_[b] && slot_[b]->stop_object();
    if (!any) return fail_arg("wide batch: step_until needs a member with stop criteria (set_stop)");
    int queued = 0, alive = 0;
    float total = 0.f;
    if (int rc = read_stops(true, &alive)) return rc;
    while (alive > 0 && queued < max_steps) {
        const int c = chunk < max_steps - queued ? chunk : max_steps - queued;
        float ms = 0.f;
        if (int rc = step(c, digits, &ms)) return rc;
        queued += c, total += ms;
        if (int rc = read_stops(true, &alive)) return rc;
    }
    if (steps) *steps = queued;
    if (elapsed_ms) *elapsed_ms = total;
    return 0;
}

}  // namespace bitnet_host

using bitnet_host::Decoder;
using bitnet_host::WideBatch;

extern "C" {
void *bitnet_host_wide_batch_create(int n_slots) {
    try {
        WideBatch *b = new WideBatch(n_slots);
        if (!b->dead()) return b;
        delete b;
    } catch (...) {
    }
    return nullptr;
}
void bitnet_host_wide_batch_destroy(void *b) { delete static_cast<WideBatch *>(b); }
const char *bitnet_host_wide_batch_error(void *b) { return b ? static_cast<WideBatch *>(b)->error().c_str() : "null wide batch"; }
int bitnet_host_wide_batch_set_slot(void *b, int slot, void *decoder) {
    return b ? static_cast<WideBatch *>(b)->set_slot(slot, static_cast<Decoder *>(decoder)) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_wide_batch_step(void *b, int n, int digits, float *elapsed_ms) {
    return b ? static_cast<WideBatch *>(b)->step(n, digits, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_wide_batch_live(void *b) {
    int n = 0;
    if (!b) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    const int rc = static_cast<WideBatch *>(b)->live(&n);
    return rc ? (rc < 0 ? rc : -rc) : n;
}
int bitnet_host_wide_batch_step_until(void *b, int max_steps, int chunk, int digits, int *steps, float *elapsed_ms) {
    return b ? static_cast<WideBatch *>(b)->step_until(max_steps, chunk, digits, steps, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_wide_batch_tail_launches(void *b, int *out3) {
    if (!b || !out3) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    static_cast<WideBatch *>(b)->tail_launches(out3);
    return 0;
}
int64_t bitnet_host_wide_batch_table_writes(void *b) { return b ? static_cast<WideBatch *>(b)->table_writes() : -1; }
}
