// batch_decoder.cpp -- see batch_decoder.hpp.  Owns buffers, the launch order and one captured graph; every launch is a bitnet_hip_* entry point.
#include "batch_decoder.hpp"

#include "stream_timer.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace bitnet_host {

namespace {
enum { kRowPos = 0, kRowHist, kRowLogits, kRowTok, kRowPickPos, kRowPickHist, kRowForced, kRowLayers };
}  // namespace

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

int BatchDecoder::fail(const char *what) {
    const char *e = bitnet_hip_get_last_error();
    err_ = std::string(what) + ": " + (e ? e : "error");
    return BITNET_HIP_ERR_EXECUTION;
}

int BatchDecoder::fail_arg(const std::string &what) {
    err_ = what;
    return BITNET_HIP_ERR_INVALID_ARGUMENT;
}

BatchDecoder::BatchDecoder(int n_slots) : n_(n_slots) {
    dead_ = true;
    if (n_slots < 1 || n_slots > BITNET_HIP_BATCH_MAX) {
        err_ = "batch: 1.." + std::to_string(BITNET_HIP_BATCH_MAX) + " slots";
        n_ = 0;
        return;
    }
    if (const char *e = getenv("BITNET_HOST_LOGITS_WGS")) logits_wgs_ = atoi(e) > 0 ? atoi(e) : logits_wgs_;
    if (bitnet_hip_init(-1) != 0) {
        const char *e = bitnet_hip_get_last_error();
        err_ = e ? e : "bitnet_hip_init failed";
        return;
    }
    hipStream_t s;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        err_ = "hipStreamCreate failed";
        return;
    }
    stream_ = s;
    dead_ = false;
}

void BatchDecoder::drop_graph() {
    if (graph_exec_) hipGraphExecDestroy((hipGraphExec_t)graph_exec_);
    if (graph_) hipGraphDestroy((hipGraph_t)graph_);
    graph_exec_ = graph_ = nullptr;
}

BatchDecoder::~BatchDecoder() {
    if (stream_) hipStreamSynchronize((hipStream_t)stream_);
    drop_graph();
    if (sample_tab_) bitnet_hip_sample_batch_destroy(sample_tab_);  // before the members (and their samplers) are released
    if (stop_tab_) bitnet_hip_stop_batch_destroy(stop_tab_);        // likewise: it takes its live pointer back from every bound object
    // the buffers before the stream goes and before the members are let go, as ever (one this line forgot would still be freed, as a member)
    release_all(tables_, x_, x2_, qkv_, attn_scratch_, qa_x_, qa_x2_, qa_att_, qa_h_, scratch_, st_x_, st_x2_, lp_table_);
    if (stream_) hipStreamDestroy((hipStream_t)stream_);
    for (int b = 0; b < n_; ++b)
        if (slot_[b]) {
            slot_[b]->batch_ = nullptr;
            bitnet_host_release(slot_[b]);
        }
    if (root_) bitnet_host_release(root_);
}

// The batch's own activation buffers: n_ vectors each, vector b at b times the batch-1 size; zero-filled once (an idle slot's vectors must hold
// finite values, and QAct bytes past a vector's last group are never written).
int BatchDecoder::ensure_buffers() {
    if (x_) return 0;
    const Config &c = root_->config();
    const size_t n = (size_t)n_, H = c.hidden, QD = (size_t)c.n_heads * c.head_dim, KD = (size_t)c.n_kv_heads * c.head_dim;
    const size_t qh = bitnet_hip_qact_bytes(H), qq = bitnet_hip_qact_bytes(QD), qf = bitnet_hip_qact_bytes((size_t)c.ffn), sb = bitnet_hip_qact_stats_bytes(H);
    const size_t as = bitnet_hip_attention_scratch_bytes((size_t)c.n_kv_heads, (size_t)c.max_pos);
    const size_t rows = kRowLayers + 2 * (size_t)c.n_layers;
    struct {
        DevMem *b;
        size_t bytes;
    } want[] = {{&x_, n * H * 4},  {&x2_, n * H * 4},  {&qkv_, n * (QD + 2 * KD) * 4},           {&attn_scratch_, n * as},
                {&qa_x_, n * qh},  {&qa_x2_, n * qh},  {&qa_att_, n * qq},                       {&qa_h_, n * qf},
                {&st_x_, n * sb},  {&st_x2_, n * sb},  {&scratch_, n * 8 * (size_t)logits_wgs_}, {&tables_, rows * n * sizeof(void *)},
                {&lp_table_, n * sizeof(bitnet_hip_logprob_args)}};  // zero-filled: every entry empty
    for (auto &w : want) HCHK(w.b->alloc_zeroed_bytes(w.bytes));
    host_tables_.assign(rows * n, nullptr);
    BCHK(bitnet_hip_sample_batch_create((size_t)c.vocab, n, &sample_tab_));
    BCHK(bitnet_hip_stop_batch_create(n, &stop_tab_));
    // One pass of the chain with every slot idle (all-NULL tables: the gather, the attention and the head touch nothing, the GEMVs run on the
    // zero-filled vectors): every kernel is loaded and its dynamic-LDS limit raised BEFORE the first capture, which must see launches only.
    if (int rc = launches(true)) return rc;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    return 0;
}

// a vacated slot's vectors go back to zeros: an idle slot's values run through the GEMVs of every later step and must stay finite
int BatchDecoder::clear_vectors(int b) {
    const Config &c = root_->config();
    const size_t H = c.hidden, QD = (size_t)c.n_heads * c.head_dim;
    const size_t qh = bitnet_hip_qact_bytes(H), qq = bitnet_hip_qact_bytes(QD), qf = bitnet_hip_qact_bytes((size_t)c.ffn), sb = bitnet_hip_qact_stats_bytes(H);
    struct {
        void *p;
        size_t bytes;
    } v[] = {{x_, H * 4}, {x2_, H * 4}, {qa_x_, qh}, {qa_x2_, qh}, {qa_att_, qq}, {qa_h_, qf}, {st_x_, sb}, {st_x2_, sb}};
    for (auto &e : v) HCHK(hipMemset((char *)e.p + (size_t)b * e.bytes, 0, e.bytes));
    return 0;
}

std::vector<void *> BatchDecoder::sampling_sig() const {
    std::vector<void *> sig((size_t)n_, nullptr);
    for (int b = 0; b < n_; ++b)
        if (slot_[b] && slot_[b]->sampling()) {
            void *bo[3];
            slot_[b]->batch_objects(bo);
            sig[(size_t)b] = bo[2];
        }
    return sig;
}

int BatchDecoder::set_slot(int b, Decoder *d) {
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (b < 0 || b >= n_) return fail_arg("batch: slot index out of range");
    if (d) {
        if (d->dead()) return fail_arg("batch: dead decoder");
        if (d->batch_ && !(d->batch_ == this && slot_[b] == d)) return fail_arg("batch: this decoder already sits in a slot");
        if (d->batch_) return 0;  // the same member into its own slot
        void *g[7];
        d->global_objects(g);
        if (!g[0]) return fail_arg("batch: model globals not set");
        if (!d->qact_path()) {
            err_ = "batch: every member must run on producer-quantised activations (qact_path())";
            return BITNET_HIP_ERR_UNSUPPORTED;
        }
        if (root_ && d->root() != root_) return fail_arg("batch: a member of another owner (all members share one owner's weights)");
        bool others = false;
        for (int i = 0; i < n_; ++i) others |= slot_[i] && i != b;
        if (others && d->kv_f16() != kv_f16_) return fail_arg("batch: mixed KV cache types (all members f32 or all f16)");
        if (!root_) {
            root_ = d->root();
            root_->refs_++;
        }
        if (int rc = ensure_buffers()) return rc;
        if (!others && d->kv_f16() != kv_f16_) {
            kv_f16_ = d->kv_f16();
            drop_graph();  // the attention launch's flag word is baked into the captured chain
        }
    }
    if (slot_[b]) {
        if (int rc = bind_sampler(b, nullptr)) return rc;  // its sampler leaves the table before the member can be destroyed
        if (stop_bound_[b]) {
            BCHK(bitnet_hip_stop_batch_set(stop_tab_, (size_t)b, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
            stop_bound_[b] = nullptr;
        }
        slot_[b]->batch_ = nullptr;
        bitnet_host_release(slot_[b]);
        slot_[b] = nullptr;
        if (!d)
            if (int rc = clear_vectors(b)) return rc;
    }
    if (d) {
        d->refs_++;
        d->batch_ = this;
        slot_[b] = d;
    }
    tables_dirty_ = true;
    return 0;
}

// slot b's entry of the sampling table: member d's sampler with its logits row, position, history and forced count, or empty (d == nullptr)
int BatchDecoder::bind_sampler(int b, Decoder *d) {
    void *g[7] = {}, *bo[3] = {};
    if (d) {
        d->global_objects(g);
        d->batch_objects(bo);
    }
    if (!bo[2] && !bound_[b]) return 0;
    BCHK(bitnet_hip_sample_batch_set(sample_tab_, (size_t)b, (bitnet_hip_sampler *)bo[2], (const float *)bo[1], nullptr, (int32_t *)g[5], (int32_t *)g[4],
                                     (const int32_t *)bo[0]));
    bound_[b] = bo[2];
    return 0;
}

// The stop table follows its members: slot b binds member b's stop object while the member has criteria on.  First every entry whose object
// goes (an object sits in one slot at a time), then the new ones.  Synchronous copies, between steps.
int BatchDecoder::bind_stops() {
    if (!stop_tab_) return 0;
    bitnet_hip_stop *want[BITNET_HIP_BATCH_MAX] = {};
    for (int b = 0; b < n_; ++b) want[b] = slot_[b] ? slot_[b]->stop_object() : nullptr;
    for (int b = 0; b < n_; ++b)
        if (stop_bound_[b] && stop_bound_[b] != want[b]) {
            BCHK(bitnet_hip_stop_batch_set(stop_tab_, (size_t)b, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
            stop_bound_[b] = nullptr;
        }
    for (int b = 0; b < n_; ++b) {
        stop_in_chain_ |= want[b] != nullptr;
        if (!want[b] || stop_bound_[b] == want[b]) continue;
        void *g[7], *bo[3];
        slot_[b]->global_objects(g);
        slot_[b]->batch_objects(bo);
        BCHK(bitnet_hip_stop_batch_set(stop_tab_, (size_t)b, want[b], (int32_t *)g[5], (const int32_t *)g[4], (size_t)slot_[b]->config().max_pos,
                                       (int32_t *)bo[0], nullptr));
        stop_bound_[b] = want[b];
    }
    return 0;
}

int BatchDecoder::live(int *out) {
    if (dead_ || !out) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    *out = 0;
    if (!stop_tab_) return 0;
    if (int rc = bind_stops()) return rc;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    int32_t n = 0;
    BCHK(bitnet_hip_stop_batch_live(stop_tab_, &n));
    *out = n;
    return 0;
}

int BatchDecoder::step_until(int max_steps, int chunk, int *steps, float *elapsed_ms) {
    if (steps) *steps = 0;
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (max_steps < 0 || chunk < 1) return fail_arg("batch: step_until takes max_steps >= 0 and chunk >= 1");
    bool any = false;
    for (int b = 0; b < n_; ++b) any |= slot_[b] && slot_[b]->stop_object();
    if (!any) return fail_arg("batch: step_until needs a member with stop criteria (set_stop)");
    int queued = 0, alive = 0;
    float total = 0.f;
    if (int rc = live(&alive)) return rc;
    while (alive > 0 && queued < max_steps) {
        const int c = chunk < max_steps - queued ? chunk : max_steps - queued;
        float ms = 0.f;
        if (int rc = step(c, true, &ms)) return rc;
        queued += c, total += ms;
        if (int rc = live(&alive)) return rc;
    }
    if (steps) *steps = queued;
    if (elapsed_ms) *elapsed_ms = total;
    return 0;
}

int BatchDecoder::upload_tables() {
    const Config &c = root_->config();
    const size_t n = (size_t)n_;
    for (int b = 0; b < n_; ++b) {
        Decoder *d = slot_[b];
        void *g[7] = {}, *bo[3] = {};
        if (d) {
            d->global_objects(g);
            d->batch_objects(bo);
        }
        const bool greedy = d && !d->sampling();
        host_tables_[kRowPos * n + b] = d ? g[5] : nullptr;
        host_tables_[kRowHist * n + b] = d ? g[4] : nullptr;
        host_tables_[kRowLogits * n + b] = d ? bo[1] : nullptr;
        host_tables_[kRowTok * n + b] = nullptr;  // the picked token goes into the history only (Decoder keeps a token word of its own for probes)
        host_tables_[kRowPickPos * n + b] = greedy ? g[5] : nullptr;  // a sampling member gets logits only: the sampling launch picks and advances
        host_tables_[kRowPickHist * n + b] = greedy ? g[4] : nullptr;
        host_tables_[kRowForced * n + b] = greedy ? bo[0] : nullptr;
        for (int l = 0; l < c.n_layers; ++l) {
            uint64_t h[4];
            void *p[4] = {};
            if (d) d->layer_objects(l, h, p);
            host_tables_[(kRowLayers + 2 * (size_t)l) * n + b] = p[2];
            host_tables_[(kRowLayers + 2 * (size_t)l + 1) * n + b] = p[3];
        }
    }
    HCHK(hipMemcpy(tables_, host_tables_.data(), host_tables_.size() * sizeof(void *), hipMemcpyHostToDevice));
    // the sampling table follows: first every entry whose sampler goes (a sampler sits in one slot at a time), then the sampling members'
    for (int b = 0; b < n_; ++b) {
        void *bo[3] = {};
        if (slot_[b] && slot_[b]->sampling()) slot_[b]->batch_objects(bo);
        if (bound_[b] && bound_[b] != bo[2])
            if (int rc = bind_sampler(b, nullptr)) return rc;
    }
    for (int b = 0; b < n_; ++b)
        if (slot_[b] && slot_[b]->sampling())
            if (int rc = bind_sampler(b, slot_[b])) return rc;
    tables_dirty_ = false;
    return 0;
}

// One batched step: Decoder::step_launches' QAct order at attention form 0, every launch carrying n_ vectors.
int BatchDecoder::launches(bool warm) {
    void *s = stream_;
    const Config &c = root_->config();
    const size_t n = (size_t)n_, H = c.hidden, NH = c.n_heads, NK = c.n_kv_heads, MP = c.max_pos;
    auto row = [&](size_t r) { return tables_ + r * n; };
    void *g[7];
    root_->global_objects(g);
    uint64_t h0[4];
    void *p0[4];
    root_->layer_objects(0, h0, p0);
    BCHK(bitnet_hip_embed_q_batch_dev(g[0], (const int32_t *const *)row(kRowHist), (const int32_t *const *)row(kRowPos), n, H, (size_t)c.vocab, x_,
                                      (const float *)p0[0], qa_x_, st_x_, s));
    for (int l = 0; l < c.n_layers; ++l) {
        uint64_t h[4], hn[4];
        void *p[4], *pn[4] = {};
        root_->layer_objects(l, h, p);
        const bool more = l + 1 < c.n_layers;
        if (more) root_->layer_objects(l + 1, hn, pn);
        const float *attn_norm = (const float *)p[0], *ffn_norm = (const float *)p[1];
        BCHK(bitnet_hip_gemv_q_batch_dev(h[0], n, qa_x_, st_x_, attn_norm, c.eps, nullptr, 0, qkv_, nullptr, nullptr, nullptr, s));
        BCHK(bitnet_hip_attention_decode_batch_dev(qkv_, (const float *)g[2], (const float *)g[3], row(kRowLayers + 2 * (size_t)l), row(kRowLayers + 2 * (size_t)l + 1),
                                                   (const int32_t *const *)row(kRowPos), n, NH, NK, (size_t)c.head_dim, MP, attn_scratch_,
                                                   kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, nullptr, qa_att_, s));
        BCHK(bitnet_hip_gemv_q_batch_dev(h[1], n, qa_att_, nullptr, nullptr, 0.f, x_, 0, x2_, qa_x2_, ffn_norm, st_x2_, s));
        BCHK(bitnet_hip_gemv_q_batch_dev(h[2], n, qa_x2_, st_x2_, ffn_norm, c.eps, nullptr, BITNET_HIP_FUSE_SILU_MUL, nullptr, qa_h_, nullptr, nullptr, s));
        BCHK(bitnet_hip_gemv_q_batch_dev(h[3], n, qa_h_, nullptr, nullptr, 0.f, x2_, 0, x_, more ? qa_x_.get() : nullptr, more ? (const float *)pn[0] : nullptr,
                                         more ? st_x_.get() : nullptr, s));
    }
    BCHK(bitnet_hip_logits_f16_batch_dev(g[0], x_, (const float *)g[1], c.eps, H, (size_t)c.vocab, n, (float *const *)row(kRowLogits), scratch_,
                                         (size_t)logits_wgs_, (int32_t *const *)row(kRowTok), (int32_t *const *)row(kRowPickPos),
                                         (int32_t *const *)row(kRowPickHist), (const int32_t *const *)row(kRowForced), s));
    // every sampling member in ONE launch that reads per-slot sampler state through the sampling table (an empty entry: nothing to do); in the
    // chain from the first step at which any member samples, and in the warm pass (all entries empty) so that the kernel is loaded
    if (warm || sample_in_chain_) BCHK(bitnet_hip_sample_batch_dev(sample_tab_, s));
    // the logits tap of every member that has it on, after the pick; in the chain from the first step at which any member has, and in the warm pass
    if (warm || lp_in_chain_) BCHK(bitnet_hip_logprob_batch_dev(lp_table_, n, (size_t)c.vocab, s));
    // the stop criteria of every member that has them, last; in the chain from the first step at which any member has, and in the warm pass
    if (warm || stop_in_chain_) BCHK(bitnet_hip_stop_batch_dev(stop_tab_, s));
    return 0;
}

int BatchDecoder::step(int n, bool use_graph, float *elapsed_ms) {
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (n < 0) return fail_arg("batch: negative step count");
    int occupied = 0;
    for (int b = 0; b < n_; ++b) {
        Decoder *d = slot_[b];
        if (!d) continue;
        ++occupied;
        const int p = d->position();
        if (p < 0) return BITNET_HIP_ERR_GPU;
        if (p + n > d->config().max_pos - 1) return fail_arg("KV cache overflow");  // T:1190-1194
    }
    if (!occupied) return fail_arg("batch: every slot is empty");
    const std::vector<void *> sig = sampling_sig();  // a member may have switched its sampling since the last step: the pick tables follow
    if (tables_dirty_ || sig != tables_sig_) {
        if (int rc = upload_tables()) return rc;
        tables_sig_ = sig;
    }
    for (void *sp : sig) sample_in_chain_ |= sp != nullptr;
    {
        // the logprob table follows its members: records, scratch and top_n of each, an empty entry for a member without and for an empty slot
        bitnet_hip_logprob_args lp[BITNET_HIP_BATCH_MAX] = {};
        for (int b = 0; b < n_; ++b)
            if (slot_[b]) slot_[b]->logprob_entry(&lp[b]);
        if (memcmp(lp, lp_host_, sizeof(lp)) != 0) {
            HCHK(hipMemcpy(lp_table_, lp, (size_t)n_ * sizeof(lp[0]), hipMemcpyHostToDevice));
            memcpy(lp_host_, lp, sizeof(lp));
        }
        for (int b = 0; b < n_; ++b) lp_in_chain_ |= lp[b].records_dev != nullptr;
    }
    if (int rc = bind_stops()) return rc;
    hipStream_t s = (hipStream_t)stream_;
    if (use_graph) {
        // the first sampling member ever adds the sampling launch to the chain, the first with logprobs on the logprob launch, the first with
        // stop criteria the stop launch
        if (graph_exec_ && (sample_in_chain_ != graph_sig_ || lp_in_chain_ != graph_lp_sig_ || stop_in_chain_ != graph_stop_sig_)) drop_graph();
        if (!graph_exec_) {
            hipGraph_t gr = nullptr;
            HCHK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
            const int rc = launches();
            const hipError_t e = hipStreamEndCapture(s, &gr);
            if (rc != 0) {
                if (gr) hipGraphDestroy(gr);
                return rc;
            }
            HCHK(e);
            hipGraphExec_t ex = nullptr;
            HCHK(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0));
            graph_ = gr;
            graph_exec_ = ex;
            graph_sig_ = sample_in_chain_;
            graph_lp_sig_ = lp_in_chain_;
            graph_stop_sig_ = stop_in_chain_;
            ++captures_;
        }
    }
    StreamTimer timer;
    HCHK(timer.start(s));
    for (int i = 0; i < n; ++i) {
        if (use_graph) {
            HCHK(hipGraphLaunch((hipGraphExec_t)graph_exec_, s));
        } else if (int rc = launches()) {
            return rc;
        }
    }
    HCHK(timer.stop(s, elapsed_ms));
    return 0;
}

int BatchDecoder::graph_nodes() const {
    if (!graph_) return 0;
    size_t n = 0;
    if (hipGraphGetNodes((hipGraph_t)graph_, nullptr, &n) != hipSuccess || !n) return 0;
    std::vector<hipGraphNode_t> nodes(n);
    if (hipGraphGetNodes((hipGraph_t)graph_, nodes.data(), &n) != hipSuccess) return 0;
    int kernels = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        if (hipGraphNodeGetType(nodes[i], &t) == hipSuccess && t == hipGraphNodeTypeKernel) ++kernels;
    }
    return kernels;
}

}  // namespace bitnet_host

using bitnet_host::BatchDecoder;
using bitnet_host::Decoder;

extern "C" {
void *bitnet_host_batch_create(int n_slots) {
    try {
        return new BatchDecoder(n_slots);
    } catch (...) {
        return nullptr;
    }
}
void bitnet_host_batch_destroy(void *b) { delete static_cast<BatchDecoder *>(b); }
const char *bitnet_host_batch_error(void *b) { return b ? static_cast<BatchDecoder *>(b)->error().c_str() : "null batch"; }
int bitnet_host_batch_set_slot(void *b, int slot, void *decoder) {
    return b ? static_cast<BatchDecoder *>(b)->set_slot(slot, static_cast<Decoder *>(decoder)) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_batch_step(void *b, int n, int use_graph, float *elapsed_ms) {
    return b ? static_cast<BatchDecoder *>(b)->step(n, use_graph != 0, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_batch_live(void *b) {
    int n = 0;
    if (!b) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    const int rc = static_cast<BatchDecoder *>(b)->live(&n);
    return rc ? (rc < 0 ? rc : -rc) : n;
}
int bitnet_host_batch_step_until(void *b, int max_steps, int chunk, int *steps, float *elapsed_ms) {
    return b ? static_cast<BatchDecoder *>(b)->step_until(max_steps, chunk, steps, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_batch_captures(void *b) { return b ? static_cast<BatchDecoder *>(b)->captures() : 0; }
int bitnet_host_batch_graph_nodes(void *b) { return b ? static_cast<BatchDecoder *>(b)->graph_nodes() : 0; }
}
