// decoder.cpp -- see decoder.hpp.  Host orchestration only; every device operation is a
// bitnet_hip_* call (include/bitnet_hip.h) or plain HIP memory / stream / graph plumbing.
#include "decoder.hpp"
#include "grammar_host.hpp"

#include "blake3.hpp"
#include "stream_timer.hpp"

#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>

namespace bitnet_host {

#define HCHK(expr)                                                                     \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            char _b[256];                                                              \
            snprintf(_b, sizeof(_b), "HIP error %s at %s:%d (%s)", hipGetErrorName(_e), __FILE__, __LINE__, #expr); \
            err_ = _b;                                                                 \
            return BITNET_HIP_ERR_GPU;                                                 \
        }                                                                              \
    } while (0)
#define BCHK(expr)                       \
    do {                                 \
        int _rc = (expr);                \
        if (_rc != 0) return fail(#expr); \
    } while (0)

int Decoder::fail_arg(const char *what) {
    err_ = what;
    return BITNET_HIP_ERR_INVALID_ARGUMENT;
}

int Decoder::fail(const char *what) {
    const char *e = bitnet_hip_get_last_error();
    err_ = std::string(what) + ": " + (e ? e : "error");
    return BITNET_HIP_ERR_EXECUTION;
}

static std::string config_problem(const Config &c) {
    char b[160];
    if (c.hidden <= 0 || c.n_layers <= 0 || c.n_heads <= 0 || c.n_kv_heads <= 0 || c.head_dim <= 0 || c.ffn <= 0 || c.vocab <= 0 || c.max_pos <= 1) {
        snprintf(b, sizeof(b), "config: every dimension must be positive (hidden %d, layers %d, heads %d/%d, head_dim %d, ffn %d, vocab %d, max_pos %d)",
                 c.hidden, c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim, c.ffn, c.vocab, c.max_pos);
        return b;
    }
    if (c.n_heads % c.n_kv_heads != 0) return "config: num_heads must be divisible by num_key_value_heads";  // T:215-220
    if (c.head_dim != 128) return "config: head_dim must be 128 (attention kernels)";
    if (c.n_heads / c.n_kv_heads > 4) return "config: at most 4 query heads per KV head (attention kernels)";
    if (c.hidden % 512 != 0 || c.hidden > 8192) return "config: hidden must be a multiple of 512, <= 8192 (logits kernel)";
    if (c.n_layers > 4096 || c.max_pos > (1 << 20)) return "config: n_layers / max_pos out of range";
    return "";
}

DecoderStreams::~DecoderStreams() {
    for (void *e : sp_tev_)
        if (e) hipEventDestroy((hipEvent_t)e);
    if (sp_ev_pack_) hipEventDestroy((hipEvent_t)sp_ev_pack_);
    if (sp_ev_gather_) hipEventDestroy((hipEvent_t)sp_ev_gather_);
    if (comm_stream_) hipStreamDestroy((hipStream_t)comm_stream_);
    if (stream_) hipStreamDestroy((hipStream_t)stream_);
}

Decoder::Decoder(const Config &cfg, bool own_norms) : c_(cfg), layers_(cfg.n_layers > 0 && cfg.n_layers <= 4096 ? (size_t)cfg.n_layers : 0) {
    // A rejected configuration or a failed allocation leaves a DEAD object: error() says why, every other entry point
    // returns an error without touching a member (c_ used to keep the rejected n_layers while layers_ was empty).
    dead_ = true;
    err_ = config_problem(cfg);
    if (!err_.empty()) {
        layers_.clear();
        return;
    }
    if (const char *e = getenv("BITNET_HOST_LOGITS_WGS")) logits_wgs_ = atoi(e) > 0 ? atoi(e) : logits_wgs_;  // tuning knob
    if (const char *e = getenv("BITNET_TRACE_DIR")) trace_dir_ = e;  // the reference's switch (crates/bitnet-trace/src/lib.rs:113-117)
    if (const char *e = getenv("BITNET_HOST_KV16")) kv_f16_ = atoi(e) != 0;  // opt-in f16 KV cache (long contexts)
    if (const char *e = getenv("BITNET_HOST_ACT")) act_mode_ = atoi(e) != 0 ? 1 : 0;  // 0: exact f32 activations between the kernels
    if (const char *e = getenv("BITNET_HOST_PREFILL_CHAIN")) prefill_chain_ = atoi(e) != 0 ? 1 : 0;  // the prompt forward's f16 activation chain
    if (const char *e = getenv("BITNET_HOST_HEAD_SCREEN")) head_screen_on_ = atoi(e) != 0;  // 0: every step on the full f16 head
    if (const char *e = getenv("BITNET_HOST_SCREEN_WGS")) screen_wgs_ = atoi(e) > 0 && atoi(e) <= 65535 ? atoi(e) : screen_wgs_;  // tuning knob
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
    const size_t H = c_.hidden, D = c_.head_dim, half = D / 2;
    {
        // bitnet_hip_gemv_attn_merge_dev's shape limits (include/bitnet_hip.h)
        const int group = c_.n_kv_heads > 0 ? c_.n_heads / c_.n_kv_heads : 0;
        merge_ok_ = c_.head_dim == 128 && (group == 1 || group == 2 || group == 4) && c_.n_heads % c_.n_kv_heads == 0 &&
                    (size_t)c_.n_heads * 128 <= 4096;
        merge8_ok_ = merge_ok_ && (size_t)c_.n_heads * 128 <= 2560;  // bitnet_hip_gemv_attn_merge_rec_q_dev with 8 records
    }
    // Every allocation of a decoder's life that is not grown on demand, on ONE failure path: a hipError_t is true when it is an error, so the
    // first failure ends the chain, and the members free what they hold.
    const size_t F = (size_t)c_.ffn, QD = (size_t)c_.n_heads * D;
    bool bad = x_.alloc(H) || x2_.alloc(H) || qkv_.alloc(QD + 2 * (size_t)c_.n_kv_heads * D) || att_.alloc(QD) || h_.alloc(F);
    // QAct records + LayerNorm statistics pairs of the four vectors that travel between the step's GEMVs (zero-filled
    // once: bytes past a vector's last group are never written and must read as zero digits)
    bad = bad || qa_x_.alloc_zeroed(bitnet_hip_qact_bytes(H)) || qa_x2_.alloc_zeroed(bitnet_hip_qact_bytes(H)) || qa_att_.alloc_zeroed(bitnet_hip_qact_bytes(QD)) ||
          qa_h_.alloc_zeroed(bitnet_hip_qact_bytes(F)) || st_x_.alloc_zeroed_bytes(bitnet_hip_qact_stats_bytes(H)) || st_x2_.alloc_zeroed_bytes(bitnet_hip_qact_stats_bytes(H));
    bad = bad || ref_n_.alloc(H > F ? H : F) || ref_gu_.alloc(2 * F) || ref_t_.alloc(H) || logits_.alloc((size_t)c_.vocab);
    bad = bad || scratch_.alloc(8 * (size_t)(logits_wgs_ > screen_wgs_ ? logits_wgs_ : screen_wgs_));
    if (const size_t wb = bitnet_hip_head_screen_ws_bytes(H, (size_t)c_.vocab, (size_t)screen_wgs_))  // 0: no screened head at this hidden size
        bad = bad || screen_ws_.alloc_zeroed_bytes(wb);
    // zero-filled: the merging o-projection reads records of chunks past the context (and gives them zero weight)
    bad = bad || attn_scratch_.alloc_zeroed_bytes(bitnet_hip_attention_scratch_bytes((size_t)c_.n_kv_heads, (size_t)c_.max_pos));
    bad = bad || pos_.alloc(1) || n_forced_.alloc(1) || token_.alloc(1) || history_.alloc((size_t)c_.max_pos + 2);
    bad = bad || rope_sin_.alloc((size_t)c_.max_pos * half) || rope_cos_.alloc((size_t)c_.max_pos * half);
    for (auto &L : layers_) {
        const size_t n = (size_t)c_.n_kv_heads * (((size_t)c_.max_pos + 63) / 64 * 64) * D;  // whole 64-position tiles
        // the decode attention reads whole 64-position tiles and multiplies slots past the context by exact zeros:
        // they must hold finite bit patterns (include/bitnet_hip.h), so the caches start zero-filled
        bad = bad || L.kcache.alloc_zeroed(n) || L.vcache.alloc_zeroed(n);
        if (own_norms) bad = bad || L.attn_norm.alloc(H) || L.ffn_norm.alloc(H);
    }
    if (own_norms) bad = bad || final_norm_.alloc(H);
    if (bad) {
        err_ = "device allocation failed";
        return;
    }
    // RoPE tables exactly as build_tables does (crates/bitnet-rope/src/lib.rs:59-93)
    std::vector<float> sn((size_t)c_.max_pos * half), cs((size_t)c_.max_pos * half), inv(half);
    for (size_t i = 0; i < half; ++i) inv[i] = 1.0f / powf(c_.rope_theta, (2.0f * (float)i) / (float)D);
    for (int p = 0; p < c_.max_pos; ++p)
        for (size_t i = 0; i < half; ++i) {
            const float angle = (float)p * inv[i];
            sn[(size_t)p * half + i] = sinf(angle);
            cs[(size_t)p * half + i] = cosf(angle);
        }
    if (hipMemcpy(rope_sin_, sn.data(), sn.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(rope_cos_, cs.data(), cs.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        err_ = "rope table upload failed";
    if (!err_.empty()) return;
    dead_ = false;
    reset();
}

// Borrowing decoder: built as any other (own buffers, caches, stream) but for the norm vectors: those, the final norm, the weight handles,
// the embedding table and its screening image are the OWNER's.
Decoder::Decoder(Decoder &owner, int) : Decoder(owner.c_, false) {
    if (dead_) return;
    if (owner.dead_ || owner.owner_ || !owner.embed_) {
        dead_ = true;
        err_ = owner.owner_ ? "create_shared: the owner borrows its weights itself" : "create_shared: the owner holds no model (set_globals / every layer first)";
        return;
    }
    for (const auto &L : owner.layers_)
        if (!L.qkv || !L.o || !L.gateup || !L.down) {
            dead_ = true;
            err_ = "create_shared: the owner holds no model (set_globals / every layer first)";
            return;
        }
    for (size_t l = 0; l < layers_.size(); ++l) {
        Layer &L = layers_[l];
        const Layer &O = owner.layers_[l];
        L.attn_norm.borrow(O.attn_norm), L.ffn_norm.borrow(O.ffn_norm);
        L.qkv = O.qkv, L.o = O.o, L.gateup = O.gateup, L.down = O.down, L.q_ok = O.q_ok;
    }
    final_norm_.borrow(owner.final_norm_);
    embed_.borrow(owner.embed_);
    screen_.borrow(owner.screen_);
    weight_bytes_ = owner.weight_bytes_;
    act_mode_ = owner.act_mode_;
    owner_ = &owner;
    owner.borrowers_++;
}

int Decoder::weights_locked() {
    if (owner_) return fail_arg("this decoder borrows its weights (create_shared): set them on the owner");
    if (borrowers_ > 0) return fail_arg("the weights are shared with live borrowers (create_shared): destroy them first");
    return 0;
}

int Decoder::set_attention_form(int form) {
    if (form != -1 && form != 0) return fail_arg("set_attention_form: -1 (automatic) or 0 (64-position records + combine)");
    attn_form_ = form;
    return 0;
}

void Decoder::batch_objects(void *ptrs[3]) {
    refresh_logits();  // the batch writes this row from now on
    ptrs[0] = n_forced_, ptrs[1] = logits_, ptrs[2] = sampler_;
}

// What is not memory, in the order the memory needs: the graphs before the buffers they name, the sampler and the stop object before the
// buffers they point into.  The members follow -- every DevBuf frees what it owns, a borrowed view nothing -- and the streams go last
// (DecoderStreams).
Decoder::~Decoder() {
    drop_graphs();
    if (sampler_) bitnet_hip_sampler_destroy(sampler_);
    if (stop_) bitnet_hip_stop_destroy(stop_);
    if (owner_) {  // borrowed handles stay the owner's
        owner_->borrowers_--;
        return;
    }
    for (auto &L : layers_)
        for (bitnet_hip_weights_t h : {L.qkv, L.o, L.gateup, L.down})
            if (h) bitnet_hip_weights_free(h);
}

// A layer that already holds weights gives them back first, and every captured step graph goes (the graphs
// hold the OLD matrices' device pointers).
void Decoder::release_layer(Layer &L) {
    for (bitnet_hip_weights_t *h : {&L.qkv, &L.o, &L.gateup, &L.down}) {
        if (!*h) continue;
        size_t ab = 0;
        if (bitnet_hip_weights_info(*h, nullptr, nullptr, &ab) == 0) weight_bytes_ -= ab < weight_bytes_ ? ab : weight_bytes_;
        bitnet_hip_weights_free(*h);
        *h = 0;
    }
    drop_graphs();
}

void Decoder::drop_graphs() {
    for (int i = 0; i < kGraphs; ++i) {
        if (graph_exec_[i]) hipGraphExecDestroy((hipGraphExec_t)graph_exec_[i]);
        if (graph_[i]) hipGraphDestroy((hipGraph_t)graph_[i]);
        graph_exec_[i] = graph_[i] = nullptr;
    }
    graphs_screened_ = -1;
}

// Plain greedy decode reads no logits: the tap, the sampler and the tracer are the step's only readers of logits_, and a batch slot writes it.
bool Decoder::screen_step(bool need_logits) const {
    return head_screen_on_ && screen_ && screen_ws_ && !sampling_ && lp_top_n_ < 0 && !batch_ && !need_logits;
}

int Decoder::ensure_screen_image() {
    if (owner_) {
        if (int rc = owner_->ensure_screen_image()) {
            err_ = owner_->err_;
            return rc;
        }
        screen_.borrow(owner_->screen_);
        return 0;
    }
    const size_t H = c_.hidden, V = c_.vocab, bytes = bitnet_hip_head_screen_bytes(H, V);
    if (!bytes || !embed_) return 0;  // no instance for this hidden size, or no table yet (set_globals builds it)
    if (!screen_) HCHK(screen_.alloc(bytes));
    BCHK(bitnet_hip_head_screen_build_dev(embed_, H, V, screen_, stream_));
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    return 0;
}

int Decoder::set_head_screen(bool on) {
    if (on && !screen_)
        if (int rc = ensure_screen_image()) return rc;
    if (on != head_screen_on_) drop_graphs();
    head_screen_on_ = on;
    return 0;
}

int Decoder::head_screen_stats(uint32_t out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (!screen_ws_) return 0;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    HCHK(hipMemcpy(out, screen_x() + (size_t)c_.hidden, 12, hipMemcpyDeviceToHost));  // the counter words follow the saved input
    return 0;
}

int Decoder::refresh_logits() {
    if (!logits_stale_) return 0;
    BCHK(bitnet_hip_logits_f16_dev(embed_, screen_x(), final_norm_, c_.eps, (size_t)c_.hidden, (size_t)c_.vocab, logits_, scratch_, (size_t)logits_wgs_,
                                   nullptr, nullptr, nullptr, nullptr, stream_));
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    logits_stale_ = false;
    return 0;
}

int Decoder::pick_token(void *stream, bool record, bool need_logits) {
    hipStream_t s = (hipStream_t)stream;
    const size_t H = c_.hidden;
    pick_screened_ = screen_step(need_logits);
    if (pick_screened_) {
        // the full head's token from the int8 screen + the surviving rows of the f16 table; logits_ stays as it is (refresh_logits)
        BCHK(bitnet_hip_logits_screen_dev(embed_, x_, final_norm_, c_.eps, H, (size_t)c_.vocab, screen_, screen_ws_, scratch_, (size_t)screen_wgs_, token_, pos_,
                                          history_, n_forced_, s));
    } else if (!sampling_) {
        // greedy token (T:1589, T:1599-1630, sampling.rs:189-202)
        BCHK(bitnet_hip_logits_f16_dev(embed_, x_, final_norm_, c_.eps, H, (size_t)c_.vocab, logits_, scratch_, (size_t)logits_wgs_, token_, pos_,
                                       history_, n_forced_, s));
    } else {
        BCHK(bitnet_hip_logits_f16_dev(embed_, x_, final_norm_, c_.eps, H, (size_t)c_.vocab, logits_, scratch_, (size_t)logits_wgs_, nullptr, nullptr,
                                       nullptr, nullptr, s));
        BCHK(bitnet_hip_sample_dev(sampler_, logits_, (size_t)c_.vocab, token_, pos_, history_, n_forced_, s));
    }
    if (record && lp_top_n_ >= 0) {
        // the logits tap, after the pick (engine.rs:1182-1210): the position is p + 1 by now and history[p + 1] holds the token
        bitnet_hip_logprob_args a;
        logprob_entry(&a);
        BCHK(bitnet_hip_logprob_dev(&a, (size_t)c_.vocab, s));
    }
    // the stop criteria, last: does the token just placed end the sequence -- and if it ended earlier, hold the sequence where it stopped
    if (stop_on_) BCHK(bitnet_hip_stop_dev(stop_, pos_, history_, (size_t)c_.max_pos, n_forced_, token_, s));
    return 0;
}

int Decoder::arm_stop(bool keep_generated) {
    if (!stop_on_) return 0;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    BCHK(bitnet_hip_stop_arm(stop_, keep_generated ? 1 : 0));
    return 0;
}

int Decoder::set_stop(const bitnet_hip_stop_config *cfg) {
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    if (!cfg) {
        if (!stop_on_) return 0;
        drop_graphs();
        stop_on_ = false;
        HCHK(hipMemcpy(n_forced_, &host_forced_, 4, hipMemcpyHostToDevice));  // a stop may have raised it
        return 0;
    }
    if (!stop_) {
        BCHK(bitnet_hip_stop_create(cfg, &stop_));
        // one launch that cannot act (no position lies inside a history of one entry): the kernel is loaded before a capture can meet it
        BCHK(bitnet_hip_stop_dev(stop_, pos_, history_, 1, n_forced_, nullptr, stream_));
        HCHK(hipStreamSynchronize((hipStream_t)stream_));
    } else {
        BCHK(bitnet_hip_stop_configure(stop_, cfg));
    }
    if (!stop_on_) drop_graphs();  // the launch is part of the captured step
    stop_on_ = true;
    BCHK(bitnet_hip_stop_arm(stop_, 0));
    HCHK(hipMemcpy(n_forced_, &host_forced_, 4, hipMemcpyHostToDevice));
    return 0;
}

int Decoder::stop_state(bitnet_hip_stop_state *out) {
    if (!out) return fail_arg("stop_state: null output");
    if (!stop_on_) return fail_arg("stop_state: no stop criteria (set_stop first)");
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    BCHK(bitnet_hip_stop_get_state(stop_, out));
    return 0;
}

int Decoder::resume() {
    if (!stop_on_) return fail_arg("resume: no stop criteria (set_stop first)");
    if (int rc = arm_stop(true)) return rc;
    HCHK(hipMemcpy(n_forced_, &host_forced_, 4, hipMemcpyHostToDevice));
    return 0;
}

int Decoder::run_until_stop(int max_steps, int chunk, int *steps, float *elapsed_ms) {
    if (steps) *steps = 0;
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (!stop_on_) return fail_arg("run_until_stop: no stop criteria (set_stop first)");
    if (max_steps < 0 || chunk < 1) return fail_arg("run_until_stop: max_steps >= 0 and chunk >= 1 expected");
    bitnet_hip_stop_state st;
    if (int rc = stop_state(&st)) return rc;
    int queued = 0;
    float total = 0.f;
    while (st.reason == BITNET_HIP_STOP_NONE && queued < max_steps) {
        const int c = chunk < max_steps - queued ? chunk : max_steps - queued;
        float ms = 0.f;
        if (int rc = run(c, true, true, &ms)) return rc;
        queued += c, total += ms;
        BCHK(bitnet_hip_stop_get_state(stop_, &st));  // run() returned synchronised
    }
    if (steps) *steps = st.reason != BITNET_HIP_STOP_NONE && queued ? queued - st.frozen_steps : queued;
    if (elapsed_ms) *elapsed_ms = total;
    return 0;
}

int Decoder::graph_nodes(bool with_logits) {
    if (!embed_) return fail_arg("model globals not set");
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    const int form = form_at(p);
    if (int rc = ensure_graph(with_logits, form)) return rc < 0 ? rc : -rc;
    hipGraph_t g = (hipGraph_t)graph_[2 * form + (with_logits ? 1 : 0)];
    size_t n = 0;
    HCHK(hipGraphGetNodes(g, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    if (n) HCHK(hipGraphGetNodes(g, nodes.data(), &n));
    int kernels = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        if (hipGraphNodeGetType(nodes[i], &t) == hipSuccess && t == hipGraphNodeTypeKernel) ++kernels;
    }
    return kernels;
}

void Decoder::logprob_entry(bitnet_hip_logprob_args *out) const {
    *out = bitnet_hip_logprob_args{};
    if (lp_top_n_ < 0) return;
    out->logits_dev = logits_, out->pos_dev = pos_, out->history_dev = history_;
    out->records_dev = lp_records_, out->scratch_dev = lp_scratch_;
    out->capacity = (uint32_t)c_.max_pos, out->top_n = (uint32_t)lp_top_n_;
}

int Decoder::set_logprobs(int top_n) {
    if (top_n < -1 || top_n > BITNET_HIP_LOGPROB_TOP_MAX) return fail_arg("set_logprobs: top_n must be -1 (off) or 0..20");
    if (top_n == lp_top_n_) return 0;
    if (top_n >= 0 && (!lp_records_ || !lp_scratch_)) {  // both or neither: a call that failed between the two is made good by the next
        const size_t rb = (size_t)c_.max_pos * sizeof(bitnet_hip_logprob_record), sb = bitnet_hip_logprob_scratch_bytes((size_t)c_.vocab);
        if (!sb) return fail_arg("set_logprobs: vocabulary out of range");
        HCHK(lp_records_.alloc((size_t)c_.max_pos));
        HCHK(hipMemset(lp_records_, 0xff, rb));
        HCHK(lp_scratch_.alloc_zeroed(sb));
        // one launch of an empty entry: the kernel is loaded before a capture can meet it
        bitnet_hip_logprob_args none{};
        BCHK(bitnet_hip_logprob_dev(&none, (size_t)c_.vocab, stream_));
        HCHK(hipStreamSynchronize((hipStream_t)stream_));
    }
    drop_graphs();  // the launch and its top_n are part of the captured step
    lp_top_n_ = top_n;
    return 0;
}

int Decoder::logprobs(int first, int n, bitnet_hip_logprob_record *out) {
    if (lp_top_n_ < 0) return fail_arg("logprobs: switched off (set_logprobs first)");
    if (first < 0 || n < 0 || first > c_.max_pos || n > c_.max_pos - first) return fail_arg("logprobs: range outside [0, max_pos)");
    if (n > 0 && !out) return fail_arg("logprobs: null output");
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    if (n > 0) HCHK(hipMemcpy(out, lp_records_ + first, (size_t)n * sizeof(bitnet_hip_logprob_record), hipMemcpyDeviceToHost));
    return 0;
}

int Decoder::set_sampling(const bitnet_hip_sampling_config *cfg) {
    if (!cfg) return set_sampling_ex(nullptr);
    const bitnet_hip_sampling_config_ex x{*cfg, 0.0f, 1.0f, 0.0f, 0.0f};
    return set_sampling_ex(&x);
}

int Decoder::set_sampling_ex(const bitnet_hip_sampling_config_ex *cfg) {
    if (!cfg) {
        if (sampling_) drop_graphs();
        sampling_ = false;
        return 0;
    }
    if (!sampler_) {
        BCHK(bitnet_hip_sampler_create_ex((size_t)c_.vocab, cfg, &sampler_));
    } else {
        BCHK(bitnet_hip_sampler_configure_ex(sampler_, cfg));
    }
    if (!sampling_) drop_graphs();
    sampling_ = true;
    return 0;
}

int Decoder::set_mirostat(const bitnet_hip_mirostat_config *cfg) {
    if (!cfg) {  // off; a decoder that never sampled has nothing to switch off
        if (sampler_) BCHK(bitnet_hip_sampler_set_mirostat(sampler_, nullptr));
        return 0;
    }
    if (!sampling_ || !sampler_) return fail_arg("set_mirostat: sampling is off (set_sampling first)");
    // the mode is read from device memory by the sampling launch: the captured graphs follow it and stay
    BCHK(bitnet_hip_sampler_set_mirostat(sampler_, cfg));
    return 0;
}

int Decoder::mirostat_state(float *mu, uint64_t *fallbacks) {
    if (mu) *mu = 0.0f;
    if (fallbacks) *fallbacks = 0;
    if (!sampler_) return 0;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    BCHK(bitnet_hip_sampler_mirostat_state(sampler_, mu, fallbacks));
    return 0;
}

int Decoder::set_constraints(const bitnet_hip_constraints *cfg) {
    if (!cfg && !sampler_) return 0;  // off on a decoder that never sampled: nothing to switch off
    if (cfg && (!sampling_ || !sampler_)) return fail_arg("set_constraints: sampling is off (set_sampling first; temperature 0 is greedy)");
    HCHK(hipStreamSynchronize((hipStream_t)stream_));  // on or off, the config is copied synchronously: no queued step may still read the old one
    // bias, bans and the hold list are reached through device memory by the sampling launch: the captured graphs follow them and stay
    BCHK(bitnet_hip_sampler_set_constraints(sampler_, cfg));
    return 0;
}

int Decoder::constraints_state(uint64_t *chosen) {
    if (!chosen) return fail_arg("constraints_state: null pointer");
    *chosen = 0;
    if (!sampler_) return 0;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    BCHK(bitnet_hip_sampler_constraints_state(sampler_, chosen));
    return 0;
}

int Decoder::set_grammar(bitnet_hip_grammar *g, int start) {
    if (!g && !sampler_) return 0;  // off on a decoder that never sampled: nothing to switch off
    if (g && (!sampling_ || !sampler_)) return fail_arg("set_grammar: sampling is off (set_sampling first; temperature 0 is greedy)");
    HCHK(hipStreamSynchronize((hipStream_t)stream_));  // the words are copied synchronously: no queued step may still read the old ones
    // the mode bit, the table addresses and the state are reached through device memory by the sampling launch: the captured graphs follow and stay
    BCHK(bitnet_hip_sampler_set_grammar(sampler_, g, start));
    return 0;
}

int Decoder::set_grammar_state(int state) {
    if (!sampling_ || !sampler_) return fail_arg("set_grammar_state: sampling is off (set_sampling and set_grammar first)");
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    BCHK(bitnet_hip_sampler_set_grammar_state(sampler_, state));
    return 0;
}

int Decoder::grammar_state(int32_t *state, uint64_t *steps, uint64_t *violations) {
    if (state) *state = -1;
    if (steps) *steps = 0;
    if (violations) *violations = 0;
    if (!sampler_) return 0;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    BCHK(bitnet_hip_sampler_grammar_state(sampler_, state, steps, violations));
    return 0;
}

int Decoder::sampling_draws(uint64_t *out) {
    if (!out) {
        err_ = "sampling_draws: null pointer";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    *out = 0;
    if (sampler_) BCHK(bitnet_hip_sampler_draws(sampler_, out));
    return 0;
}

// the four fused handles of a layer from its seven uploaded projections; frees the seven on every path
int Decoder::adopt_projections(Layer &L, bitnet_hip_weights_t h[7]) {
    const bitnet_hip_weights_t qkv[3] = {h[0], h[1], h[2]}, gu[2] = {h[4], h[5]};
    int rc = bitnet_hip_weights_concat(qkv, 3, 0, &L.qkv);
    if (!rc) rc = bitnet_hip_weights_concat(gu, 2, 1, &L.gateup);
    if (!rc) {
        L.o = h[3];
        L.down = h[6];
        h[3] = h[6] = 0;
    }
    const std::string keep = rc ? (bitnet_hip_get_last_error() ? bitnet_hip_get_last_error() : "error") : "";
    for (int i = 0; i < 7; ++i)
        if (h[i]) bitnet_hip_weights_free(h[i]), h[i] = 0;
    if (rc) {
        release_layer(L);
        err_ = "weights_concat: " + keep;
        return BITNET_HIP_ERR_EXECUTION;
    }
    for (bitnet_hip_weights_t hh : {L.qkv, L.o, L.gateup, L.down}) {
        size_t ab = 0;
        bitnet_hip_weights_info(hh, nullptr, nullptr, &ab);
        weight_bytes_ += ab;
    }
    // LayerNorm applied after the product for the two normalised projections (bitnet_hip_weights_bind_ln)
    BCHK(bitnet_hip_weights_bind_ln(L.qkv, L.attn_norm, stream_));
    BCHK(bitnet_hip_weights_bind_ln(L.gateup, L.ffn_norm, stream_));
    L.q_ok = bitnet_hip_gemv_q_supported(L.qkv) && bitnet_hip_gemv_q_supported(L.o) && bitnet_hip_gemv_q_supported(L.gateup) &&
             bitnet_hip_gemv_q_supported(L.down) && c_.hidden <= 4096;
    return 0;
}

// The step runs on producer-quantised activations (include/bitnet_hip.h "QAct") when every layer's matrices are on that
// path and the mode asks for it; otherwise on exact f32 activations (round 1's kernels).
bool Decoder::qact_path() const {
    if (act_mode_ == 0) return false;
    for (const auto &L : layers_)
        if (!L.q_ok) return false;
    return true;
}

int Decoder::set_act_mode(int mode) {
    if (owner_) return fail_arg("this decoder borrows its weights (create_shared): the activation mode is the owner's");
    if (mode != 0 && mode != 1) {
        err_ = "activation mode must be 0 (exact f32) or 1 (QAct)";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (mode != act_mode_) drop_graphs();
    act_mode_ = mode;
    return 0;
}

int Decoder::set_layer_qk256(int layer, const LayerWeightsQk256 &w) {
    if (int rc = weights_locked()) return rc;
    if (layer < 0 || (size_t)layer >= layers_.size()) return fail_arg("layer index out of range");
    Layer &L = layers_[(size_t)layer];
    release_layer(L);
    const size_t H = c_.hidden, QD = (size_t)c_.n_heads * c_.head_dim, KD = (size_t)c_.n_kv_heads * c_.head_dim, F = c_.ffn;
    auto stride = [](size_t cols) { return (cols + 255) / 256 * 64; };
    HCHK(hipMemcpy(L.attn_norm, w.attn_norm, H * 4, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(L.ffn_norm, w.ffn_norm, H * 4, hipMemcpyHostToDevice));
    bitnet_hip_weights_t h[7] = {0};
    const uint8_t *src[7] = {w.q, w.k, w.v, w.o, w.gate, w.up, w.down};
    const size_t n[7] = {QD, KD, KD, H, F, F, H}, k[7] = {H, H, H, QD, H, H, F};
    for (int i = 0; i < 7; ++i) {
        if (bitnet_hip_weights_upload_qk256(src[i], n[i] * stride(k[i]), n[i], k[i], stride(k[i]), &h[i]) != 0) {
            const int rc = fail("bitnet_hip_weights_upload_qk256");
            for (int j = 0; j < i; ++j) bitnet_hip_weights_free(h[j]);
            return rc;
        }
    }
    return adopt_projections(L, h);
}

int Decoder::set_layer_i2s(int layer, const LayerWeightsI2s &w) {
    if (int rc = weights_locked()) return rc;
    if (layer < 0 || (size_t)layer >= layers_.size()) return fail_arg("layer index out of range");
    Layer &L = layers_[(size_t)layer];
    release_layer(L);
    const size_t H = c_.hidden, QD = (size_t)c_.n_heads * c_.head_dim, KD = (size_t)c_.n_kv_heads * c_.head_dim, F = c_.ffn;
    const size_t n[7] = {QD, KD, KD, H, F, F, H}, k[7] = {H, H, H, QD, H, H, F};
    HCHK(hipMemcpy(L.attn_norm, w.attn_norm, H * 4, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(L.ffn_norm, w.ffn_norm, H * 4, hipMemcpyHostToDevice));
    bitnet_hip_weights_t h[7] = {0};
    for (int i = 0; i < 7; ++i) {
        const size_t pk = (k[i] + 3) / 4, nb = (k[i] + w.block_size - 1) / w.block_size;
        if (bitnet_hip_weights_upload_i2s(w.w[i], pk * n[i], w.scales[i], nb * n[i], n[i], k[i], w.block_size, &h[i]) != 0) {
            const int rc = fail("bitnet_hip_weights_upload_i2s");
            for (int j = 0; j < i; ++j) bitnet_hip_weights_free(h[j]);
            return rc;
        }
    }
    return adopt_projections(L, h);
}

int Decoder::set_layer_specs(int layer, const float *attn_norm, const float *ffn_norm, const ProjSpec p[7]) {
    if (int rc = weights_locked()) return rc;
    if (layer < 0 || (size_t)layer >= layers_.size()) return fail_arg("layer index out of range");
    Layer &L = layers_[(size_t)layer];
    const size_t H = c_.hidden, QD = (size_t)c_.n_heads * c_.head_dim, KD = (size_t)c_.n_kv_heads * c_.head_dim, F = c_.ffn;
    const size_t n[7] = {QD, KD, KD, H, F, F, H}, k[7] = {H, H, H, QD, H, H, F};
    if (p[0].qk256 != p[1].qk256 || p[0].qk256 != p[2].qk256 || p[4].qk256 != p[5].qk256) {
        err_ = "q|k|v (and gate|up) must share one I2_S flavour to be fused";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    release_layer(L);
    HCHK(hipMemcpy(L.attn_norm, attn_norm, H * 4, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(L.ffn_norm, ffn_norm, H * 4, hipMemcpyHostToDevice));
    bitnet_hip_weights_t h[7] = {0};
    for (int i = 0; i < 7; ++i) {
        int rc;
        if (p[i].qk256) {
            const size_t stride = (k[i] + 255) / 256 * 64;
            rc = bitnet_hip_weights_upload_qk256(p[i].bytes, p[i].len, n[i], k[i], stride, &h[i]);
        } else {
            rc = bitnet_hip_weights_upload_coded(p[i].bytes, p[i].len, p[i].scales, p[i].n_scales, n[i], k[i], p[i].block, p[i].code_map, &h[i]);
        }
        if (rc != 0) {
            rc = fail("weights upload");
            for (int j = 0; j < i; ++j) bitnet_hip_weights_free(h[j]);
            return rc;
        }
    }
    return adopt_projections(L, h);
}

int Decoder::set_globals(const uint16_t *embed_f16, const float *final_norm) {
    if (int rc = weights_locked()) return rc;
    if (int rc = refresh_logits()) return rc;  // logits still owed from a screened step belong to the table that is about to go
    const size_t n = (size_t)c_.vocab * c_.hidden * 2;
    if (!embed_) HCHK(embed_.alloc(n));
    HCHK(hipMemcpy(embed_, embed_f16, n, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(final_norm_, final_norm, (size_t)c_.hidden * 4, hipMemcpyHostToDevice));
    if (head_screen_on_ || screen_) return ensure_screen_image();  // the image follows the table
    return 0;
}

int Decoder::reset() {
    host_forced_ = 0;
    if (sampler_) BCHK(bitnet_hip_sampler_reset(sampler_));
    if (int rc = arm_stop(false)) return rc;  // a new request
    HCHK(hipMemset(pos_, 0, 4));
    HCHK(hipMemset(n_forced_, 0, 4));
    HCHK(hipMemset(history_, 0, ((size_t)c_.max_pos + 2) * 4));
    if (lp_records_) {
        HCHK(hipMemset(lp_records_, 0xff, (size_t)c_.max_pos * sizeof(bitnet_hip_logprob_record)));
        HCHK(hipMemset(lp_scratch_, 0, 16));  // a clean hand-over, as bitnet_hip_sampler_reset re-arms the sampler's
    }
    return 0;
}

int Decoder::feed(const int32_t *tokens, int n) {
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    const int base = p > host_forced_ ? p : host_forced_;
    if (n < 0 || (n > 0 && !tokens)) {
        err_ = "feed: null tokens";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= c_.vocab) {  // TransformerModel::embed's index_select fails on it (T:1390-1426)
            char b[96];
            snprintf(b, sizeof(b), "token id %d out of range [0, %d)", tokens[i], c_.vocab);
            err_ = b;
            return BITNET_HIP_ERR_INVALID_ARGUMENT;
        }
    if (base + n > c_.max_pos) {
        err_ = "KV cache overflow";  // T:1190-1194
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    HCHK(hipMemcpy(history_ + base, tokens, (size_t)n * 4, hipMemcpyHostToDevice));
    host_forced_ = base + n;
    HCHK(hipMemcpy(n_forced_, &host_forced_, 4, hipMemcpyHostToDevice));
    return arm_stop(false);  // new prompt tokens: a new request, and no stop sequence may reach back across them
}

int Decoder::position() {
    int p = -1;
    if (hipMemcpy(&p, pos_, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        err_ = "position readback failed";
        return -1;
    }
    return p;
}

// The decode attention in the form and cache type this decoder runs: form 0 two kernels (64-position records), 1 and 3 records only
// (the o-projection merges them), 2 two kernels with 128-position records; out / qout: f32 output and / or its QAct.
int Decoder::attn_launch(Layer &L, int form, float *out, void *qout) {
    // forms (form_at): 0 = 64-position records + combine, 1 = 64-position records merged by the o-projection (<= 256 keys),
    //                  2 = 128-position records + combine, 3 = as 1 with the 8-record merge (257..kMerge8MaxKeys keys, QAct path)
    const int flags = (form == 2 ? BITNET_HIP_ATTN_WIDE : 0) | ((form & 1) ? BITNET_HIP_ATTN_PARTIAL : 0) | (kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0);
    BCHK(bitnet_hip_attention_decode_q_dev(qkv_, rope_sin_, rope_cos_, L.kcache, L.vcache, (size_t)c_.n_heads, (size_t)c_.n_kv_heads, (size_t)c_.head_dim,
                                           (size_t)c_.max_pos, pos_, attn_scratch_, flags, out, qout, stream_));
    return 0;
}

int Decoder::set_kv_f16(bool on) {
    if (position() != 0 || host_forced_ != 0) {
        err_ = "set_kv_f16: only on a fresh sequence (reset() first): a cache is f16 or f32 for its whole life";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (on != kv_f16_) {
        drop_graphs();
        for (auto &L : layers_) {  // stale bytes of the other type could be NaN / Inf patterns in this one
            const size_t n = (size_t)c_.n_kv_heads * (((size_t)c_.max_pos + 63) / 64 * 64) * c_.head_dim;
            HCHK(hipMemset(L.kcache, 0, n * sizeof(float)));
            HCHK(hipMemset(L.vcache, 0, n * sizeof(float)));
        }
    }
    kv_f16_ = on;
    return 0;
}

// Reads a device f32 vector back after the kernel that wrote it and leaves one trace record (reference format).
struct Decoder::Tracer {
    std::string dir;
    int seq = 0;
    void *stream = nullptr;
    std::string err;
    bool dump(const std::string &name, const char *stage, int layer, const float *dev, size_t n) {
        std::vector<float> h(n);
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(h.data(), dev, n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            err = "trace: read-back failed";
            return false;
        }
        double ss = 0.0;
        for (float v : h) ss += (double)v * (double)v;
        const double rms = std::sqrt(ss / (double)n);
        std::string file = name;
        for (char &c : file)
            if (c == '/' || c == '\\') c = '_';
        FILE *f = fopen((dir + "/" + file + ".trace").c_str(), "w");
        if (!f) {
            err = "trace: cannot write into " + dir;
            return false;
        }
        fprintf(f, "{\n  \"name\": \"%s\",\n  \"shape\": [\n    1,\n    %zu\n  ],\n  \"dtype\": \"F32\",\n  \"blake3\": \"%s\",\n  \"rms\": %.17g,\n"
                   "  \"num_elements\": %zu,\n  \"seq\": %d,\n  \"layer\": %d,\n  \"stage\": \"%s\"\n}",
                name.c_str(), n, Blake3::hex(h.data(), n * 4).c_str(), rms, n, seq, layer, stage);
        fclose(f);
        return true;
    }
};
#define TRACE(name, stage, layer, ptr, n)                                   \
    do {                                                                    \
        if (tr && !tr->dump(name, stage, layer, ptr, n)) {                  \
            err_ = tr->err;                                                 \
            return BITNET_HIP_ERR_EXECUTION;                                \
        }                                                                   \
    } while (0)

// One decode step = TransformerModel::forward (T:1557-1597) on one token + logits.
int Decoder::step_launches(bool with_logits, int form, Tracer *tr) {
    void *s = stream_;
    const size_t H = c_.hidden;
    const size_t tQD = (size_t)c_.n_heads * c_.head_dim, tKD = (size_t)c_.n_kv_heads * c_.head_dim;
    const std::string tp = tr ? "t" + std::to_string(tr->seq) + "/" : "";
    if (tr && (form & 1)) form = 0;  // the merging o-projection never materialises the attention output
    if (form == 3 && !qact_path()) form = 0;  // the 8-record merge exists on the QAct path only
    if (qact_path()) {
        // Every vector that travels between two GEMVs goes as a QAct written by its producer's epilogue (x: embedding /
        // down-projection, attention output: combine kernel or merging o-projection, x2: o-projection, h: gate|up).
        const size_t NH = (size_t)c_.n_heads, NK = (size_t)c_.n_kv_heads, MP = (size_t)c_.max_pos;
        BCHK(bitnet_hip_embed_q_dev(embed_, history_, pos_, H, (size_t)c_.vocab, x_, layers_[0].attn_norm, qa_x_, st_x_, s));
        TRACE(tp + "embeddings", "embeddings", -1, x_, H);
        for (size_t l = 0; l < layers_.size(); ++l) {
            Layer &L = layers_[l];
            const std::string bp = tp + "blk" + std::to_string(l) + "/";
            BCHK(bitnet_hip_gemv_q_dev(L.qkv, qa_x_, st_x_, L.attn_norm, c_.eps, nullptr, 0, qkv_, nullptr, nullptr, nullptr, s));
            TRACE(bp + "q_proj", "q_proj", (int)l, qkv_, tQD);
            TRACE(bp + "k_proj", "k_proj", (int)l, qkv_ + tQD, tKD);
            TRACE(bp + "v_proj", "v_proj", (int)l, qkv_ + tQD + tKD, tKD);
            if (form & 1) {
                if (int rc = attn_launch(L, form, nullptr, nullptr)) return rc;
                BCHK(bitnet_hip_gemv_attn_merge_rec_q_dev(L.o, attn_scratch_, NH, NK, MP, pos_, x2_, x_, qa_x2_, L.ffn_norm, st_x2_, form == 3 ? 8 : 4, s));
            } else {
                if (int rc = attn_launch(L, form, tr ? att_.get() : nullptr, qa_att_)) return rc;
                TRACE(bp + "attn_out", "attn_out", (int)l, att_, tQD);
                BCHK(bitnet_hip_gemv_q_dev(L.o, qa_att_, nullptr, nullptr, 0.f, x_, 0, x2_, qa_x2_, L.ffn_norm, st_x2_, s));
            }
            TRACE(bp + "attn_residual", "attn_residual", (int)l, x2_, H);
            BCHK(bitnet_hip_gemv_q_dev(L.gateup, qa_x2_, st_x2_, L.ffn_norm, c_.eps, nullptr, BITNET_HIP_FUSE_SILU_MUL, tr ? h_.get() : nullptr, qa_h_, nullptr, nullptr, s));
            TRACE(bp + "ffn_hidden", "ffn_hidden", (int)l, h_, (size_t)c_.ffn);
            const bool more = l + 1 < layers_.size();
            BCHK(bitnet_hip_gemv_q_dev(L.down, qa_h_, nullptr, nullptr, 0.f, x2_, 0, x_, more ? qa_x_.get() : nullptr, more ? layers_[l + 1].attn_norm.get() : nullptr,
                                       more ? st_x_.get() : nullptr, s));
            TRACE(bp + "ffn_out", "ffn_out", (int)l, x_, H);
        }
        if (tr) TRACE("t" + std::to_string(tr->seq) + "_all_layers_out", "all_layers_out", -1, x_, H);
        if (with_logits) {
            if (int rc = pick_token(s, !tr, tr != nullptr)) return rc;
            TRACE(tp + "logits", "logits", -1, logits_, (size_t)c_.vocab);
        } else {
            BCHK(bitnet_hip_advance_pos_dev(pos_, s));
        }
        return 0;
    }
    BCHK(bitnet_hip_embed_f16_dev(embed_, history_, pos_, 1, H, (size_t)c_.vocab, x_, s));
    TRACE(tp + "embeddings", "embeddings", -1, x_, H);
    for (size_t l = 0; l < layers_.size(); ++l) {
        Layer &L = layers_[l];
        const std::string bp = tp + "blk" + std::to_string(l) + "/";
        // attention_norm -> q,k,v (T:1015, T:288-290), fused into one launch
        BCHK(bitnet_hip_gemv_fused_dev(L.qkv, x_, qkv_, 1, L.attn_norm, c_.eps, nullptr, 0, s));
        TRACE(bp + "q_proj", "q_proj", (int)l, qkv_, tQD);
        TRACE(bp + "k_proj", "k_proj", (int)l, qkv_ + tQD, tKD);
        TRACE(bp + "v_proj", "v_proj", (int)l, qkv_ + tQD + tKD, tKD);
        if (form == 2) {
            if (int rc = attn_launch(L, 2, att_, nullptr)) return rc;
            TRACE(bp + "attn_out", "attn_out", (int)l, att_, tQD);
            BCHK(bitnet_hip_gemv_fused_dev(L.o, att_, x2_, 1, nullptr, 0.f, x_, 0, s));
        } else if (form == 1) {
            // short contexts: one attention launch; the o-projection merges the chunk records itself
            if (int rc = attn_launch(L, 1, nullptr, nullptr)) return rc;
            BCHK(bitnet_hip_gemv_attn_merge_dev(L.o, attn_scratch_, (size_t)c_.n_heads, (size_t)c_.n_kv_heads, (size_t)c_.max_pos, pos_, x2_, x_, s));
        } else {
            if (int rc = attn_launch(L, 0, att_, nullptr)) return rc;
            TRACE(bp + "attn_out", "attn_out", (int)l, att_, tQD);
            // o_proj + residual (T:542, T:1073)
            BCHK(bitnet_hip_gemv_fused_dev(L.o, att_, x2_, 1, nullptr, 0.f, x_, 0, s));
        }
        TRACE(bp + "attn_residual", "attn_residual", (int)l, x2_, H);
        // post_attention_layernorm -> gate, up -> silu(gate)*up (T:1104, T:756-781)
        BCHK(bitnet_hip_gemv_fused_dev(L.gateup, x2_, h_, 1, L.ffn_norm, c_.eps, nullptr, BITNET_HIP_FUSE_SILU_MUL, s));
        TRACE(bp + "ffn_hidden", "ffn_hidden", (int)l, h_, (size_t)c_.ffn);
        // down_proj + residual (T:789, T:1125)
        BCHK(bitnet_hip_gemv_fused_dev(L.down, h_, x_, 1, nullptr, 0.f, x2_, 0, s));
        TRACE(bp + "ffn_out", "ffn_out", (int)l, x_, H);
    }
    if (tr) TRACE("t" + std::to_string(tr->seq) + "_all_layers_out", "all_layers_out", -1, x_, H);
    if (with_logits) {
        // final norm + tied logits + greedy token (T:1589, T:1599-1630, sampling.rs:189-202)
        if (int rc = pick_token(s, !tr, tr != nullptr)) return rc;
        TRACE(tp + "logits", "logits", -1, logits_, (size_t)c_.vocab);
    } else {
        BCHK(bitnet_hip_advance_pos_dev(pos_, s));
    }
    return 0;
}

int Decoder::trace_step(const char *dir, bool with_logits) {
    if (!embed_) {
        err_ = "model globals not set";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (!dir || !*dir) {
        err_ = "trace_step: no directory";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (p + 1 > c_.max_pos - 1) {
        err_ = "KV cache overflow";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (!with_logits && p + 1 > host_forced_) {
        err_ = "trace_step(with_logits = false) past the fed tokens";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    Tracer tr;
    tr.dir = dir;
    tr.seq = p;  // token position of this step (the reference counts 0 = first position)
    tr.stream = stream_;
    const int rc = step_launches(with_logits, form_at(p), &tr);
    if (rc) return rc;
    if (with_logits) picked(pick_screened_);
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    return 0;
}

// The same step UNFUSED, in the reference's own op order (T:977-1134), every projection on the reference-order kernel
// (BITNET_HIP_KERNEL_EXACT: bit-identical to the scalar CPU loops): LayerNorm rows -> GEMV -> attention -> GEMV ->
// residual add -> LayerNorm rows -> GEMV (gate|up tiles) -> silu*mul -> GEMV -> residual add.  Slow (one thread per
// output row); bench.py and the tests hold the fast step's logits against it at the full model size.
int Decoder::step_launches_reference(bool with_logits) {
    void *s = stream_;
    const size_t H = c_.hidden, F = c_.ffn;
    const int K = BITNET_HIP_KERNEL_EXACT;
    BCHK(bitnet_hip_embed_f16_dev(embed_, history_, pos_, 1, H, (size_t)c_.vocab, x_, s));
    for (auto &L : layers_) {
        BCHK(bitnet_hip_norm_rows_dev(x_, L.attn_norm, ref_n_, 1, H, c_.eps, 0, s));
        BCHK(bitnet_hip_matmul_kernel_dev(L.qkv, ref_n_, qkv_, 1, K, s));
        if (int rc = attn_launch(L, 0, att_, nullptr)) return rc;
        BCHK(bitnet_hip_matmul_kernel_dev(L.o, att_, ref_t_, 1, K, s));
        BCHK(bitnet_hip_add_dev(x_, ref_t_, x2_, H, s));
        BCHK(bitnet_hip_norm_rows_dev(x2_, L.ffn_norm, ref_n_, 1, H, c_.eps, 0, s));
        BCHK(bitnet_hip_matmul_kernel_dev(L.gateup, ref_n_, ref_gu_, 1, K, s));  // alternating 16-row (gate, up) tiles
        BCHK(bitnet_hip_silu_mul_dev(ref_gu_, ref_gu_ + 16, h_, F, 16, s));
        BCHK(bitnet_hip_matmul_kernel_dev(L.down, h_, ref_t_, 1, K, s));
        BCHK(bitnet_hip_add_dev(x2_, ref_t_, x_, H, s));
    }
    if (with_logits) {
        if (int rc = pick_token(s, false)) return rc;
    } else {
        BCHK(bitnet_hip_advance_pos_dev(pos_, s));
    }
    return 0;
}

int Decoder::run_reference(int n, bool with_logits) {
    if (!embed_) {
        err_ = "model globals not set";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (c_.ffn % 16 != 0) {
        err_ = "run_reference: ffn must be a multiple of 16";
        return BITNET_HIP_ERR_UNSUPPORTED;
    }
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (p + n > c_.max_pos - 1) {
        err_ = "KV cache overflow";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < n; ++i) {
        const int rc = step_launches_reference(with_logits);
        if (rc) return rc;
        if (with_logits) picked(pick_screened_);
    }
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    // the reference-order kernels rebuilt a row-major copy of every matrix: give them back (one copy of the weights on the device)
    for (auto &L : layers_)
        for (bitnet_hip_weights_t h : {L.qkv, L.o, L.gateup, L.down})
            if (h) bitnet_hip_weights_trim(h);
    return 0;
}

// Which attention form a step at `pos` (pos + 1 keys) takes; the host knows every step's position.
int Decoder::form_at(int pos) const {
    // BITNET_HOST_ATTN_MERGE = the largest record count the o-projection merges: 0 none (also negative values and text that is no number: atoi), 1..7 four (<= 256 keys), unset or >= 8 eight
    static const int merge_env = getenv("BITNET_HOST_ATTN_MERGE") ? atoi(getenv("BITNET_HOST_ATTN_MERGE")) : 8;
    static const bool wide_env = !(getenv("BITNET_HOST_ATTN_WIDE") && atoi(getenv("BITNET_HOST_ATTN_WIDE")) == 0);
    const int keys = pos + 1;
    if (attn_form_ >= 0) return attn_form_;  // set_attention_form
    if (merge_env > 0 && merge_ok_ && keys <= (int)bitnet_hip_attention_merge_max_keys()) return 1;
    // 257..kMerge8MaxKeys keys: the same 64-position records, merged eight at a time by a prologue that asks for each value once
    // (EXPERIMENTS 15; the QAct path only: k_gemv_mfma's merge stays at 4 records).
    // (257..512 keys as four 128-position records merged by the o-projection measured SLOWER than 64-position records + combine --
    // c2 1201-1214 vs 1224 tok/s, round 2 -- and was removed in round 3: the wide attention kernel is +1.5 us at these lengths)
    if (merge_env >= 8 && merge8_ok_ && qact_path() && keys <= kMerge8MaxKeys && keys <= (int)bitnet_hip_attention_merge_q_max_keys()) return 3;
    if (wide_env && c_.n_kv_heads * ((keys + 63) / 64) > 256) return 2;  // more 64-position chunks than CUs
    return 0;
}

int Decoder::prepare_graphs(bool with_logits) {
    if (!embed_) {
        err_ = "model globals not set";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    unsigned forms = 0;
    for (int pos = 0; pos + 1 < c_.max_pos; ++pos) forms |= 1u << form_at(pos);
    for (int f = 0; f < kGraphs / 2; ++f)
        if (forms & (1u << f))
            if (int rc = ensure_graph(with_logits, f)) return rc;
    return 0;
}

int Decoder::ensure_graph(bool with_logits, int form) {
    const int gi = 2 * form + (with_logits ? 1 : 0);
    if (graphs_screened_ != (int)screen_step(false)) drop_graphs();  // captured under another head (a batch slot taken or left since)
    if (graph_exec_[gi]) return 0;
    graphs_screened_ = (int)screen_step(false);
    hipStream_t s = (hipStream_t)stream_;
    hipGraph_t g = nullptr;
    HCHK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    const int rc = step_launches(with_logits, form);
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc != 0) {
        if (g) hipGraphDestroy(g);
        return rc;
    }
    HCHK(e);
    hipGraphExec_t ex = nullptr;
    HCHK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    graph_[gi] = g;
    graph_exec_[gi] = ex;
    return 0;
}

int Decoder::run(int n, bool with_logits, bool use_graph, float *elapsed_ms) {
    if (!embed_) {
        err_ = "model globals not set";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (p + n > c_.max_pos - 1) {
        err_ = "KV cache overflow";  // T:1190-1194
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (!with_logits && p + n > host_forced_) {
        // a step without logits samples nothing: the NEXT position's token must already be in the history
        err_ = "run(with_logits = false) past the fed tokens: nothing would choose the next token";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    if (!trace_dir_.empty()) {  // BITNET_TRACE_DIR: every step eagerly, with read-backs (slow by design)
        for (int i = 0; i < n; ++i) {
            const int rc = trace_step(trace_dir_.c_str(), with_logits);
            if (rc) return rc;
        }
        if (elapsed_ms) *elapsed_ms = 0.f;
        return 0;
    }
    hipStream_t s = (hipStream_t)stream_;
    if (use_graph) {
        for (int i = 0; i < n; ++i) {  // every form this run needs (at most three captures)
            int rc = ensure_graph(with_logits, form_at(p + i));
            if (rc) return rc;
        }
    }
    StreamTimer timer;
    HCHK(timer.start(s));
    for (int i = 0; i < n; ++i) {
        if (use_graph) {
            HCHK(hipGraphLaunch((hipGraphExec_t)graph_exec_[2 * form_at(p + i) + (with_logits ? 1 : 0)], s));
        } else {
            int rc = step_launches(with_logits, form_at(p + i));
            if (rc) return rc;
        }
        if (with_logits) picked(screen_step(false));
    }
    HCHK(timer.stop(s, elapsed_ms));
    return 0;
}

// The prompt forward as an f16 ACTIVATION CHAIN (bitnet_hip_matmul_f16_dev): every projection reads f16 rows that the kernel producing
// them wrote -- the o- / down-projection's epilogue leaves x (f32, the residual stream), f16(gamma_next * x) and the LayerNorm statistics
// partials; the attention writes f16 rows; gate|up's epilogue writes f16(silu(gate) * up) -- so no row quantiser / conversion launch sits
// between two matmuls (four per layer otherwise: 69 us of a 925 us BitNet32-F16 layer at 4096 tokens, and the f32 round trips they read).
// Taken at digits = 2 (the f16-activation precision class) when every projection of the model takes the chain; automatic for the
// block-scaled format, whose matmul runs on f16 activations anyway; BITNET_HOST_PREFILL_CHAIN=1 forces it for QK256 (whose int8 digit
// matmul is the faster kernel: the default there stays the digit planes), =0 switches it off.
bool Decoder::chain_applies(int digits) const {
    if (force_scaled_ || digits != 2 || prefill_chain_ == 0 || layers_.empty()) return false;
    bool scaled_all = true;
    for (const auto &L : layers_) {
        for (bitnet_hip_weights_t h : {L.qkv, L.o, L.gateup, L.down})
            if (!h || !bitnet_hip_matmul_f16_supported(h)) return false;
        size_t rows = 0, cols = 0, ab = 0;
        if (bitnet_hip_weights_info(L.qkv, &rows, &cols, &ab) != 0) return false;
        scaled_all = scaled_all && ab > rows * cols / 4;  // algorithmic bytes beyond the 2-bit codes: block scales
    }
    return prefill_chain_ == 1 || scaled_all;
}

// The int8 digit form (QK256's prompt matmul) keeps its row quantisers, but the two inputs no LayerNorm touches travel as f16: the
// attention writes f16 rows, gate|up's epilogue writes f16(silu(gate) * up), and the o- / down-projection's quantisers read them
// (BITNET_HIP_FUSE_X_F16 / _Y_F16): half the bytes on both sides of the two largest hand-overs.  digits = 2 only (an f16 row holds 11
// bits of each element: more than the 2-digit planes take from most elements, fewer than 3 or 4 digits).
bool Decoder::handover16_applies(int digits) const {
    if (force_scaled_ || digits != 2 || prefill_chain_ == 0 || layers_.empty()) return false;
    for (const auto &L : layers_)
        for (bitnet_hip_weights_t h : {L.o, L.gateup, L.down}) {
            size_t rows = 0, cols = 0, ab = 0;
            if (!h || bitnet_hip_weights_info(h, &rows, &cols, &ab) != 0) return false;
            if (ab != rows * (cols / 4) || cols % 256 != 0 || rows % 16 != 0) return false;  // unscaled 2-bit codes, the tiled matmul's shapes
        }
    return c_.ffn % 4 == 0;
}

// q|k|v and gate|up of the digit-plane prompt forward (unscaled matrices, digits = 2) on the block-scaled fp6 x fp4 MFMA reading RESIDENT fp4 images
// (bitnet_hip_weights_fp4_image: built here once per model, 22.6 MB per layer at the 2B-4T widths; the 2-bit tiles stay the decode copy) -- the
// same integers as the int8 planes, bit for bit, with no code expansion in the K loop.  BITNET_HOST_PREFILL_FP6=0 keeps the int8 planes.
int Decoder::fp6_flag(int digits) {
    if (digits != 2 || layers_.empty()) return 0;
    if (prefill_fp6_ < 0) {
        const char *e = getenv("BITNET_HOST_PREFILL_FP6");
        prefill_fp6_ = e ? (atoi(e) != 0 ? 1 : 0) : 1;
        for (const auto &L : layers_) {
            if (!prefill_fp6_) break;
            for (bitnet_hip_weights_t h : {L.qkv, L.gateup})
                if (!h || bitnet_hip_weights_fp4_image(h, 1, stream_) != 0) {  // scaled / other code maps: the form does not apply to this model
                    prefill_fp6_ = 0;
                    break;
                }
        }
        if (!prefill_fp6_)
            for (const auto &L : layers_)
                for (bitnet_hip_weights_t h : {L.qkv, L.gateup})
                    if (h) (void)bitnet_hip_weights_fp4_image(h, 0, stream_);
    }
    return prefill_fp6_ ? BITNET_HIP_FUSE_FP6_DIGITS : 0;
}

// (Decoder::prefill explains; BITNET_HOST_PREFILL_HYBRID=0 keeps the int8 digit planes for all four projections, =2 takes the f16 form at
// any length.)  Only for long shares -- where the hidden-row launches of 64-token tiles come to 400 workgroups or more (from 2497 tokens at
// hidden 2560: 40 token tiles x 10 row blocks): measured, QK256, same box -- 4096 tokens 21.5 -> 20.3 ms, 3072 tokens 17.3 -> 16.4, 8192 tokens 45.3 -> 43.4, but 2048
// tokens 11.8 -> 12.0 and 1024 tokens (also one rank's share of the 8-GPU prompt) 7.2 -> 7.8 ms.
bool Decoder::hybrid_applies(size_t n_rows) {
    if (prefill_hybrid_ < 0) {
        const char *e = getenv("BITNET_HOST_PREFILL_HYBRID");
        prefill_hybrid_ = !e ? 1 : atoi(e) == 2 ? 2 : atoi(e) != 0 ? 1 : 0;
    }
    if (!prefill_hybrid_ || layers_.empty()) return false;
    if (prefill_hybrid_ != 2 && ((size_t)c_.hidden / 256) * ((n_rows + 63) / 64) < 400) return false;
    for (const auto &L : layers_)
        if (bitnet_hip_matmul_f16_supported(L.o) != 1 || bitnet_hip_matmul_f16_supported(L.down) != 1) return false;
    return true;
}

int Decoder::ensure_chain_buffers(size_t N) {
    const size_t H = c_.hidden, QD = (size_t)c_.n_heads * c_.head_dim, F = c_.ffn;
    const size_t NP = (N + 63) / 64 * 64, nst = H / 64;
    hipStream_t s = (hipStream_t)stream_;
    if ((int)NP > pfc_cap_) {
        release_all(pf_xh_, pf_atth_, pf_hh_, pf_stats_);
        pfc_cap_ = 0;
        HCHK(pf_xh_.alloc(NP * H * 2));
        HCHK(pf_atth_.alloc(NP * QD * 2));
        HCHK(pf_hh_.alloc(NP * F * 2));
        HCHK(pf_stats_.alloc(nst * NP * 2));
        // rows past the prompt are read by the last token tile (never stored): they must hold finite values
        HCHK(hipMemsetAsync(pf_xh_, 0, NP * H * 2, s));
        HCHK(hipMemsetAsync(pf_atth_, 0, NP * QD * 2, s));
        HCHK(hipMemsetAsync(pf_hh_, 0, NP * F * 2, s));
        HCHK(hipMemsetAsync(pf_stats_, 0, nst * NP * 2 * sizeof(float), s));
        pfc_cap_ = (int)NP;
    }
    return 0;
}

// The QK256 prompt forward with NO row quantiser launch (round 5): q|k|v and gate|up run the fp6 x fp4 form on QB32 rows -- block-scaled 15-bit
// fixed point, one exponent per 32 columns of a token -- that the kernel PRODUCING the residual stream wrote: the o- / down-projection (f16 matrix
// cores, 320-row workgroups: the hybrid forward's launches) leaves x (f32), QB32(gamma_next * x) and the LayerNorm statistics partials in its
// epilogue (BITNET_HIP_FUSE_YH_QB32); LayerNorm is applied after the product (as on the f16 chain and in the decode step).  Only where the hybrid
// forward applies (long prompts: the producers then run 64-token tiles) and every q|k|v / gate|up matrix takes the form.  OPT-IN
// (BITNET_HOST_PREFILL_QB32=1): measured same-box it is a tie with the quantiser launches (18.91-18.93 vs 18.97-19.00 ms at 4096 tokens: the 41.5 us of
// quantisers per layer come back as +17 / +6.5 us in gate|up / q|k|v and +9 us per producing launch -- the prompt forward runs at a power limit, and the
// memory-bound quantisers were also the matrix pipes' rest: EXPERIMENTS 8.3), and the default keeps the form that is bit-identical to the int8 planes.
bool Decoder::qb32_applies(int digits, size_t n_rows) {
    if (prefill_qb32_ < 0) {
        const char *e = getenv("BITNET_HOST_PREFILL_QB32");
        prefill_qb32_ = e ? (atoi(e) != 0 ? 1 : 0) : 0;
    }
    if (force_scaled_ || !prefill_qb32_ || digits != 2 || !handover16_applies(digits) || !hybrid_applies(n_rows) || !fp6_flag(digits)) return false;
    for (const auto &L : layers_)
        for (bitnet_hip_weights_t h : {L.qkv, L.gateup})
            if (!h || bitnet_hip_matmul_qb32_supported(h) != 1) return false;
    return true;
}

// The form of ONE prompt forward over N rows, decided once, and the only place a forward grows a buffer beyond ensure_prompt_buffers: the
// f16 hand-over rows (chain, QB32, h16) and the QB32 rows.  RULE: every growth of a buffer happens here or in ensure_prompt_buffers, before
// the forward's first launch; the repeat after a saturation asks again under force_scaled_, gets the plain digit-plane form, and grows and
// frees nothing.  sharded: the token-parallel forward's restriction -- never the chain or QB32 forms, no fp6 flag on q|k|v and gate|up, no
// f6od (and, running no prompt_layers, last_prefill_path_ left as it is).
int Decoder::prompt_form(size_t N, int digits, bool sharded, PromptForm *out) {
    PromptForm f;
    f.digits = digits;
    f.chain = !sharded && chain_applies(digits);
    f.qb = !sharded && !f.chain && qb32_applies(digits, N);
    f.h16 = !f.chain && !f.qb && handover16_applies(digits);
    // Hybrid (unscaled matrices): the two projections whose inputs ARE f16 rows (the attention output, silu * up) multiply them on the f16
    // matrix cores as they stand (k_gemm_f16a, 320-row workgroups: one round of the chip at 4096 tokens) -- no quantiser launch, no second
    // rounding of values that were rounded to f16 already; q|k|v and gate|up keep the faster int8 digit planes behind their LayerNorm.
    f.hybrid = f.h16 && hybrid_applies(N);
    if (!sharded) {
        if (prefill_fp6_od_ < 0) {  // experiment: o / down on the fp6 form too (non-hybrid)
            const char *e = getenv("BITNET_HOST_PREFILL_FP6_OD");
            prefill_fp6_od_ = e && atoi(e) != 0 ? 1 : 0;
        }
        f.f6 = (f.chain || f.qb) ? 0 : fp6_flag(digits);
        f.f6od = prefill_fp6_od_ ? f.f6 : 0;
    }
    if (f.f16_rows())
        if (int rc = ensure_chain_buffers(N)) return rc;
    const size_t NP = (N + 63) / 64 * 64;
    if (f.qb && (int)NP > pf_qb_cap_) {
        release_all(pf_qb_);
        pf_qb_cap_ = 0;
        HCHK(pf_qb_.alloc(bitnet_hip_qb32_bytes(NP, (size_t)c_.hidden)));
        HCHK(hipMemsetAsync(pf_qb_, 0, bitnet_hip_qb32_bytes(NP, (size_t)c_.hidden), (hipStream_t)stream_));
        pf_qb_cap_ = (int)NP;
    }
    *out = f;
    return 0;
}

// The attention of one layer of a prompt forward over the N rows in pf_qkv_, by the operator the driver names: the whole-prompt operator on
// a fresh sequence; the continuation operator on a live one, which reads the past keys from the cache and takes every slot at or beyond
// op.past from the new rows; the packed operator over every member's own caches of the layer; the decode attention over the rows' own caches.
int Decoder::prompt_attention(Layer &L, size_t N, void *out, bool out_f16, const AttnOp &op) {
    const size_t NH = (size_t)c_.n_heads, NK = (size_t)c_.n_kv_heads, D = (size_t)c_.head_dim, MP = (size_t)c_.max_pos;
    const int flags = (kv_f16_ ? BITNET_HIP_ATTN_CACHE_F16 : 0) | (out_f16 ? BITNET_HIP_ATTN_OUT_F16 : 0);
    const size_t li = (size_t)(&L - layers_.data());
    if (op.kind == AttnOp::Rows) {
        // a wide step (step_wide, WideBatch::step): the N rows are N members' current tokens, each over its OWN caches of this layer at its own
        // position; the tables and the cache type are the operator's (the members'), not necessarily this driver's
        const int rflags = (op.kv_f16 ? BITNET_HIP_ATTN_CACHE_F16 : 0) | (out_f16 ? BITNET_HIP_ATTN_OUT_F16 : 0);
        BCHK(bitnet_hip_attention_decode_rows_dev(pf_qkv_, rope_sin_, rope_cos_, op.tables + (2 * li) * BITNET_HIP_WIDE_MAX,
                                                  op.tables + (2 * li + 1) * BITNET_HIP_WIDE_MAX,
                                                  reinterpret_cast<const int32_t *const *>(op.tables + 2 * layers_.size() * BITNET_HIP_WIDE_MAX), N, NH, NK, D, MP,
                                                  op.key_bound, wide_scratch_, rflags, out, stream_));
    } else if (op.kind == AttnOp::Pack) {
        // a pack (prefill_packed): the N rows are several members' segments, each over its OWN caches of this layer
        void *kc[BITNET_HIP_PACK_MAX], *vc[BITNET_HIP_PACK_MAX];
        for (size_t i = 0; i < op.n; ++i) kc[i] = op.members[i]->layers_[li].kcache, vc[i] = op.members[i]->layers_[li].vcache;
        BCHK(bitnet_hip_attention_packed_dev(pf_qkv_, N, rope_sin_, rope_cos_, op.n, op.row0, op.len, op.pasts, kc, vc, NH, NK, D, MP, pf_attn_ws_, pf_attn_ws_bytes_,
                                             out, flags, stream_));
    } else if (op.kind == AttnOp::Continue)
        BCHK(bitnet_hip_attention_extend_dev(pf_qkv_, rope_sin_, rope_cos_, L.kcache, L.vcache, NH, NK, D, MP, op.past, N, pf_attn_ws_, pf_attn_ws_bytes_, out, flags, stream_));
    else if (out_f16)
        BCHK(bitnet_hip_attention_prefill_flags_dev(pf_qkv_, rope_sin_, rope_cos_, L.kcache, L.vcache, NH, NK, D, MP, N, pf_attn_ws_, pf_attn_ws_bytes_, out, flags, stream_));
    else if (kv_f16_)
        BCHK(bitnet_hip_attention_prefill_kv16_dev(pf_qkv_, rope_sin_, rope_cos_, L.kcache, L.vcache, NH, NK, D, MP, N, pf_attn_ws_, pf_attn_ws_bytes_, static_cast<float *>(out), stream_));
    else
        BCHK(bitnet_hip_attention_prefill_dev(pf_qkv_, rope_sin_, rope_cos_, L.kcache, L.vcache, NH, NK, D, MP, N, pf_attn_ws_, pf_attn_ws_bytes_, static_cast<float *>(out), stream_));
    return 0;
}

// The four projections of a layer, each in the form f names.  The two chains (bitnet_hip_matmul_f16_dev / _qb32_dev) hand rows from kernel to
// kernel -- the o- / down-projection's epilogue leaves x (f32, the residual stream), f16 or QB32 rows of gamma_next * x and the LayerNorm
// statistics partials; the attention writes f16 rows; gate|up's epilogue writes f16(silu(gate) * up) -- so no row quantiser / conversion
// launch sits between two matmuls; the digit planes (bitnet_hip_matmul_fused_dev) quantise their rows themselves, from f32 or, with the f16
// hand-over, from the f16 rows of the attention and of gate|up.
// q|k|v of layer l.  In front of the first layer the chains convert the embedded rows once (one statistics partial per row; a producing
// epilogue leaves hidden / 64 of them).
int Decoder::project_qkv(size_t l, size_t N, const PromptForm &f) {
    Layer &L = layers_[l];
    const size_t H = c_.hidden, n_stats = l == 0 ? 1 : H / 64;
    if (f.chain) {
        if (l == 0) BCHK(bitnet_hip_rows_to_f16_dev(pf_x_, L.attn_norm, N, H, pf_xh_, pf_stats_, stream_));
        BCHK(bitnet_hip_matmul_f16_dev(L.qkv, pf_xh_, N, pf_stats_, n_stats, L.attn_norm, c_.eps, pf_qkv_, nullptr, 0, nullptr, nullptr, nullptr, stream_));
    } else if (f.qb) {
        if (l == 0) BCHK(bitnet_hip_rows_to_qb32_dev(pf_x_, L.attn_norm, N, H, pf_qb_, pf_stats_, stream_));
        BCHK(bitnet_hip_matmul_qb32_dev(L.qkv, pf_qb_, N, pf_stats_, n_stats, L.attn_norm, c_.eps, pf_qkv_, nullptr, 0, nullptr, nullptr, nullptr, stream_));
    } else
        BCHK(bitnet_hip_matmul_fused_dev(L.qkv, pf_x_, pf_qkv_, N, L.attn_norm, c_.eps, nullptr, f.f6, f.digits, pf_gemm_ws_, pf_gemm_ws_bytes_, stream_));
    return 0;
}

// o and down: rows in (in16 where the form hands f16 rows, else in32), the residual stream pf_x_ in and out.  next_norm: the LayerNorm the
// chains prepare the next matmul's rows for, or null behind the last layer, which hands over nothing.
int Decoder::project_residual(bitnet_hip_weights_t w, size_t N, const PromptForm &f, const float *in32, const void *in16, const float *next_norm) {
    if (f.chain || f.qb || f.hybrid) {
        void *hand = !next_norm ? nullptr : f.chain ? pf_xh_.get() : f.qb ? pf_qb_.get() : nullptr;
        BCHK(bitnet_hip_matmul_f16_dev(w, in16, N, nullptr, 0, nullptr, 0.f, pf_x_, pf_x_, hand && f.qb ? BITNET_HIP_FUSE_YH_QB32 : 0, hand, hand ? next_norm : nullptr,
                                       hand ? pf_stats_.get() : nullptr, stream_));
    } else
        BCHK(bitnet_hip_matmul_fused_dev(w, f.h16 ? static_cast<const float *>(in16) : in32, pf_x_, N, nullptr, 0.f, pf_x_, f.h16 ? BITNET_HIP_FUSE_X_F16 | f.f6od : 0,
                                         f.digits, pf_gemm_ws_, pf_gemm_ws_bytes_, stream_));
    return 0;
}

int Decoder::project_o(Layer &L, size_t N, const PromptForm &f) { return project_residual(L.o, N, f, pf_att_, pf_atth_, L.ffn_norm); }

int Decoder::project_down(Layer &L, size_t N, const PromptForm &f, const float *next_norm) { return project_residual(L.down, N, f, pf_h_, pf_hh_, next_norm); }

int Decoder::project_gateup(Layer &L, size_t N, const PromptForm &f) {
    const size_t n_stats = (size_t)c_.hidden / 64;  // always behind an o-projection's epilogue
    if (f.chain)
        BCHK(bitnet_hip_matmul_f16_dev(L.gateup, pf_xh_, N, pf_stats_, n_stats, L.ffn_norm, c_.eps, nullptr, nullptr, BITNET_HIP_FUSE_SILU_MUL, pf_hh_, nullptr, nullptr, stream_));
    else if (f.qb)
        BCHK(bitnet_hip_matmul_qb32_dev(L.gateup, pf_qb_, N, pf_stats_, n_stats, L.ffn_norm, c_.eps, nullptr, nullptr, BITNET_HIP_FUSE_SILU_MUL, pf_hh_, nullptr, nullptr, stream_));
    else
        BCHK(bitnet_hip_matmul_fused_dev(L.gateup, pf_x_, f.h16 ? static_cast<float *>(pf_hh_.get()) : pf_h_, N, L.ffn_norm, c_.eps, nullptr,
                                         BITNET_HIP_FUSE_SILU_MUL | (f.h16 ? BITNET_HIP_FUSE_Y_F16 : 0) | f.f6, f.digits, pf_gemm_ws_, pf_gemm_ws_bytes_, stream_));
    return 0;
}

// Every layer over the N rows in pf_x_ (embeddings in, residual stream of the last block out) in the form f, with the attention op names.
int Decoder::prompt_layers(size_t N, const PromptForm &f, const AttnOp &op) {
    // last_prefill_path(): the plain loop is recorded as it starts, a chain once it went through (one that a launcher refuses at this shape
    // leaves the record as it was)
    if (!f.chain && !f.qb) last_prefill_path_ = 0;
    for (size_t l = 0; l < layers_.size(); ++l) {
        Layer &L = layers_[l];
        if (int rc = project_qkv(l, N, f)) return rc;
        if (int rc = prompt_attention(L, N, f.f16_rows() ? pf_atth_ : pf_att_, f.f16_rows(), op)) return rc;
        if (int rc = project_o(L, N, f)) return rc;
        if (int rc = project_gateup(L, N, f)) return rc;
        if (int rc = project_down(L, N, f, l + 1 < layers_.size() ? layers_[l + 1].attn_norm.get() : nullptr)) return rc;
    }
    if (f.chain || f.qb) last_prefill_path_ = f.chain ? 1 : 2;
    return 0;
}

// THE SATURATION RULE, for every driver (prompt_forward, packed_forward, wide_forward): f16 hand-over rows carry no row scale, so a value
// beyond +-65504 (outlier channels x gamma: none in the synthetic models, possible in a real checkpoint) is clamped AND counted
// (bitnet_hip_f16_saturations).  A forward that clamped anything is repeated -- whole -- on the digit planes: 30-bit fixed point behind a
// per-row power-of-two scale (digits = 4: a row whose outlier is 10^5 times its typical element still keeps 13 bits of those; the 2-digit and
// row-scaled f16 forms would flush them), before anything reads its rows (no silent saturation).  fill embeds the rows into
// pf_x_: the layers overwrite them, so the repeat embeds again; no driver moves a position before this returns, so the repeat rewrites the
// same cache slots.  force_scaled_ is clear on every return path.
template <class Fill> int Decoder::forward_with_repeat(size_t N, int digits, const AttnOp &op, const Fill &fill) {
    struct Clear {
        bool &b;
        ~Clear() { b = false; }
    } clear{force_scaled_};
    PromptForm f;
    if (int rc = prompt_form(N, digits, false, &f)) return rc;
    (void)bitnet_hip_f16_saturations(1);  // a fresh count for this forward
    if (int rc = fill()) return rc;
    if (int rc = prompt_layers(N, f, op)) return rc;
    if (!f.f16_rows()) return 0;
    HCHK(hipStreamSynchronize((hipStream_t)stream_));
    if (bitnet_hip_f16_saturations(1) == 0) return 0;
    force_scaled_ = true;
    ++saturation_fallbacks_;
    if (int rc = prompt_form(N, 4, false, &f)) return rc;
    if (int rc = fill()) return rc;
    return prompt_layers(N, f, op);
}

// The span check of a prompt entry on one decoder: tokens [p, p + n) must have been fed and must fit the cache (T:1190-1194).  No p + n: a
// huge n must not wrap.  positive: a count below 1 reads as tokens nobody fed (score has a refusal of its own for it, after these two).
// -> the refusal's text, or null.
const char *Decoder::span_problem(int p, int n, bool positive) const {
    if ((positive && n <= 0) || n > host_forced_ - p) return "prefill: feed() the prompt tokens first";
    return overflow_problem(p, n);
}

const char *Decoder::overflow_problem(int p, int n) const { return n > c_.max_pos - 1 - p ? "KV cache overflow" : nullptr; }  // (step_wide: nothing to be fed)

// The member-set refusals of prefill_packed and step_wide, in their order, the text on the driver under the entry's name; also: a refusal of
// the entry's own (or null) that ranks between the count and the members.
int Decoder::check_members(Decoder *const *members, int n_members, int cap, const std::string &entry, const char *also) {
    Decoder &drv = *members[0];
    auto refuse = [&](const std::string &what) { return drv.fail_arg((entry + ": " + what).c_str()); };
    if (n_members < 1 || n_members > cap) return refuse("n_members must be 1.." + std::to_string(cap));
    if (also) return drv.fail_arg(also);
    for (int i = 0; i < n_members; ++i) {
        Decoder *d = members[i];
        if (!d) return refuse("null member");
        if (d->dead_) return refuse("dead member");
        for (int j = 0; j < i; ++j)
            if (members[j] == d) return refuse("a member is repeated");
        if (d->root() != drv.root()) return refuse("all members must run on the same weights (an owner and its borrowers)");
        if (d->kv_f16_ != drv.kv_f16_) return refuse("mixed KV cache types");
        if (!d->embed_) return drv.fail_arg("model globals not set");
    }
    return 0;
}

int Decoder::prefill(int n, bool with_logits, int digits, float *elapsed_ms) {
    if (!embed_) return fail_arg("model globals not set");
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (p != 0) return fail_arg("prefill needs a fresh sequence (position 0): reset() first");
    if (const char *e = span_problem(0, n)) return fail_arg(e);
    return prompt_forward(0, n, with_logits, digits, elapsed_ms);
}

int Decoder::extend(int n, bool with_logits, int digits, float *elapsed_ms) {
    if (!embed_) return fail_arg("model globals not set");
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (const char *e = span_problem(p, n)) return fail_arg(e);
    return prompt_forward(p, n, with_logits, digits, elapsed_ms);  // at p == 0 this IS prefill
}

int Decoder::rewind(int n) {
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (n < 0 || n > p) {
        err_ = "rewind: n must be in [0, position()]";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    // the cache bytes stay: the decode attention gives slots beyond the position zero weight, and the continuation operator takes every slot at
    // or beyond its past length from the new rows
    const int32_t np = n;
    HCHK(hipMemcpy(pos_, &np, 4, hipMemcpyHostToDevice));
    if (host_forced_ > n) host_forced_ = n;
    HCHK(hipMemcpy(n_forced_, &host_forced_, 4, hipMemcpyHostToDevice));
    return arm_stop(true);  // the stop and the window go (the tokens behind n are no longer the sequence's), the count stays
}

// The device pointer tables of fork and shift, allocated and filled once: this decoder's K caches [n_layers], its V caches [n_layers], then room for
// fork's destinations.
int Decoder::ensure_fork_tables() {
    if (fork_tables_) return 0;
    const size_t L = layers_.size(), M = BITNET_HIP_BATCH_MAX;
    std::vector<void *> t(2 * L, nullptr);
    HCHK(fork_tables_.alloc((2 + 2 * M) * L));
    for (size_t l = 0; l < L; ++l) t[l] = layers_[l].kcache, t[L + l] = layers_[l].vcache;
    if (hipError_t e = hipMemcpy(fork_tables_, t.data(), 2 * L * sizeof(void *), hipMemcpyHostToDevice)) {
        fork_tables_.reset();  // "built once": a table that is held is a table that is filled
        HCHK(e);
    }
    return 0;
}

int Decoder::shift_forced(int forced, int keep, int discard) { return forced <= keep ? forced : forced <= keep + discard ? keep : forced - discard; }

int Decoder::shift(int keep, int discard) {
    // every refusal comes before the first write
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (keep < 0) return fail_arg("shift: keep must be >= 0");
    if (discard < 1) return fail_arg("shift: discard must be >= 1");
    if (keep > p || discard > p - keep) return fail_arg("shift: keep + discard must be <= position()");
    if (int rc = ensure_fork_tables()) return rc;
    const size_t L = layers_.size(), n_hist = (size_t)c_.max_pos + 2;
    hipStream_t s = (hipStream_t)stream_;
    // the history first (a host round trip of at most 16 KB): a failure here leaves the caches as they were
    std::vector<int32_t> h(n_hist), nh(n_hist, 0);
    HCHK(hipMemcpy(h.data(), history_, n_hist * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < keep; ++i) nh[(size_t)i] = h[(size_t)i];
    // entries [keep + discard, max_pos) move down (entry p, the unconsumed picked or fed token, travels to p - discard); zero beyond
    for (int i = keep + discard; i < c_.max_pos; ++i) nh[(size_t)(i - discard)] = h[(size_t)i];
    BCHK(bitnet_hip_kv_shift_dev(fork_tables_, fork_tables_ + L, rope_sin_, rope_cos_, L, (size_t)c_.n_kv_heads, (size_t)c_.head_dim, (size_t)c_.max_pos,
                                 (size_t)keep, (size_t)discard, (size_t)p, kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, s));
    HCHK(hipMemcpyAsync(history_, nh.data(), n_hist * 4, hipMemcpyHostToDevice, s));
    if (lp_records_) {
        // record q > keep + discard becomes record q - discard, those in (keep, keep + discard] go, everything above the new last one is cleared
        const size_t rs = sizeof(bitnet_hip_logprob_record), first = (size_t)keep + (size_t)discard + 1, n_move = (size_t)p + 1 > first ? (size_t)p + 1 - first : 0;
        std::vector<uint8_t> recs(n_move * rs);
        HCHK(hipStreamSynchronize(s));
        if (n_move) {
            HCHK(hipMemcpy(recs.data(), lp_records_ + first, n_move * rs, hipMemcpyDeviceToHost));
            HCHK(hipMemcpy(lp_records_ + keep + 1, recs.data(), n_move * rs, hipMemcpyHostToDevice));
        }
        const size_t tail = (size_t)keep + 1 + n_move;  // = max(p - discard, keep) + 1
        if (tail < (size_t)c_.max_pos) HCHK(hipMemset(lp_records_ + tail, 0xff, ((size_t)c_.max_pos - tail) * rs));
    }
    HCHK(hipStreamSynchronize(s));
    // the position and the forced count go last: a HIP runtime error above returns with caches and history already moved under the OLD position,
    // a state only reset() leaves cleanly (as with any HIP error of this class: BITNET_HIP_ERR_GPU, error() names the call)
    const int32_t np = p - discard;
    HCHK(hipMemcpy(pos_, &np, 4, hipMemcpyHostToDevice));
    host_forced_ = shift_forced(host_forced_, keep, discard);
    HCHK(hipMemcpy(n_forced_, &host_forced_, 4, hipMemcpyHostToDevice));
    return arm_stop(true);  // as rewind: the stop and the window go, the count stays
}

int Decoder::fork(Decoder &src, Decoder *const *dsts, int n_dst, int n) { return src.fork_from_this(dsts, n_dst, n); }

const char *Decoder::fork_refusal(Decoder *const *dsts, int n_dst, const Decoder *src, const Decoder *root, bool kv_f16) {
    if (n_dst < 1 || n_dst > BITNET_HIP_BATCH_MAX) return "n_dst must be 1..8";
    if (!dsts) return "null destination";
    for (int i = 0; i < n_dst; ++i) {
        Decoder *d = dsts[i];
        if (!d) return "null destination";
        if (d->dead_) return "dead destination";
        if (d == src) return "a destination is the source itself: use rewind";
        for (int j = 0; j < i; ++j)
            if (dsts[j] == d) return "a destination is repeated";
        if (d->root() != root) return "source and destination must run on the same weights (an owner and its borrowers)";
        if (d->kv_f16_ != kv_f16) return "mixed KV cache types";
        if (d->batch_) return "a destination sits in a batch slot: leave the batch first";
    }
    return nullptr;
}

int Decoder::fork_arrive(Decoder *const *dsts, int n_dst, int n, int forced, const int32_t *hist, bool hist_on_device, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < n_dst; ++i) {
        // history[0 .. n]: entry n is the unconsumed picked or fed token, as rewind(n) leaves it; zero beyond, as after reset() + n steps
        HCHK(hipMemcpyAsync(dsts[i]->history_, hist, ((size_t)n + 1) * 4, hist_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        HCHK(hipMemsetAsync(dsts[i]->history_ + n + 1, 0, ((size_t)c_.max_pos + 1 - (size_t)n) * 4, s));
    }
    HCHK(hipStreamSynchronize(s));
    const int32_t np = n;
    for (int i = 0; i < n_dst; ++i) {
        Decoder *d = dsts[i];
        HCHK(hipMemcpy(d->pos_, &np, 4, hipMemcpyHostToDevice));
        d->host_forced_ = forced;
        HCHK(hipMemcpy(d->n_forced_, &forced, 4, hipMemcpyHostToDevice));
        if (d->sampler_) BCHK(bitnet_hip_sampler_reset(d->sampler_));
        // a destination's log-probabilities start at the fork point
        if (d->lp_top_n_ >= 0) HCHK(hipMemset(d->lp_records_, 0xff, (size_t)c_.max_pos * sizeof(bitnet_hip_logprob_record)));
        if (int rc = d->arm_stop(false)) return rc;  // a destination carries no stop state
    }
    return 0;
}

int Decoder::fork_from_this(Decoder *const *dsts, int n_dst, int n) {
    // every refusal comes before the first write
    if (const char *why = fork_refusal(dsts, n_dst, this, root(), kv_f16_)) return fail_arg((std::string("fork: ") + why).c_str());
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (n < 0 || n > p) return fail_arg("fork: n must be in [0, position()]");

    // one root, hence one Config: every cache has this decoder's geometry
    const size_t L = layers_.size(), M = BITNET_HIP_BATCH_MAX;
    std::vector<void *> t((2 + 2 * M) * L, nullptr);
    if (int rc = ensure_fork_tables()) return rc;
    void **dst_k = fork_tables_ + 2 * L, **dst_v = dst_k + M * L;
    hipStream_t s = (hipStream_t)stream_;
    if (n > 0) {
        for (int i = 0; i < n_dst; ++i)
            for (size_t l = 0; l < L; ++l) t[(2 + (size_t)i) * L + l] = dsts[i]->layers_[l].kcache, t[(2 + M + (size_t)i) * L + l] = dsts[i]->layers_[l].vcache;
        HCHK(hipMemcpy(dst_k, t.data() + 2 * L, 2 * M * L * sizeof(void *), hipMemcpyHostToDevice));
        BCHK(bitnet_hip_kv_fork_dev(fork_tables_, fork_tables_ + L, dst_k, dst_v, L, (size_t)n_dst, (size_t)c_.n_kv_heads, (size_t)c_.head_dim, (size_t)c_.max_pos,
                                    (size_t)n, kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, s));
    }
    return fork_arrive(dsts, n_dst, n, host_forced_ < n ? host_forced_ : n, history_, true, s);
}

int Decoder::cached_prefix(const int32_t *tokens, int n) {
    if (n < 0 || (n > 0 && !tokens)) {
        err_ = "cached_prefix: null tokens";
        return -1;
    }
    const int p = position();
    if (p < 0) return -1;
    const int m = n < p ? n : p;
    std::vector<int32_t> h((size_t)m);
    if (m > 0 && hipMemcpy(h.data(), history_, (size_t)m * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        err_ = "cached_prefix: history readback failed";
        return -1;
    }
    int i = 0;
    while (i < m && h[(size_t)i] == tokens[i]) ++i;
    return i;
}

// History tokens [p, p + n) through every layer as [n, *] matrices; p = the position (0: a fresh sequence and the whole-prompt attention;
// otherwise the continuation operator over the p cached positions).  The callers hold the guards.
int Decoder::prompt_forward(int p, int n, bool with_logits, int digits, float *elapsed_ms) {
    const size_t H = c_.hidden, N = (size_t)n;
    const size_t attn_need = p == 0 ? bitnet_hip_attention_prefill_workspace_bytes((size_t)c_.n_heads, (size_t)c_.n_kv_heads, N)
                                    : bitnet_hip_attention_extend_workspace_bytes((size_t)c_.n_heads, (size_t)c_.n_kv_heads, (size_t)p, N);
    if (int rc = ensure_prompt_buffers(n, attn_need)) return rc;
    hipStream_t s = (hipStream_t)stream_;
    StreamTimer timer;
    HCHK(timer.start(s));
    AttnOp op;
    op.kind = p == 0 ? AttnOp::Whole : AttnOp::Continue, op.past = (size_t)p;
    const auto fill = [&]() -> int {
        BCHK(bitnet_hip_embed_f16_dev(embed_, history_, pos_, N, H, (size_t)c_.vocab, pf_x_, s));  // rows history[*pos_ + i], *pos_ == p
        return 0;
    };
    if (int rc = forward_with_repeat(N, digits, op, fill)) return rc;  // (a repeated continuation rewrites only the new positions)
    if (int rc = finish_prefill(p + n, pf_x_ + (N - 1) * H, with_logits)) return rc;
    HCHK(timer.stop(s, elapsed_ms));
    return 0;
}

int Decoder::prefill_packed(Decoder *const *members, const int *n, int n_members, bool with_logits, int digits, float *elapsed_ms) {
    if (!members || !members[0] || members[0]->dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;  // no driver to carry the text
    Decoder &drv = *members[0];
    // every refusal comes before the first write
    if (int rc = check_members(members, n_members, BITNET_HIP_PACK_MAX, "prefill_packed", n ? nullptr : "prefill_packed: null lengths")) return rc;
    std::vector<int32_t> past((size_t)n_members), len((size_t)n_members);
    for (int i = 0; i < n_members; ++i) {
        Decoder *d = members[i];
        const int p = d->position();
        if (p < 0) {
            drv.err_ = d->err_;
            return BITNET_HIP_ERR_GPU;
        }
        if (n[i] < 1) return drv.fail_arg("prefill_packed: every member takes at least 1 token");
        if (const char *e = d->span_problem(p, n[i])) return drv.fail_arg(e);
        past[(size_t)i] = p, len[(size_t)i] = n[i];
    }
    return drv.packed_forward(members, past, len, with_logits, digits, elapsed_ms);
}

// The pack's rows: member i's n_i tokens from row row0_i on, row0 a multiple of the packed attention's row alignment; the rows between a member's
// last token and the next member's first are padding (the embeddings of the history entries that follow -- fed, picked or zero: valid tokens --
// so every matmul row is finite and of a token's scale; the attention neither reads nor caches them).  This decoder is the driver.
int Decoder::packed_forward(Decoder *const *members, const std::vector<int32_t> &past, const std::vector<int32_t> &len, bool with_logits, int digits,
                            float *elapsed_ms) {
    const size_t H = c_.hidden, NH = (size_t)c_.n_heads, NK = (size_t)c_.n_kv_heads, M = past.size();
    const size_t align = bitnet_hip_attention_packed_row_align(NH, NK);
    if (align == 0) return fail_arg("prefill_packed: head counts out of range");
    std::vector<int32_t> row0(M);
    size_t N = 0;
    for (size_t i = 0; i < M; ++i) {
        row0[i] = (int32_t)((N + align - 1) / align * align);
        N = (size_t)row0[i] + (size_t)len[i];
    }
    const size_t attn_need = bitnet_hip_attention_packed_workspace_bytes(NH, NK, N, M, past.data(), len.data());
    if (attn_need == 0) return fail_arg("prefill_packed: sizes out of range");
    if (int rc = ensure_prompt_buffers((int)N, attn_need)) return rc;
    hipStream_t s = (hipStream_t)stream_;
    StreamTimer timer;
    HCHK(timer.start(s));
    const auto fill = [&]() -> int {
        for (size_t i = 0; i < M; ++i) {
            Decoder *d = members[i];
            // rows history[p + r]: the member's tokens, then (up to the next member's first row) what follows them in its history, as far as the history goes
            const size_t want = i + 1 < M ? (size_t)row0[i + 1] - (size_t)row0[i] : (size_t)len[i], have = (size_t)c_.max_pos + 2 - (size_t)past[i];
            const size_t rows = want < have ? want : have;
            float *dst = pf_x_ + (size_t)row0[i] * H;
            BCHK(bitnet_hip_embed_f16_dev(d->embed_, d->history_, d->pos_, rows, H, (size_t)c_.vocab, dst, s));
            for (size_t r = rows; r < want; ++r)  // (a member within a tile of the cache's end: its last token again)
                HCHK(hipMemcpyAsync(dst + r * H, dst + ((size_t)len[i] - 1) * H, H * 4, hipMemcpyDeviceToDevice, s));
        }
        return 0;
    };
    AttnOp op;  // (its pointers are this frame's vectors: they outlive both attempts)
    op.kind = AttnOp::Pack, op.members = members, op.n = M, op.row0 = row0.data(), op.len = len.data(), op.pasts = past.data();
    if (int rc = forward_with_repeat(N, digits, op, fill)) return rc;
    // the hand-over: every member's own head, pick and log-probability record on its own stream, from its last token's row
    HCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < M; ++i) {
        Decoder *d = members[i];
        const int rc = d->finish_prefill(past[i] + len[i], pf_x_ + ((size_t)row0[i] + (size_t)len[i] - 1) * H, with_logits);
        if (rc) {
            if (d != this) err_ = d->err_;
            return rc;
        }
    }
    HCHK(timer.stop(s, elapsed_ms));
    return 0;
}

int Decoder::step_wide(Decoder *const *members, int n_members, int n_steps, int digits, float *elapsed_ms) {
    if (!members || !members[0] || members[0]->dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;  // no driver to carry the text
    Decoder &drv = *members[0];
    // every refusal comes before the first write
    if (int rc = check_members(members, n_members, BITNET_HIP_WIDE_MAX, "step_wide", n_steps < 1 ? "step_wide: n_steps must be at least 1" : nullptr)) return rc;
    int max_p = 0;
    for (int i = 0; i < n_members; ++i) {
        Decoder *d = members[i];
        const int p = d->position();
        if (p < 0) {
            drv.err_ = d->err_;
            return BITNET_HIP_ERR_GPU;
        }
        if (const char *e = d->overflow_problem(p, n_steps)) return drv.fail_arg(e);
        max_p = p > max_p ? p : max_p;
    }
    return drv.wide_forward(members, n_members, n_steps, max_p, digits, elapsed_ms);
}

// The wide step's chain, n_steps times: gather, layers under the rows attention (with the saturation rule: forward_with_repeat), head,
// hand-over, then the samplers and logits taps member by member.  This decoder is the driver; max_p = the largest position before the call.
int Decoder::wide_forward(Decoder *const *members, int M, int n_steps, int max_p, int digits, float *elapsed_ms, WideTail *tail) {
    const size_t H = c_.hidden, V = (size_t)c_.vocab, NL = layers_.size(), W = BITNET_HIP_WIDE_MAX;
    hipStream_t s = (hipStream_t)stream_;
    const size_t ws_need = bitnet_hip_score_workspace_bytes((size_t)M, H, V);
    if (ws_need == 0) return fail_arg("step_wide: dimensions too large");
    if (!tail && !wide_tables_) HCHK(wide_tables_.alloc((2 * NL + 6) * W));
    if (M > wide_cap_ || ws_need > wide_ws_bytes_) {
        const size_t cap = (size_t)(M > wide_cap_ ? M : wide_cap_), sb = bitnet_hip_attention_scratch_bytes((size_t)c_.n_kv_heads, (size_t)c_.max_pos);
        release_all(wide_scratch_, wide_logits_, wide_nll_, wide_am_, wide_tgt_, wide_ws_);
        wide_cap_ = 0, wide_ws_bytes_ = 0;
        const size_t wb = bitnet_hip_score_workspace_bytes(cap, H, V);
        HCHK(wide_scratch_.alloc_bytes(cap * sb));
        HCHK(hipMemsetAsync(wide_scratch_, 0, cap * sb, s));  // the combine requests records past the context (and drops them by index): valid, finite memory
        HCHK(wide_logits_.alloc(cap * V));
        HCHK(wide_nll_.alloc(cap));
        HCHK(wide_am_.alloc(cap));
        HCHK(wide_tgt_.alloc(cap));
        HCHK(hipMemsetAsync(wide_tgt_, 0xff, cap * 4, s));  // target -1: no NLL, the head leaves logits and argmax
        HCHK(wide_ws_.alloc(wb));
        wide_cap_ = (int)cap, wide_ws_bytes_ = wb;
    }
    if (int rc = ensure_prompt_buffers(M, 16)) return rc;
    // the pointer tables, uploaded once per call: [2 l] / [2 l + 1] layer l's K / V caches, then position, history, forced count, logits row and
    // the pick's token / position entries (NULL for a member that samples: its sampler does the hand-over); a tail brings its own, uploaded
    if (!tail) {
        std::vector<void *> t((2 * NL + 6) * W, nullptr);
        for (int i = 0; i < M; ++i) {
            Decoder *d = members[i];
            for (size_t l = 0; l < NL; ++l) t[(2 * l) * W + i] = d->layers_[l].kcache, t[(2 * l + 1) * W + i] = d->layers_[l].vcache;
            void **g = t.data() + 2 * NL * W;
            if (d->refresh_logits()) return fail("step_wide: refresh_logits");  // the pick writes this row from now on
            g[0 * W + i] = d->pos_, g[1 * W + i] = d->history_, g[2 * W + i] = d->n_forced_, g[3 * W + i] = d->logits_;
            g[4 * W + i] = d->sampling_ ? nullptr : d->token_.get(), g[5 * W + i] = d->sampling_ ? nullptr : d->pos_.get();
        }
        HCHK(hipMemcpy(wide_tables_, t.data(), t.size() * sizeof(void *), hipMemcpyHostToDevice));
    }
    void *const *const tables = tail ? tail->tables : wide_tables_.get();
    void *const *g = tables + 2 * NL * W;
    const int32_t *const *pos_t = reinterpret_cast<const int32_t *const *>(g), *const *hist_t = reinterpret_cast<const int32_t *const *>(g + W);
    StreamTimer timer;
    HCHK(timer.start(s));
    const auto fill = [&]() -> int {
        BCHK(bitnet_hip_embed_rows_dev(embed_, hist_t, pos_t, (size_t)M, H, V, pf_x_, s));
        return 0;
    };
    for (int step = 0; step < n_steps; ++step) {
        AttnOp op;  // (the positions move only in the pick below, so a repeated step rewrites the same cache slots)
        op.kind = AttnOp::Rows, op.n = (size_t)M, op.key_bound = (size_t)(max_p + step + 1), op.tables = tables, op.kv_f16 = members[0]->kv_f16_;
        if (int rc = forward_with_repeat((size_t)M, digits, op, fill)) return rc;
        BCHK(bitnet_hip_score_f16_dev(embed_, pf_x_, final_norm_, c_.eps, H, V, (size_t)M, wide_tgt_, wide_nll_, wide_am_, wide_logits_, (size_t)M, wide_ws_,
                                      wide_ws_bytes_, s));
        BCHK(bitnet_hip_pick_rows_dev(wide_logits_, wide_am_, (size_t)M, V, reinterpret_cast<float *const *>(g + 3 * W), reinterpret_cast<int32_t *const *>(g + 4 * W),
                                      reinterpret_cast<int32_t *const *>(g + 5 * W), reinterpret_cast<int32_t *const *>(g + W),
                                      reinterpret_cast<const int32_t *const *>(g + 2 * W), s));
        if (tail) {  // a WideBatch's tail: every sampling member, every tap, every member with criteria -- one launch each, or none
            if (tail->sample) {
                if (bitnet_hip_sample_batch_dev(tail->sample, s) != 0) return fail("wide batch: bitnet_hip_sample_batch_dev");
                ++tail->launches[0];
            }
            if (tail->taps) {
                if (bitnet_hip_logprob_rows_dev(tail->taps, tail->n_taps, V, s) != 0) return fail("wide batch: bitnet_hip_logprob_rows_dev");
                ++tail->launches[1];
            }
            if (tail->stop) {
                if (bitnet_hip_stop_batch_dev(tail->stop, s) != 0) return fail("wide batch: bitnet_hip_stop_batch_dev");
                ++tail->launches[2];
            }
            continue;
        }
        for (int i = 0; i < M; ++i) {  // pick_token's arrangement, on the driver's stream: the member's own sampler, then its own record
            Decoder *d = members[i];
            if (d->sampling_) {
                if (bitnet_hip_sample_dev(d->sampler_, d->logits_, V, d->token_, d->pos_, d->history_, d->n_forced_, s) != 0) return fail("step_wide: bitnet_hip_sample_dev");
            }
            if (d->lp_top_n_ >= 0) {
                bitnet_hip_logprob_args a;
                d->logprob_entry(&a);
                if (bitnet_hip_logprob_dev(&a, V, s) != 0) return fail("step_wide: bitnet_hip_logprob_dev");
            }
        }
        for (int i = 0; i < M; ++i) {  // the members' stop criteria, behind every sampler and tap launch of the step
            Decoder *d = members[i];
            if (d->stop_on_ && bitnet_hip_stop_dev(d->stop_, d->pos_, d->history_, (size_t)c_.max_pos, d->n_forced_, d->token_, s) != 0)
                return fail("step_wide: bitnet_hip_stop_dev");
        }
    }
    HCHK(timer.stop(s, elapsed_ms));
    return 0;
}

// The per-row buffers of a prompt forward of n rows and its attention workspace, grown on demand.
int Decoder::ensure_prompt_buffers(int n, size_t attn_need) {
    const size_t H = c_.hidden, QD = (size_t)c_.n_heads * c_.head_dim, KD = (size_t)c_.n_kv_heads * c_.head_dim, F = c_.ffn;
    if (n > pf_cap_ || attn_need > pf_attn_ws_bytes_) {
        const size_t N = (size_t)(n > pf_cap_ ? n : pf_cap_);  // the row buffers never shrink: a short turn at a long context keeps the prompt's
        const size_t attn_bytes = attn_need > pf_attn_ws_bytes_ ? attn_need : pf_attn_ws_bytes_;
        release_all(pf_x_, pf_qkv_, pf_att_, pf_h_, pf_gemm_ws_, pf_attn_ws_);
        pf_cap_ = 0;
        pf_attn_ws_bytes_ = 0;
        pf_gemm_ws_bytes_ = bitnet_hip_matmul_workspace_bytes(N, H > F ? H : F, 4);
        pf_attn_ws_bytes_ = attn_bytes;
        HCHK(pf_x_.alloc(N * H));
        HCHK(pf_qkv_.alloc(N * (QD + 2 * KD)));
        HCHK(pf_att_.alloc(N * QD));
        HCHK(pf_h_.alloc(N * F));
        HCHK(pf_gemm_ws_.alloc(pf_gemm_ws_bytes_));
        HCHK(pf_attn_ws_.alloc(pf_attn_ws_bytes_));
        pf_cap_ = (int)N;
    }
    return 0;
}

int Decoder::prefill_sharded(int n, int rank, int world, bitnet_host_allgather_fn gather, void *gather_ctx, bool with_logits, int digits,
                             bool wire_f16, float *elapsed_ms) {
    if (!embed_) return fail_arg("model globals not set");
    if (sampling_) {
        err_ = "prefill_sharded: not available with sampling on (set_sampling(NULL) first)";
        return BITNET_HIP_ERR_UNSUPPORTED;
    }
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !gather)) return fail_arg("prefill_sharded: bad rank / world / gather");
    if (n <= 0 || n % (2 * world * 64) != 0) {
        char b[128];
        snprintf(b, sizeof(b), "prompt length %d must be a positive multiple of %d (2 * world * 64) for world %d", n, 2 * world * 64, world);
        return fail_arg(b);
    }
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (p != 0) return fail_arg("prefill needs a fresh sequence (position 0): reset() first");
    if (const char *e = span_problem(0, n)) return fail_arg(e);
    const size_t H = c_.hidden, QD = (size_t)c_.n_heads * c_.head_dim, KD = (size_t)c_.n_kv_heads * c_.head_dim;
    const size_t NH = (size_t)c_.n_heads, NK = (size_t)c_.n_kv_heads, D = (size_t)c_.head_dim, MP = (size_t)c_.max_pos;
    const int chunk = n / (2 * world), nq = 2 * chunk;
    const size_t N = (size_t)nq, esz = wire_f16 ? 2 : 4;
    // the per-row buffers of the unsharded prefill, sized for this rank's rows, and the form's own: all growth before the first launch
    if (int rc = ensure_prompt_buffers(nq, bitnet_hip_attention_prefill_sharded_workspace_bytes(NH, NK, N, (size_t)n))) return rc;
    PromptForm f;
    if (int rc = prompt_form(N, digits, true, &f)) return rc;
    if (nq > sp_cap_ || n > sp_ctx_) {
        release_all(sp_kv_send_, sp_kv_all_, sp_block_pos_, sp_tokens_);
        sp_cap_ = sp_ctx_ = 0;
        HCHK(sp_kv_send_.alloc(N * 2 * KD * 4));
        HCHK(sp_kv_all_.alloc((size_t)n * 2 * KD * 4));
        HCHK(sp_block_pos_.alloc(N / 64));
        HCHK(sp_tokens_.alloc(N));
        sp_cap_ = nq;
        sp_ctx_ = n;
    }
    hipStream_t s = (hipStream_t)stream_;
    if (world > 1 && !comm_stream_) {  // the collective's own stream + the two events that tie it to the compute stream
        // all three or none: a later call must never find the stream set and an event missing
        hipStream_t cs = nullptr;
        hipEvent_t e1 = nullptr, e2 = nullptr;
        hipError_t er = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        if (er == hipSuccess) er = hipEventCreateWithFlags(&e1, hipEventDisableTiming);
        if (er == hipSuccess) er = hipEventCreateWithFlags(&e2, hipEventDisableTiming);
        if (er != hipSuccess) {
            if (e2) (void)hipEventDestroy(e2);
            if (e1) (void)hipEventDestroy(e1);
            if (cs) (void)hipStreamDestroy(cs);
            HCHK(er);
        }
        comm_stream_ = cs;
        sp_ev_pack_ = e1;
        sp_ev_gather_ = e2;
    }
    {
        // this rank's rows: chunk `rank`, then chunk 2 world - 1 - rank
        std::vector<int32_t> hist((size_t)n), tok(N), bp(N / 64);
        HCHK(hipMemcpy(hist.data(), history_, (size_t)n * 4, hipMemcpyDeviceToHost));
        const int starts[2] = {rank * chunk, (2 * world - 1 - rank) * chunk};
        for (int h = 0; h < 2; ++h)
            for (int i = 0; i < chunk; ++i) {
                tok[(size_t)h * chunk + i] = hist[(size_t)starts[h] + i];
                if (i % 64 == 0) bp[((size_t)h * chunk + i) / 64] = starts[h] + i;
            }
        HCHK(hipMemcpy(sp_tokens_, tok.data(), N * 4, hipMemcpyHostToDevice));
        HCHK(hipMemcpy(sp_block_pos_, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
    }
    // optional per-phase timing: 8 events per layer (6 on the compute stream, 2 around the collective on its own stream)
    const bool timing = sp_timing_;
    if (timing && sp_tev_.size() < layers_.size() * 8) {
        const size_t want = layers_.size() * 8;
        while (sp_tev_.size() < want) {
            hipEvent_t e = nullptr;
            HCHK(hipEventCreate(&e));
            sp_tev_.push_back(e);
        }
    }
    size_t li = 0;
    auto mark = [&](int idx, hipStream_t st) -> hipError_t { return timing ? hipEventRecord((hipEvent_t)sp_tev_[li * 8 + (size_t)idx], st) : hipSuccess; };
    StreamTimer timer;
    HCHK(timer.start(s));
    BCHK(bitnet_hip_embed_f16_dev(embed_, sp_tokens_, nullptr, N, H, (size_t)c_.vocab, pf_x_, s));
    const size_t ld = QD + 2 * KD, per_rank = N * 2 * KD * esz;
    // (f.h16: f16 hand-over of the attention output and of silu * up; f.hybrid: o / down on the f16 matrix cores -- long shares only)
    float *att_out = f.h16 ? static_cast<float *>(pf_atth_.get()) : pf_att_;
    const int aflags = (kv_f16_ ? BITNET_HIP_ATTN_CACHE_F16 : 0) | (f.h16 ? BITNET_HIP_ATTN_OUT_F16 : 0);
    // its own loop: the attention has two phases around the collective, and the timing marks sit between the launches
    for (size_t l = 0; l < layers_.size(); ++l) {
        Layer &L = layers_[l];
        HCHK(mark(0, s));
        if (int rc = project_qkv(l, N, f)) return rc;
        // the raw (pre-RoPE) k|v rows this rank contributes, compact, f32 or f16
        BCHK(bitnet_hip_pack_cols_dev(pf_qkv_, ld, QD, 2 * KD, N, world > 1 ? sp_kv_send_ : sp_kv_all_, wire_f16 ? 1 : 0, s));
        HCHK(mark(1, s));
        if (world > 1) {
            // the collective runs on its own stream beside the query-side preparation (RoPE + f16 pack of this rank's q rows);
            // the k / v slabs and the attention follow once it has finished
            HCHK(hipEventRecord((hipEvent_t)sp_ev_pack_, s));
            HCHK(hipStreamWaitEvent((hipStream_t)comm_stream_, (hipEvent_t)sp_ev_pack_, 0));
            HCHK(mark(6, (hipStream_t)comm_stream_));
            if (gather(gather_ctx, sp_kv_send_, sp_kv_all_, per_rank, comm_stream_) != 0) {
                err_ = "prefill_sharded: the all-gather callback failed";
                return BITNET_HIP_ERR_EXECUTION;
            }
            HCHK(mark(7, (hipStream_t)comm_stream_));
            HCHK(hipEventRecord((hipEvent_t)sp_ev_gather_, (hipStream_t)comm_stream_));
            BCHK(bitnet_hip_attention_prefill_gathered_phase_dev(pf_qkv_, ld, sp_block_pos_, N, sp_kv_all_, (size_t)n, (size_t)world, wire_f16 ? 1 : 0, rope_sin_,
                                                                 rope_cos_, L.kcache, L.vcache, aflags, NH, NK, D, MP, pf_attn_ws_, pf_attn_ws_bytes_, att_out, 1, s));
            HCHK(mark(2, s));
            HCHK(hipStreamWaitEvent(s, (hipEvent_t)sp_ev_gather_, 0));
            HCHK(mark(3, s));
        } else {
            HCHK(mark(2, s));
            HCHK(mark(3, s));
            HCHK(mark(6, s));
            HCHK(mark(7, s));
        }
        BCHK(bitnet_hip_attention_prefill_gathered_phase_dev(pf_qkv_, ld, sp_block_pos_, N, sp_kv_all_, (size_t)n, (size_t)world, wire_f16 ? 1 : 0, rope_sin_,
                                                             rope_cos_, L.kcache, L.vcache, aflags, NH, NK, D, MP, pf_attn_ws_, pf_attn_ws_bytes_, att_out,
                                                             world > 1 ? 2 : 0, s));
        HCHK(mark(4, s));
        if (int rc = project_o(L, N, f)) return rc;
        if (int rc = project_gateup(L, N, f)) return rc;
        if (int rc = project_down(L, N, f, nullptr)) return rc;  // (no chain here: nothing is handed to the next layer)
        HCHK(mark(5, s));
        ++li;
    }
    {
        // The last prompt position sits in chunk 2 world - 1 = rank 0's second chunk: its last local row.  EVERY rank gets that row
        // (one more gather of `hidden` floats per rank through the same callback and stream ties: slot 0 is rank 0's), so any rank can
        // continue decoding -- with logits and the first sampled token -- on the cache it filled.
        const float *last = pf_x_ + (N - 1) * H;
        if (world > 1) {
            HCHK(hipMemcpyAsync(sp_kv_send_, last, H * 4, hipMemcpyDeviceToDevice, s));
            HCHK(hipEventRecord((hipEvent_t)sp_ev_pack_, s));
            HCHK(hipStreamWaitEvent((hipStream_t)comm_stream_, (hipEvent_t)sp_ev_pack_, 0));
            if (gather(gather_ctx, sp_kv_send_, sp_kv_all_, H * 4, comm_stream_) != 0) {
                err_ = "prefill_sharded: the all-gather callback failed (last row)";
                return BITNET_HIP_ERR_EXECUTION;
            }
            HCHK(hipEventRecord((hipEvent_t)sp_ev_gather_, (hipStream_t)comm_stream_));
            HCHK(hipStreamWaitEvent(s, (hipEvent_t)sp_ev_gather_, 0));
            last = static_cast<const float *>(sp_kv_all_.get());
        }
        const int rc = finish_prefill(n, last, with_logits);
        if (rc) return rc;
    }
    HCHK(timer.stop(s, elapsed_ms));
    if (timing) {
        if (comm_stream_) HCHK(hipStreamSynchronize((hipStream_t)comm_stream_));
        std::vector<float> ph[4];
        for (size_t l = 0; l < layers_.size(); ++l) {
            auto dt = [&](int a, int b) {
                float t = 0.f;
                (void)hipEventElapsedTime(&t, (hipEvent_t)sp_tev_[l * 8 + (size_t)a], (hipEvent_t)sp_tev_[l * 8 + (size_t)b]);
                return t * 1e3f;
            };
            ph[0].push_back(dt(0, 1) + dt(4, 5));
            ph[1].push_back(dt(1, 2) + dt(3, 4));
            ph[2].push_back(dt(2, 3));
            ph[3].push_back(dt(6, 7));
        }
        for (int i = 0; i < 4; ++i) {
            std::sort(ph[i].begin(), ph[i].end());
            sp_phase_us_[i] = ph[i].empty() ? 0.f : ph[i][ph[i].size() / 2];
        }
    }
    return 0;
}

int Decoder::score(int n, int digits, float *nll_out, int32_t *argmax_out, float *logits_out, int logits_rows, float *elapsed_ms) {
    if (!embed_) return fail_arg("model globals not set");
    if (!nll_out || (logits_rows > 0 && !logits_out)) return fail_arg("score: null pointer");
    if (const char *e = span_problem(0, n, false)) return fail_arg(e);  // (the position itself is prefill's to check, below)
    if (n < 2) return fail_arg("score: n must be >= 2 (row r is scored against token r + 1)");
    if (logits_rows < 0 || logits_rows > n) return fail_arg("score: logits_rows must be in [0, n]");
    const size_t H = c_.hidden, V = (size_t)c_.vocab, N = (size_t)n;
    const size_t need = bitnet_hip_score_workspace_bytes(N, H, V);
    if (need == 0) return fail_arg("score: dimensions too large");
    if (n > sc_cap_ || need > sc_ws_bytes_) {
        release_all(sc_tgt_, sc_am_, sc_nll_, sc_ws_);
        sc_cap_ = 0;
        sc_ws_bytes_ = 0;
        HCHK(sc_tgt_.alloc(N));
        HCHK(sc_am_.alloc(N));
        HCHK(sc_nll_.alloc(N));
        HCHK(sc_ws_.alloc(need));
        sc_cap_ = n;
        sc_ws_bytes_ = need;
    }
    if (logits_rows > sc_logits_cap_) {
        release_all(sc_logits_);
        sc_logits_cap_ = 0;
        HCHK(sc_logits_.alloc((size_t)logits_rows * V));
        sc_logits_cap_ = logits_rows;
    }
    hipStream_t s = (hipStream_t)stream_;
    StreamTimer timer;
    HCHK(timer.start(s));
    if (int rc = prefill(n, true, digits, nullptr)) return rc;
    // row r predicts token r + 1 of the history (the prompt); the last row has no target
    HCHK(hipMemcpyAsync(sc_tgt_, history_ + 1, (N - 1) * 4, hipMemcpyDeviceToDevice, s));
    HCHK(hipMemsetAsync(sc_tgt_ + (N - 1), 0xff, 4, s));
    BCHK(bitnet_hip_score_f16_dev(embed_, pf_x_, final_norm_, c_.eps, H, V, N, sc_tgt_, sc_nll_, argmax_out ? sc_am_.get() : nullptr,
                                  logits_rows > 0 ? sc_logits_.get() : nullptr, (size_t)logits_rows, sc_ws_, sc_ws_bytes_, s));
    HCHK(timer.stop(s, elapsed_ms));
    HCHK(hipMemcpy(nll_out, sc_nll_, (N - 1) * 4, hipMemcpyDeviceToHost));
    if (argmax_out) HCHK(hipMemcpy(argmax_out, sc_am_, N * 4, hipMemcpyDeviceToHost));
    if (logits_rows > 0) HCHK(hipMemcpy(logits_out, sc_logits_, (size_t)logits_rows * V * 4, hipMemcpyDeviceToHost));
    return 0;
}

int Decoder::finish_prefill(int n, const float *last_row, bool with_logits) {
    // hand over to the single-token state: residual stream of the last position, position counter
    if (n <= 0 || n > c_.max_pos - 1) {
        err_ = "KV cache overflow";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream_;
    const size_t H = c_.hidden;
    if (last_row) HCHK(hipMemcpyAsync(x_, last_row, H * 4, hipMemcpyDeviceToDevice, s));
    const int32_t last = n - 1;
    HCHK(hipMemcpyAsync(pos_, &last, 4, hipMemcpyHostToDevice, s));
    HCHK(hipStreamSynchronize(s));  // `last` is a stack variable
    if (with_logits && last_row) {
        if (int rc = pick_token(s)) return rc;
        picked(pick_screened_);
    } else {
        BCHK(bitnet_hip_advance_pos_dev(pos_, s));
    }
    HCHK(hipStreamSynchronize(s));
    return 0;
}

void Decoder::layer_objects(int layer, uint64_t handles[4], void *ptrs[4]) const {
    if (layer < 0 || (size_t)layer >= layers_.size()) {
        for (int i = 0; i < 4; ++i) handles[i] = 0, ptrs[i] = nullptr;
        return;
    }
    const Layer &L = layers_[(size_t)layer];
    handles[0] = L.qkv, handles[1] = L.o, handles[2] = L.gateup, handles[3] = L.down;
    ptrs[0] = L.attn_norm, ptrs[1] = L.ffn_norm, ptrs[2] = L.kcache, ptrs[3] = L.vcache;
}

void Decoder::global_objects(void *ptrs[7]) const {
    ptrs[0] = embed_, ptrs[1] = final_norm_, ptrs[2] = rope_sin_, ptrs[3] = rope_cos_, ptrs[4] = history_, ptrs[5] = pos_, ptrs[6] = stream_;
}

int Decoder::history(int32_t *out, int n) {
    if (!out || n < 0 || n > c_.max_pos + 2) {
        err_ = "history: n out of range";
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    HCHK(hipMemcpy(out, history_, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}
int Decoder::last_logits(float *out) {
    if (int rc = refresh_logits()) return rc;  // after a screened step: the full head once, on the head input that step saved
    HCHK(hipMemcpy(out, logits_, (size_t)c_.vocab * 4, hipMemcpyDeviceToHost));
    return 0;
}
int Decoder::last_hidden(float *out) {
    HCHK(hipMemcpy(out, x_, (size_t)c_.hidden * 4, hipMemcpyDeviceToHost));
    return 0;
}

// kind: 0 q|k|v, 1 attention, 2 o_proj, 3 gate|up, 4 down, 5 logits+argmax
int Decoder::probe_kernel(int kind, int reps, float *us_per_launch, double *bytes_per_launch) {
    hipStream_t s = (hipStream_t)stream_;
    const int p0 = position();
    hipGraph_t g = nullptr;
    HCHK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    int rc = 0;
    const size_t H = c_.hidden;
    int launches = 0;
    const bool qp = qact_path();
    for (size_t li = 0; li < layers_.size(); ++li) {
        Layer &L = layers_[li];
        if (qp && kind <= 4) {
            const bool more = li + 1 < layers_.size();
            switch (kind) {
                case 0: rc = bitnet_hip_gemv_q_dev(L.qkv, qa_x_, st_x_, L.attn_norm, c_.eps, nullptr, 0, qkv_, nullptr, nullptr, nullptr, stream_); break;
                case 1: rc = attn_launch(L, form_at(p0 > 0 ? p0 : 0) == 2 ? 2 : 0, nullptr, qa_att_); break;
                case 2: rc = bitnet_hip_gemv_q_dev(L.o, qa_att_, nullptr, nullptr, 0.f, x_, 0, x2_, qa_x2_, L.ffn_norm, st_x2_, stream_); break;
                case 3: rc = bitnet_hip_gemv_q_dev(L.gateup, qa_x2_, st_x2_, L.ffn_norm, c_.eps, nullptr, BITNET_HIP_FUSE_SILU_MUL, nullptr, qa_h_, nullptr, nullptr, stream_); break;
                default:
                    // x_ is both the residual stream's next value and (kind 2) its old one in the real step; here it is only written
                    rc = bitnet_hip_gemv_q_dev(L.down, qa_h_, nullptr, nullptr, 0.f, x2_, 0, ref_t_, more ? qa_x_.get() : nullptr, more ? layers_[li + 1].attn_norm.get() : nullptr,
                                               more ? st_x_.get() : nullptr, stream_);
                    break;
            }
            ++launches;
            if (rc) break;
            continue;
        }
        switch (kind) {
            case 0: rc = bitnet_hip_gemv_fused_dev(L.qkv, x_, qkv_, 1, L.attn_norm, c_.eps, nullptr, 0, stream_); break;
            case 1: rc = attn_launch(L, form_at(p0 > 0 ? p0 : 0) == 2 ? 2 : 0, att_, nullptr); break;
            case 2: rc = bitnet_hip_gemv_fused_dev(L.o, att_, x2_, 1, nullptr, 0.f, x_, 0, stream_); break;
            case 3: rc = bitnet_hip_gemv_fused_dev(L.gateup, x2_, h_, 1, L.ffn_norm, c_.eps, nullptr, BITNET_HIP_FUSE_SILU_MUL, stream_); break;
            case 4: rc = bitnet_hip_gemv_fused_dev(L.down, h_, x_, 1, nullptr, 0.f, x2_, 0, stream_); break;
            default:  // the head form a plain step runs now
                if (screen_step(false))
                    rc = bitnet_hip_logits_screen_dev(embed_, x_, final_norm_, c_.eps, H, (size_t)c_.vocab, screen_, screen_ws_, scratch_, (size_t)screen_wgs_,
                                                      token_, nullptr, nullptr, nullptr, stream_);
                else
                    rc = bitnet_hip_logits_f16_dev(embed_, x_, final_norm_, c_.eps, H, (size_t)c_.vocab, logits_, scratch_,
                                                   (size_t)logits_wgs_, token_, nullptr, nullptr, nullptr, stream_);
                break;
        }
        ++launches;
        if (rc || kind > 4) break;
    }
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc) {
        if (g) hipGraphDestroy(g);
        return fail("probe_kernel launch");
    }
    HCHK(e);
    hipGraphExec_t ex = nullptr;
    HCHK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    HCHK(hipGraphLaunch(ex, s));  // warm
    HCHK(hipStreamSynchronize(s));
    StreamTimer timer;
    HCHK(timer.start(s));
    for (int i = 0; i < reps; ++i) HCHK(hipGraphLaunch(ex, s));
    float ms = 0.f;
    HCHK(timer.stop(s, &ms));
    hipGraphExecDestroy(ex);
    hipGraphDestroy(g);
    (void)p0;
    if (kind > 4) picked(screen_step(false));  // the head ran on x_ as it stands: logits_ is that head's, at once or on demand
    if (us_per_launch) *us_per_launch = ms * 1e3f / (float)(reps * launches);
    if (bytes_per_launch) {
        size_t ab = 0;
        const Layer &L = layers_[0];
        const double kv = 2.0 * c_.n_kv_heads * (double)(position() + 1) * c_.head_dim * (kv_f16_ ? 2 : 4);
        if (qp && kind <= 4 && kind != 1) {
            // QAct path: codes + scales + the activation records read (+ statistics pairs) + what the launch writes
            const double qH = (double)bitnet_hip_qact_bytes(H), qF = (double)bitnet_hip_qact_bytes((size_t)c_.ffn), sH = (double)bitnet_hip_qact_stats_bytes(H);
            const bitnet_hip_weights_t hh = kind == 0 ? L.qkv : kind == 2 ? L.o : kind == 3 ? L.gateup : L.down;
            bitnet_hip_weights_info(hh, nullptr, nullptr, &ab);
            const double io = kind == 0 ? qH + sH + 4.0 * H + 4.0 * (c_.n_heads + 2 * c_.n_kv_heads) * c_.head_dim   // + g_r
                            : kind == 2 ? (double)bitnet_hip_qact_bytes((size_t)c_.n_heads * c_.head_dim) + 12.0 * H + qH + sH  // residual in, f32 out, gamma, QAct + stats out
                            : kind == 3 ? qH + sH + 8.0 * c_.ffn + qF                                                 // g_r of both halves, QAct out
                                        : qF + 12.0 * H + qH + sH;
            *bytes_per_launch = (double)ab + io;
            return 0;
        }
        switch (kind) {  // algorithmic bytes of one launch: codes + scales + vector in + vector out
            case 0: bitnet_hip_weights_info(L.qkv, nullptr, nullptr, &ab); *bytes_per_launch = (double)ab + 8.0 * H + 4.0 * (c_.n_heads + 2 * c_.n_kv_heads) * c_.head_dim; break;
            case 1: *bytes_per_launch = kv + 8.0 * c_.n_heads * c_.head_dim; break;
            case 2: bitnet_hip_weights_info(L.o, nullptr, nullptr, &ab); *bytes_per_launch = (double)ab + 4.0 * c_.n_heads * c_.head_dim + 8.0 * H; break;
            case 3: bitnet_hip_weights_info(L.gateup, nullptr, nullptr, &ab); *bytes_per_launch = (double)ab + 8.0 * H + 4.0 * c_.ffn; break;
            case 4: bitnet_hip_weights_info(L.down, nullptr, nullptr, &ab); *bytes_per_launch = (double)ab + 4.0 * c_.ffn + 8.0 * H; break;
            default:
                if (screen_step(false)) {
                    // the int8 image + ub written and read + the rows the last launch rescored + x and gamma
                    uint32_t st[3] = {0, 0, 0};
                    if (int rc2 = head_screen_stats(st)) return rc2;
                    *bytes_per_launch = (double)bitnet_hip_head_screen_bytes(H, (size_t)c_.vocab) + 8.0 * c_.vocab + 2.0 * (double)st[0] * H + 8.0 * H;
                } else {
                    *bytes_per_launch = 2.0 * (double)c_.vocab * H + 8.0 * H + 4.0 * c_.vocab;
                }
                break;
        }
    }
    return 0;
}

int Decoder::probe_gateup(int reps, float *us_per_launch, double *bytes_per_launch) {
    return probe_kernel(3, reps, us_per_launch, bytes_per_launch);
}

}  // namespace bitnet_host

using bitnet_host::Decoder;

namespace {
// a null handle or a dead decoder (rejected configuration, failed allocation): nothing but error() / destroy may be called
inline Decoder *live(void *d) {
    Decoder *p = static_cast<Decoder *>(d);
    return p && !p->dead() ? p : nullptr;
}
}  // namespace
#define LIVE(rc)           \
    Decoder *D = live(d);  \
    if (!D) return rc

extern "C" {
void *bitnet_host_create(const bitnet_host_config *cfg) {
    bitnet_host::Config c;
    c.hidden = cfg->hidden;
    c.n_layers = cfg->n_layers;
    c.n_heads = cfg->n_heads;
    c.n_kv_heads = cfg->n_kv_heads;
    c.head_dim = cfg->head_dim;
    c.ffn = cfg->ffn;
    c.vocab = cfg->vocab;
    c.max_pos = cfg->max_pos;
    c.eps = cfg->eps;
    c.rope_theta = cfg->rope_theta;
    // Nothing is thrown across the C boundary: a configuration the kernels cannot take comes back as a decoder
    // whose error() says why (every later call on it fails), allocation failures as nullptr.
    try {
        return new Decoder(c);
    } catch (...) {
        return nullptr;
    }
}
void *bitnet_host_create_shared(void *owner) {
    Decoder *o = live(owner);
    if (!o) return nullptr;
    try {
        Decoder *d = new Decoder(*o, 0);
        if (d->owner()) o->refs_++;  // a live borrower keeps its owner
        return d;
    } catch (...) {
        return nullptr;
    }
}
// Drops one reference; the last one deletes the object and, for a borrower, lets go of its owner.
void bitnet_host_release(void *d) {
    Decoder *p = static_cast<Decoder *>(d);
    while (p && --p->refs_ == 0) {
        Decoder *o = p->owner();
        delete p;
        p = o;
    }
}
void bitnet_host_destroy(void *d) { bitnet_host_release(d); }
int bitnet_host_set_attention_form(void *d, int form) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_attention_form(form); }
const char *bitnet_host_error(void *d) { return d ? static_cast<Decoder *>(d)->error().c_str() : "null decoder"; }
int bitnet_host_set_layer_qk256(void *d, int layer, const float *attn_norm, const float *ffn_norm, const uint8_t *q,
                                const uint8_t *k, const uint8_t *v, const uint8_t *o, const uint8_t *gate,
                                const uint8_t *up, const uint8_t *down) {
    bitnet_host::LayerWeightsQk256 w{attn_norm, ffn_norm, q, k, v, o, gate, up, down};
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->set_layer_qk256(layer, w);
}
int bitnet_host_set_layer_i2s(void *d, int layer, const float *attn_norm, const float *ffn_norm, const uint8_t *const *w7,
                              const float *const *scales7, size_t block_size) {
    bitnet_host::LayerWeightsI2s w;
    w.attn_norm = attn_norm;
    w.ffn_norm = ffn_norm;
    for (int i = 0; i < 7; ++i) {
        w.w[i] = w7[i];
        w.scales[i] = scales7[i];
    }
    w.block_size = block_size;
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->set_layer_i2s(layer, w);
}
int bitnet_host_set_globals(void *d, const uint16_t *embed_f16, const float *final_norm) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->set_globals(embed_f16, final_norm);
}
int bitnet_host_reset(void *d) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->reset(); }
int bitnet_host_set_sampling(void *d, const bitnet_hip_sampling_config *cfg) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_sampling(cfg); }
int bitnet_host_set_sampling_ex(void *d, const bitnet_hip_sampling_config_ex *cfg) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_sampling_ex(cfg); }
int bitnet_host_set_mirostat(void *d, const bitnet_hip_mirostat_config *cfg) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_mirostat(cfg); }
int bitnet_host_mirostat_state(void *d, float *mu, uint64_t *fallbacks) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->mirostat_state(mu, fallbacks); }
int bitnet_host_set_constraints(void *d, const bitnet_hip_constraints *cfg) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_constraints(cfg); }
int bitnet_host_constraints_state(void *d, uint64_t *chosen) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->constraints_state(chosen); }
int bitnet_host_set_grammar(void *d, bitnet_hip_grammar *g, int start_state) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_grammar(g, start_state); }
int bitnet_host_set_grammar_state(void *d, int state) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_grammar_state(state); }
int bitnet_host_grammar_state(void *d, int32_t *state, uint64_t *steps, uint64_t *violations) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->grammar_state(state, steps, violations);
}
int bitnet_host_sampling_draws(void *d, uint64_t *out) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->sampling_draws(out); }
int bitnet_host_set_stop(void *d, const bitnet_hip_stop_config *cfg) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_stop(cfg); }
int bitnet_host_stop_state(void *d, bitnet_hip_stop_state *out) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->stop_state(out); }
int bitnet_host_resume(void *d) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->resume(); }
int bitnet_host_run_until_stop(void *d, int max_steps, int chunk, int *steps, float *elapsed_ms) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->run_until_stop(max_steps, chunk, steps, elapsed_ms);
}
int bitnet_host_graph_nodes(void *d, int with_logits) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->graph_nodes(with_logits != 0); }
int bitnet_host_set_logprobs(void *d, int top_n) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_logprobs(top_n); }
int bitnet_host_logprobs(void *d, int first, int n, void *records_out) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->logprobs(first, n, static_cast<bitnet_hip_logprob_record *>(records_out));
}
int bitnet_host_feed(void *d, const int32_t *tokens, int n) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->feed(tokens, n); }
int bitnet_host_set_kv_f16(void *d, int on) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_kv_f16(on != 0); }
int bitnet_host_set_act_mode(void *d, int mode) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_act_mode(mode); }
int bitnet_host_act_mode(void *d) { LIVE(0); return D->qact_path() ? 1 : 0; }
int bitnet_host_prepare_graphs(void *d, int with_logits) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->prepare_graphs(with_logits != 0); }
int bitnet_host_run_reference(void *d, int n, int with_logits) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->run_reference(n, with_logits != 0); }
int bitnet_host_run(void *d, int n, int with_logits, int use_graph, float *elapsed_ms) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->run(n, with_logits != 0, use_graph != 0, elapsed_ms);
}
int bitnet_host_prefill(void *d, int n, int with_logits, int digits, float *elapsed_ms) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->prefill(n, with_logits != 0, digits, elapsed_ms);
}
int bitnet_host_extend(void *d, int n, int with_logits, int digits, float *elapsed_ms) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->extend(n, with_logits != 0, digits, elapsed_ms);
}
int bitnet_host_prefill_packed(void *const *members, const int32_t *n, int n_members, int with_logits, int digits, float *elapsed_ms) {
    if (!members || !live(members[0])) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    Decoder *ms[BITNET_HIP_PACK_MAX] = {};
    ms[0] = live(members[0]);  // the driver carries the error text, whatever n_members is
    for (int i = 1; i < n_members && i < BITNET_HIP_PACK_MAX; ++i) ms[i] = live(members[i]);  // a null or dead handle: refused as a null member
    return Decoder::prefill_packed(ms, n, n_members, with_logits != 0, digits, elapsed_ms);
}
int bitnet_host_step_wide(void *const *members, int n_members, int n_steps, int digits, float *elapsed_ms) {
    if (!members || !live(members[0])) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    Decoder *ms[BITNET_HIP_WIDE_MAX] = {};
    ms[0] = live(members[0]);  // the driver carries the error text, whatever n_members is
    for (int i = 1; i < n_members && i < BITNET_HIP_WIDE_MAX; ++i) ms[i] = static_cast<Decoder *>(members[i]);  // (a dead member is told from a null one)
    return Decoder::step_wide(ms, n_members, n_steps, digits, elapsed_ms);
}
int bitnet_host_rewind(void *d, int n) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->rewind(n);
}
int bitnet_host_shift(void *d, int keep, int discard) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->shift(keep, discard);
}
int bitnet_host_fork(void *src, void *const *dsts, int n_dst, int n) {
    Decoder *S = live(src);
    if (!S) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    Decoder *ds[BITNET_HIP_BATCH_MAX] = {};
    if (dsts)
        for (int i = 0; i < n_dst && i < BITNET_HIP_BATCH_MAX; ++i) ds[i] = static_cast<Decoder *>(dsts[i]);
    return Decoder::fork(*S, dsts ? ds : nullptr, n_dst, n);
}
int bitnet_host_cached_prefix(void *d, const int32_t *tokens, int n) {
    LIVE(-1);
    return D->cached_prefix(tokens, n);
}
int bitnet_host_prefill_sharded(void *d, int n, int rank, int world, bitnet_host_allgather_fn gather, void *gather_ctx, int with_logits,
                                int digits, int wire_f16, float *elapsed_ms) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->prefill_sharded(n, rank, world, gather, gather_ctx, with_logits != 0, digits, wire_f16 != 0, elapsed_ms);
}
int bitnet_host_rccl_allgather(void *nccl_comm, const void *send_dev, void *recv_dev, size_t bytes_per_rank, void *stream) {
    // ncclResult_t ncclAllGather(const void *sendbuff, void *recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream)
    using fn_t = int (*)(const void *, void *, size_t, int, void *, void *);
    static fn_t fn = [] {
        void *h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        return h ? reinterpret_cast<fn_t>(dlsym(h, "ncclAllGather")) : nullptr;
    }();
    if (!fn || !nccl_comm) return -1;
    return fn(send_dev, recv_dev, bytes_per_rank, /* ncclUint8 */ 1, nccl_comm, stream);
}
int bitnet_host_set_phase_timing(void *d, int on) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    D->set_phase_timing(on != 0);
    return 0;
}
int bitnet_host_phase_times(void *d, float out[4]) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    if (!out) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    D->phase_times(out);
    return 0;
}
int bitnet_host_finish_prefill(void *d, int n, const float *last_row, int with_logits) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->finish_prefill(n, last_row, with_logits != 0);
}
int bitnet_host_score(void *d, int n, int digits, float *nll_out, int32_t *argmax_out, float *logits_out, int logits_rows, float *elapsed_ms) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->score(n, digits, nll_out, argmax_out, logits_out, logits_rows, elapsed_ms);
}
void bitnet_host_layer_objects(void *d, int layer, uint64_t *handles4, void **ptrs4) {
    for (int i = 0; i < 4; ++i) handles4[i] = 0, ptrs4[i] = nullptr;
    if (Decoder *D = live(d)) D->layer_objects(layer, handles4, ptrs4);
}
void bitnet_host_global_objects(void *d, void **ptrs7) {
    for (int i = 0; i < 7; ++i) ptrs7[i] = nullptr;
    if (Decoder *D = live(d)) D->global_objects(ptrs7);
}
int bitnet_host_position(void *d) { LIVE(-1); return D->position(); }
int bitnet_host_form_at(void *d, int pos) { LIVE(-1); return pos < 0 ? -1 : D->form_at(pos); }
int bitnet_host_last_prefill_path(void *d) { LIVE(-1); return D->last_prefill_path(); }
int bitnet_host_saturation_fallbacks(void *d) { LIVE(-1); return D->saturation_fallbacks(); }
int bitnet_host_history(void *d, int32_t *out, int n) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->history(out, n); }
int bitnet_host_set_head_screen(void *d, int on) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->set_head_screen(on != 0); }
int bitnet_host_head_screen(void *d) { LIVE(-1); return D->head_screen() ? 1 : 0; }
int bitnet_host_head_screen_stats(void *d, uint32_t *out3) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    if (!out3) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    return D->head_screen_stats(out3);
}
int bitnet_host_last_logits(void *d, float *out) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->last_logits(out); }
int bitnet_host_last_hidden(void *d, float *out) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->last_hidden(out); }
int bitnet_host_blake3_hex(const void *data, size_t len, char *out65) {
    if (!out65 || (!data && len)) return -1;
    const std::string h = bitnet_host::Blake3::hex(data, len);
    memcpy(out65, h.c_str(), 65);
    return 0;
}
int bitnet_host_trace_step(void *d, const char *dir, int with_logits) { LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT); return D->trace_step(dir, with_logits != 0); }
int bitnet_host_probe_gateup(void *d, int reps, float *us_per_launch, double *bytes_per_launch) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->probe_gateup(reps, us_per_launch, bytes_per_launch);
}
int bitnet_host_probe_kernel(void *d, int kind, int reps, float *us_per_launch, double *bytes_per_launch) {
    LIVE(BITNET_HIP_ERR_INVALID_ARGUMENT);
    return D->probe_kernel(kind, reps, us_per_launch, bytes_per_launch);
}
uint64_t bitnet_host_weight_bytes(void *d) { LIVE(0); return D->weight_bytes(); }
uint64_t bitnet_host_device_bytes(void) { return bitnet_host::dev_bytes_live.load(); }
}
