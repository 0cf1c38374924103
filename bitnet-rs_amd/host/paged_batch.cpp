// paged_batch.cpp -- see paged_batch.hpp.  Owns the pools, the page bookkeeping and the device page tables; the forward is WideBatch's step on
// cache-less members with the paged attention in every layer, and every launch is a bitnet_hip_* entry point.
#include "paged_batch.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>

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

int PagedBatch::fail(const char *what) {
    const char *e = bitnet_hip_get_last_error();
    err_ = std::string(what) + ": " + (e ? e : "error");
    return BITNET_HIP_ERR_EXECUTION;
}

int PagedBatch::fail_arg(const std::string &what) {
    err_ = what;
    return BITNET_HIP_ERR_INVALID_ARGUMENT;
}

PagedBatch::PagedBatch(Decoder &root, size_t n_pages, int n_slots) {
    for (int &s : seq_) s = -1;
    if (root.dead_ || root.owner_ || !root.embed_) {
        err_ = "paged batch: the root must be a live owner that holds its model";
        return;
    }
    if (n_slots < 1 || n_slots > BITNET_HIP_WIDE_MAX) {
        err_ = "paged batch: 1.." + std::to_string(BITNET_HIP_WIDE_MAX) + " slots";
        return;
    }
    const Config &c = root.c_;
    const size_t NL = root.layers_.size(), NK = (size_t)c.n_kv_heads;
    kv_f16_ = root.kv_f16_;
    const size_t pb = bitnet_hip_kv_pool_bytes(n_pages, NK, (size_t)c.head_dim, kv_f16_ ? 1 : 0);
    chunks_ = ((size_t)c.max_pos + 63) / 64;
    const size_t max_splits = chunks_ < 16 ? chunks_ : 16;  // the library's own choice never exceeds 16 (csrc/paged_splits.hpp)
    const size_t sb = bitnet_hip_attention_paged_shared_scratch_bytes((size_t)n_slots, NK, max_splits, max_splits);  // shared splits: at most 16 too
    if (!pb || !sb) {
        err_ = "paged batch: n_pages / the model's attention geometry is not one the paged attention takes";
        return;
    }
    // the pools start zero-filled: the attention multiplies slots past a position by exact zeros, so they must hold finite bit patterns
    kpool_.resize(NL), vpool_.resize(NL), pool_host_.assign(2 * NL, nullptr);
    bool bad = false;
    for (size_t l = 0; l < NL && !bad; ++l) {
        bad = kpool_[l].alloc_zeroed(pb) || vpool_[l].alloc_zeroed(pb);
        pool_host_[l] = kpool_[l].get(), pool_host_[NL + l] = vpool_[l].get();
    }
    bad = bad || pool_dev_.alloc(2 * NL) || tables_.alloc_zeroed((size_t)n_slots * chunks_) || table_ptrs_.alloc_zeroed(BITNET_HIP_WIDE_MAX) ||
          scratch_.alloc_zeroed(sb) || hipMemcpy(pool_dev_, pool_host_.data(), 2 * NL * sizeof(void *), hipMemcpyHostToDevice);
    if (bad) {
        err_ = "paged batch: device allocation failed";
        return;
    }
    pool_bytes_ = 2 * NL * pb;
    n_pages_ = n_pages;
    pool_.reset(new PagePool((uint32_t)n_pages));
    attn_.kpools = pool_host_.data(), attn_.vpools = pool_host_.data() + NL, attn_.n_pages = n_pages;
    attn_.tables = table_ptrs_.get(), attn_.scratch = scratch_.get();
    wide_.reset(new WideBatch(n_slots));
    if (wide_->dead()) {
        err_ = wide_->error();
        return;
    }
    wide_->set_paged(&attn_);
    leader_.assign(BITNET_HIP_WIDE_MAX, 0), shared_pages_.assign(BITNET_HIP_WIDE_MAX, 0), layer_rows_.assign(NL, 0);
    root_ = &root;
    root_->refs_++;
    n_ = n_slots;
    dead_ = false;
}

PagedBatch::~PagedBatch() {
    for (int b = 0; b < n_; ++b)
        if (slot_[b]) release(b);
    wide_.reset();  // its tables and its reference on the root go before ours
    if (root_) bitnet_host_release(root_);
}

int PagedBatch::check_slot(int slot, bool want_member) {
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (slot < 0 || slot >= n_) return fail_arg("paged batch: slot index out of range");
    if (want_member && !slot_[slot]) return fail_arg("paged batch: the slot is empty");
    if (!want_member && slot_[slot]) return fail_arg("paged batch: the slot is taken (release it first)");
    return 0;
}

// a cache-less borrower of the root with the pool's cache type; null with the error text set
Decoder *PagedBatch::new_member() {
    Decoder *m = nullptr;
    try {
        m = new Decoder(*root_, 0, true);
    } catch (...) {
    }
    if (!m || m->dead_) {
        err_ = m ? "paged batch: creating a member: " + m->err_ : "paged batch: creating a member failed";
        delete m;
        return nullptr;
    }
    root_->refs_++;  // a live borrower keeps its owner (bitnet_host_release lets go of it)
    m->kv_f16_ = kv_f16_;
    return m;
}

int PagedBatch::upload_table(int slot) {
    const PagePool::Seq *s = pool_->find(seq_[slot]);
    if (s && !s->pages.empty())
        HCHK(hipMemcpy(tables_ + (size_t)slot * chunks_, s->pages.data(), s->pages.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
}

int PagedBatch::arrive(Decoder *dst, int n, const Decoder &from) {
    const int rc = root_->fork_arrive(&dst, 1, n, from.host_forced_ < n ? from.host_forced_ : n, from.history_, true, root_->stream_);
    if (rc) err_ = root_->err_;
    return rc;
}

int PagedBatch::seat(int slot, Decoder *m, int seq) {
    if (int rc = wide_->set_slot(slot, m)) {
        err_ = wide_->error();
        pool_->release(seq);
        bitnet_host_release(m);
        return rc;
    }
    slot_[slot] = m, seq_[slot] = seq;
    dense_stale_ = true;
    return 0;
}

int PagedBatch::admit(int slot, Decoder &src, int n) {
    if (int rc = check_slot(slot, false)) return rc;
    if (src.dead_ || src.no_cache_) return fail_arg("paged batch: admit takes a live staging decoder with caches of its own");
    if (src.root() != root_) return fail_arg("paged batch: the staging decoder must run on the root's weights (the owner or a borrower)");
    if (src.kv_f16_ != kv_f16_) return fail_arg("paged batch: mixed KV cache types (the pools have the root's)");
    const int p = src.position();
    if (p < 0) {
        err_ = src.err_;
        return BITNET_HIP_ERR_GPU;
    }
    if (n < 1 || n > p) return fail_arg("paged batch: admit: n must be in [1, position()] of the staging decoder");
    if (((size_t)n + 63) / 64 > pool_->pages_free())
        return fail_arg("paged batch: the pool has too few free pages (" + std::to_string(pool_->pages_free()) + " free, " + std::to_string((n + 63) / 64) + " needed)");
    if (int rc = src.ensure_fork_tables()) {
        err_ = src.err_;
        return rc;
    }
    Decoder *m = new_member();
    if (!m) return BITNET_HIP_ERR_GPU;
    const int seq = pool_->create();
    pool_->reserve(seq, n - 1);  // cannot fail: the pages were counted above
    if (int rc = seat(slot, m, seq)) return rc;
    const Config &c = root_->c_;
    const size_t NL = root_->layers_.size();
    int rc = upload_table(slot);
    if (!rc && bitnet_hip_kv_page_in_dev(src.fork_tables_, src.fork_tables_ + NL, pool_dev_, pool_dev_ + NL, tables_ + (size_t)slot * chunks_, n_pages_, NL,
                                         (size_t)c.n_kv_heads, (size_t)c.head_dim, (size_t)c.max_pos, (size_t)n, kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, root_->stream_))
        rc = fail("bitnet_hip_kv_page_in_dev");
    if (!rc) rc = arrive(m, n, src);
    return rc ? unseat(slot, rc) : 0;
}

// a runtime failure behind seat(): the slot, its pages and the member go again, the error text stays
int PagedBatch::unseat(int slot, int rc) {
    const std::string why = err_;
    release(slot);
    err_ = why;
    return rc;
}

int PagedBatch::fork(int from, int to) {
    if (int rc = check_slot(from, true)) return rc;
    if (int rc = check_slot(to, false)) return rc;
    Decoder *src = slot_[from];
    const int p = src->position();
    if (p < 0) {
        err_ = src->err_;
        return BITNET_HIP_ERR_GPU;
    }
    Decoder *m = new_member();
    if (!m) return BITNET_HIP_ERR_GPU;
    if (int rc = seat(to, m, pool_->fork(seq_[from]))) return rc;
    int rc = upload_table(to);
    if (!rc) rc = arrive(m, p, *src);
    return rc ? unseat(to, rc) : 0;
}

int PagedBatch::release(int slot) {
    if (int rc = check_slot(slot, true)) return rc;
    Decoder *m = slot_[slot];
    if (int rc = wide_->set_slot(slot, nullptr)) {
        err_ = wide_->error();
        return rc;
    }
    pool_->release(seq_[slot]);
    slot_[slot] = nullptr, seq_[slot] = -1;
    dense_stale_ = true;
    bitnet_host_release(m);
    return 0;
}

int PagedBatch::extract(int slot, Decoder &dst) {
    if (int rc = check_slot(slot, true)) return rc;
    Decoder *m = slot_[slot], *d = &dst;
    if (const char *why = Decoder::fork_refusal(&d, 1, m, root_, kv_f16_)) return fail_arg(std::string("paged batch: extract: ") + why);
    const int p = m->position();
    if (p < 0) {
        err_ = m->err_;
        return BITNET_HIP_ERR_GPU;
    }
    if (int rc = dst.ensure_fork_tables()) {
        err_ = dst.err_;
        return rc;
    }
    const Config &c = root_->c_;
    const size_t NL = root_->layers_.size();
    BCHK(bitnet_hip_kv_page_out_dev(pool_dev_, pool_dev_ + NL, tables_ + (size_t)slot * chunks_, n_pages_, dst.fork_tables_, dst.fork_tables_ + NL, NL,
                                    (size_t)c.n_kv_heads, (size_t)c.head_dim, (size_t)c.max_pos, (size_t)p, kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, root_->stream_));
    return arrive(d, p, *m);
}

int PagedBatch::open(int slot) {
    if (int rc = check_slot(slot, false)) return rc;
    Decoder *m = new_member();
    if (!m) return BITNET_HIP_ERR_GPU;
    return seat(slot, m, pool_->create());
}

int PagedBatch::prefill(const int *slots, const int *n, int count, bool with_logits, int digits, float *elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    // every refusal comes before the first write, the page count included (as step() counts: fresh pages up to the last new position, and a
    // private copy of the page of the first append for every sharer but the last)
    if (!slots || !n || count < 1 || count > BITNET_HIP_PACK_MAX) return fail_arg("paged batch: prefill: 1.." + std::to_string(BITNET_HIP_PACK_MAX) + " listed members");
    std::vector<Decoder *> members((size_t)count);
    std::vector<int32_t> past((size_t)count), len((size_t)count);
    std::vector<const uint32_t *> tabs((size_t)count);
    size_t need = 0;
    std::map<uint32_t, uint32_t> sharers;
    for (int i = 0; i < count; ++i) {
        if (int rc = check_slot(slots[i], true)) return rc;
        for (int j = 0; j < i; ++j)
            if (slots[j] == slots[i]) return fail_arg("paged batch: prefill: a slot is listed twice");
        Decoder *m = members[(size_t)i] = slot_[slots[i]];
        const int p = m->position();
        if (p < 0) {
            err_ = m->err_;
            return BITNET_HIP_ERR_GPU;
        }
        if (n[i] < 1) return fail_arg("paged batch: prefill: every member takes at least 1 token");
        if (const char *e = m->span_problem(p, n[i])) return fail_arg(e);
        past[(size_t)i] = p, len[(size_t)i] = n[i], tabs[(size_t)i] = tables_ + (size_t)slots[i] * chunks_;
        const std::vector<uint32_t> &pg = pool_->find(seq_[slots[i]])->pages;
        const size_t want = (size_t)(p + n[i] - 1) / 64 + 1;
        need += want > pg.size() ? want - pg.size() : 0;
        if ((size_t)p / 64 < pg.size() && pool_->ref_count(pg[(size_t)p / 64]) > 1) {
            uint32_t &left = sharers.emplace(pg[(size_t)p / 64], pool_->ref_count(pg[(size_t)p / 64])).first->second;
            if (left > 1) ++need, --left;
        }
    }
    if (need > pool_->pages_free())
        return fail_arg("paged batch: the pool has too few free pages for this prefill (" + std::to_string(pool_->pages_free()) + " free, " + std::to_string(need) + " needed)");
    std::vector<uint32_t> pairs;
    std::vector<int> changed;
    for (int i = 0; i < count; ++i) {
        const PagePool::Reserve first = pool_->reserve(seq_[slots[i]], past[(size_t)i]), rest = pool_->reserve(seq_[slots[i]], past[(size_t)i] + len[(size_t)i] - 1);
        if (first.copy) pairs.push_back(first.src), pairs.push_back(first.dst);
        if (first.grew || rest.grew) changed.push_back(slots[i]);
    }
    const Config &c = root_->c_;
    const size_t NL = root_->layers_.size();
    if (!pairs.empty())
        BCHK(bitnet_hip_kv_page_copy_dev(pool_dev_, pool_dev_ + NL, n_pages_, pairs.data(), pairs.size() / 2, NL, (size_t)c.n_kv_heads, (size_t)c.head_dim,
                                         kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, root_->stream_));
    for (int b : changed)
        if (int rc = upload_table(b)) return rc;
    // the root drives: its prompt buffers, its stream; the members bring history, position and their own heads
    const int rc = root_->packed_forward(members.data(), past, len, with_logits, digits, elapsed_ms, &attn_, tabs.data());
    if (rc) err_ = root_->err_;
    return rc;
}

int PagedBatch::set_share(int min_pages) {
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (min_pages < 0) return fail_arg("paged batch: set_share: min_pages must be 0 (off) or at least 1");
    share_min_ = min_pages;
    return 0;
}

// Dense row i = the i-th occupied slot.  A group = the rows whose page lists start with the same page; its run = their longest common leading run,
// capped at min position >> 6 (the page that takes an append is never in it, now or later in the step: positions only grow).
void PagedBatch::find_groups(const int *pos) {
    int rows[BITNET_HIP_WIDE_MAX], M = 0;
    for (int b = 0; b < n_; ++b)
        if (slot_[b]) rows[M++] = b;
    bool seen[BITNET_HIP_WIDE_MAX] = {}, any = false;
    for (int i = 0; i < M; ++i) leader_[(size_t)i] = i, shared_pages_[(size_t)i] = 0;
    for (int i = 0; i < M; ++i) {
        if (seen[i]) continue;
        const std::vector<uint32_t> &lead = pool_->find(seq_[rows[i]])->pages;
        if (lead.empty()) continue;
        std::vector<int> members;
        size_t run = lead.size();
        for (int j = i; j < M; ++j) {
            const std::vector<uint32_t> &pg = pool_->find(seq_[rows[j]])->pages;
            if (seen[j] || pg.empty() || pg[0] != lead[0]) continue;
            seen[j] = true;
            members.push_back(j);
            size_t k = 0, cap = (size_t)pos[rows[j]] >> 6;
            if (cap > pg.size()) cap = pg.size();
            if (cap > run) cap = run;
            while (k < cap && pg[k] == lead[k]) ++k;
            run = k;
        }
        if (members.size() < 2 || run < (size_t)share_min_) continue;
        for (int j : members) leader_[(size_t)j] = i, shared_pages_[(size_t)j] = (int32_t)run;
        any = true;
    }
    if (any) attn_.leader = leader_.data(), attn_.shared_pages = shared_pages_.data(), attn_.shared_layer_rows = layer_rows_.data();
}

int PagedBatch::step(int n, int digits, float *elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (dead_) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    // every refusal comes before the first write: the pages all members need are counted first -- fresh ones up to position + n - 1, and a
    // private copy of the page of the first append for every sharer but the last (reserve() lets go of the shared page as it copies)
    if (n < 1) return fail_arg("paged batch: n_steps must be at least 1");
    int M = 0, pos[BITNET_HIP_WIDE_MAX] = {};
    size_t need = 0;
    std::map<uint32_t, uint32_t> sharers;  // shared first-append pages: references left as the members before took their copies
    for (int b = 0; b < n_; ++b) {
        Decoder *m = slot_[b];
        if (!m) continue;
        ++M;
        const int p = pos[b] = m->position();
        if (p < 0) {
            err_ = m->err_;
            return BITNET_HIP_ERR_GPU;
        }
        if (const char *e = m->overflow_problem(p, n)) return fail_arg(e);
        const std::vector<uint32_t> &pg = pool_->find(seq_[b])->pages;
        const size_t want = (size_t)(p + n - 1) / 64 + 1;
        need += want > pg.size() ? want - pg.size() : 0;
        if ((size_t)p / 64 < pg.size() && pool_->ref_count(pg[(size_t)p / 64]) > 1) {
            uint32_t &left = sharers.emplace(pg[(size_t)p / 64], pool_->ref_count(pg[(size_t)p / 64])).first->second;
            if (left > 1) ++need, --left;
        }
    }
    if (!M) return fail_arg("paged batch: no member to step (every slot is empty)");
    if (need > pool_->pages_free())
        return fail_arg("paged batch: the pool has too few free pages for " + std::to_string(n) + " more positions of every member (" + std::to_string(pool_->pages_free()) +
                        " free, " + std::to_string(need) + " needed)");
    std::vector<uint32_t> pairs;
    bool changed[BITNET_HIP_WIDE_MAX] = {};
    for (int b = 0; b < n_; ++b) {
        if (!slot_[b]) continue;
        // the page of the first append must be private (a fork that diverges: copy-on-write), the pages behind it are fresh; counted above
        const PagePool::Reserve first = pool_->reserve(seq_[b], pos[b]), rest = pool_->reserve(seq_[b], pos[b] + n - 1);
        if (first.copy) pairs.push_back(first.src), pairs.push_back(first.dst);
        changed[b] = first.grew || rest.grew;
    }
    const Config &c = root_->c_;
    const size_t NL = root_->layers_.size();
    if (!pairs.empty())
        BCHK(bitnet_hip_kv_page_copy_dev(pool_dev_, pool_dev_ + NL, n_pages_, pairs.data(), pairs.size() / 2, NL, (size_t)c.n_kv_heads, (size_t)c.head_dim,
                                         kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, root_->stream_));
    for (int b = 0; b < n_; ++b)
        if (changed[b])
            if (int rc = upload_table(b)) return rc;
    // Row i = the i-th occupied slot.  WideBatch's dense list is the occupied AND un-parked slots; the two agree because nothing here parks a
    // member: a PagedBatch never calls WideBatch::step_until (the only caller of read_stops(park = true)) and does not hand its WideBatch out.
    if (dense_stale_) {
        const uint32_t *t[BITNET_HIP_WIDE_MAX] = {};
        int i = 0;
        for (int b = 0; b < n_; ++b)
            if (slot_[b]) t[i++] = tables_ + (size_t)b * chunks_;
        HCHK(hipMemcpy(table_ptrs_, t, sizeof(t), hipMemcpyHostToDevice));
        dense_stale_ = false;
    }
    attn_.leader = attn_.shared_pages = nullptr, attn_.shared_layer_rows = nullptr;
    shared_rows_ = 0;
    layer_rows_.assign(layer_rows_.size(), 0);
    if (share_min_ > 0) find_groups(pos);
    const int rc = wide_->step(n, digits, elapsed_ms);
    if (rc) err_ = wide_->error();
    for (size_t r : layer_rows_) shared_rows_ += r;
    return rc;
}

}  // namespace bitnet_host

using bitnet_host::Decoder;
using bitnet_host::PagedBatch;

extern "C" {
void *bitnet_host_paged_batch_create(void *root, size_t n_pages, int n_slots) {
    if (!root) return nullptr;
    try {
        return new PagedBatch(*static_cast<Decoder *>(root), n_pages, n_slots);
    } catch (...) {
        return nullptr;
    }
}
void bitnet_host_paged_batch_destroy(void *b) { delete static_cast<PagedBatch *>(b); }
const char *bitnet_host_paged_batch_error(void *b) { return b ? static_cast<PagedBatch *>(b)->error().c_str() : "null paged batch"; }
int bitnet_host_paged_batch_admit(void *b, int slot, void *src, int n) {
    return b && src ? static_cast<PagedBatch *>(b)->admit(slot, *static_cast<Decoder *>(src), n) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_paged_batch_fork(void *b, int from, int to) { return b ? static_cast<PagedBatch *>(b)->fork(from, to) : BITNET_HIP_ERR_INVALID_ARGUMENT; }
int bitnet_host_paged_batch_release(void *b, int slot) { return b ? static_cast<PagedBatch *>(b)->release(slot) : BITNET_HIP_ERR_INVALID_ARGUMENT; }
int bitnet_host_paged_batch_extract(void *b, int slot, void *dst) {
    return b && dst ? static_cast<PagedBatch *>(b)->extract(slot, *static_cast<Decoder *>(dst)) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_paged_batch_step(void *b, int n, int digits, float *elapsed_ms) {
    return b ? static_cast<PagedBatch *>(b)->step(n, digits, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
int bitnet_host_paged_batch_open(void *b, int slot) { return b ? static_cast<PagedBatch *>(b)->open(slot) : BITNET_HIP_ERR_INVALID_ARGUMENT; }
int bitnet_host_paged_batch_prefill(void *b, const int32_t *slots, const int32_t *n, int count, int with_logits, int digits, float *elapsed_ms) {
    return b ? static_cast<PagedBatch *>(b)->prefill(slots, n, count, with_logits != 0, digits, elapsed_ms) : BITNET_HIP_ERR_INVALID_ARGUMENT;
}
void *bitnet_host_paged_batch_member(void *b, int slot) {
    Decoder *m = b ? static_cast<PagedBatch *>(b)->member(slot) : nullptr;
    if (m) m->refs_++;
    return m;
}
int bitnet_host_paged_batch_set_share(void *b, int min_pages) { return b ? static_cast<PagedBatch *>(b)->set_share(min_pages) : BITNET_HIP_ERR_INVALID_ARGUMENT; }
int64_t bitnet_host_paged_batch_shared_rows(void *b) { return b ? (int64_t) static_cast<PagedBatch *>(b)->shared_rows() : -1; }
int64_t bitnet_host_paged_batch_pages_in_use(void *b) { return b ? (int64_t) static_cast<PagedBatch *>(b)->pages_in_use() : -1; }
int64_t bitnet_host_paged_batch_pages_free(void *b) { return b ? (int64_t) static_cast<PagedBatch *>(b)->pages_free() : -1; }
uint64_t bitnet_host_paged_batch_pool_bytes(void *b) { return b ? (uint64_t) static_cast<PagedBatch *>(b)->pool_bytes() : 0; }
void *bitnet_host_create_shared_no_cache(void *owner) {
    Decoder *o = static_cast<Decoder *>(owner);
    if (!o || o->dead()) return nullptr;
    try {
        Decoder *d = new Decoder(*o, 0, true);
        if (d->owner()) o->refs_++;  // a live borrower keeps its owner
        return d;
    } catch (...) {
        return nullptr;
    }
}
}
