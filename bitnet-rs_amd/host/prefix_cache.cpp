// prefix_cache.cpp -- see prefix_cache.hpp.
#include "prefix_cache.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>

namespace bitnet_host {

// HIP and library calls of the cache: the text on the cache (restore copies it to the first destination)
#define PC_HIP(expr)                                                                                                    \
    do {                                                                                                                \
        hipError_t _e = (expr);                                                                                         \
        if (_e != hipSuccess) {                                                                                         \
            char _b[256];                                                                                               \
            snprintf(_b, sizeof(_b), "HIP error %s at %s:%d (%s)", hipGetErrorName(_e), __FILE__, __LINE__, #expr);     \
            err_ = _b;                                                                                                  \
            return BITNET_HIP_ERR_GPU;                                                                                  \
        }                                                                                                               \
    } while (0)
#define PC_LIB(expr)                                                 \
    do {                                                             \
        if ((expr) != 0) {                                           \
            const char *_e = bitnet_hip_get_last_error();            \
            err_ = std::string(#expr) + ": " + (_e ? _e : "error");  \
            return BITNET_HIP_ERR_EXECUTION;                         \
        }                                                            \
    } while (0)

int PrefixCache::refuse(const char *what) {
    err_ = what;
    return BITNET_HIP_ERR_INVALID_ARGUMENT;
}

void PrefixCache::drop(const std::vector<uint64_t> &ids) {
    for (uint64_t id : ids) payloads_.erase(id);  // the DevBuf frees the snapshot
}

int PrefixCache::insert(Decoder &src, int n, uint64_t now_seconds, uint64_t *id) {
    // every refusal comes before the first allocation and the first change of the index
    if (src.dead()) return refuse("insert: dead decoder");
    if (bound_ && src.root() != root_) return refuse("insert: the decoder runs on other weights than the cache is bound to");
    if (bound_ && src.kv_f16() != kv_f16_) return refuse("insert: mixed KV cache types");
    const int p = src.position();
    if (p < 0) return refuse("insert: position readback failed");
    if (n < 1 || n > p) return refuse("insert: n must be in [1, position()]");
    const PrefixIndexConfig &ic = index_.config();
    if ((size_t)n < ic.min_prefix_length) {
        err_ = "insert: prefix length " + std::to_string(n) + " is below minimum " + std::to_string(ic.min_prefix_length);
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    const Config &c = src.config();
    const int flags = src.kv_f16() ? BITNET_HIP_ATTN_KV_F16 : 0;
    const size_t L = (size_t)c.n_layers, bytes = bitnet_hip_kv_snapshot_bytes(L, (size_t)c.n_kv_heads, (size_t)c.head_dim, (size_t)n, flags);
    if (!bytes) return refuse("insert: the decoder's geometry has no snapshot form");
    if (bytes > ic.max_memory_bytes || ic.max_entries == 0) return refuse("insert: unable to free space for new prefix cache entry (it exceeds the cache's limits)");

    Payload pl;
    pl.bytes = bytes, pl.n = n, pl.forced = src.host_forced_ < n ? src.host_forced_ : n;
    pl.history.resize((size_t)n + 1);
    DevBuf<void *> tables;
    if (!bound_) PC_HIP(tables.alloc(2 * (size_t)BITNET_HIP_BATCH_MAX * L));
    if (int rc = src.ensure_fork_tables()) {
        err_ = src.error();
        return rc;
    }
    PC_HIP(hipMemcpy(pl.history.data(), src.history_, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));  // the key; every decoder call returns synchronised

    // The index first: it evicts until both limits hold, then replaces an entry with the same key (prefix_index.hpp), and what went frees its
    // device memory BEFORE the new snapshot is allocated -- the snapshots never hold more than max_memory_bytes together.
    std::vector<uint64_t> gone;
    uint64_t nid = 0;
    const bool ok = index_.insert(pl.history.data(), (size_t)n, bytes, now_seconds, &nid, &gone);
    drop(gone);
    if (!ok) return refuse(("insert: " + index_.error()).c_str());
    const auto save = [&]() -> int {
        hipStream_t s = (hipStream_t)src.stream_;
        PC_HIP(pl.snapshot.alloc(bytes));
        PC_LIB(bitnet_hip_kv_save_dev(src.fork_tables_, src.fork_tables_ + L, L, (size_t)c.n_kv_heads, (size_t)c.head_dim, (size_t)c.max_pos, (size_t)n, flags,
                                      pl.snapshot, s));
        PC_HIP(hipStreamSynchronize(s));
        return 0;
    };
    if (int rc = save()) {
        index_.invalidate(pl.history.data(), (size_t)n, nullptr);  // no entry without its snapshot (the victims above stay gone)
        return rc;
    }
    payloads_.emplace(nid, std::move(pl));
    if (!bound_) bound_ = true, root_ = src.root(), kv_f16_ = src.kv_f16(), cfg_ = c, tables_ = std::move(tables);
    if (id) *id = nid;
    return 0;
}

bool PrefixCache::lookup(const int32_t *tokens, int n, int *matched, uint64_t *id) {
    size_t m = 0;
    if (!index_.lookup(tokens, n > 0 && tokens ? (size_t)n : 0, &m, id)) return false;
    if (matched) *matched = (int)m;
    return true;
}

int PrefixCache::restore(uint64_t id, Decoder *const *dsts, int n_dst, int n_positions) {
    Decoder *first = dsts && n_dst >= 1 && dsts[0] && !dsts[0]->dead() ? dsts[0] : nullptr;
    auto report = [&](int rc) {
        if (rc && first) first->set_error(err_);
        return rc;
    };
    // every refusal comes before the first write
    auto it = payloads_.find(id);
    if (const char *why = Decoder::fork_refusal(dsts, n_dst, nullptr, bound_ ? root_ : (first ? first->root() : nullptr), bound_ ? kv_f16_ : (first && first->kv_f16())))
        return report(refuse((std::string("restore: ") + why).c_str()));
    if (it == payloads_.end()) return report(refuse("restore: the cache holds no such entry (never inserted, evicted or invalidated)"));
    const Payload &pl = it->second;
    if (n_positions < 0 || n_positions > pl.n) return report(refuse("restore: n_positions must be in [0, the entry's length]"));

    // one root, hence one Config: every destination cache has the geometry the snapshot was saved from
    const size_t L = (size_t)cfg_.n_layers, M = BITNET_HIP_BATCH_MAX;
    hipStream_t s = (hipStream_t)first->stream_;
    auto body = [&]() -> int {
        if (n_positions > 0) {
            std::vector<void *> t(2 * M * L, nullptr);
            for (int i = 0; i < n_dst; ++i)
                for (size_t l = 0; l < L; ++l) t[(size_t)i * L + l] = dsts[i]->layers_[l].kcache, t[(M + (size_t)i) * L + l] = dsts[i]->layers_[l].vcache;
            PC_HIP(hipMemcpy(tables_, t.data(), t.size() * sizeof(void *), hipMemcpyHostToDevice));
            PC_LIB(bitnet_hip_kv_restore_dev(pl.snapshot, (size_t)pl.n, tables_, tables_ + M * L, L, (size_t)n_dst, (size_t)cfg_.n_kv_heads,
                                             (size_t)cfg_.head_dim, (size_t)cfg_.max_pos, (size_t)n_positions, kv_f16_ ? BITNET_HIP_ATTN_KV_F16 : 0, s));
        }
        return 0;
    };
    if (int rc = body()) return report(rc);
    if (int rc = first->fork_arrive(dsts, n_dst, n_positions, pl.forced < n_positions ? pl.forced : n_positions, pl.history.data(), false, s)) {
        err_ = first->error();
        return rc;
    }
    return 0;
}

bool PrefixCache::invalidate(const int32_t *tokens, int n) {
    uint64_t id = 0;
    if (!index_.invalidate(tokens, n > 0 && tokens ? (size_t)n : 0, &id)) return false;
    payloads_.erase(id);
    return true;
}

void PrefixCache::clear() {
    index_.clear();
    payloads_.clear();
    tables_.reset();
    bound_ = false, root_ = nullptr;
}

bool PrefixCache::entry(uint64_t id, int *n_positions, uint64_t *snapshot_bytes, int *forced) const {
    auto it = payloads_.find(id);
    if (it == payloads_.end()) return false;
    if (n_positions) *n_positions = it->second.n;
    if (snapshot_bytes) *snapshot_bytes = it->second.bytes;
    if (forced) *forced = it->second.forced;
    return true;
}

bool PrefixCache::serves(Decoder &d) const { return !bound_ || (d.root() == root_ && d.kv_f16() == kv_f16_); }

int Decoder::prefill_cached(PrefixCache &cache, int n, bool with_logits, int digits, int *hit, float *elapsed_ms) {
    if (hit) *hit = 0;
    if (!embed_) return fail_arg("model globals not set");
    const int p = position();
    if (p < 0) return BITNET_HIP_ERR_GPU;
    if (p != 0) return fail_arg("prefill needs a fresh sequence (position 0): reset() first");
    if (const char *e = span_problem(0, n)) return fail_arg(e);
    std::vector<int32_t> t((size_t)n);
    if (hipMemcpy(t.data(), history_, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail_arg("prefill_cached: history readback failed");
    int m = 0;
    uint64_t id = 0;
    // a cache bound to other weights or another cache type holds nothing for this decoder: a miss, and not looked up
    if (!cache.serves(*this) || !cache.lookup(t.data(), n, &m, &id)) return prompt_forward(0, n, with_logits, digits, elapsed_ms);  // prefill, whose guards are held above
    const int k = m < n - 1 ? m : n - 1;  // at least one token is computed: its row gives the logits
    Decoder *self = this;
    if (int rc = cache.restore(id, &self, 1, k)) return rc;
    // restore left history[0 .. k] and zeros beyond, as fork does: the rest of the prompt goes in again, at slot k
    if (int rc = feed(t.data() + k, n - k)) return rc;
    if (hit) *hit = k;
    return extend(n - k, with_logits, digits, elapsed_ms);
}

}  // namespace bitnet_host

using bitnet_host::Decoder;
using bitnet_host::PrefixCache;

extern "C" {
void *bitnet_host_prefix_cache_create(size_t max_entries, size_t max_memory_bytes, int policy, size_t min_prefix_length, uint64_t ttl_seconds) {
    if (policy < 0 || policy > 3) return nullptr;
    bitnet_host::PrefixIndexConfig c;
    c.max_entries = max_entries, c.max_memory_bytes = max_memory_bytes, c.eviction_policy = (bitnet_host::EvictionPolicy)policy;
    c.min_prefix_length = min_prefix_length, c.ttl_seconds = ttl_seconds;
    try {
        return new PrefixCache(c);
    } catch (...) {
        return nullptr;
    }
}
void bitnet_host_prefix_cache_destroy(void *cache) { delete static_cast<PrefixCache *>(cache); }
const char *bitnet_host_prefix_cache_error(void *cache) { return cache ? static_cast<PrefixCache *>(cache)->error().c_str() : "null prefix cache"; }
// Nothing is thrown across the C boundary: an allocation failure of the host containers comes back as an error code.
#define PC_TRY(rc_null, ...)                             \
    PrefixCache *P = static_cast<PrefixCache *>(cache);  \
    if (!P) return rc_null;                              \
    try {                                                \
        __VA_ARGS__                                      \
    } catch (...) {                                      \
        return BITNET_HIP_ERR_EXECUTION;                 \
    }
int bitnet_host_prefix_cache_insert(void *cache, void *decoder, int n, uint64_t now_seconds, uint64_t *id_out) {
    PC_TRY(BITNET_HIP_ERR_INVALID_ARGUMENT, Decoder *D = static_cast<Decoder *>(decoder); if (!D) return BITNET_HIP_ERR_INVALID_ARGUMENT;
           return P->insert(*D, n, now_seconds, id_out);)
}
int bitnet_host_prefix_cache_lookup(void *cache, const int32_t *tokens, int n, int *matched, uint64_t *id_out) {
    PC_TRY(-1, if (n < 0 || (n > 0 && !tokens)) return -1; return P->lookup(tokens, n, matched, id_out) ? 1 : 0;)
}
int bitnet_host_prefix_cache_restore(void *cache, uint64_t id, void *const *dsts, int n_dst, int n_positions) {
    PC_TRY(BITNET_HIP_ERR_INVALID_ARGUMENT, Decoder * ds[BITNET_HIP_BATCH_MAX] = {};
           for (int i = 0; dsts && i < n_dst && i < BITNET_HIP_BATCH_MAX; ++i) ds[i] = static_cast<Decoder *>(dsts[i]);
           int whole = 0; if (n_positions == -1 && P->entry(id, &whole, nullptr, nullptr)) n_positions = whole;
           return P->restore(id, dsts ? ds : nullptr, n_dst, n_positions);)
}
int bitnet_host_prefix_cache_invalidate(void *cache, const int32_t *tokens, int n) {
    PC_TRY(-1, if (n < 0 || (n > 0 && !tokens)) return -1; return P->invalidate(tokens, n) ? 1 : 0;)
}
int bitnet_host_prefix_cache_clear(void *cache) { PC_TRY(BITNET_HIP_ERR_INVALID_ARGUMENT, P->clear(); return 0;) }
int bitnet_host_prefix_cache_stats(void *cache, bitnet_host_prefix_stats *out) {
    PC_TRY(BITNET_HIP_ERR_INVALID_ARGUMENT, if (!out) return BITNET_HIP_ERR_INVALID_ARGUMENT; const bitnet_host::PrefixIndexStats s = P->stats();
           out->hit_rate = s.hit_rate, out->miss_rate = s.miss_rate, out->avg_prefix_match_length = s.avg_prefix_match_length;
           out->eviction_count = s.eviction_count, out->memory_usage = s.memory_usage; return 0;)
}
int bitnet_host_prefix_cache_len(void *cache) { PC_TRY(-1, return (int)P->len();) }
int bitnet_host_prefix_cache_entry(void *cache, uint64_t id, int *n_positions, uint64_t *snapshot_bytes, int *forced) {
    PC_TRY(BITNET_HIP_ERR_INVALID_ARGUMENT, return P->entry(id, n_positions, snapshot_bytes, forced) ? 0 : BITNET_HIP_ERR_INVALID_ARGUMENT;)
}
int bitnet_host_prefill_cached(void *d, void *cache, int n, int with_logits, int digits, int *hit, float *elapsed_ms) {
    Decoder *D = static_cast<Decoder *>(d);
    if (!D || D->dead()) return BITNET_HIP_ERR_INVALID_ARGUMENT;
    if (!cache) {
        D->set_error("prefill_cached: null prefix cache");
        return BITNET_HIP_ERR_INVALID_ARGUMENT;
    }
    return D->prefill_cached(*static_cast<PrefixCache *>(cache), n, with_logits != 0, digits, hit, elapsed_ms);
}
}
