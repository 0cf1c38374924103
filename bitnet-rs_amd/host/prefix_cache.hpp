// prefix_cache.hpp -- PrefixCache: the reference's prompt prefix cache (crates/bitnet-inference/src/prefix_cache.rs) with the cached state on the
// device.  The index (prefix_index.hpp: trie, limits, eviction policies, statistics) is the reference's; where its CacheEntry holds opaque host
// bytes (`cached_state`, :64-77), an entry here holds ONE compact device snapshot (bitnet_hip_kv_save_dev, include/bitnet_hip_kvsnap.h): the first
// n positions of every layer's K and V and nothing else -- 153,600 bytes per position at the 2B-4T shape in f32, where a live decoder kept for
// Decoder::fork costs max_pos of them.  A hit is ONE bitnet_hip_kv_restore_dev launch into up to 8 decoders.
//
// The fork-equivalence contract: restore(id, dsts, n_dst, k) leaves every destination exactly as Decoder::fork(src, dsts, n_dst, k) would have,
// had src still been in its state at insert time -- position, forced count, history, sampler reset, log-probability records, stop state, cache
// slots < k, every other cache byte untouched, captured graphs still valid (decoder.hpp, fork).  The refusals are fork's.
// SINGLE-THREADED USE, as the decoders it serves.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "decoder.hpp"
#include "dev_buffer.hpp"
#include "prefix_index.hpp"

namespace bitnet_host {

class PrefixCache {
  public:
    explicit PrefixCache(const PrefixIndexConfig &cfg) : index_(cfg) {}
    PrefixCache(const PrefixCache &) = delete;
    PrefixCache &operator=(const PrefixCache &) = delete;

    const std::string &error() const { return err_; }
    size_t len() const { return index_.len(); }
    PrefixIndexStats stats() const { return index_.stats(); }

    // Caches the first n positions of src, 0 < n <= src.position(), under the key history[0, n): allocates bitnet_hip_kv_snapshot_bytes, ONE
    // save launch on src's stream, synchronises.  The entry keeps what fork carries: n + 1 history entries (entry n: the unconsumed picked or
    // fed token) and min(src's forced count, n).  Its size in the index is the snapshot's bytes; entries the index evicts or replaces on the
    // way free their device memory BEFORE the new snapshot is allocated, so the snapshots together never exceed max_memory_bytes (a HIP error
    // in the allocation or the launch behind that leaves no new entry, and the victims gone).  The first insert BINDS the cache to src.root()
    // and src.kv_f16() (clear() unbinds).  LIFETIME: the root is remembered as an address and only compared, so the cache must not outlive the
    // owner it is bound to -- clear() (or destroy) the cache before that owner goes; another model created at the same address would pass the
    // comparison with other cache sizes.  src is only read and may sit in a batch slot.  now_seconds: the caller's monotonic clock, for the TTL
    // policy.  *id (nullable): the new entry's id.
    // Refused, with nothing modified: a dead decoder; n out of range; a key shorter than min_prefix_length; a decoder with another root or
    // cache type than the cache is bound to (the root is compared, never dereferenced); a snapshot larger than max_memory_bytes, or
    // max_entries == 0.
    int insert(Decoder &src, int n, uint64_t now_seconds, uint64_t *id);
    // Host only: the longest entry whose whole key is a prefix of tokens[0, n).  True: *matched its length, *id its id.
    bool lookup(const int32_t *tokens, int n, int *matched, uint64_t *id);
    // The first n_positions (0 <= n_positions <= the entry's length) of entry `id` into n_dst = 1..8 destinations: ONE restore launch on the
    // first destination's stream; synchronises.  See the contract above.  The error text goes on the cache and on the first destination.
    // Refused, with nothing modified: fork's refusals (n_dst outside 1..8; a null, dead or repeated destination; one of another root or cache
    // type; one sitting in a BatchDecoder slot); an id the cache does not hold (never inserted, evicted, invalidated); n_positions out of range.
    int restore(uint64_t id, Decoder *const *dsts, int n_dst, int n_positions);
    // The entry keyed exactly tokens[0, n) goes, with its device memory: true if there was one.
    bool invalidate(const int32_t *tokens, int n);
    // Every entry and its device memory go, the statistics are reset, and the cache is unbound.
    void clear();
    // length in positions, snapshot bytes and forced count (what a restore of the whole entry hands over) of an entry, or false
    bool entry(uint64_t id, int *n_positions, uint64_t *snapshot_bytes, int *forced) const;
    // false for a decoder of another root or cache type than the cache is bound to: nothing here is its to restore
    bool serves(Decoder &d) const;

  private:
    int refuse(const char *what);
    void drop(const std::vector<uint64_t> &ids);
    struct Payload {
        DevBuf<void> snapshot;
        size_t bytes = 0;
        int n = 0;                     // positions
        int forced = 0;                // min(src's forced count, n)
        std::vector<int32_t> history;  // n + 1 entries
    };
    PrefixIndex index_;
    std::unordered_map<uint64_t, Payload> payloads_;
    std::string err_;
    // the binding: what every entry was saved from, and every destination must match
    bool bound_ = false;
    const Decoder *root_ = nullptr;  // compared only
    bool kv_f16_ = false;
    Config cfg_;
    DevBuf<void *> tables_;  // restore's destination tables: K [8][n_layers], V [8][n_layers]
};

}  // namespace bitnet_host

// C shim for the Python bindings (ctypes), as decoder.hpp's.
extern "C" {
typedef struct bitnet_host_prefix_stats {
    double hit_rate, miss_rate, avg_prefix_match_length;
    uint64_t eviction_count, memory_usage;
} bitnet_host_prefix_stats;
// policy: 0 LRU, 1 LFU, 2 FIFO, 3 TTL (another value: NULL).  The reference's defaults are 1024, 512 MiB, LRU, 4, 3600.
void *bitnet_host_prefix_cache_create(size_t max_entries, size_t max_memory_bytes, int policy, size_t min_prefix_length, uint64_t ttl_seconds);
void bitnet_host_prefix_cache_destroy(void *cache);
const char *bitnet_host_prefix_cache_error(void *cache);
int bitnet_host_prefix_cache_insert(void *cache, void *decoder, int n, uint64_t now_seconds, uint64_t *id_out);  // PrefixCache::insert
// PrefixCache::lookup: 1 a hit (*matched, *id_out), 0 a miss, negative an error
int bitnet_host_prefix_cache_lookup(void *cache, const int32_t *tokens, int n, int *matched, uint64_t *id_out);
// PrefixCache::restore; n_positions -1: the whole entry
int bitnet_host_prefix_cache_restore(void *cache, uint64_t id, void *const *dsts, int n_dst, int n_positions);
int bitnet_host_prefix_cache_invalidate(void *cache, const int32_t *tokens, int n);  // 1 an entry went, 0 none, negative an error
int bitnet_host_prefix_cache_clear(void *cache);
int bitnet_host_prefix_cache_stats(void *cache, bitnet_host_prefix_stats *out);
int bitnet_host_prefix_cache_len(void *cache);  // entries, or negative for a null handle
// length in positions, snapshot bytes and forced count of entry `id` (each nullable): 0, or INVALID_ARGUMENT for an id the cache does not hold
int bitnet_host_prefix_cache_entry(void *cache, uint64_t id, int *n_positions, uint64_t *snapshot_bytes, int *forced);
// Decoder::prefill_cached; *hit: positions restored
int bitnet_host_prefill_cached(void *d, void *cache, int n, int with_logits, int digits, int *hit, float *elapsed_ms);
}
