// prefix_index.hpp -- the reference's PrefixCache (crates/bitnet-inference/src/prefix_cache.rs) without its payload: the token trie, longest-prefix
// lookup (:173), insert (:212), evict (:269: LRU / LFU / FIFO / TTL under an entry limit and a byte limit), invalidate, clear and the statistics,
// over OPAQUE entries -- an id and a byte size.  Whoever owns the payloads (host/prefix_cache.hpp: one device snapshot per entry) is told which ids
// went.  Plain host C++, no HIP include: tests/host/prefix_index_check.cpp builds it alone under the sanitizers.
//
// Kept from the reference, quirks included:
//   - lookup returns the longest entry whose WHOLE key is a prefix of the query; an entry longer than the query is no match;
//   - insert evicts until both limits hold and ONLY THEN replaces an entry with the same key, so a replacement at a full cache evicts a victim it
//     would not have needed (the victim may be the old entry itself), and the old entry's bytes count against the byte limit until it is replaced;
//   - an entry that can never fit (max_entries == 0, or larger than max_memory_bytes) empties the index and then fails "unable to free space":
//     a caller that wants such an insert refused with nothing modified checks the size first (PrefixCache::insert does);
//   - LFU ties go to the older last_access; TTL evicts the oldest expired entry and falls back to the oldest entry when none has expired;
//   - clear also resets the statistics; hit / miss rates are 0 before the first lookup.
// The ONE deliberate difference is time, and it makes the index deterministic: where the reference stamps last_access / created_at with
// Instant::now(), every stamp here is the next value of a 64-bit sequence counter (no two stamps tie), and TTL compares a caller-supplied
// monotonic `now_seconds` with the now_seconds of the entry's insert.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace bitnet_host {

enum class EvictionPolicy : int { LRU = 0, LFU = 1, FIFO = 2, TTL = 3 };

// PrefixCacheConfig and its defaults (prefix_cache.rs:46-56)
struct PrefixIndexConfig {
    size_t max_entries = 1024;
    size_t max_memory_bytes = (size_t)512 * 1024 * 1024;
    EvictionPolicy eviction_policy = EvictionPolicy::LRU;
    size_t min_prefix_length = 4;
    uint64_t ttl_seconds = 3600;
};

// PrefixCacheStats (prefix_cache.rs:83-96)
struct PrefixIndexStats {
    double hit_rate = 0.0, miss_rate = 0.0;
    uint64_t eviction_count = 0;
    size_t memory_usage = 0;
    double avg_prefix_match_length = 0.0;
};

class PrefixIndex {
  public:
    struct Entry {
        std::vector<int32_t> key;
        size_t size_bytes = 0;
        uint64_t hits = 0;
        uint64_t last_access = 0, created_at = 0;  // sequence stamps
        uint64_t inserted_seconds = 0;             // the insert's now_seconds (TTL)
    };

    explicit PrefixIndex(const PrefixIndexConfig &cfg = PrefixIndexConfig()) : cfg_(cfg), root_(new Node) {}

    const PrefixIndexConfig &config() const { return cfg_; }
    size_t len() const { return entries_.size(); }
    const std::string &error() const { return err_; }
    const Entry *find(uint64_t id) const {
        auto it = entries_.find(id);
        return it == entries_.end() ? nullptr : &it->second;
    }

    // The longest entry whose whole key is a prefix of tokens[0, n): true, *matched its length and *id its id; the entry's hits and last_access
    // move.  Every call counts as a lookup.
    bool lookup(const int32_t *tokens, size_t n, size_t *matched, uint64_t *id) {
        ++lookups_;
        const Node *node = root_.get();
        bool found = false;
        size_t best_len = 0;
        uint64_t best_id = 0;
        for (size_t d = 0; d < n; ++d) {
            auto it = node->children.find(tokens[d]);
            if (it == node->children.end()) break;
            node = it->second.get();
            if (node->has_entry) found = true, best_len = d + 1, best_id = node->entry;
        }
        if (!found) return false;
        Entry &e = entries_.at(best_id);
        e.hits += 1;
        e.last_access = ++clock_;
        ++hits_;
        matched_total_ += best_len;
        if (matched) *matched = best_len;
        if (id) *id = best_id;
        return true;
    }

    // Stores an entry of size_bytes under tokens[0, n): false with error() set for a key shorter than min_prefix_length and when eviction cannot
    // make room.  Ids that left the index on the way -- evicted, or replaced -- are appended to *gone (also when the insert then fails).
    bool insert(const int32_t *tokens, size_t n, size_t size_bytes, uint64_t now_seconds, uint64_t *id, std::vector<uint64_t> *gone) {
        if (n < cfg_.min_prefix_length) {
            err_ = "prefix length " + std::to_string(n) + " is below minimum " + std::to_string(cfg_.min_prefix_length);
            return false;
        }
        // evict until there is room -- BEFORE the same-key entry is looked for, as the reference does
        while (entries_.size() >= cfg_.max_entries || size_bytes > cfg_.max_memory_bytes || memory_ > cfg_.max_memory_bytes - size_bytes) {
            uint64_t victim = 0;
            if (!evict(now_seconds, &victim)) {
                err_ = "unable to free space for new prefix cache entry";
                return false;
            }
            if (gone) gone->push_back(victim);
        }
        uint64_t old = 0;
        if (exact(tokens, n, &old)) {
            remove(old);
            if (gone) gone->push_back(old);
        }
        const uint64_t nid = next_id_++;
        Entry e;
        e.key.assign(tokens, tokens + n);
        e.size_bytes = size_bytes;
        e.last_access = e.created_at = ++clock_;
        e.inserted_seconds = now_seconds;
        memory_ += size_bytes;
        entries_.emplace(nid, std::move(e));
        Node *node = root_.get();
        for (size_t d = 0; d < n; ++d) {
            std::unique_ptr<Node> &child = node->children[tokens[d]];
            if (!child) child.reset(new Node);
            node = child.get();
        }
        node->has_entry = true, node->entry = nid;
        if (id) *id = nid;
        return true;
    }

    // One victim by the policy; false when the index is empty.
    bool evict(uint64_t now_seconds, uint64_t *victim) {
        if (entries_.empty()) return false;
        auto older = [](const Entry &a, const Entry &b) { return a.created_at < b.created_at; };
        const Entry *best = nullptr;
        uint64_t best_id = 0;
        auto take_min = [&](auto less, auto eligible) {
            for (const auto &kv : entries_)
                if (eligible(kv.second) && (!best || less(kv.second, *best))) best = &kv.second, best_id = kv.first;
        };
        auto all = [](const Entry &) { return true; };
        switch (cfg_.eviction_policy) {
            case EvictionPolicy::LRU:
                take_min([](const Entry &a, const Entry &b) { return a.last_access < b.last_access; }, all);
                break;
            case EvictionPolicy::LFU:
                take_min([](const Entry &a, const Entry &b) { return a.hits != b.hits ? a.hits < b.hits : a.last_access < b.last_access; }, all);
                break;
            case EvictionPolicy::FIFO:
                take_min(older, all);
                break;
            case EvictionPolicy::TTL:
                take_min(older, [&](const Entry &e) { return now_seconds >= e.inserted_seconds && now_seconds - e.inserted_seconds >= cfg_.ttl_seconds; });
                if (!best) take_min(older, all);  // nothing has expired: the oldest
                break;
        }
        remove(best_id);
        ++evictions_;
        if (victim) *victim = best_id;
        return true;
    }

    // Removes the entry whose key is exactly tokens[0, n): true and *id if there was one.
    bool invalidate(const int32_t *tokens, size_t n, uint64_t *id) {
        uint64_t old = 0;
        if (!exact(tokens, n, &old)) return false;
        remove(old);
        if (id) *id = old;
        return true;
    }

    // Every entry goes, and the statistics with them (ids are not reused).
    void clear() {
        root_.reset(new Node);
        entries_.clear();
        memory_ = 0;
        lookups_ = hits_ = matched_total_ = evictions_ = 0;
    }

    PrefixIndexStats stats() const {
        PrefixIndexStats s;
        if (lookups_) s.hit_rate = (double)hits_ / (double)lookups_, s.miss_rate = 1.0 - s.hit_rate;
        if (hits_) s.avg_prefix_match_length = (double)matched_total_ / (double)hits_;
        s.eviction_count = evictions_;
        s.memory_usage = memory_;
        return s;
    }

  private:
    struct Node {
        std::map<int32_t, std::unique_ptr<Node>> children;
        bool has_entry = false;
        uint64_t entry = 0;
    };

    bool exact(const int32_t *tokens, size_t n, uint64_t *id) const {
        const Node *node = root_.get();
        for (size_t d = 0; d < n; ++d) {
            auto it = node->children.find(tokens[d]);
            if (it == node->children.end()) return false;
            node = it->second.get();
        }
        if (!node->has_entry) return false;
        *id = node->entry;
        return true;
    }

    // the entry, its bytes, its trie leaf and every ancestor the leaf leaves empty
    void remove(uint64_t id) {
        auto it = entries_.find(id);
        if (it == entries_.end()) return;
        const std::vector<int32_t> key = std::move(it->second.key);
        memory_ -= it->second.size_bytes;
        entries_.erase(it);
        std::vector<Node *> path{root_.get()};
        for (int32_t t : key) {
            auto c = path.back()->children.find(t);
            if (c == path.back()->children.end()) return;
            path.push_back(c->second.get());
        }
        if (path.back()->has_entry && path.back()->entry == id) path.back()->has_entry = false;
        for (size_t d = key.size(); d > 0; --d) {
            const Node *leaf = path[d];
            if (leaf->has_entry || !leaf->children.empty()) break;
            path[d - 1]->children.erase(key[d - 1]);
        }
    }

    PrefixIndexConfig cfg_;
    std::unique_ptr<Node> root_;
    std::unordered_map<uint64_t, Entry> entries_;
    std::string err_;
    uint64_t next_id_ = 0, clock_ = 0;
    size_t memory_ = 0;
    uint64_t lookups_ = 0, hits_ = 0, matched_total_ = 0, evictions_ = 0;
};

}  // namespace bitnet_host
