// prefix_index_check.cpp -- host/prefix_index.hpp (the prefix cache's trie, limits, eviction policies and statistics) as a stand-alone program:
// built by the host compiler under the address and undefined-behaviour sanitizers and run by tests/test_prefix_index.py.
//   no argument:   the scripted cases -- the reference's own unit tests (crates/bitnet-inference/src/prefix_cache.rs, mod tests) restated on opaque
//                  entries, and the cases it has none for: each policy's victim, the LFU tie, the TTL fallback, both limits, "unable to free
//                  space", evict-before-replace, every statistics field by value.  Prints "prefix_index_check: ok".
//   <script file>: one operation per line against one index, one result line each -- the differential sweep's side of the comparison with
//                  the dictionary model in the test.
//                    C max_entries max_bytes policy min_len ttl   (first line)
//                    L tokens..            -> L hit matched id
//                    I size now tokens..   -> I ok id gone..
//                    E now                 -> E ok victim
//                    V tokens..            -> V ok id
//                    X                     -> X
//                    S                     -> S len evictions memory hit_rate miss_rate avg
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "prefix_index.hpp"

using namespace bitnet_host;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

typedef std::vector<int32_t> Toks;

static PrefixIndexConfig cfg(size_t max_entries, size_t max_bytes, EvictionPolicy p, size_t min_len = 1, uint64_t ttl = 3600) {
    PrefixIndexConfig c;
    c.max_entries = max_entries, c.max_memory_bytes = max_bytes, c.eviction_policy = p, c.min_prefix_length = min_len, c.ttl_seconds = ttl;
    return c;
}
// every key is a heap block of exactly its length: a read past a key is a sanitizer report
static bool ins(PrefixIndex &x, const Toks &t, size_t size, uint64_t now = 0, uint64_t *id = nullptr, std::vector<uint64_t> *gone = nullptr) {
    return x.insert(t.data(), t.size(), size, now, id, gone);
}
static long hit(PrefixIndex &x, const Toks &t, uint64_t *id = nullptr) {  // matched length, or -1
    size_t m = 0;
    return x.lookup(t.data(), t.size(), &m, id) ? (long)m : -1;
}

static void scripted() {
    const size_t MB = 1 << 20;
    {  // the defaults are the reference's
        PrefixIndexConfig d;
        CHECK(d.max_entries == 1024 && d.max_memory_bytes == 512 * MB && d.eviction_policy == EvictionPolicy::LRU && d.min_prefix_length == 4 &&
              d.ttl_seconds == 3600);
    }
    {  // exact key, a longer query, the longest of two, an entry longer than the query, siblings, the empty index
        PrefixIndex x(cfg(1024, 512 * MB, EvictionPolicy::LRU));
        CHECK(hit(x, {1, 2, 3}) == -1 && x.len() == 0);
        uint64_t a = 99, b = 99, got = 99;
        CHECK(ins(x, {10, 20, 30, 40}, 128, 0, &a));
        CHECK(hit(x, {10, 20, 30, 40}, &got) == 4 && got == a);
        CHECK(hit(x, {10, 20, 30, 40, 50, 60}, &got) == 4 && got == a);
        CHECK(hit(x, {10, 20, 30}) == -1);  // the entry at depth 4 is not reached
        CHECK(ins(x, {10, 20}, 16, 0, &b) && a != b);
        CHECK(hit(x, {10, 20, 30, 40, 50}, &got) == 4 && got == a);
        CHECK(hit(x, {10, 20, 30}, &got) == 2 && got == b);
        CHECK(hit(x, {10, 20, 99}, &got) == 2 && got == b);
        CHECK(hit(x, {10}) == -1 && hit(x, {}) == -1 && hit(x, {11, 20}) == -1);
        uint64_t s3 = 0, s4 = 0;
        CHECK(ins(x, {1, 2, 3}, 8, 0, &s3) && ins(x, {1, 2, 4}, 8, 0, &s4));
        CHECK(hit(x, {1, 2, 3, 99}, &got) == 3 && got == s3);
        CHECK(hit(x, {1, 2, 4, 99}, &got) == 3 && got == s4);
        CHECK(x.len() == 4 && x.stats().memory_usage == 128 + 16 + 8 + 8);
        CHECK(x.find(a) && x.find(a)->size_bytes == 128 && x.find(a)->key == Toks({10, 20, 30, 40}) && !x.find(12345));
    }
    {  // min_prefix_length
        PrefixIndex x(cfg(1024, 512 * MB, EvictionPolicy::LRU, 4));
        CHECK(!ins(x, {1, 2}, 8) && x.error() == "prefix length 2 is below minimum 4" && x.len() == 0);
        CHECK(!ins(x, {1, 2, 3}, 8) && ins(x, {1, 2, 3, 4}, 8) && x.len() == 1);
    }
    {  // replacing a key: one entry, the new id and size, the old id reported gone, hits start again
        PrefixIndex x(cfg(1024, 512 * MB, EvictionPolicy::LRU));
        uint64_t a = 0, b = 0, got = 0;
        std::vector<uint64_t> gone;
        CHECK(ins(x, {1, 2, 3}, 16, 0, &a) && hit(x, {1, 2, 3}) == 3);
        CHECK(ins(x, {1, 2, 3}, 40, 0, &b, &gone) && a != b && gone == std::vector<uint64_t>({a}));
        CHECK(x.len() == 1 && x.stats().memory_usage == 40 && !x.find(a) && x.find(b)->hits == 0);
        CHECK(hit(x, {1, 2, 3}, &got) == 3 && got == b && x.stats().eviction_count == 0);
    }
    {  // LRU: the victim is the entry whose last access (insert or lookup) is oldest
        PrefixIndex x(cfg(2, 512 * MB, EvictionPolicy::LRU));
        uint64_t a = 0, b = 0, c = 0;
        std::vector<uint64_t> gone;
        CHECK(ins(x, {1}, 8, 0, &a) && ins(x, {2}, 8, 0, &b));
        CHECK(hit(x, {1}) == 1);
        CHECK(ins(x, {3}, 8, 0, &c, &gone) && gone == std::vector<uint64_t>({b}));
        CHECK(hit(x, {1}) == 1 && hit(x, {2}) == -1 && hit(x, {3}) == 1 && x.stats().eviction_count == 1);
    }
    {  // LFU: the fewest hits; a tie goes to the older last access
        PrefixIndex x(cfg(3, 512 * MB, EvictionPolicy::LFU));
        uint64_t a = 0, b = 0, c = 0, v = 0;
        CHECK(ins(x, {1}, 8, 0, &a) && ins(x, {2}, 8, 0, &b) && ins(x, {3}, 8, 0, &c));
        for (int i = 0; i < 5; ++i) CHECK(hit(x, {1}) == 1);
        CHECK(hit(x, {3}) == 1 && hit(x, {2}) == 1);  // b and c: one hit each, c's the older access
        CHECK(x.evict(0, &v) && v == c);
        CHECK(x.evict(0, &v) && v == b);               // one hit against five
        CHECK(x.evict(0, &v) && v == a && !x.evict(0, &v) && x.stats().eviction_count == 3);
        // never looked up at all: the tie is between the inserts' stamps
        CHECK(ins(x, {7}, 8, 0, &a) && ins(x, {8}, 8, 0, &b) && x.evict(0, &v) && v == a);
    }
    {  // FIFO: by creation, whatever was looked up since
        PrefixIndex x(cfg(3, 512 * MB, EvictionPolicy::FIFO));
        uint64_t id[5] = {}, v = 0;
        for (int32_t i = 0; i < 3; ++i) CHECK(ins(x, {i}, 8, 0, &id[i]));
        CHECK(hit(x, {0}) == 1 && hit(x, {0}) == 1);
        std::vector<uint64_t> gone;
        CHECK(ins(x, {3}, 8, 0, &id[3], &gone) && ins(x, {4}, 8, 0, &id[4], &gone) && gone == std::vector<uint64_t>({id[0], id[1]}));
        CHECK(x.len() == 3 && x.evict(0, &v) && v == id[2]);
    }
    {  // TTL: the oldest EXPIRED entry; when none has expired, the oldest
        PrefixIndex x(cfg(8, 512 * MB, EvictionPolicy::TTL, 1, 100));
        uint64_t a = 0, b = 0, c = 0, v = 0;
        CHECK(ins(x, {1}, 8, 1000, &a) && ins(x, {2}, 8, 1050, &b) && ins(x, {3}, 8, 1090, &c));
        CHECK(x.evict(1099, &v) && v == a);  // nothing has expired (99 s): falls back to the oldest
        CHECK(ins(x, {1}, 8, 1095, &a));     // now the youngest
        CHECK(x.evict(1150, &v) && v == b);  // b is exactly 100 s old: expired; c (60 s) and a (55 s) are not
        CHECK(x.evict(1195, &v) && v == c);  // c 105 s, a 100 s: both expired, the older goes
        CHECK(x.evict(1195, &v) && v == a && x.len() == 0);
        // expiry counts from the entry's own insert, not from its last lookup
        CHECK(ins(x, {5}, 8, 2000, &a) && ins(x, {6}, 8, 2090, &b) && hit(x, {5}) == 1);
        CHECK(x.evict(2100, &v) && v == a);
    }
    {  // the byte limit: evicts until the new entry fits
        PrefixIndex x(cfg(100, 64, EvictionPolicy::LRU));
        uint64_t a = 0, b = 0, c = 0;
        std::vector<uint64_t> gone;
        CHECK(ins(x, {1}, 32, 0, &a) && ins(x, {2}, 32, 0, &b) && x.stats().memory_usage == 64 && x.len() == 2);
        CHECK(ins(x, {3}, 32, 0, &c, &gone) && gone == std::vector<uint64_t>({a}) && x.stats().memory_usage == 64 && x.len() == 2);
        gone.clear();
        CHECK(ins(x, {4}, 64, 0, &a, &gone) && gone == std::vector<uint64_t>({b, c}) && x.stats().memory_usage == 64 && x.len() == 1);
        // "unable to free space": the reference empties the cache trying, and so does the index
        gone.clear();
        CHECK(!ins(x, {5}, 65, 0, nullptr, &gone) && x.error() == "unable to free space for new prefix cache entry");
        CHECK(gone == std::vector<uint64_t>({a}) && x.len() == 0 && x.stats().memory_usage == 0 && x.stats().eviction_count == 4);
        CHECK(ins(x, {5}, 64) && ins(x, {6}, 0) && x.len() == 2);  // an entry of no bytes always fits beside a full one
    }
    {  // the entry limit, and an index that may hold nothing
        PrefixIndex x(cfg(1, 512 * MB, EvictionPolicy::LRU));
        CHECK(ins(x, {1}, 8) && ins(x, {2}, 8) && ins(x, {3}, 8) && x.len() == 1 && x.stats().eviction_count == 2);
        CHECK(hit(x, {3}) == 1 && hit(x, {1}) == -1);
        PrefixIndex none(cfg(0, 512 * MB, EvictionPolicy::LRU));
        CHECK(!ins(none, {1}, 8) && none.error() == "unable to free space for new prefix cache entry" && none.len() == 0);
    }
    {  // evict-before-replace: at a full index a replacement first evicts a victim it would not have needed ...
        PrefixIndex x(cfg(2, 512 * MB, EvictionPolicy::LRU));
        uint64_t a = 0, b = 0, b2 = 0;
        std::vector<uint64_t> gone;
        CHECK(ins(x, {1}, 8, 0, &a) && ins(x, {2}, 8, 0, &b));
        CHECK(ins(x, {2}, 8, 0, &b2, &gone) && gone == std::vector<uint64_t>({a, b}));  // a evicted, then b replaced
        CHECK(x.len() == 1 && x.stats().eviction_count == 1 && hit(x, {1}) == -1 && hit(x, {2}) == 1);
        // ... which may be the old entry itself: then nothing is left to replace, and the other entry survives
        PrefixIndex y(cfg(2, 512 * MB, EvictionPolicy::LRU));
        gone.clear();
        CHECK(ins(y, {1}, 8, 0, &a) && ins(y, {2}, 8, 0, &b) && ins(y, {1}, 8, 0, &b2, &gone) && gone == std::vector<uint64_t>({a}));
        CHECK(y.len() == 2 && y.stats().eviction_count == 1 && hit(y, {2}) == 1);
        // and the old entry's bytes count against the byte limit until it is replaced
        PrefixIndex z(cfg(8, 100, EvictionPolicy::FIFO));
        gone.clear();
        CHECK(ins(z, {1}, 40, 0, &a) && ins(z, {2}, 50, 0, &b) && ins(z, {2}, 20, 0, &b2, &gone) && gone == std::vector<uint64_t>({a, b}));
        CHECK(z.len() == 1 && z.stats().memory_usage == 20);
    }
    {  // invalidate: exact keys only, siblings and prefixes stay, the trie is pruned
        PrefixIndex x(cfg(1024, 512 * MB, EvictionPolicy::LRU));
        uint64_t a = 0, b = 0, c = 0, got = 0;
        CHECK(ins(x, {1, 2, 3}, 8, 0, &a) && ins(x, {1, 2, 4}, 8, 0, &b) && ins(x, {1, 2}, 8, 0, &c));
        CHECK(!x.invalidate(Toks({1}).data(), 1, &got) && !x.invalidate(Toks({1, 2, 3, 4}).data(), 4, &got) && x.len() == 3);
        CHECK(x.invalidate(Toks({1, 2, 3}).data(), 3, &got) && got == a && x.len() == 2 && x.stats().memory_usage == 16);
        CHECK(hit(x, {1, 2, 3}, &got) == 2 && got == c && hit(x, {1, 2, 4}, &got) == 3 && got == b);
        CHECK(x.invalidate(Toks({1, 2}).data(), 2, &got) && got == c && hit(x, {1, 2, 3}) == -1 && hit(x, {1, 2, 4}) == 3);
        CHECK(x.invalidate(Toks({1, 2, 4}).data(), 3, &got) && x.len() == 0 && x.stats().eviction_count == 0);  // an invalidation is no eviction
    }
    {  // statistics, every field by value; clear resets them
        PrefixIndex x(cfg(2, 512 * MB, EvictionPolicy::LRU));
        PrefixIndexStats s = x.stats();
        CHECK(s.hit_rate == 0.0 && s.miss_rate == 0.0 && s.eviction_count == 0 && s.memory_usage == 0 && s.avg_prefix_match_length == 0.0);
        CHECK(ins(x, {1, 2}, 8) && ins(x, {1, 2, 3, 4}, 24));
        CHECK(hit(x, {1, 2, 3, 4, 5}) == 4 && hit(x, {1, 2, 99}) == 2 && hit(x, {9, 8, 7}) == -1 && hit(x, {1}) == -1);
        s = x.stats();
        CHECK(s.hit_rate == 0.5 && s.miss_rate == 0.5 && s.avg_prefix_match_length == 3.0 && s.memory_usage == 32 && s.eviction_count == 0);
        CHECK(hit(x, {1, 2}) == 2);
        s = x.stats();
        CHECK(s.hit_rate == 0.6 && s.miss_rate == 1.0 - 0.6 && s.avg_prefix_match_length == 8.0 / 3.0);
        CHECK(ins(x, {5}, 100) && x.stats().eviction_count == 1 && x.stats().memory_usage == 108);  // {1, 2, 3, 4} went: the older access
        x.clear();
        s = x.stats();
        CHECK(x.len() == 0 && s.hit_rate == 0.0 && s.miss_rate == 0.0 && s.eviction_count == 0 && s.memory_usage == 0 && s.avg_prefix_match_length == 0.0);
        CHECK(hit(x, {1, 2}) == -1 && ins(x, {1, 2}, 8) && hit(x, {1, 2}) == 2 && x.stats().hit_rate == 0.5);
    }
    {  // a key as long as a context: no recursion to run out of stack on
        PrefixIndex x(cfg(4, 512 * MB, EvictionPolicy::LRU));
        Toks t(4096);
        for (size_t i = 0; i < t.size(); ++i) t[i] = (int32_t)(i * 7919 % 128256);
        uint64_t v = 0;
        CHECK(ins(x, t, 1) && hit(x, t) == 4096 && x.evict(0, &v) && hit(x, t) == -1);
    }
}

static int run_script(const char *path) {
    std::ifstream in(path);
    if (!in) return 2;
    std::string line;
    std::unique_ptr<PrefixIndex> x;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        char op = 0;
        ls >> op;
        auto rest = [&]() {
            Toks t;
            int64_t v;
            while (ls >> v) t.push_back((int32_t)v);
            return t;
        };
        if (op == 'C') {
            size_t me = 0, mb = 0, ml = 0;
            int pol = 0;
            uint64_t ttl = 0;
            ls >> me >> mb >> pol >> ml >> ttl;
            x.reset(new PrefixIndex(cfg(me, mb, (EvictionPolicy)pol, ml, ttl)));
            continue;
        }
        if (!x) return 3;
        if (op == 'L') {
            const Toks t = rest();
            size_t m = 0;
            uint64_t id = 0;
            const bool ok = x->lookup(t.data(), t.size(), &m, &id);
            std::printf("L %d %zu %" PRIu64 "\n", (int)ok, ok ? m : (size_t)0, ok ? id : (uint64_t)0);
        } else if (op == 'I') {
            size_t size = 0;
            uint64_t now = 0, id = 0;
            ls >> size >> now;
            const Toks t = rest();
            std::vector<uint64_t> gone;
            const bool ok = x->insert(t.data(), t.size(), size, now, &id, &gone);
            std::printf("I %d %" PRIu64, (int)ok, ok ? id : (uint64_t)0);
            for (uint64_t g : gone) std::printf(" %" PRIu64, g);
            std::printf("\n");
        } else if (op == 'E') {
            uint64_t now = 0, v = 0;
            ls >> now;
            const bool ok = x->evict(now, &v);
            std::printf("E %d %" PRIu64 "\n", (int)ok, ok ? v : (uint64_t)0);
        } else if (op == 'V') {
            const Toks t = rest();
            uint64_t id = 0;
            const bool ok = x->invalidate(t.data(), t.size(), &id);
            std::printf("V %d %" PRIu64 "\n", (int)ok, ok ? id : (uint64_t)0);
        } else if (op == 'X') {
            x->clear();
            std::printf("X\n");
        } else if (op == 'S') {
            const PrefixIndexStats s = x->stats();
            std::printf("S %zu %" PRIu64 " %zu %.17g %.17g %.17g\n", x->len(), s.eviction_count, s.memory_usage, s.hit_rate, s.miss_rate, s.avg_prefix_match_length);
        } else {
            return 4;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return run_script(argv[1]);
    scripted();
    if (failures) {
        std::printf("prefix_index_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("prefix_index_check: ok\n");
    return 0;
}
