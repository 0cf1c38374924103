// kv_pool.hpp -- the host side of the paged KV cache: which page of the device pools (include/bitnet_hip_paged.h) belongs to which sequence.
// Plain host C++, the standard library only, no HIP: a free list, a reference count per page, and per sequence the list of its page ids --
// what the reference keeps in PagedKvCache's page table (crates/bitnet-inference/src/kv_cache_optimized.rs).  It moves no byte: the caller
// uploads the tables and issues the page copies it is told about.
//
// Rules.  A page is free (count 0, on the free list) or held by count >= 1 sequences.  fork() shares every page of a sequence.  The page
// that takes a sequence's next append must be private to it: reserve() says when it is not and hands out a private one to copy into
// (copy-on-write).  An operation that cannot be served changes nothing.
#pragma once

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace bitnet_host {

class PagePool {
  public:
    struct Seq {
        std::vector<uint32_t> pages;  // page of positions [64 i, 64 i + 64) at index i
        int n = 0;                    // positions it has room reserved for (reserve)
    };
    struct Reserve {
        bool ok = false;        // false: the pool has too few free pages; nothing changed
        bool grew = false;      // pages were appended: the sequence's table changed
        bool copy = false;      // the page of the next append was shared: copy page src into dst (now the sequence's, private) before appending
        uint32_t src = 0, dst = 0;
    };

    explicit PagePool(uint32_t n_pages) : count_(n_pages, 0) {
        free_.reserve(n_pages);
        for (uint32_t p = n_pages; p > 0; --p) free_.push_back(p - 1);  // page 0 is handed out first
    }

    // a new, empty sequence
    int create() {
        const int id = next_id_++;
        seqs_[id] = Seq();
        return id;
    }
    bool has(int seq) const { return seqs_.count(seq) != 0; }
    const Seq *find(int seq) const {
        auto it = seqs_.find(seq);
        return it == seqs_.end() ? nullptr : &it->second;
    }

    // Room for positions [0, upto_pos] (an append lands at upto_pos): fresh pages are appended up to the page of upto_pos, and if that page
    // is shared with another sequence it is replaced by a private one.  This is the ONE way a sequence's n moves: n = the positions it has
    // room reserved for, at least upto_pos + 1 afterwards.
    Reserve reserve(int seq, int upto_pos) {
        Reserve r;
        auto it = seqs_.find(seq);
        if (it == seqs_.end() || upto_pos < 0) return r;
        Seq &s = it->second;
        const size_t want = (size_t)upto_pos / 64 + 1, have = s.pages.size();
        const size_t fresh = want > have ? want - have : 0;
        const bool shared = fresh == 0 && count_[s.pages[want - 1]] > 1;
        if (fresh + (shared ? 1 : 0) > free_.size()) return r;
        for (size_t i = 0; i < fresh; ++i) s.pages.push_back(take());
        if (shared) {
            r.copy = true, r.src = s.pages[want - 1], r.dst = take();
            --count_[r.src];
            s.pages[want - 1] = r.dst;
        }
        if (s.n < upto_pos + 1) s.n = upto_pos + 1;
        r.ok = true, r.grew = fresh > 0 || shared;
        return r;
    }

    // a new sequence that shares every page of `seq`; -1: no such sequence
    int fork(int seq) {
        auto it = seqs_.find(seq);
        if (it == seqs_.end()) return -1;
        const Seq copy = it->second;
        for (uint32_t p : copy.pages) ++count_[p];
        const int id = next_id_++;
        seqs_[id] = copy;
        return id;
    }

    bool release(int seq) {
        auto it = seqs_.find(seq);
        if (it == seqs_.end()) return false;
        for (uint32_t p : it->second.pages)
            if (--count_[p] == 0) free_.push_back(p);
        seqs_.erase(it);
        return true;
    }

    size_t pages_free() const { return free_.size(); }
    size_t pages_in_use() const { return count_.size() - free_.size(); }
    uint32_t ref_count(uint32_t page) const { return page < count_.size() ? count_[page] : 0; }
    const std::map<int, Seq> &sequences() const { return seqs_; }

  private:
    uint32_t take() {
        const uint32_t p = free_.back();
        free_.pop_back();
        count_[p] = 1;
        return p;
    }
    std::vector<uint32_t> count_, free_;
    std::map<int, Seq> seqs_;
    int next_id_ = 0;
};

}  // namespace bitnet_host
