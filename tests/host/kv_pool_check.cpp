// kv_pool_check.cpp -- stand-alone checker of host/kv_pool.hpp (its own main; tests/test_kv_pool.py builds it with the sanitizers and runs it).
// A seeded random sequence of create / reserve / fork / release against a dictionary model (sequence id -> page ids); after every operation
// the reference counts equal the table entries that name each page, in use + free = the pool, and a refused operation changed nothing.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "kv_pool.hpp"

using bitnet_host::PagePool;

#define CHECK(c) \
    if (!(c)) std::fprintf(stderr, "kv_pool_check:%d: %s\n", __LINE__, #c), std::exit(1)

static void audit(const PagePool &pool, const std::map<int, std::vector<uint32_t>> &model, uint32_t n_pages) {
    std::vector<uint32_t> named(n_pages, 0);
    CHECK(pool.sequences().size() == model.size());
    for (const auto &kv : model) {
        const PagePool::Seq *s = pool.find(kv.first);
        CHECK(s && s->pages == kv.second);
        CHECK((size_t)(s->n + 63) / 64 <= s->pages.size());
        for (uint32_t p : kv.second) {
            CHECK(p < n_pages);
            ++named[p];
        }
    }
    size_t used = 0;
    for (uint32_t p = 0; p < n_pages; ++p) {
        CHECK(pool.ref_count(p) == named[p]);  // the counts sum to the table entries, page by page
        used += named[p] != 0;
    }
    CHECK(pool.pages_in_use() == used && pool.pages_free() == n_pages - used);
}

static void sweep(uint32_t n_pages, unsigned seed, int n_ops) {
    PagePool pool(n_pages);
    std::map<int, std::vector<uint32_t>> model;
    std::mt19937 rng(seed);
    auto pick = [&]() {
        auto it = model.begin();
        std::advance(it, rng() % model.size());
        return it->first;
    };
    for (int op = 0; op < n_ops; ++op) {
        const unsigned what = rng() % 10;
        if (model.empty() || what == 0) {
            const int id = pool.create();
            CHECK(!model.count(id));
            model[id] = {};
        } else if (what <= 5) {  // reserve: grow by up to three pages, or ask for the page the sequence already has
            const int id = pick();
            std::vector<uint32_t> &m = model[id];
            const int upto = (int)(m.size() * 64) + (int)(rng() % 200) - 64;
            const size_t free_before = pool.pages_free();
            const size_t want = upto < 0 ? 0 : (size_t)upto / 64 + 1, fresh = want > m.size() ? want - m.size() : 0;
            const bool shared = want > 0 && fresh == 0 && pool.ref_count(m[want - 1]) > 1;  // before the call
            const PagePool::Reserve r = pool.reserve(id, upto);
            if (upto < 0) {
                CHECK(!r.ok);
            } else if (!r.ok) {
                CHECK(fresh + (shared ? 1 : 0) > free_before);  // refused only for want of pages (the audit below: nothing changed)
            } else {
                CHECK(fresh + (shared ? 1 : 0) <= free_before && r.copy == shared && r.grew == (fresh > 0 || shared));
                for (size_t i = 0; i < fresh; ++i) {
                    const uint32_t p = pool.find(id)->pages[m.size()];
                    CHECK(pool.ref_count(p) == 1);  // a page handed out was free
                    m.push_back(p);
                }
                if (r.copy) {
                    CHECK(r.src == m[want - 1] && r.dst != r.src);
                    m[want - 1] = r.dst;
                }
                CHECK(pool.ref_count(m[want - 1]) == 1);  // the page of the next append is private
                CHECK(free_before - pool.pages_free() == fresh + (r.copy ? 1 : 0));
                CHECK(pool.find(id)->n > upto);
            }
        } else if (what <= 7) {
            const int id = pick(), child = pool.fork(id);
            CHECK(child >= 0 && !model.count(child));
            model[child] = model[id];
        } else {
            const int id = pick();
            CHECK(pool.release(id));
            model.erase(id);
            CHECK(!pool.release(id) && pool.fork(id) == -1 && !pool.reserve(id, 0).ok);
        }
        audit(pool, model, n_pages);
    }
    while (!model.empty()) {
        CHECK(pool.release(model.begin()->first));
        model.erase(model.begin());
    }
    audit(pool, model, n_pages);
    CHECK(pool.pages_free() == n_pages && pool.pages_in_use() == 0);
}

int main() {
    sweep(1, 1, 300);
    sweep(7, 2, 3000);
    sweep(64, 3, 6000);
    std::puts("kv_pool_check: ok");
    return 0;
}
