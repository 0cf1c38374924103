// dev_buffer_check.cpp -- host/dev_buffer.hpp against a fake HIP runtime, on the CPU (tests/test_dev_buffer.py builds and runs it under the
// address and undefined-behaviour sanitizers).  The fake is malloc / free with counters: live blocks, live bytes, high-water bytes, "fail the
// n-th allocation from now".  Every property is asserted here, with the counts: the exit-time leak report is not relied on.
#include "dev_buffer.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>

namespace {
std::map<void *, size_t> g_blocks;  // live blocks of the fake device
size_t g_live = 0, g_high = 0, g_frees = 0;
int g_fail_in = 0;  // > 0: that many allocations from now, the last of them fails
int g_failed = 0;
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes);
    g_blocks[*p] = bytes;
    g_live += bytes;
    g_high = g_live > g_high ? g_live : g_high;
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    if (!p) return hipSuccess;
    const auto it = g_blocks.find(p);
    if (it == g_blocks.end()) {
        fprintf(stderr, "hipFree of a pointer that is not a live block (double free, or a borrowed pointer freed)\n");
        abort();
    }
    g_live -= it->second;
    g_blocks.erase(it);
    ++g_frees;
    free(p);
    return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t bytes) {
    memset(p, v, bytes);  // out of the block's bounds: the address sanitizer reports it
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t) { return hipMemset(p, v, bytes); }
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

using bitnet_host::dev_bytes_live;
using bitnet_host::DevBuf;
using bitnet_host::DevMem;
using bitnet_host::release_all;

// the counter of the type and the fake's own count, together, after every step
#define LIVE(bytes, blocks) CHECK(dev_bytes_live.load() == (uint64_t)(bytes) && g_live == (size_t)(bytes) && g_blocks.size() == (size_t)(blocks))

int main() {
    LIVE(0, 0);
    {  // alloc, and alloc over a held buffer: the old block goes first
        DevBuf<float> a;
        CHECK(a.get() == nullptr && !a);
        CHECK(a.alloc(10) == hipSuccess && a.get() != nullptr);
        LIVE(40, 1);
        float *first = a;  // the implicit conversion
        CHECK(first == a.get() && a + 3 == first + 3);
        const size_t frees = g_frees;
        g_high = g_live;
        CHECK(a.alloc(100) == hipSuccess);
        CHECK(g_frees == frees + 1 && g_high == 400);  // freed before the new block was taken: never 40 + 400
        LIVE(400, 1);
        a.reset();
        CHECK(a.get() == nullptr);
        LIVE(0, 0);
        a.reset();  // twice is nothing
        LIVE(0, 0);
        CHECK(a.alloc(3) == hipSuccess);
        LIVE(12, 1);
    }  // the destructor frees
    LIVE(0, 0);
    {  // alloc(0) takes one byte; DevBuf<void> counts bytes; the zero-fill fills what was asked for
        DevBuf<int32_t> z;
        CHECK(z.alloc(0) == hipSuccess && z.get() != nullptr);
        LIVE(1, 1);
        DevBuf<void> v;
        CHECK(v.alloc(7) == hipSuccess);
        LIVE(8, 2);
        DevBuf<double> d;
        CHECK(d.alloc_zeroed(5) == hipSuccess);
        LIVE(48, 3);
        for (int i = 0; i < 5; ++i) CHECK(d[i] == 0.0);
        DevBuf<uint8_t> e;
        CHECK(e.alloc_zeroed_bytes(0) == hipSuccess);  // one byte held, none filled
        LIVE(49, 4);
    }
    LIVE(0, 0);
    {  // move leaves the source empty, and frees what the target held
        DevBuf<float> a, b;
        CHECK(a.alloc(4) == hipSuccess && b.alloc(8) == hipSuccess);
        float *pa = a;
        LIVE(48, 2);
        b = std::move(a);
        CHECK(a.get() == nullptr && b.get() == pa);
        LIVE(16, 1);
        DevBuf<float> c(std::move(b));
        CHECK(b.get() == nullptr && c.get() == pa);
        LIVE(16, 1);
        a.reset(), b.reset();  // the sources own nothing
        LIVE(16, 1);
    }
    LIVE(0, 0);
    {  // a borrowed pointer is never freed, can be pointed elsewhere, and the borrower may go before or after it borrowed
        DevBuf<float> owner, other;
        CHECK(owner.alloc(16) == hipSuccess && other.alloc(2) == hipSuccess);
        LIVE(72, 2);
        const size_t frees = g_frees;
        {
            DevBuf<float> view;
            view.borrow(owner);
            CHECK(view.get() == owner.get());
            LIVE(72, 2);
            view.borrow(other);  // re-borrowed: nothing freed
            CHECK(view.get() == other.get() && g_frees == frees);
            view.reset();
            CHECK(view.get() == nullptr && g_frees == frees);
            view.borrow(owner);
            DevBuf<float> moved(std::move(view));  // a moved view is still a view
            CHECK(moved.get() == owner.get());
        }
        CHECK(g_frees == frees);
        LIVE(72, 2);
        DevBuf<float> held;
        CHECK(held.alloc(1) == hipSuccess);
        LIVE(76, 3);
        held.borrow(owner);  // borrowing over an owned block frees the block
        CHECK(g_frees == frees + 1);
        LIVE(72, 2);
        CHECK(held.alloc(5) == hipSuccess && held.get() != owner.get());  // and allocating over a view leaves the viewed block alone
        LIVE(92, 3);
    }
    LIVE(0, 0);
    {  // a failed alloc leaves the buffer empty -- also when it held a block -- and the count where it belongs
        DevBuf<float> a;
        g_fail_in = 1;
        CHECK(a.alloc(10) == hipErrorOutOfMemory && a.get() == nullptr);
        LIVE(0, 0);
        CHECK(a.alloc(10) == hipSuccess);
        LIVE(40, 1);
        g_fail_in = 1;
        CHECK(a.alloc_zeroed(20) == hipErrorOutOfMemory && a.get() == nullptr);
        LIVE(0, 0);
    }
    LIVE(0, 0);
    {  // a group that grows: released as a whole, then allocated -- the peak is max(old, new), not old + new
        DevBuf<float> x;
        DevBuf<int32_t> y;
        DevBuf<void> w;
        CHECK(x.alloc(100) == hipSuccess && y.alloc(50) == hipSuccess && w.alloc(1000) == hipSuccess);
        const size_t old_total = 400 + 200 + 1000, new_total = 800 + 400 + 3000;
        LIVE(old_total, 3);
        g_high = g_live;
        release_all(x, y, w);
        CHECK(!x && !y && !w);
        LIVE(0, 0);
        CHECK(x.alloc(200) == hipSuccess && y.alloc(100) == hipSuccess && w.alloc(3000) == hipSuccess);
        LIVE(new_total, 3);
        CHECK(g_high == new_total);
        // ... and a growth that fails half way keeps what it got, owned: the next attempt starts clean, the destructor frees the rest
        g_high = g_live;
        release_all(x, y, w);
        g_fail_in = 2;
        CHECK(x.alloc(10) == hipSuccess && y.alloc(10) == hipErrorOutOfMemory);
        CHECK(x.get() && !y && !w);
        LIVE(40, 1);
        release_all(x, y, w);
        CHECK(x.alloc(1) == hipSuccess && y.alloc(1) == hipSuccess && w.alloc(1) == hipSuccess);
        LIVE(9, 3);
        CHECK(g_high == new_total);
    }
    LIVE(0, 0);
    {  // a table of differently typed buffers through the untyped base (BatchDecoder::ensure_buffers)
        DevBuf<float> f;
        DevBuf<void *> t;
        struct {
            DevMem *b;
            size_t bytes;
        } want[] = {{&f, 12}, {&t, 4 * sizeof(void *)}};
        for (auto &w : want) CHECK(w.b->alloc_zeroed_bytes(w.bytes) == hipSuccess);
        CHECK(f[2] == 0.f && t[3] == nullptr);
        LIVE(12 + 4 * sizeof(void *), 2);
    }
    LIVE(0, 0);
    if (g_failed) {
        fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("dev_buffer_check: ok\n");
    return 0;
}
