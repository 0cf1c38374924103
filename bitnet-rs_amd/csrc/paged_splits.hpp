// paged_splits.hpp -- how many workgroups share one (sequence, KV head) of the paged decode attention when the caller leaves the choice to the
// library.  A pure host function of (n_seq, n_kv_heads, key_bound); plain C++, no HIP, so a host program can compile it too.
//
//   pages    = ceil(key_bound / 64)                      the most pages a sequence of the launch can hold
//   fill     = ceil(kPagedTargetWgs / (n_seq * n_kv))    splits that bring the grid to about two workgroups per CU (256 CUs)
//   n_splits = min(pages, kPagedMaxAutoSplits, fill), at least 1
// 64 sequences x 5 KV heads already make 320 workgroups: 2 splits.  8 sequences x 5 heads at 4096 keys: 13.  The cap keeps the merge, which is
// serial in the split count, short beside the stream it follows.
#pragma once

#include <cstddef>

namespace bitnet_hip {

constexpr size_t kPagedTargetWgs = 512;
constexpr size_t kPagedMaxAutoSplits = 16;

inline size_t attn_paged_auto_splits(size_t n_seq, size_t n_kv_heads, size_t key_bound) {
    if (n_seq == 0 || n_seq > 64 || n_kv_heads == 0 || n_kv_heads > 65535 || key_bound == 0) return 0;  // what the launch refuses: no rule
    const size_t pages = (key_bound + 63) / 64, base = n_seq * n_kv_heads;
    size_t n = (kPagedTargetWgs + base - 1) / base;
    if (n > kPagedMaxAutoSplits) n = kPagedMaxAutoSplits;
    if (n > pages) n = pages;
    return n < 1 ? 1 : n;
}

}  // namespace bitnet_hip
