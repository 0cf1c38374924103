// paged_shared_splits.hpp -- how many workgroups share one (fork group, KV head) of the shared-page pass (kernels_pagedshared.hip) when the caller
// leaves the choice to the library.  A pure host function, the sibling of paged_splits.hpp; plain C++, no HIP.
//
//   fill            = ceil(kPagedTargetWgs / (n_groups * n_kv))   splits that bring the grid to about two workgroups per CU
//   n_shared_splits = min(shared_pages, kPagedMaxAutoSplits, fill), at least 1
// One group of 64 forks over 4096 shared positions and 5 KV heads: min(64, 16, 103) = 16 workgroups per head, 4 pages each.  Every split costs
// each member one more record in the merge, so the cap is the one of the private splits.
#pragma once

#include <cstddef>

#include "paged_splits.hpp"

namespace bitnet_hip {

// shared_pages: the longest shared run of the launch
inline size_t attn_paged_shared_auto_splits(size_t n_groups, size_t n_kv_heads, size_t shared_pages) {
    if (n_groups == 0 || n_groups > 64 || n_kv_heads == 0 || n_kv_heads > 65535 || shared_pages == 0) return 0;  // nothing shared, or what the launch refuses
    const size_t base = n_groups * n_kv_heads;
    size_t n = (kPagedTargetWgs + base - 1) / base;
    if (n > kPagedMaxAutoSplits) n = kPagedMaxAutoSplits;
    if (n > shared_pages) n = shared_pages;
    return n < 1 ? 1 : n;
}

}  // namespace bitnet_hip
