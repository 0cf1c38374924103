// kv_paged.hpp -- the PAGED form of the KV cache, stated once: the index arithmetic every kernel that touches a page pool shares (the
// attention's split rule has its own header, paged_splits.hpp).  Integer arithmetic only, host and device, like kv_layout.hpp (which this file leaves as it is).
//
// A POOL is one layer's K or V storage for every sequence: n_pages PAGES of 64 positions.  A page id selects the same 64 positions in every
// layer's K pool and V pool.  In 32-bit words, R = kv_rows(f16) per position and head:
//   K page  [n_kv][R][64]    V page  [n_kv][64][R]
// so the (KV head, 64-position chunk) TILE inside a page is byte for byte the tile of kv_layout.hpp's contiguous cache: R * 64 contiguous words,
// position-fastest for K, dimension-fastest for V.  Where the contiguous cache has a head's chunk at kv_chunk_words(chunk, R), the pool has it at
// kv_page_tile_words(table[chunk], kvh, n_kv, R): a new base address per chunk and no new element order.
// A SEQUENCE is a device array uint32_t table[kv_table_entries(max_pos)] of page ids plus its position; entries past the page of the position
// are never read.  A page id >= n_pages inside the context makes the sequence idle in the attention and is skipped by the movers: the table is
// device memory, so only the kernels can check it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "kv_layout.hpp"

namespace bitnet_hip {

// words of one page (all KV heads)
__host__ __device__ constexpr size_t kv_page_words(size_t n_kv, size_t rows) { return n_kv * rows * kKvChunk; }
// words before the tile of KV head kvh in page `page`
__host__ __device__ constexpr size_t kv_page_tile_words(size_t page, size_t kvh, size_t n_kv, size_t rows) { return (page * n_kv + kvh) * rows * kKvChunk; }
// entries of a sequence's page table
__host__ __device__ constexpr size_t kv_table_entries(size_t max_pos) { return (max_pos + kKvChunk - 1) / kKvChunk; }

}  // namespace bitnet_hip
