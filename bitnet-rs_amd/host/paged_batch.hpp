// paged_batch.hpp -- continuous batching over a PAGED KV cache: up to 64 sequences whose keys live in one pool of 64-position pages
// (include/bitnet_hip_paged.h) instead of 2 x n_layers caches of max_pos positions each.  The reference states the memory model in
// crates/bitnet-inference/src/kv_cache_optimized.rs (PagedKvCache); here the pool is device memory and the attention reads through page tables.
//
// A PagedBatch owns, on its root's device: the 2 x n_layers pools of n_pages pages, the PagePool that says which page is whose (kv_pool.hpp),
// one device page table per slot, and the attention's scratch.  Its members are decoders it creates itself: borrowers of the root's weights
// WITHOUT caches of their own (Decoder's no_cache switch) that keep history, position, logits row, sampler, tap and stop state -- member(slot)
// hands one out to set those up and to read last_logits() / history().  A member holding L positions occupies ceil(L / 64) pages; pages that
// forks share are counted once.
//
//   admit(slot, src, n)   the first n positions of an ordinary staging decoder `src` (prefilled the usual way) become the slot's sequence:
//                         ceil(n / 64) pages reserved, ONE bitnet_hip_kv_page_in_dev launch, and the sequence state taken over as
//                         Decoder::fork hands it to a destination (history[0 .. n], position n, forced count, a reset sampler).
//   fork(from, to)        slot `to` becomes a copy of slot `from` that SHARES every page: no key byte moves.  The first step of either
//                         copies the one page both would append to (copy-on-write), and only that one.
//   release(slot)         the member goes; pages nobody else names return to the pool.
//   extract(slot, dst)    ONE bitnet_hip_kv_page_out_dev launch into the ordinary decoder dst plus the state, as fork: the bridge back to
//                         PrefixCache, BeamSearch, shift and run().  The member stays.
//   open(slot)            seats an EMPTY member (position 0, no pages): the caller feeds its prompt through member(slot).
//   prefill(slots, n, ..) the listed members take n[i] of their fed tokens in ONE packed prompt forward whose every layer attends through
//                         bitnet_hip_attention_paged_prefill_dev: the new keys go straight into pages, the past is read from its pages.  Pages are
//                         reserved for all listed members or for none; at most ONE bitnet_hip_kv_page_copy_dev launch for members whose last page
//                         is shared; only changed tables are uploaded.  Each member ends as Decoder::prefill_packed leaves a member.  At position
//                         0 it is a prompt's prefill, later a chunk of one or the continuation of a fork.
//   step(n, digits)       reserves pages for n appends of every member (refused as a whole, nothing changed, when the pool is too small), at
//                         most ONE bitnet_hip_kv_page_copy_dev launch for the forks that diverge, a table upload only for tables that changed,
//                         then WideBatch's step: Decoder::wide_forward with AttnOp::Paged in every layer -- bitnet_hip_attention_decode_paged_dev
//                         in place of the rows attention -- and WideBatch's one-launch tails.
//   set_share(min_pages)  0 (the default): step as above.  >= 1: after its reservation and copy-on-write launch step finds the FORK GROUPS from the
//                         host page lists -- members with the same first page; the run is their longest common leading run of pages, capped at
//                         min over members of position >> 6; fewer than 2 members or a run below min_pages = ungrouped -- once for all n steps
//                         (only tail entries change while stepping), and every layer calls bitnet_hip_attention_decode_paged_shared_dev: the
//                         group's shared pages are read once per group.  With no group found the step is the default one.
// Not here: eviction, paged forms of shift / beam / the snapshot movers (extract is the bridge).  SINGLE-THREADED USE, as every batch of this layer.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "kv_pool.hpp"
#include "wide_batch.hpp"

namespace bitnet_host {

class PagedBatch {
  public:
    PagedBatch(Decoder &root, size_t n_pages, int n_slots);  // n_slots 1..BITNET_HIP_WIDE_MAX; the pools take the root's cache type
    ~PagedBatch();
    PagedBatch(const PagedBatch &) = delete;
    PagedBatch &operator=(const PagedBatch &) = delete;
    const std::string &error() const { return err_; }
    bool dead() const { return dead_; }
    // every refusal below leaves pool, tables and members as they were
    int admit(int slot, Decoder &src, int n);  // slot empty; src alive, on the root's weights, with caches of the pool's type; 1 <= n <= src.position()
    int fork(int from, int to);
    int release(int slot);
    int extract(int slot, Decoder &dst);  // dst as a destination of Decoder::fork
    int step(int n, int digits, float *elapsed_ms);
    int set_share(int min_pages);                        // refused when negative
    size_t shared_rows() const { return shared_rows_; }  // rows x layers the last step sent through the shared pass
    int open(int slot);
    int prefill(const int *slots, const int *n, int count, bool with_logits, int digits, float *elapsed_ms);
    Decoder *member(int slot) const { return slot >= 0 && slot < n_ ? slot_[slot] : nullptr; }
    size_t pages_in_use() const { return pool_ ? pool_->pages_in_use() : 0; }
    size_t pages_free() const { return pool_ ? pool_->pages_free() : 0; }
    size_t pool_bytes() const { return pool_bytes_; }  // device bytes of all 2 x n_layers pools

  private:
    int fail(const char *what);
    int fail_arg(const std::string &what);
    int check_slot(int slot, bool want_member);
    Decoder *new_member();
    int upload_table(int slot);
    int seat(int slot, Decoder *m, int seq);  // the member into the wide batch and the slot; on refusal both go
    int unseat(int slot, int rc);             // a runtime failure behind seat(): release(slot), the error text and rc kept
    int arrive(Decoder *dst, int n, const Decoder &from);  // fork's state hand-over behind what is queued on the root's stream
    bool dead_ = true;
    std::string err_;
    int n_ = 0;
    Decoder *root_ = nullptr;
    bool kv_f16_ = false;
    size_t n_pages_ = 0, chunks_ = 0, pool_bytes_ = 0;
    std::unique_ptr<PagePool> pool_;
    Decoder *slot_[BITNET_HIP_WIDE_MAX] = {};
    int seq_[BITNET_HIP_WIDE_MAX];
    std::vector<DevBuf<void>> kpool_, vpool_;
    std::vector<void *> pool_host_;          // [2 * n_layers]: K pools, then V pools
    DevBuf<void *> pool_dev_;                // the same on the device, for the movers
    DevBuf<uint32_t> tables_;                // [n_slots][chunks_]
    DevBuf<const uint32_t *> table_ptrs_;    // [BITNET_HIP_WIDE_MAX], row i = dense member i
    bool dense_stale_ = true;
    DevBuf<void> scratch_;
    PagedAttn attn_;
    int share_min_ = 0;
    size_t shared_rows_ = 0;
    std::vector<int32_t> leader_, shared_pages_;  // [BITNET_HIP_WIDE_MAX] over the dense rows
    std::vector<size_t> layer_rows_;              // [n_layers]
    void find_groups(const int *pos);             // fills leader_ / shared_pages_, points attn_ at them when a group exists
    std::unique_ptr<WideBatch> wide_;
};

}  // namespace bitnet_host

extern "C" {
void *bitnet_host_paged_batch_create(void *root, size_t n_pages, int n_slots);  // never NULL for a live root: a dead batch carries the error text
void bitnet_host_paged_batch_destroy(void *b);
const char *bitnet_host_paged_batch_error(void *b);
int bitnet_host_paged_batch_admit(void *b, int slot, void *src, int n);
int bitnet_host_paged_batch_fork(void *b, int from, int to);
int bitnet_host_paged_batch_release(void *b, int slot);
int bitnet_host_paged_batch_extract(void *b, int slot, void *dst);
int bitnet_host_paged_batch_step(void *b, int n, int digits, float *elapsed_ms);
int bitnet_host_paged_batch_open(void *b, int slot);
int bitnet_host_paged_batch_prefill(void *b, const int32_t *slots, const int32_t *n, int count, int with_logits, int digits, float *elapsed_ms);
void *bitnet_host_paged_batch_member(void *b, int slot);  // the slot's decoder with one reference MORE (bitnet_host_destroy drops it), or NULL
int bitnet_host_paged_batch_set_share(void *b, int min_pages);
int64_t bitnet_host_paged_batch_shared_rows(void *b);
int64_t bitnet_host_paged_batch_pages_in_use(void *b);
int64_t bitnet_host_paged_batch_pages_free(void *b);
uint64_t bitnet_host_paged_batch_pool_bytes(void *b);
// Decoder's no_cache switch on its own: a borrower of `owner` without KV caches (what a PagedBatch creates for its slots)
void *bitnet_host_create_shared_no_cache(void *owner);
}
