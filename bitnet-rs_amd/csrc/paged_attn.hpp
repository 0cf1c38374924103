// paged_attn.hpp -- what kernels_kvpaged.hip (k_attn_paged, the paged decode attention) lends kernels_pagedshared.hip (the shared-page pass in front
// of it): the record format, the kernel's arguments, the entry's refusals and the launch.  k_attn_paged has ONE body; the shared entry runs it as
// its suffix pass through attn_paged_launch with an AttnPagedLead.
#pragma once

#include <cstddef>
#include <cstdint>

#include "common.hpp"
#include "kv_layout.hpp"

namespace bitnet_hip {

constexpr int kPgMaxGroup = 4;
constexpr int kPgD = kKvDim;
constexpr int kPgRec = kAttnRecFloats;  // (m, l)[4], o[4][128]
constexpr size_t kPgTicketWords = (size_t)kWideMax;  // arrival counters per KV head, whatever n_seq is: one scratch serves every batch size
static_assert(kPgRec == 2 * kPgMaxGroup + kPgMaxGroup * kPgD, "record layout");
static_assert(kPgRec * sizeof(float) % 16 == 0, "records stay 16-byte aligned");

struct AttnPagedArgs {
    const float *qkv, *rope_sin, *rope_cos;
    uint32_t *kpool, *vpool;
    const uint32_t *const *tables;
    const int *const *pos_ptrs;
    uint32_t *tickets;  // [kWideMax][n_kv]
    float *records;     // [n_seq][n_kv][n_splits][kPgRec]
    float *out;         // one of the two
    _Float16 *out_h;
    unsigned n_pages;
    int n_heads, n_kv, group, key_bound, n_splits;
};

// The suffix form of the launch: sequence b walks chunks first[b], first[b] + n_splits, ... (clamped to the page of its position, so the append
// always happens) and, where first[b] > 0, its merge starts with the n_lead records [b][kvh][0 .. n_lead) of `records` in index order.
struct AttnPagedLead {
    const float *records;  // [n_seq][n_kv][n_lead][kPgRec], written by an earlier launch of the stream
    int n_lead;
    int first[kWideMax];
};

// every refusal of bitnet_hip_attention_decode_paged_dev, then the argument fill; *n_splits 0 is resolved by the library's rule
int attn_paged_front(const char *entry, const float *qkv, const float *rope_sin, const float *rope_cos, void *kpool, void *vpool, size_t n_pages,
                     const uint32_t *const *table_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq, size_t n_heads, size_t n_kv_heads, size_t head_dim,
                     size_t max_pos, size_t key_bound, size_t *n_splits, void *scratch, int flags, void *out, AttnPagedArgs *a);
// lead == nullptr: today's launch
hipError_t attn_paged_launch(bool f16, const AttnPagedArgs &a, const AttnPagedLead *lead, size_t n_seq, hipStream_t stream);

}  // namespace bitnet_hip
