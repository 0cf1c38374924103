// wide_batch.hpp -- continuous batching over the WIDE decode step: up to 64 decoders held in slots, one matrix forward per step, and a tail of
// at most THREE launches per step however many members sample, record or carry stop criteria.
//
// Decoder::step_wide (decoder.hpp) is a call, not an object: every call validates its members, builds and uploads (2 * n_layers + 6) * 64
// pointers, and ends every step with one bitnet_hip_sample_dev per sampling member, one bitnet_hip_logprob_dev per tapped member and one
// bitnet_hip_stop_dev per member with criteria -- 59 us per member at 64 members (EXPERIMENTS.md 24), more than the forward itself.  A
// WideBatch is the held member set BatchDecoder (batch_decoder.hpp) is for 8 slots: the slots, the pointer tables, a 64-entry sampler table
// (bitnet_hip_sample_batch_create_wide), a 64-entry tap table (bitnet_hip_logprob_rows_dev) and the 64-entry stop table
// (bitnet_hip_stop_batch_*) live in the batch, and a step's tail behind bitnet_hip_pick_rows_dev is, in this order,
//     ONE bitnet_hip_sample_batch_dev   if any member samples,
//     ONE bitnet_hip_logprob_rows_dev   if any member's tap is on,
//     ONE bitnet_hip_stop_batch_dev     if any member has criteria;
// an all-greedy batch launches none of them.  Decoder::step_wide itself is unchanged, launch order included.
//
// THE CONTRACT.  The DENSE MEMBER LIST of a step is the occupied, un-parked slots in slot order.  After step(n) every member is BIT FOR BIT
// what Decoder::step_wide(the same dense list, n, digits) leaves on twin decoders: KV caches, history, position, forced count, last_logits(),
// sampler state (draws, chosen, Mirostat's mu, the grammar state), log-probability records and stop state.  The forward IS step_wide's
// (Decoder::wide_forward, given a tail); the tail's kernels run the single launches' bodies per entry, and no member's tail reads another's.
//
// THE DRIVER is the weights' owner (the members' root()), member or not: the logits matrix, the head's workspace, the attention scratch and the
// prompt buffers are the root's, allocated once, and do not move when the lowest slot empties.  The forward runs on the root's stream, its
// saturation_fallbacks() counts a repeated step, and the members' cache type travels with the attention operator (the root's own may differ).
//
// The tables are rewritten only when a slot changes, a member is parked or un-parked, or a member's sampler / tap / criteria differ from what
// the tables were built for (a signature compare per step, as BatchDecoder::sampling_sig); a step with nothing changed uploads nothing
// (table_writes()).  What a step still reads back is each dense member's position, for the overflow refusal and the attention's key bound.
//
// step_until() PARKS a member it finds stopped: the member stays in its slot, frozen and untouched, but leaves the dense list, so it stops
// costing a row.  THE DENSE ROW COUNT THEN CHANGES: the tokens of the members that go on are step_wide's of the SHORTER list -- the same
// arithmetic class, possibly other matmul tiles, hence not necessarily the bits the longer list would have produced.  set_slot() clears a
// slot's parked mark.  A member's stop object sits in one stop table at a time: a member with criteria belongs to one batch (of either kind)
// whose tables are live.
//
// ADMISSION of new requests into a running batch needs no code of its own:
//   1. feed() the newcomer's n prompt tokens;
//   2. ONE Decoder::prefill_packed over all newcomers with n > 1, n - 1 tokens each, with_logits = false: no head launch at all (a newcomer
//      with n == 1 is fed only);
//   3. set_slot() each newcomer.  The next step consumes the last prompt token and picks the first generated one.
// Single-threaded use, as Decoder and BatchDecoder.
#pragma once

#include <string>
#include <vector>

#include "decoder.hpp"

namespace bitnet_host {

class WideBatch {
  public:
    explicit WideBatch(int n_slots);  // 1..BITNET_HIP_WIDE_MAX
    ~WideBatch();
    WideBatch(const WideBatch &) = delete;
    WideBatch &operator=(const WideBatch &) = delete;
    const std::string &error() const { return err_; }
    bool dead() const { return dead_; }
    int n_slots() const { return n_; }
    // Puts `d` into slot b (replacing what is there) or clears it (d == nullptr), between steps.  step_wide's member rules: alive, the same
    // root() and the same kv_f16() as the other members, in no other slot of this batch.  Holds a reference on the member until the slot
    // changes.  Clears the slot's parked mark.  Refused with nothing changed.
    int set_slot(int b, Decoder *d);
    // n wide steps of the dense member list.  Refused as step_wide refuses, with nothing modified: n < 1, an empty dense list, model globals
    // not set, "KV cache overflow" if any member would pass max_pos - 1.  Synchronises before returning.
    int step(int n, int digits, float *elapsed_ms);
    // un-parked members with criteria that have not stopped yet (synchronises; 0 when no member has criteria)
    int live(int *out);
    // Queues `chunk` steps (the last chunk clipped), then ONE 4-byte read of the stop table's live counter; only when it says that somebody has
    // stopped are the un-parked members' 24-byte stop states read, one small copy each, to park every member found stopped; ends
    // when no un-parked member with criteria is live or max_steps steps are queued.  Members already stopped at entry are parked before the
    // first chunk.  *steps: the steps queued.  Members without criteria run every queued step.  Refuses a batch in which no member has criteria.
    int step_until(int max_steps, int chunk, int digits, int *steps, float *elapsed_ms);
    // sampling, tap and stop launches the last step() call issued (n per kind that is in the tail, 0 otherwise)
    void tail_launches(int out[3]) const;
    // uploads of a tail table or the pointer tables since creation
    int64_t table_writes() const { return table_writes_; }

  private:
    // what the tables were built for, per slot
    struct Sig {
        Decoder *d = nullptr;  // null: empty or parked -- no row, no tail entry
        void *kcache0 = nullptr;  // layer 0's K cache: set_kv_f16 on a member in its slot allocates the caches anew
        void *sampler = nullptr;
        bitnet_hip_logprob_args tap = {};
        bitnet_hip_stop *stop = nullptr;
    };
    int fail(const char *what);
    int fail_arg(const std::string &what);
    int ensure_tables();
    void drop_tables();
    void signature(std::vector<Sig> &out) const;
    int rebuild(const std::vector<Sig> &want);
    int read_stops(bool park, int *live);
    bool dead_ = false;
    std::string err_;
    int n_ = 0;
    Decoder *slot_[BITNET_HIP_WIDE_MAX] = {};
    bool parked_[BITNET_HIP_WIDE_MAX] = {};
    Decoder *root_ = nullptr;  // the driver; a reference is held from the first member's arrival until the last member leaves
    std::vector<Sig> sig_;     // what the device tables hold
    bool built_ = false;
    DevBuf<void *> tables_;    // wide_forward's layout, [2 * n_layers + 6][64], row i = dense member i
    bitnet_hip_sample_batch *sample_tab_ = nullptr;  // n_ entries by SLOT
    DevBuf<bitnet_hip_logprob_args> tap_tab_;        // n_ entries by slot
    std::vector<bitnet_hip_logprob_args> tap_dev_;   // ... and what they hold (a slot's entry outlives its member until the next rebuild)
    bitnet_hip_stop_batch *stop_tab_ = nullptr;      // n_ entries by slot
    int tail_[3] = {0, 0, 0};
    int64_t table_writes_ = 0;
};

}  // namespace bitnet_host

extern "C" {
void *bitnet_host_wide_batch_create(int n_slots);  // NULL for n_slots outside 1..64
void bitnet_host_wide_batch_destroy(void *b);
const char *bitnet_host_wide_batch_error(void *b);
int bitnet_host_wide_batch_set_slot(void *b, int slot, void *decoder);  // decoder NULL clears the slot
int bitnet_host_wide_batch_step(void *b, int n, int digits, float *elapsed_ms);
int bitnet_host_wide_batch_live(void *b);  // WideBatch::live, or a negative error code
int bitnet_host_wide_batch_step_until(void *b, int max_steps, int chunk, int digits, int *steps, float *elapsed_ms);
int bitnet_host_wide_batch_tail_launches(void *b, int *out3);
int64_t bitnet_host_wide_batch_table_writes(void *b);  // -1 for a null handle
}
