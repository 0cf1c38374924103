// batch_decoder.hpp -- one decode step for up to 8 live sequences through ONE launch chain.
//
// The reference's forward takes [B, T, H] and KVCache::new(config, batch_size, ..) carries a batch dimension
// (crates/bitnet-transformer/src/lib.rs:281, :1146-1160, :1215-1245, :1437-1478): a lock-step batch.  Here a slot holds a Decoder -- an owner
// or decoders borrowing its weights (Decoder(owner), bitnet_host_create_shared) -- and every occupied slot takes a with-logits decode step
// together, each at its OWN position: embed -> per layer q|k|v, attention, o, gate|up, down -> head -> pick, on the batched entry points
// (bitnet_hip_*_batch_dev) in Decoder::step_launches' QAct order.  A batch-1 step is ~155 dependent launches whose cost is the launch
// (EXPERIMENTS.md 4.1); the batch pays them once for all its members, and reads every weight matrix once.
//
// After step(n) every member is in the state its own run(n, with_logits = true) would have left under attention form 0
// (Decoder::set_attention_form(0)): KV caches, history, position, forced count, last_logits() and sampler state, BIT FOR BIT -- the batched
// kernels restate the batch-1 arithmetic per vector.  Forced tokens are honoured as in run(), so a feed() between steps works.  NOT
// maintained: last_hidden() (the residual stream lives in the batch's own buffers).
//
// Scheduling is set_slot(): members join and leave between steps (continuous batching); prompts go through the member's own prefill / extend
// before it joins -- or through ONE Decoder::prefill_packed for up to 64 members at once, each at its own position with its own number of new tokens
// (members already sitting in slots included) -- or the member takes over a live sequence's prefix (Decoder::fork: one copy launch for up to 8 members).  The step is ONE linear chain on one stream (no forked capture branches), captured once per batch: slot changes rewrite the
// device pointer tables the kernels read and need no re-capture.  Sampling goes the same way: a sampling member gets logits only from the head, and
// ONE bitnet_hip_sample_batch_dev launch after it serves every sampling member through a device table of per-slot sampler state (an empty
// entry: nothing to do), so a member switching its sampling on or off, a sampling member leaving or a greedy one taking its place re-captures
// nothing.  That launch joins the chain at the first step at which any member samples -- the one re-capture sampling can cost, once in a
// batch's life; a batch that never had a sampling member launches the chain without it.  The logits tap (Decoder::set_logprobs) goes the same
// way again: the members' bitnet_hip_logprob_args form one more device table (a member with logprobs off, or an empty slot: an empty entry),
// ONE bitnet_hip_logprob_batch_dev launch follows the head and the sampling launch, and it joins the chain at the first step at which any
// member has logprobs on -- one re-capture, once; from then on members switching, joining or leaving re-capture nothing, and a batch that never
// had such a member runs the chain it always ran.  After step(n) a member's records are bit for bit those of its own run(n) under
// set_attention_form(0).  Single-threaded use.
#pragma once

#include <string>
#include <vector>

#include "decoder.hpp"

namespace bitnet_host {

class BatchDecoder {
  public:
    explicit BatchDecoder(int n_slots);
    ~BatchDecoder();
    BatchDecoder(const BatchDecoder &) = delete;
    BatchDecoder &operator=(const BatchDecoder &) = delete;
    const std::string &error() const { return err_; }
    bool dead() const { return dead_; }
    int n_slots() const { return n_; }
    Decoder *member(int b) const { return b >= 0 && b < n_ ? slot_[b] : nullptr; }  // what slot b holds (BeamSearch binds to the first n_beams)
    void *stream() const { return stream_; }                                        // the stream every step runs on
    // Puts `d` into slot b (replacing what is there) or clears it (d == nullptr).  Every member: the same owner (or the owner itself), the
    // same KV type, on the QAct path, in no other slot.  Holds a reference on the member until the slot changes.
    int set_slot(int b, Decoder *d);
    // n with-logits steps for every occupied slot.  Refuses with "KV cache overflow" if any member would pass max_pos - 1 (positions are read
    // once, before the first launch).  Synchronises before returning.
    int step(int n, bool use_graph, float *elapsed_ms);
    // Members with stop criteria (Decoder::set_stop): the batch owns a stop table (bitnet_hip_stop_batch_*), binds each such member's object to
    // its slot, and the chain gains ONE bitnet_hip_stop_batch_dev launch behind the sampling and logprob launches -- from the first step at which
    // a member has criteria on, as the sampling launch joins the chain.  A stopped member stays frozen in its slot and keeps costing its row
    // until the scheduler takes it out.
    // live(): members with criteria that have not stopped yet (synchronises; 0 when no member has criteria).
    int live(int *out);
    // step(chunk) until no member with criteria is live or max_steps steps are queued (the last chunk clipped); one 4-byte read per chunk.
    // *steps: the steps queued.  Refuses a batch in which no member has criteria.  Members without criteria simply run every queued step.
    int step_until(int max_steps, int chunk, int *steps, float *elapsed_ms);
    int captures() const { return captures_; }  // graph captures so far
    int graph_nodes() const;                    // kernel nodes of the captured chain, 0 if none is held

  private:
    int fail(const char *what);
    int fail_arg(const std::string &what);
    int ensure_buffers();
    int upload_tables();
    int bind_sampler(int b, Decoder *d);
    int bind_stops();  // the stop table follows its members' criteria
    int launches(bool warm = false);  // warm: the pass over all-idle tables that ensure_buffers runs once
    int clear_vectors(int b);
    void drop_graph();
    bool dead_ = false;
    std::string err_;
    int n_ = 0;
    Decoder *slot_[BITNET_HIP_BATCH_MAX] = {};
    Decoder *root_ = nullptr;  // whose weights the batch runs on (a reference is held from the first member on)
    bool kv_f16_ = false;
    void *stream_ = nullptr;
    // device pointer tables, [row][n_] pointers each: rows 0..5 = embed/attention positions, histories, logits rows, pick tokens, pick positions,
    // pick histories, forced counts (row 6), then per layer K caches and V caches
    DevBuf<void *> tables_;
    std::vector<void *> host_tables_;
    bool tables_dirty_ = true;
    DevBuf<float> x_, x2_, qkv_, attn_scratch_;
    DevBuf<void> qa_x_, qa_x2_, qa_att_, qa_h_, scratch_;
    DevBuf<double> st_x_, st_x2_;
    int logits_wgs_ = 512;
    void *graph_ = nullptr, *graph_exec_ = nullptr;
    std::vector<void *> sampling_sig() const;  // per slot the sampler of a sampling member (null: fused greedy pick, or empty) ...
    std::vector<void *> tables_sig_;           // ... and the one the uploaded pick and sampling tables were built for
    bitnet_hip_sample_batch *sample_tab_ = nullptr;  // n_ entries, one launch (bitnet_hip_sample_batch_dev)
    void *bound_[BITNET_HIP_BATCH_MAX] = {};         // the sampler each of its entries holds
    bool sample_in_chain_ = false;  // some member has sampled: the sampling launch is part of every step from then on
    bool graph_sig_ = false;        // ... and whether the captured chain has it
    DevBuf<bitnet_hip_logprob_args> lp_table_;                // device: [n_] entries, one launch (bitnet_hip_logprob_batch_dev)
    bitnet_hip_logprob_args lp_host_[BITNET_HIP_BATCH_MAX] = {};  // what it holds
    bool lp_in_chain_ = false;      // some member has had logprobs on: the logprob launch is part of every step from then on
    bool graph_lp_sig_ = false;     // ... and whether the captured chain has it
    bitnet_hip_stop_batch *stop_tab_ = nullptr;          // n_ entries, one launch (bitnet_hip_stop_batch_dev)
    bitnet_hip_stop *stop_bound_[BITNET_HIP_BATCH_MAX] = {};  // the object each of its entries holds
    bool stop_in_chain_ = false;    // some member has had criteria: the stop launch is part of every step from then on
    bool graph_stop_sig_ = false;   // ... and whether the captured chain has it
    int captures_ = 0;
};

}  // namespace bitnet_host

extern "C" {
void *bitnet_host_batch_create(int n_slots);
void bitnet_host_batch_destroy(void *b);
const char *bitnet_host_batch_error(void *b);
int bitnet_host_batch_set_slot(void *b, int slot, void *decoder);  // decoder NULL clears the slot
int bitnet_host_batch_step(void *b, int n, int use_graph, float *elapsed_ms);
int bitnet_host_batch_live(void *b);         // BatchDecoder::live, or a negative error code
int bitnet_host_batch_step_until(void *b, int max_steps, int chunk, int *steps, float *elapsed_ms);  // BatchDecoder::step_until
int bitnet_host_batch_captures(void *b);     // graph captures so far
int bitnet_host_batch_graph_nodes(void *b);  // kernel nodes of the captured chain, 0 if none
}
