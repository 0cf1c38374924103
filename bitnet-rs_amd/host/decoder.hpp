// decoder.hpp -- host-side decode loop over the C ABI (include/bitnet_hip.h).
//
// The reference keeps the autoregressive loop in host code (Rust) and calls kernels:
//   TransformerModel::{embed, forward, logits}   crates/bitnet-transformer/src/lib.rs:1390, 1557, 1599
//   TransformerBlock::forward                    :977-1134
//   KVCache / LayerKVCache                       :1138-1256
//   greedy loop                                  crates/bitnet-cli/src/main.rs:1282-1477
//   parity entry points                          crates/bitnet-inference/src/parity.rs:30-111,157-223
// Rust is not available in this build environment, so this is the same structure in
// C++: it owns no arithmetic, only buffers, the launch order and a captured hipGraph
// per decode step.  Everything it launches goes through bitnet_hip_* entry points.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "bitnet_hip.h"
#include "dev_buffer.hpp"

extern "C" {
// The collective of the token-parallel prefill as the host supplies it: gather `bytes_per_rank` bytes from every rank into
// recv ([world][bytes_per_rank], rank order), ordered on `stream` (a hipStream_t) like a kernel launch.  0 = success.
typedef int (*bitnet_host_allgather_fn)(void *ctx, const void *send_dev, void *recv_dev, size_t bytes_per_rank, void *stream);
}

namespace bitnet_host {

// ModelConfig fields the path needs (crates/bitnet-common/src/config.rs:25-46; GGUF keys
// crates/bitnet-models/src/gguf_simple.rs:646-777).
struct Config {
    int hidden = 2560, n_layers = 30, n_heads = 20, n_kv_heads = 5, head_dim = 128;
    int ffn = 6912, vocab = 128256, max_pos = 4096;
    float eps = 1e-5f;          // rms_norm_eps, default 1e-5 (T:957)
    float rope_theta = 10000.f;  // DEFAULT_ROPE_BASE (crates/bitnet-rope/src/lib.rs:11)
};

// One layer's host-side weights in the reference's layouts.
struct LayerWeightsQk256 {
    const float *attn_norm, *ffn_norm;                       // [hidden]
    const uint8_t *q, *k, *v, *o, *gate, *up, *down;         // QK256 bytes [out, ceil(in/256)*64]
};
// Ternary I2_S with f32 block scales (K/cpu/quantized_matmul.rs:47-56).
struct LayerWeightsI2s {
    const float *attn_norm, *ffn_norm;
    const uint8_t *w[7];      // q,k,v,o,gate,up,down: [out, in/4]
    const float *scales[7];   // [out, in/block]
    size_t block_size;
};

// One projection as a loader hands it over: QK256 bytes, or 2-bit codes + f32 block scales
// with an explicit code map (bitnet_hip_weights_upload_coded).
struct ProjSpec {
    bool qk256 = true;
    const uint8_t *bytes = nullptr;
    size_t len = 0;
    const float *scales = nullptr;  // coded only: [rows, cols / block]
    size_t n_scales = 0, block = 32;
    int8_t code_map[4] = {-2, -1, 0, 1};
};

// A decoder's streams and events, as a BASE of Decoder: bases go after members, so every DevBuf member is freed before its streams are destroyed.
struct DecoderStreams {
    void *stream_ = nullptr;
    void *comm_stream_ = nullptr, *sp_ev_pack_ = nullptr, *sp_ev_gather_ = nullptr;  // the all-gather's own stream and its two ties to the compute stream
    std::vector<void *> sp_tev_;                                                     // the sharded prefill's timing events (set_phase_timing)
    ~DecoderStreams();
};

class PrefixCache;  // prefix_cache.hpp
class WideBatch;    // wide_batch.hpp

// The tail of a wide step when a WideBatch drives it (Decoder::wide_forward): the device pointer tables in wide_forward's own layout, built and
// uploaded by the batch for its dense member list, and the three tail tables -- each launched ONCE per step behind bitnet_hip_pick_rows_dev, in
// this order, or not at all when null.  launches[]: the launches issued, counted up by wide_forward.
struct WideTail {
    void *const *tables = nullptr;                   // [2 * n_layers + 6][BITNET_HIP_WIDE_MAX]
    bitnet_hip_sample_batch *sample = nullptr;       // bitnet_hip_sample_batch_dev: some member samples
    const bitnet_hip_logprob_args *taps = nullptr;   // bitnet_hip_logprob_rows_dev over n_taps entries: some member's tap is on
    size_t n_taps = 0;
    bitnet_hip_stop_batch *stop = nullptr;           // bitnet_hip_stop_batch_dev: some member has criteria
    int launches[3] = {0, 0, 0};
};

class Decoder : private DecoderStreams {
    friend class PrefixCache;  // saves from and restores into the caches, history and counters exactly as fork does
    friend class WideBatch;    // holds members in slots and drives wide_forward on their root with a tail of its own

  public:
    explicit Decoder(const Config &cfg) : Decoder(cfg, true) {}
    ~Decoder();
    Decoder(const Decoder &) = delete;
    Decoder &operator=(const Decoder &) = delete;

    // A decoder that BORROWS the owner's weights: the owner's configuration, its weight handles, norm vectors, embedding table and final norm
    // (the same device pointers: bitnet_hip_weights_bind_ln binds a handle to ONE gamma pointer), and everything else its own -- KV caches,
    // history, position, sampler, stream, graphs, prompt buffers.  Several conversations then share one copy of the weights (the reference
    // gives its KVCache a batch dimension instead, T:1146-1160).  The owner must hold every layer and the globals already.  A borrower refuses
    // set_layer_*, set_globals (hence load_gguf) and set_act_mode; the owner refuses set_layer_* / set_globals while borrowers exist.  The
    // owner must outlive its borrowers: the C shim's reference count sees to that (bitnet_host_destroy defers).  SINGLE-THREADED USE: an owner,
    // its borrowers and a batch that holds them are driven from one host thread.
    Decoder(Decoder &owner, int);
    Decoder *owner() const { return owner_; }
    Decoder *root() { return owner_ ? owner_ : this; }
    int borrowers() const { return borrowers_; }
    // the C shim's intrusive reference count (bitnet_host_destroy, BatchDecoder slots, borrowers of an owner)
    int refs_ = 1;
    void *batch_ = nullptr;  // the BatchDecoder whose slot holds this decoder, or null
    // -1 (default): the attention form follows the position (form_at); 0: 64-position records + combine at EVERY position -- the form the
    // batched step runs, so run() under form 0 gives the numbers a batch must reproduce (the merging o-projection and the wide form round
    // differently).  Drops nothing: graphs are kept per form.
    int set_attention_form(int form);
    // what a batch needs beside layer_objects / global_objects: {forced count, logits row, sampler (null until set_sampling)}
    // (a logits row that waits for its lazy recomputation -- see set_head_screen -- is brought up to date first: others will write it)
    void batch_objects(void *ptrs[3]);
    // The SCREENED greedy head (bitnet_hip_logits_screen_dev): on (default; env BITNET_HOST_HEAD_SCREEN=0 switches it off), a with-logits step
    // with sampling off, the logits tap off, no tracer and no batch slot picks its token through the int8 screening image of the embedding
    // table -- built on the device when set_globals fills the table, vocab * hidden + 8 * vocab bytes, the owner's for a borrower -- and
    // rescoring of the few rows the screen cannot exclude: the full head's token bit for bit, from half its bytes, and no logits vector.
    // last_logits() after such a step runs the full head once on the head input the screen saved: the bits the full head would have left.
    // Hidden sizes without a screening instance keep the full head.  Drops the captured graphs.
    int set_head_screen(bool on);
    bool head_screen() const { return screen_step(false); }  // would a plain greedy step take the screened head now?
    // device counters of this decoder's screened head: rows the last launch rescored, launches, rows rescored by all launches.  Synchronises.
    int head_screen_stats(uint32_t out[3]);
    bool sampling() const { return sampling_; }
    float eps() const { return c_.eps; }

    const Config &config() const { return c_; }
    const std::string &error() const { return err_; }
    bool dead() const { return dead_; }  // construction failed: only error() and the destructor may be used
    void set_error(const std::string &e) { err_ = e; }

    // weights (uploaded once; fused q|k|v and interleaved gate/up handles are built here)
    int set_layer_qk256(int layer, const LayerWeightsQk256 &w);
    int set_layer_i2s(int layer, const LayerWeightsI2s &w);
    // q,k,v,o,gate,up,down in any mix of storage forms (q|k|v and gate|up must agree)
    int set_layer_specs(int layer, const float *attn_norm, const float *ffn_norm, const ProjSpec p[7]);
    int set_globals(const uint16_t *embed_f16, const float *final_norm);

    // KVCache::clear (T:1251-1255) + token history (+ the sampler's counts and word counter)
    int reset();
    // The reference's Sampler (crates/bitnet-cli/src/sampling.rs) on the device, behind every with-logits step:
    // cfg == NULL = greedy argmax as before (same kernels, same tokens).  Switching on / off drops the captured graphs,
    // a new config on an existing sampler does not (the graphs read it from device memory).
    int set_sampling(const bitnet_hip_sampling_config *cfg);
    // the same with min-p, typical-p and the additive penalties (bitnet_hip_sampling_config_ex); set_sampling is this with neutral values
    int set_sampling_ex(const bitnet_hip_sampling_config_ex *cfg);
    // Mirostat v2 on this decoder's sampler (bitnet_hip_sampler_set_mirostat): needs sampling on; NULL = off.  Drops no graphs: the launch reads
    // the mode from device memory.  reset() restores mu = 2 * tau, rewind() and shift() leave it as they leave the counts, fork() resets each
    // destination's with its sampler.
    int set_mirostat(const bitnet_hip_mirostat_config *cfg);
    int mirostat_state(float *mu, uint64_t *fallbacks);  // synchronises; 0 / 0 without a sampler
    // Logit constraints on this decoder's sampler (bitnet_hip_sampler_set_constraints: logit bias, bans, an allowed set, an EOS hold-off, an
    // n-gram block): needs sampling on -- greedy decoding with constraints is set_sampling with temperature 0; NULL = off.  Drops no graphs: the
    // launch reaches the config through device memory.  The config belongs to this decoder.  reset() zeroes the count of chosen tokens, rewind()
    // and shift() leave it as they leave the counts, fork() resets each destination's with its sampler.
    int set_constraints(const bitnet_hip_constraints *cfg);
    int constraints_state(uint64_t *chosen);  // synchronises; 0 without a sampler
    // Grammar-constrained decoding on this decoder's sampler (bitnet_hip_sampler_set_grammar: a token automaton whose state moves with every
    // chosen token, on the device): needs sampling on -- greedy decoding under a grammar is set_sampling with temperature 0; NULL = off, a no-op
    // without a sampler.  Synchronises the stream before the copy and drops no graphs: the launch reaches the mode bit, the tables and the state
    // through device memory.  The handle stays the caller's and may serve many decoders (it counts its bindings).  reset() puts the state back
    // to `start`; rewind(), fork() and shift() do NOT move a sampler, so the state stays where the tokens since dropped left it: after rewind(n)
    // the caller sets it with set_grammar_state(the state bitnet_hip_grammar_walk gives for the generated tokens that remain).  C exports:
    // grammar_host.hpp.
    int set_grammar(bitnet_hip_grammar *g, int start);
    int set_grammar_state(int state);
    int grammar_state(int32_t *state, uint64_t *steps, uint64_t *violations);  // synchronises; -1 / 0 / 0 without a sampler or a grammar
    int sampling_draws(uint64_t *out);
    // The reference's logits tap on the generation path (GenerationConfig::{logits_tap_steps, logits_topk, logits_cb}, crates/bitnet-inference/src/
    // config.rs:87-93, engine.rs:1182-1210; the CLI's LogitStep records, crates/bitnet-cli/src/main.rs:1337-1373) on the device: top_n = -1 (default)
    // off, 0..BITNET_HIP_LOGPROB_TOP_MAX on.  On, every with-logits step appends ONE bitnet_hip_logprob_dev launch after the pick -- run, prefill /
    // extend / score / finish_prefill with logits -- which leaves record [position of the token just placed]: that token (chosen, or forced: echo
    // log-probabilities), its raw logit, the row's log-sum-exp and the top_n (id, logit) pairs; a prompt of n tokens with logits leaves record n.
    // Steps without logits, run_reference and trace_step record nothing.  Switching on allocates max_pos records (cleared to 0xFF bytes: token
    // -1 = never written) and the kernel's scratch, once.  Switching on or off, or another top_n, drops the captured graphs as set_sampling does;
    // off, the step is launch for launch what it was.  reset() clears the records, rewind() leaves them, fork() clears those of every destination
    // that has them (a destination's log-probabilities start at the fork point; the source is untouched).
    int set_logprobs(int top_n);
    int logprob_top_n() const { return lp_top_n_; }
    // Synchronises and copies records [first, first + n) to the host.  Refuses a range outside [0, max_pos) and a decoder with logprobs off.
    int logprobs(int first, int n, bitnet_hip_logprob_record *out);
    // what a batch binds for this member: its bitnet_hip_logprob_args, an empty entry (null records) with logprobs off
    void logprob_entry(bitnet_hip_logprob_args *out) const;
    // STOP CRITERIA on the device (bitnet_hip_stop_*, include/bitnet_hip.h): stop token ids, EOS, a token budget and stop sequences of token ids,
    // the reference's StopCriteria / check_stop (crates/bitnet-generation/src/lib.rs:119-144) and should_stop (crates/bitnet-inference/src/
    // engine.rs:1315-1348).  cfg == NULL: off.  On, pick_token() issues ONE bitnet_hip_stop_dev launch behind the pick and the logits tap -- in
    // run, prefill, extend, finish_prefill (so a first token that is already EOS stops), step_wide and prefill_packed -- which decides whether the
    // token just placed ends the sequence and from then on holds the sequence FROZEN through every step already queued: the position goes back
    // to the stop position, the device's forced count says "everything is forced", so no pick writes the history and the sampler's counts, word
    // counter and Mirostat's mu stay where the stop token left them.  A frozen step consumes the stop token at slot `position` again and
    // rewrites that one cache slot with the same bytes; history entries and cache slots beyond `position` keep what they held.
    // Switching on or off drops the captured graphs, as set_logprobs does; a new config on a decoder that has criteria does not (the launch
    // reads it from device memory).  Off, the launch sequence is exactly what it was (graph_nodes()).
    // set_stop, feed and reset arm fully, for a new request (count 0); rewind and shift clear the stop and the window and keep the count; a
    // fork destination carries no stop state (it is armed fully if it has criteria of its own).
    // After a stop with frozen_steps > 0, last_logits() and last_hidden() are those of the last frozen step -- the step that consumes the
    // stop token at slot `position`, under the attention form run() had queued for that step: what the first step of a resumed generation
    // computes, bit for bit while the form is the same.  With frozen_steps == 0 they are the stopping step's.
    int set_stop(const bitnet_hip_stop_config *cfg);
    bool stop_on() const { return stop_on_; }
    bitnet_hip_stop *stop_object() const { return stop_on_ ? stop_ : nullptr; }  // what a batch binds for this member
    int stop_state(bitnet_hip_stop_state *out);  // synchronises; refuses a decoder without criteria
    // Go on after a stop (or re-open the window of a running sequence): arms with the count kept -- a budget then counts the whole request --
    // and writes the host's forced count back to the device.  The next run() consumes the stop token and generates behind it.
    int resume();
    // run(chunk) until the sequence has stopped or max_steps steps are queued (the last chunk is clipped); ONE 24-byte state read per chunk in
    // place of a token read per step.  *steps: the steps up to and including the stopping one (queued - frozen_steps), or the steps queued if
    // nothing stopped; elapsed_ms: the sum over the chunks.  A sequence that has stopped already returns at once with 0 steps.
    int run_until_stop(int max_steps, int chunk, int *steps, float *elapsed_ms);
    // kernel nodes of the step graph run() would launch at the current position (captured if need be), or a negative error code
    int graph_nodes(bool with_logits);
    // Put `n` forced tokens at positions [pos, pos+n) of the history (the prompt).
    int feed(const int32_t *tokens, int n);
    // Run `n` single-token steps (T:1482-1504 body each).  with_logits=false skips the
    // logits GEMV for prompt positions nobody samples from.  Uses the captured graph
    // when use_graph, else eager launches.  Synchronises the stream before returning.
    int run(int n, bool with_logits, bool use_graph, float *elapsed_ms);
    // The same n steps UNFUSED, in the reference's op order, every projection on the reference-order (bit-exact)
    // kernel: the checker bench.py and the tests hold the fast step against at the full model size.  Eager, slow.
    int run_reference(int n, bool with_logits);
    // Activations between the step's kernels: 1 (default) = quantised once by their producer ("QAct", include/bitnet_hip.h:
    // the f16-class activation north_star names), 0 = exact f32 (round 1's kernels).  Env BITNET_HOST_ACT sets the default.
    int set_act_mode(int mode);
    // Opt-in f16 KV cache (half the bytes of the long-context decode stream; the reference's cache is f32, T:1171-1202): k / v are
    // rounded once, when appended.  Only on a fresh sequence.  Env BITNET_HOST_KV16 sets the default.
    int set_kv_f16(bool on);
    bool kv_f16() const { return kv_f16_; }
    bool qact_path() const;  // mode 1 AND every layer's matrices are on that path
    // Whole-prompt forward on a fresh sequence (position() == 0): the first n fed tokens go
    // through every layer as [n, *] matrices (TransformerModel::forward with seq_len n,
    // T:1557-1597): tiled matmuls + causal attention, KV cache filled for positions 0..n-1.
    // with_logits samples the token after the prompt exactly as run() does for the last
    // prompt position.  digits: fixed-point digits per activation in the matmuls (2..4).
    int prefill(int n, bool with_logits, int digits, float *elapsed_ms);
    // The same forward on a LIVE sequence: with p = position(), history tokens [p, p + n) go through every layer as [n, *] matrices
    // over the p positions the KV cache already holds (the reference's forward with seq_len n over a cache of past_len p: T:455-470,
    // T:704-719), on the matmul chain prefill would choose for n rows (last_prefill_path()) and with the continuation attention
    // (bitnet_hip_attention_extend_dev) in place of the whole-prompt one; it ends as prefill ends: position p + n, with_logits picks
    // the next token (argmax or the sampler) into history[p + n], run() can go on.  At p == 0 it IS prefill (same logits bit for bit).
    // n >= 1, p + n <= fed tokens, p + n <= max_pos - 1.  Both storage formats, both cache types, sampling on or off.
    // Carry-on rule: after a with-logits step the picked token sits UNCONSUMED at history[position()], and feed() writes at
    // max(position, fed) -- onto that slot.  A host that wants the picked token in the context therefore feeds it again in front of
    // the new tokens (feed([picked] + new), extend(1 + len(new))); one that does not (an end-of-turn marker it replaces) just feeds
    // the new tokens.
    int extend(int n, bool with_logits, int digits, float *elapsed_ms);
    // PACKED prompt forward: ONE launch chain for n_members = 1..64 sequences, member i at its own position p_i (fresh or live) with its own n[i]
    // new tokens -- the reference's forward over [B, T, H] (crates/bitnet-transformer/src/lib.rs:1437-1478) for sequences that are NOT in lock
    // step, as BatchDecoder is for the decode step.  History tokens [p_i, p_i + n[i]) of every member go through every layer together as the
    // rows of one matrix (member i's rows start at a multiple of bitnet_hip_attention_packed_row_align; the rows between are padding: valid
    // tokens' embeddings that no cache sees); the matmuls are row-independent, and the attention (bitnet_hip_attention_packed_dev) lets each
    // member's queries see its own keys only and fills each member's own caches.  Every member ends as its own extend(n[i], with_logits, digits)
    // leaves it: position p_i + n[i], slots [p_i, p_i + n[i]) of every layer filled, with_logits picks the next token into history[p_i + n[i]]
    // by the member's OWN argmax or sampler (with its log-probability record when its tap is on); run(), extend(), fork() and
    // BatchDecoder::step() go on, and extend's carry-on rule holds.  "As extend": the same arithmetic class, not the same bits -- the row
    // count of the whole pack selects the matmul tiles and the chain (last_prefill_path() of the driver).
    // members[0] is the DRIVER: the forward runs on its stream and in its prompt buffers (grown for the padded row total), the error text
    // goes on it, and saturation_fallbacks() of the driver counts a pack that clamped an f16 hand-over value and was repeated -- whole --
    // at 4 digits (elapsed_ms of a repeated forward -- prefill, extend, a pack, a wide step -- covers both attempts).  The tail is
    // finish_prefill on each member (its own head on its own stream).  Synchronises before returning.
    // Refused, with nothing modified: n_members outside 1..64; a null, dead or repeated member; members with different root() or kv_f16();
    // n[i] < 1; p_i + n[i] beyond the fed tokens; p_i + n[i] > max_pos - 1; model globals not set.  Members may sit in BatchDecoder slots.
    static int prefill_packed(Decoder *const *members, const int *n, int n_members, bool with_logits, int digits, float *elapsed_ms);
    // WIDE decode step: n_steps single-token steps for n_members = 1..64 live sequences through ONE matrix forward per step -- the route between
    // BatchDecoder (8 slots, the batch-1 GEMV restated per vector) and prefill_packed with n[i] = 1 (every member's row on a 64-row boundary, one
    // head launch per member).  Per step the members' current tokens history[p_i] become the M dense rows of one matrix
    // (bitnet_hip_embed_rows_dev), every layer runs on the many-row matmul chain that M rows and `digits` select (prompt_layers: every weight
    // matrix is read once), each row attends over its own member's cache at its own position (bitnet_hip_attention_decode_rows_dev, the decode
    // attention's 64-position records), all M logits rows come from one pass over the embedding table (bitnet_hip_score_f16_dev) and
    // bitnet_hip_pick_rows_dev hands each row to its member: the logits into the member's own logits buffer, and for a greedy member the token,
    // its history entry and its position.  A member that samples then draws with its own sampler, and a member whose logits tap is on records,
    // in member order on the driver's stream (one launch each, as pick_token arranges them).
    // Every member ends as its own n_steps x extend(1, true, digits) would leave it -- "as extend": the same arithmetic class, not the same bits
    // (the matmul tiles follow M, and the head rounds its operand to f16 as score() does): position p_i + n_steps; slots [p_i, p_i + n_steps) of
    // every layer filled and every other slot untouched bit for bit; history and forced tokens honoured as run() honours them (a fed token at
    // p + 1 stays); last_logits(); the sampler state; log-probability records p_i + 1 .. p_i + n_steps.  run(), extend(), fork(),
    // prefill_packed() and BatchDecoder::step() go on from there.  last_hidden() is NOT maintained.
    // members[0] is the DRIVER: the forward runs on its stream and in its prompt buffers, the error text goes on it, and its
    // saturation_fallbacks() counts a step that clamped an f16 hand-over value and was repeated -- whole -- at 4 digits (the positions move
    // only in the pick, so the repeat rewrites the same slots).  The positions are read once, before the first launch; step s bounds the
    // attention's record grid by the largest position + s + 1.  Eager launches; synchronises before returning.  The logits matrix, the head's
    // workspace, the device pointer tables and the attention scratch of 64 sequences are allocated at the first call and grow on demand.
    // Refused, with nothing modified: n_members outside 1..64; n_steps < 1; a null, dead or repeated member; members with different root() or
    // kv_f16(); model globals not set; p_i + n_steps > max_pos - 1 ("KV cache overflow").  Members may sit in BatchDecoder slots.
    static int step_wide(Decoder *const *members, int n_members, int n_steps, int digits, float *elapsed_ms);
    // Keep the first n positions of the sequence, 0 <= n <= position(): the position becomes n and the forced count min(forced, n), on
    // host and device.  The cache bytes stay as they are (the decode attention gives slots beyond the position zero weight, the
    // continuation attention never reads a slot at or beyond its past length), and so do the sampler's counts and word counter:
    // reset() remains the full clear.  A bound grammar's state stays too: set_grammar_state(walk of the tokens that remain) moves it.
    int rewind(int n);
    // CONTEXT SHIFT: keep the first `keep` positions, discard the next `discard`, slide the rest down -- the member of the live-sequence family
    // that drops tokens from the MIDDLE (the reference's KvCacheBuffer::rotate_kv / truncate, crates/bitnet-kernels/src/cuda/kv_cache.rs:305-348,
    // and WindowedKVCache, crates/bitnet-gpu-hal/src/sliding_window.rs:161-235; llama.cpp's context shift, StreamingLLM's attention sinks).  With
    // p = position(): cache slot j of every layer takes slot j + discard for j in [keep, p - discard) by ONE bitnet_hip_kv_shift_dev launch (V
    // bit for bit, K re-rotated between RoPE table rows j + discard and j; slots >= p - discard are stale as after rewind); the position
    // becomes p - discard on host and device; history entries [keep + discard, max_pos) move down by discard (entry p, the unconsumed picked or
    // fed token, travels to p - discard, as with rewind) and the history is zero beyond them; the forced count f becomes f if f <= keep, keep if
    // f <= keep + discard, else f - discard; log-probability record q > keep + discard becomes record q - discard, records in
    // (keep, keep + discard] are dropped and records above the new last one are cleared to 0xFF.  The sampler's counts and word counter, the
    // cache type, the attention form, last_logits() and the captured graphs stay (the graphs read the position from device memory);
    // last_hidden() is unspecified.  A decoder in a BatchDecoder slot may be shifted between steps.  Explicit, never automatic: every overflow
    // refusal stays.  Synchronises before returning.
    // Refused, with nothing modified: keep < 0, discard < 1, keep + discard > position().
    int shift(int keep, int discard);
    static int shift_forced(int forced, int keep, int discard);  // the forced count after shift(keep, discard)
    // FORK: every one of the n_dst (1..8) destinations takes over the first n positions of `src`, 0 <= n <= src.position() -- the reference's
    // prefix cache (crates/bitnet-inference/src/prefix_cache.rs: lookup :173, insert :212) with the state kept on the device instead of its
    // host-side cached_state bytes.  Afterwards every destination is what src would be after src.rewind(n), and src itself is untouched:
    // position n and forced count min(src's forced, n) on host and device; history[0 .. n] copied (n + 1 entries: as rewind leaves entry n
    // in place, the unconsumed picked or fed token travels) and zero beyond; cache slots < n of every layer copied by ONE
    // bitnet_hip_kv_fork_dev launch for all destinations (slots >= n keep the destination's bytes).  A destination's sampler is reset as
    // reset() does (counts and word counter cleared, config kept); its cache type, attention form, act mode and captured graphs stay (the
    // graphs read the position from device memory: nothing is re-captured).  last_logits() / last_hidden() of a destination are UNSPECIFIED
    // until its next with-logits step.  Synchronises before returning.
    // Refused, with nothing modified: n out of range; n_dst outside 1..8; a null, dead or repeated destination; a destination that is src
    // (use rewind); one with another root() (same weights); another kv_f16(); one sitting in a BatchDecoder slot (leave the batch first).
    // src may sit in a slot: it is only read, and step() returns synchronised.  The error text goes on src.
    // Best of n from ONE prompt forward: src runs prefill(P, with_logits); fork at P - 1; every destination runs run(1, with_logits) under
    // its own seed -- one decode step in place of a prompt forward -- and goes on alone or in a BatchDecoder.
    // Prefix hit: fork at the common length (cached_prefix), then extend's carry-on rule holds as after a rewind: feed() on a fork writes at
    // slot n; feed the rest of the prompt and extend() over it.
    static int fork(Decoder &src, Decoder *const *dsts, int n_dst, int n);
    // prefill through a PREFIX CACHE (prefix_cache.hpp), on a fresh sequence: the first n fed tokens are looked up; with a hit of length m the
    // entry's first min(m, n - 1) positions are restored into this decoder (one bitnet_hip_kv_restore_dev launch; at least one token stays
    // to be computed, its row gives the logits), the rest of the prompt is fed again behind them (restore clears the history beyond its
    // positions, as fork does) and extend() runs over it -- the explicit sequence fork at m, feed, extend, bit for bit.  Without a hit it IS
    // prefill(n, with_logits, digits).  *hit (nullable): the positions restored.  elapsed_ms: the prompt forward's.  It never inserts: the
    // caller decides what is worth keeping (PrefixCache::insert).  The lookup counts in the cache's statistics.
    // A HIT IS A FORK, and leaves what a fork leaves where a miss leaves what prefill leaves: the cache slots and the logits are the same
    // arithmetic class either way, but on a hit this decoder's sampler is reset (counts, word counter; config kept), its log-probability
    // records are cleared, its stop state is re-armed, and history entries beyond n -- tokens fed past the n this call takes in -- are
    // ZERO (restore clears the history beyond its positions and only [k, n) is fed again); on a miss all of those stay.  A caller that
    // needs one outcome feeds exactly n tokens and sets its sampler up after the call, or resets the sampler itself on a miss (*hit == 0).
    // A cache bound to other weights or another cache type holds nothing for this decoder: a miss without a lookup.
    // Refused as prefill refuses (not fresh, n beyond the fed tokens, "KV cache overflow") and as PrefixCache::restore refuses (this
    // decoder sits in a BatchDecoder slot).
    int prefill_cached(PrefixCache &cache, int n, bool with_logits, int digits, int *hit, float *elapsed_ms);
    // The reference's lookup for ONE live sequence: the length of the longest common prefix of tokens[0 .. n) and history[0 .. position()),
    // or -1 on error.  Costs the position read-back and one of min(n, position()) tokens.
    int cached_prefix(const int32_t *tokens, int n);
    // Token-parallel prefill of ONE long prompt over `world` GPUs, one process per GPU (BASELINE configs[4]):
    // this rank runs the first n fed tokens' zigzag chunks rank and 2 world - 1 - rank through every layer (weights are
    // replicated: all seven projections are collective-free); per layer ONE all-gather of the raw k|v rows through
    // `gather` (RCCL: bitnet_host_rccl_allgather; tests: any callable), after which every rank fills its own KV cache
    // for all n positions.  n % (2 * world * 64) == 0.  wire_f16: k|v travel as f16.
    int prefill_sharded(int n, int rank, int world, bitnet_host_allgather_fn gather, void *gather_ctx, bool with_logits, int digits,
                        bool wire_f16, float *elapsed_ms);
    // Tail of a prefill driven from outside (token-parallel prefill, bitnet-rs_amd/prefill_parallel.py):
    // the KV cache already holds positions 0..n-1; last_row (device, [hidden]) is the residual stream
    // of position n-1 or null on ranks that do not own it (then only the position counter moves).
    int finish_prefill(int n, const float *last_row, bool with_logits);
    // Teacher-forced scoring of the first n fed tokens (score.rs / eval.rs teacher forcing, parity::eval_logits_all_positions): runs
    // prefill(n, with_logits = true, digits) unchanged -- the decoder ends exactly as that call leaves it (KV cache, position, history,
    // picked token; run() can go on) -- then the tied head over ALL n rows the prompt forward left (bitnet_hip_score_f16_dev, final norm).
    // Host outputs: nll_out[n - 1] (row r against token r + 1), argmax_out[n] (nullable; entry n - 1 is the f16 head's greedy next token,
    // which can differ from the one prefill picked with the decode head in a near-tie), logits_out[logits_rows * vocab] (nullable).
    // 2 <= n <= fed tokens, n <= max_pos - 1.  Buffers grow on demand (none before the first call); elapsed_ms: prefill + head.
    int score(int n, int digits, float *nll_out, int32_t *argmax_out, float *logits_out, int logits_rows, float *elapsed_ms);
    bool chain_applies(int digits) const;
    bool handover16_applies(int digits) const;
    bool hybrid_applies(size_t n_rows);
    int last_prefill_path() const { return last_prefill_path_; }
    int saturation_fallbacks() const { return saturation_fallbacks_; }
    int fp6_flag(int digits);  // BITNET_HIP_FUSE_FP6_DIGITS for the q|k|v and gate|up launches of the digit-plane prompt forward, or 0
    int ensure_chain_buffers(size_t N);
    bool qb32_applies(int digits, size_t n_rows);  // the QK256 prompt forward on QB32 rows (no row quantiser launch): long prompts, digits = 2
    void set_phase_timing(bool on) { sp_timing_ = on; }
    void phase_times(float out[4]) const {
        for (int i = 0; i < 4; ++i) out[i] = sp_phase_us_[i];
    }
    // Device objects of one layer / of the model for such a driver: handles {qkv, o, gate|up, down},
    // pointers {attn_norm, ffn_norm, kcache, vcache}; globals {embed, final_norm, rope_sin, rope_cos,
    // history, pos, stream}.
    void layer_objects(int layer, uint64_t handles[4], void *ptrs[4]) const;
    void global_objects(void *ptrs[7]) const;
    int position();                                  // tokens consumed so far
    int history(int32_t *out, int n);                // first n tokens of the sequence
    int last_logits(float *out);                     // [vocab], of the last step run with logits
    int last_hidden(float *out);                     // residual stream after the last block (pre final norm)
    // Activation trace of ONE decode step in the reference's format (crates/bitnet-trace/src/lib.rs:46-168: one JSON file per
    // tensor -- name, shape, dtype, blake3 of the raw f32 bytes, rms, num_elements, seq, layer, stage -- in `dir`): the step
    // runs eagerly, every intermediate is materialised as f32 and read back after its kernel.  Stages: embeddings; per
    // block q_proj, k_proj, v_proj, attn_out, attn_residual, ffn_hidden, ffn_out; all_layers_out; logits.  Off the hot path.
    // run() does this for every step when BITNET_TRACE_DIR is set (the reference's switch).
    int trace_step(const char *dir, bool with_logits);
    // Dominant-kernel probe for bench.py: every layer's fused gate/up GEMV back to back in
    // one graph, `reps` replays; returns the mean time per launch and the algorithmic
    // bytes one launch reads.
    int probe_gateup(int reps, float *us_per_launch, double *bytes_per_launch);
    // Same for any kernel of the step: kind 0 q|k|v, 1 attention, 2 o_proj, 3 gate|up, 4 down, 5 logits.
    int probe_kernel(int kind, int reps, float *us_per_launch, double *bytes_per_launch);
    size_t weight_bytes() const { return weight_bytes_; }  // algorithmic bytes of all I2_S matrices
    void *stream() const { return stream_; }

  private:
    int fail(const char *what);
    int fail_arg(const char *what);
    Decoder(const Config &cfg, bool own_norms);  // own_norms false: the borrowing constructor points the norm vectors at the owner's
    bool dead_ = false;
    // attention form of a step: 0 = two kernels, 64-position chunks; 1 = one kernel + merging o-projection (short
    // contexts: 4 records); 2 = two kernels, 128-position chunks (more chunks than CUs); 3 = as 1, 8 records (QAct path)
    struct Tracer;
    int step_launches(bool with_logits, int form, Tracer *tr = nullptr);
    int step_launches_reference(bool with_logits);
    int ensure_graph(bool with_logits, int form);
  public:
    // Captures and instantiates the step graph of every attention form a sequence can reach (by position: form_at) ahead of
    // time, so that no run() pays for a capture in the middle of a generation.  Nothing executes.
    int prepare_graphs(bool with_logits);
    // Which attention form a step at `pos` takes (0..3 above): what run() will launch there with the current weights and settings.
    int form_at(int pos) const;
    // Largest key count of form 3, by measurement (EXPERIMENTS 15.2): the form is taken up to the largest live record count at
    // which it beat records + combine at that count and at every smaller one.
    static constexpr int kMerge8MaxKeys = 512;
  private:
    Decoder *owner_ = nullptr;  // borrowed weights (see the borrowing constructor)
    int borrowers_ = 0;
    int attn_form_ = -1;        // set_attention_form
    int weights_locked();       // refusal of set_layer_* / set_globals on a borrower or an owner with borrowers, else 0
    bool merge_ok_ = false;   // the o-projection can merge the attention chunk records itself (short contexts)
    bool merge8_ok_ = false;  // ... and up to 8 of them on the QAct path

    Config c_;
    std::string err_;
    struct Layer {
        DevBuf<float> attn_norm, ffn_norm;  // borrowed from the owner's layer by a borrower, as the four handles are
        bitnet_hip_weights_t qkv = 0, o = 0, gateup = 0, down = 0;
        DevBuf<float> kcache, vcache;
        bool q_ok = false;  // all four matrices take QAct inputs (bitnet_hip_gemv_q_supported)
    };
    int attn_launch(Layer &L, int form, float *out, void *qout);
    // THE PROMPT FORWARD (DESIGN.md "Prompt forward host").  Which form each projection of one forward takes, decided once by prompt_form:
    // chain = the f16 activation chain, qb = the QB32 chain, h16 = digit planes with the f16 hand-over of the attention output and silu * up,
    // hybrid = h16 with o / down on the f16 matrix cores; f6 / f6od = BITNET_HIP_FUSE_FP6_DIGITS for q|k|v, gate|up / for o, down.
    struct PromptForm {
        bool chain = false, qb = false, h16 = false, hybrid = false;
        int f6 = 0, f6od = 0, digits = 2;
        bool f16_rows() const { return chain || qb || h16; }  // f16 rows travel between kernels: the forward owes the saturation check
    };
    // The attention operator of one forward, named by its driver: the whole prompt; the continuation over `past` cached positions; a pack of n
    // members with their first rows, lengths and pasts (the driver's arrays: they must outlive the forward); n rows, each over its own
    // member's cache, with the bound of the record grid.
    struct AttnOp {
        enum Kind { Whole, Continue, Pack, Rows } kind = Whole;
        size_t past = 0, n = 0, key_bound = 0;
        void *const *tables = nullptr;  // Rows: the device pointer tables (the driver's wide_tables_, or a WideBatch's own)
        bool kv_f16 = false;            // Rows: the MEMBERS' cache type (a WideBatch drives on the root, whose own type may differ)
        Decoder *const *members = nullptr;
        const int32_t *row0 = nullptr, *len = nullptr, *pasts = nullptr;
    };
    int prompt_form(size_t N, int digits, bool sharded, PromptForm *out);  // the decision, and every buffer growth the form needs
    int project_qkv(size_t l, size_t N, const PromptForm &f);
    int project_o(Layer &L, size_t N, const PromptForm &f);
    int project_gateup(Layer &L, size_t N, const PromptForm &f);
    int project_down(Layer &L, size_t N, const PromptForm &f, const float *next_norm);  // next layer's attention norm, or null: nothing handed over
    int project_residual(bitnet_hip_weights_t w, size_t N, const PromptForm &f, const float *in32, const void *in16, const float *next_norm);
    int prompt_attention(Layer &L, size_t N, void *out, bool out_f16, const AttnOp &op);  // one layer's attention of a prompt forward
    int prompt_layers(size_t N, const PromptForm &f, const AttnOp &op);                   // every layer over the N rows in pf_x_
    // the saturation rule: form, fill, layers and -- if an f16 hand-over value clamped -- fill and layers again at 4 digits on the digit planes
    template <class Fill> int forward_with_repeat(size_t N, int digits, const AttnOp &op, const Fill &fill);  // fill: int(), the driver's lambda
    const char *span_problem(int p, int n, bool positive = true) const;  // "feed() first" / "KV cache overflow" for tokens [p, p + n), or null
    const char *overflow_problem(int p, int n) const;
    static int check_members(Decoder *const *members, int n_members, int cap, const std::string &entry, const char *also);
    int prompt_forward(int p, int n, bool with_logits, int digits, float *elapsed_ms);  // the body of prefill (p == 0) and extend
    int ensure_prompt_buffers(int n, size_t attn_need);             // the per-row buffers and the attention workspace of a prompt forward of n rows
    int packed_forward(Decoder *const *members, const std::vector<int32_t> &past, const std::vector<int32_t> &len, bool with_logits, int digits,
                       float *elapsed_ms);                          // the body of prefill_packed, on the driver
    // the body of step_wide, on the driver.  tail == null: the driver builds and uploads the pointer tables and ends every step with one sampling,
    // tap and stop launch PER MEMBER (step_wide, unchanged).  With a tail (WideBatch): the tables are the tail's and each step ends with at most
    // one launch of each kind; `this` may then be no member at all (the weights' owner).
    int wide_forward(Decoder *const *members, int M, int n_steps, int max_p, int digits, float *elapsed_ms, WideTail *tail = nullptr);
    // wide buffers (none before the first call): device pointer tables [2 * n_layers + 6][64] -- per layer K then V caches, then position, history,
    // forced count, logits row, and the pick's token / position tables (NULL for a member that samples) --, the attention scratch of wide_cap_
    // sequences (zero-filled), the head's [wide_cap_, vocab] logits, argmax, nll, targets (-1) and workspace
    DevBuf<void *> wide_tables_;
    int wide_cap_ = 0;
    DevBuf<float> wide_scratch_, wide_logits_, wide_nll_;
    DevBuf<int32_t> wide_am_, wide_tgt_;
    DevBuf<void> wide_ws_;
    size_t wide_ws_bytes_ = 0;
    void release_layer(Layer &L);  // frees the layer's handles, subtracts their bytes, drops the captured graphs
    void drop_graphs();
    // final norm + tied logits + the next token (greedy argmax or the sampler) [+ its logprob record]; need_logits: a reader of logits_
    // follows in this step (the tracer), so the full head.  Leaves pick_screened_; whoever EXECUTES the launches (not a capture) calls picked().
    int pick_token(void *stream, bool record = true, bool need_logits = false);
    bool screen_step(bool need_logits) const;
    void picked(bool screened) { logits_stale_ = screened; }
    int ensure_screen_image();  // the owner's image, built if missing (set_globals, set_head_screen)
    int refresh_logits();       // logits_ stale after a screened step: the full head once on the saved head input
    // the head input the last screened launch saved: behind ub and the lb maxima in the workspace (layout: include/bitnet_hip.h)
    float *screen_x() const { return screen_ws_.get() + ((size_t)c_.vocab + 3) / 4 * 4 + ((size_t)screen_wgs_ + 3) / 4 * 4; }
    DevBuf<void> screen_;           // int8 screening image of embed_ (borrowed with it)
    DevBuf<float> screen_ws_;       // ub, lb maxima, saved head input, counters, rescored rows (bitnet_hip_head_screen_ws_bytes); own
    bool head_screen_on_ = true;    // BITNET_HOST_HEAD_SCREEN / set_head_screen
    bool pick_screened_ = false;    // what the last pick_token issued (or captured)
    bool logits_stale_ = false;     // the last executed head was the screened one: logits_ does not hold its logits yet
    int graphs_screened_ = -1;      // screen_step(false) when the live graphs were captured (-1: none captured)
    int adopt_projections(Layer &L, bitnet_hip_weights_t h[7]);
    std::vector<Layer> layers_;  // sized once, never resized
    DevBuf<void> embed_;         // borrowed by a borrower, as final_norm_
    DevBuf<float> final_norm_;
    DevBuf<float> rope_sin_, rope_cos_;
    DevBuf<float> x_, x2_, qkv_, att_, h_, logits_;
    DevBuf<void> qa_x_, qa_x2_, qa_att_, qa_h_;  // QAct records of x, x2, attention output, silu(gate)*up
    DevBuf<double> st_x_, st_x2_;                // LayerNorm statistics pairs of x, x2
    int act_mode_ = 1;
    bool kv_f16_ = false;
    std::string trace_dir_;  // BITNET_TRACE_DIR at construction
    DevBuf<float> ref_n_, ref_gu_, ref_t_;  // unfused reference step: normalised row, gate|up tiles, projection out
    DevBuf<void> scratch_;
    DevBuf<float> attn_scratch_;
    DevBuf<int32_t> pos_, n_forced_, history_, token_;
    bitnet_hip_sampler *sampler_ = nullptr;
    bool sampling_ = false;
    int lp_top_n_ = -1;  // set_logprobs
    DevBuf<bitnet_hip_logprob_record> lp_records_;  // [max_pos]
    DevBuf<void> lp_scratch_;
    int host_forced_ = 0;
    bitnet_hip_stop *stop_ = nullptr;  // set_stop: created at the first config, kept until the decoder goes
    bool stop_on_ = false;
    int arm_stop(bool keep_generated);  // no-op without criteria
    // fork: device pointer tables, allocated at the first fork FROM this decoder: [0] its own K caches [n_layers], [1] its V caches (built once),
    // then the destinations' K [8][n_layers] and V [8][n_layers] (uploaded per call).  shift() uses [0] and [1].
    int ensure_fork_tables();
    int fork_from_this(Decoder *const *dsts, int n_dst, int n);
    // The two parts of a fork that PrefixCache::restore shares.  fork_refusal: why this destination set cannot take over a state of `root` and
    // cache type kv_f16 (src: the live source, or null), or null; the root is compared, never dereferenced.  fork_arrive: behind the cache copy
    // already queued on `stream`, every destination takes history[0 .. n] (n + 1 entries of `hist`, device or host memory) with zeros beyond,
    // position n, the forced count, a reset sampler, cleared log-probability records and no stop state; synchronises; the error text on *this.
    static const char *fork_refusal(Decoder *const *dsts, int n_dst, const Decoder *src, const Decoder *root, bool kv_f16);
    int fork_arrive(Decoder *const *dsts, int n_dst, int n, int forced, const int32_t *hist, bool hist_on_device, void *stream);
    DevBuf<void *> fork_tables_;
    // sharded prefill buffers (grown on demand)
    int sp_cap_ = 0, sp_ctx_ = 0;
    DevBuf<void> sp_kv_send_, sp_kv_all_;
    DevBuf<int32_t> sp_block_pos_, sp_tokens_;
    // per-phase timing of the sharded prefill (set_phase_timing): 8 timing events per layer on the compute / comm streams, and the
    // medians over the layers of the last timed call: [0] projections (q|k|v + pack, o, gate|up, down), [1] attention (both phases),
    // [2] the part of the all-gather the compute stream had to wait for, [3] the all-gather itself on its own stream; microseconds
    bool sp_timing_ = false;
    float sp_phase_us_[4] = {0.f, 0.f, 0.f, 0.f};
    // prefill buffers (grown on demand)
    int pf_cap_ = 0;
    DevBuf<float> pf_x_, pf_qkv_, pf_att_, pf_h_;
    DevBuf<void> pf_gemm_ws_, pf_attn_ws_;
    // the f16 activation chain of the prompt forward (prefill_chain): f16 rows handed from kernel to kernel, LayerNorm statistics partials
    int pfc_cap_ = 0;
    DevBuf<void> pf_xh_, pf_atth_, pf_hh_;
    DevBuf<float> pf_stats_;
    DevBuf<void> pf_qb_;      // QB32 rows of gamma * x (the input of q|k|v and of gate|up), bitnet_hip_qb32_bytes(pfc_cap_, hidden)
    int pf_qb_cap_ = 0;
    bool force_scaled_ = false;   // the prompt is being repeated on the row-scaled forms after an f16 hand-over value was clamped (prefill)
    int saturation_fallbacks_ = 0;
    // score buffers (grown on demand): targets, nll, argmax, dumped logits, workspace of bitnet_hip_score_f16_dev
    int sc_cap_ = 0, sc_logits_cap_ = 0;
    DevBuf<int32_t> sc_tgt_, sc_am_;
    DevBuf<float> sc_nll_, sc_logits_;
    DevBuf<void> sc_ws_;
    size_t sc_ws_bytes_ = 0;
    int last_prefill_path_ = 0;  // what the last prefill() ran: 0 digit planes (+ f16 hand-over / hybrid), 1 the f16 chain, 2 the QB32 chain
    int prefill_qb32_ = -1;   // BITNET_HOST_PREFILL_QB32: -1 not read yet; 1 = the QB32 chain where it applies (opt-in), 0 (default) = quantiser launches
    int prefill_fp6_ = -1;    // BITNET_HOST_PREFILL_FP6: -1 not yet decided, 0 int8 digit planes, 1 the fp6 x fp4 form on resident fp4 images (fp6_flag)
    int prefill_hybrid_ = -1;  // BITNET_HOST_PREFILL_HYBRID: -1 not read yet; 1 (default) o / down on the f16 matrix cores for long shares, 0 never, 2 at any length
    int prefill_fp6_od_ = -1;  // BITNET_HOST_PREFILL_FP6_OD: -1 not read yet; 1 = o / down of the non-hybrid f16 hand-over on the fp6 form too (experiment), 0 (default)
    int prefill_chain_ = -1;  // BITNET_HOST_PREFILL_CHAIN: -1 automatic (the block-scaled format, whose matmul runs on f16 activations anyway), 0 off, 1 on
    size_t pf_gemm_ws_bytes_ = 0, pf_attn_ws_bytes_ = 0;
    size_t weight_bytes_ = 0;
    static constexpr int kGraphs = 8;
    void *graph_exec_[kGraphs] = {};  // [2 * form + with_logits], forms 0..3 (form_at)
    void *graph_[kGraphs] = {};
    int logits_wgs_ = 512;  // two workgroups per CU: whole rounds on the 256 CUs (768 / 1280 workgroups are 15-20 % slower)
    int screen_wgs_ = 512;  // the screening launch's grid (BITNET_HOST_SCREEN_WGS)
};

}  // namespace bitnet_host

// C shim for the Python tests / bench (ctypes).  Not part of the kernel boundary.
extern "C" {
typedef struct bitnet_host_config {
    int32_t hidden, n_layers, n_heads, n_kv_heads, head_dim, ffn, vocab, max_pos;
    float eps, rope_theta;
} bitnet_host_config;
void *bitnet_host_create(const bitnet_host_config *cfg);
void bitnet_host_destroy(void *d);  // drops the caller's reference: the object goes when no borrower and no batch slot holds it any more
// Decoder(owner): a decoder borrowing `owner`'s weights (own KV caches, history, position, sampler, stream).  Single-threaded use.
void *bitnet_host_create_shared(void *owner);
void bitnet_host_release(void *d);  // one reference less (what bitnet_host_destroy does); a batch slot lets its member go with it
int bitnet_host_set_attention_form(void *d, int form);  // -1 automatic (form_at), 0 = 64-position records + combine everywhere
int bitnet_host_set_head_screen(void *d, int on);       // Decoder::set_head_screen
int bitnet_host_head_screen(void *d);                   // Decoder::head_screen: 1 the screened head, 0 the full head; -1 for a dead handle
int bitnet_host_head_screen_stats(void *d, uint32_t *out3);  // Decoder::head_screen_stats
const char *bitnet_host_error(void *d);
int bitnet_host_set_layer_qk256(void *d, int layer, const float *attn_norm, const float *ffn_norm,
                                const uint8_t *q, const uint8_t *k, const uint8_t *v, const uint8_t *o,
                                const uint8_t *gate, const uint8_t *up, const uint8_t *down);
int bitnet_host_set_layer_i2s(void *d, int layer, const float *attn_norm, const float *ffn_norm,
                              const uint8_t *const *w7, const float *const *scales7, size_t block_size);
int bitnet_host_set_globals(void *d, const uint16_t *embed_f16, const float *final_norm);
int bitnet_host_reset(void *d);
int bitnet_host_set_sampling(void *d, const bitnet_hip_sampling_config *cfg);  // NULL = greedy
int bitnet_host_set_sampling_ex(void *d, const bitnet_hip_sampling_config_ex *cfg);  // NULL = greedy
int bitnet_host_set_mirostat(void *d, const bitnet_hip_mirostat_config *cfg);  // NULL = off
int bitnet_host_mirostat_state(void *d, float *mu, uint64_t *fallbacks);
int bitnet_host_set_constraints(void *d, const bitnet_hip_constraints *cfg);  // NULL = off
int bitnet_host_constraints_state(void *d, uint64_t *chosen);
int bitnet_host_sampling_draws(void *d, uint64_t *out);
int bitnet_host_set_logprobs(void *d, int top_n);                             // Decoder::set_logprobs: -1 off, 0..20 on
int bitnet_host_logprobs(void *d, int first, int n, void *records_out);       // Decoder::logprobs: n bitnet_hip_logprob_record
int bitnet_host_set_stop(void *d, const bitnet_hip_stop_config *cfg);           // Decoder::set_stop; NULL = off
int bitnet_host_stop_state(void *d, bitnet_hip_stop_state *out);               // Decoder::stop_state
int bitnet_host_resume(void *d);                                               // Decoder::resume
int bitnet_host_run_until_stop(void *d, int max_steps, int chunk, int *steps, float *elapsed_ms);  // Decoder::run_until_stop
int bitnet_host_graph_nodes(void *d, int with_logits);                         // Decoder::graph_nodes
int bitnet_host_feed(void *d, const int32_t *tokens, int n);
int bitnet_host_run(void *d, int n, int with_logits, int use_graph, float *elapsed_ms);
int bitnet_host_run_reference(void *d, int n, int with_logits);
int bitnet_host_prepare_graphs(void *d, int with_logits);
int bitnet_host_set_act_mode(void *d, int mode);
int bitnet_host_set_kv_f16(void *d, int on);
int bitnet_host_act_mode(void *d);
int bitnet_host_prefill(void *d, int n, int with_logits, int digits, float *elapsed_ms);
int bitnet_host_finish_prefill(void *d, int n, const float *last_row, int with_logits);
int bitnet_host_extend(void *d, int n, int with_logits, int digits, float *elapsed_ms);  // Decoder::extend
// Decoder::prefill_packed: members[0] drives and carries the error text
int bitnet_host_prefill_packed(void *const *members, const int32_t *n, int n_members, int with_logits, int digits, float *elapsed_ms);
// Decoder::step_wide: members[0] drives and carries the error text
int bitnet_host_step_wide(void *const *members, int n_members, int n_steps, int digits, float *elapsed_ms);
int bitnet_host_rewind(void *d, int n);                                                    // Decoder::rewind
int bitnet_host_shift(void *d, int keep, int discard);                                     // Decoder::shift
int bitnet_host_fork(void *src, void *const *dsts, int n_dst, int n);                      // Decoder::fork; the error text goes on src
int bitnet_host_cached_prefix(void *d, const int32_t *tokens, int n);                      // Decoder::cached_prefix; -1 on error
int bitnet_host_score(void *d, int n, int digits, float *nll_out, int32_t *argmax_out, float *logits_out, int logits_rows, float *elapsed_ms);
// per-phase medians of the NEXT bitnet_host_prefill_sharded calls (off by default: 8 event records per layer); out[4] = projections,
// attention, exposed all-gather wait, all-gather on its own stream -- microseconds per layer, medians over the layers of the last call
int bitnet_host_set_phase_timing(void *d, int on);
int bitnet_host_phase_times(void *d, float out[4]);
int bitnet_host_prefill_sharded(void *d, int n, int rank, int world, bitnet_host_allgather_fn gather, void *gather_ctx, int with_logits,
                                int digits, int wire_f16, float *elapsed_ms);
// ncclAllGather on an existing RCCL communicator (ctx = ncclComm_t), resolved from librccl.so at first use: the host library
// itself does not link RCCL.  Pass it as `gather` with the communicator as gather_ctx.
int bitnet_host_rccl_allgather(void *nccl_comm, const void *send_dev, void *recv_dev, size_t bytes_per_rank, void *stream);
void bitnet_host_layer_objects(void *d, int layer, uint64_t *handles4, void **ptrs4);
void bitnet_host_global_objects(void *d, void **ptrs7);
int bitnet_host_position(void *d);
int bitnet_host_form_at(void *d, int pos);  // attention form (0..3, Decoder::form_at) of a step at position pos; -1 for a dead handle
int bitnet_host_last_prefill_path(void *d);     // Decoder::last_prefill_path; -1 for a dead handle
int bitnet_host_saturation_fallbacks(void *d);  // Decoder::saturation_fallbacks; -1 for a dead handle
int bitnet_host_history(void *d, int32_t *out, int n);
int bitnet_host_last_logits(void *d, float *out);
int bitnet_host_last_hidden(void *d, float *out);
int bitnet_host_trace_step(void *d, const char *dir, int with_logits);
int bitnet_host_blake3_hex(const void *data, size_t len, char *out65);  // the trace records' hash (host/blake3.hpp), 64 hex digits + NUL
int bitnet_host_probe_gateup(void *d, int reps, float *us_per_launch, double *bytes_per_launch);
int bitnet_host_probe_kernel(void *d, int kind, int reps, float *us_per_launch, double *bytes_per_launch);
uint64_t bitnet_host_weight_bytes(void *d);
uint64_t bitnet_host_device_bytes(void);  // bytes of device memory the process's decoders and batches own now (every DevBuf; not the weight handles)
}
