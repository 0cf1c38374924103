// beam_search.hpp -- beam search over a BatchDecoder: n hypotheses ranked by cumulative log-probability, with a length penalty and EOS handling.
//
// Replaces nothing in the reference, whose generation follows one hypothesis per request.  The B = n_beams beams are the decoders in the first B
// slots of a BatchDecoder (one owner's weights, one cache type).  Per token the search queues three things on the batch's stream:
//     BatchDecoder::step(1)        the batched step; every member's logits tap (switched to top_n = 2B here) leaves its record
//     bitnet_hip_beam_select_dev   the rule (include/bitnet_hip_beam.h): next beams, pool, histories
//     bitnet_hip_kv_permute_dev    the beams' caches follow their parents, in place, only the slots in which they differ
// and reads the state's 4-byte `done` word once per chunk.  The batch's captured chain is what it was: the two launches follow the step and are
// not spliced into it (graph_nodes() does not change).  A search that ends inside a chunk freezes: the remaining queued steps re-consume the same
// token at the same slot (include/bitnet_hip_beam.h, FROZEN).
//
// After run() every live beam is a live sequence -- position, history and caches are what a decoder holds that was forked from the prompt and
// took the beam's tokens through the batched step -- so BatchDecoder::step, Decoder::run and Decoder::fork may go on from it.  NOT maintained
// across a reorder: the members' log-probability records and last_logits().
// Out of scope: several searches as groups of one WideBatch; beams that sample; beams under a grammar.  Single-threaded use.
#pragma once

#include <string>
#include <vector>

#include "batch_decoder.hpp"

namespace bitnet_host {

class BeamSearch {
  public:
    // Binds to `batch` (which must outlive the search).  Refused, with nothing modified (error() says why, dead()): n_beams outside 1..8 or above
    // the batch's slots; eos < -1; max_new_tokens outside 1..2^20; alpha not finite; an empty slot among the first n_beams; a member that samples
    // (so also one under a grammar or logit constraints) or carries stop criteria; a vocabulary below 2 * n_beams.  Otherwise the members' taps
    // are switched to 2 * n_beams (Decoder::set_logprobs).
    BeamSearch(BatchDecoder &batch, int n_beams, int eos, int max_new_tokens, float alpha);
    ~BeamSearch();
    BeamSearch(const BeamSearch &) = delete;
    BeamSearch &operator=(const BeamSearch &) = delete;
    const std::string &error() const { return err_; }
    bool dead() const { return dead_; }
    // A new search from the members' state: all at ONE position with identical histories up to and including the unconsumed token there (prefill
    // on one member and Decoder::fork into the others, or prefill_cached).  Refused, with nothing modified, otherwise.
    int start();
    // Queues `chunk` times {step(1), select, permute}, reads `done`, and repeats until the search is done.  *steps: the steps queued by this call
    // (frozen ones included).  Refuses a search that was not started, chunk < 1, and -- up front, as BatchDecoder::step does -- a budget that
    // would pass max_pos - 1 ("KV cache overflow").  A search that is done returns at once with 0 steps.
    int run(int chunk, int *steps, float *elapsed_ms);
    int state(bitnet_hip_beam_state *out);  // synchronises
    struct Hypothesis {
        std::vector<int32_t> tokens;
        float score, key;
    };
    // the pool sorted by descending key, then insertion order; synchronises
    int hypotheses(std::vector<Hypothesis> *out);
    const std::vector<float> &len_weights() const { return len_weight_; }  // [max_new_tokens + 1]: (float)pow((double)len, -(double)alpha)
    int n_beams() const { return B_; }
    int max_new_tokens() const { return max_new_; }

  private:
    int fail(const char *what);
    int fail_arg(const std::string &what);
    int bind(int n_beams, int eos, int max_new_tokens, float alpha);  // the constructor's body
    bool dead_ = true, started_ = false;
    std::string err_;
    BatchDecoder &batch_;
    int B_ = 0, eos_ = -1, max_new_ = 0, prompt_pos_ = 0, queued_ = 0, done_ = 0;
    std::vector<float> len_weight_;
    bitnet_hip_beam *beam_ = nullptr;
    DevBuf<bitnet_hip_beam_member> members_;  // [B]
    DevBuf<void *> kv_tables_;                // K [B][n_layers], then V [B][n_layers]
};

}  // namespace bitnet_host

extern "C" {
// BeamSearch(batch, ...): never NULL for a non-NULL batch; bitnet_host_beam_error is non-empty when the binding was refused
void *bitnet_host_beam_create(void *batch, int n_beams, int eos, int max_new_tokens, float alpha);
void bitnet_host_beam_destroy(void *s);
const char *bitnet_host_beam_error(void *s);
int bitnet_host_beam_start(void *s);                                        // BeamSearch::start
int bitnet_host_beam_run(void *s, int chunk, int *steps, float *elapsed_ms);  // BeamSearch::run
int bitnet_host_beam_state(void *s, bitnet_hip_beam_state *out);            // BeamSearch::state
// BeamSearch::hypotheses: *n of them; lens[8], scores[8], keys[8]; tokens[8][max_new_tokens], row i holding lens[i] tokens
int bitnet_host_beam_hypotheses(void *s, int *n, int32_t *lens, int32_t *tokens, float *scores, float *keys);
int bitnet_host_beam_len_weights(void *s, float *out, int n);               // the first n <= max_new_tokens + 1 length weights
}
