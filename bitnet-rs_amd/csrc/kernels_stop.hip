// kernels_stop.hip -- the generation path's stop criteria on the device: stop token ids, EOS, a token budget and stop sequences of token ids
// (StopCriteria / StopReason / check_stop, crates/bitnet-generation/src/lib.rs:119-144; InferenceEngine::should_stop, crates/bitnet-inference/
// src/engine.rs:1315-1348; GenerationConfig's stop fields, crates/bitnet-inference/src/config.rs:67-85).
//
// One launch BEHIND the pick (and the logits tap), inside the captured step: by then *pos is P = p + 1 and history[P] holds the token the
// pick placed.  One wave per sequence decides whether that token ends the sequence, and once it has, every later launch of the wave puts
// the sequence back where it stopped.  The freeze needs no change to any other kernel:
//   * the position is restored to the stop position, so the next queued step consumes the stop token again at the same slot and rewrites
//     that cache slot with the same bytes;
//   * the forced count is raised to 0x7fffffff, so every later pick treats its position as a forced one: it writes no history entry, and
//     the sampler samples nothing, counts nothing, draws no word and leaves Mirostat's mu alone.
//
// The wave: lanes 0..31 compare the token with one stop id each; lane 4 s + q compares tokens 8 q .. 8 q + 7 of sequence s with the history
// behind P.  Two ballots (ids, sequence quarters), then lane 0 decides in check_stop's order and stores the state with plain vector stores.
// Every history index is checked against the capacity before it is read: a garbage position is a no-op.
// k_stop and k_stop_batch run one body, so per slot the batched form leaves the bits of the single one.
#include <cstring>
#include <new>

#include "common.hpp"

namespace bitnet_hip {
namespace {

constexpr int kMaxIds = BITNET_HIP_STOP_MAX_IDS, kMaxSeqs = BITNET_HIP_STOP_MAX_SEQS, kMaxLen = BITNET_HIP_STOP_MAX_SEQ_LEN;
constexpr int kFrozenForced = 0x7fffffff;
static_assert(kMaxIds <= 64 && kMaxSeqs * 4 == 64 && kMaxLen == 32, "one wave: a lane per stop id, four lanes of 8 tokens per sequence");

// device memory of one bitnet_hip_stop: the state (its first 24 bytes are bitnet_hip_stop_state), then the config
struct StopDev {
    int32_t reason, index, token, position, generated, frozen_steps;
    int32_t window, pad;  // window: tokens counted since the last arm -- how far behind P a sequence match may reach
    int32_t *live;        // the count of running members of the table that holds this object, or NULL: here, not in the launch arguments, so
                          // that a launch captured before the object joined a table keeps the table's count right too
    int32_t n_ids, eos_id, max_tokens, n_seqs;
    int32_t ids[kMaxIds];
    int32_t seq_len[kMaxSeqs];
    int32_t seq_tok[kMaxSeqs * kMaxLen];
};
constexpr size_t kCfgOfs = offsetof(StopDev, n_ids);
static_assert(sizeof(bitnet_hip_stop_state) == 24 && offsetof(StopDev, window) == 24 && offsetof(StopDev, live) == 32 && kCfgOfs == 40, "state layout");

struct StopArgs {
    StopDev *st;  // NULL: an idle entry
    int32_t *pos;
    const int32_t *history;
    int32_t *n_forced, *token;
    int32_t capacity, pad;
};

__device__ __forceinline__ int sat_inc(int v) { return v < 0x7fffffff ? v + 1 : v; }

__device__ __forceinline__ void stop_body(const StopArgs &a) {
    const int lane = threadIdx.x & 63;
    StopDev *st = a.st;
    if (st->reason != 0) {  // already stopped: hold the sequence where it stopped
        if (lane == 0) {
            *a.pos = st->position;
            if (a.token) *a.token = st->token;
            st->frozen_steps = sat_inc(st->frozen_steps);
        }
        return;
    }
    const int P = *a.pos, cap = a.capacity;
    if (P < 1 || P >= cap) return;  // nothing was placed, or a position no history entry stands for
    if (P < *a.n_forced) return;    // a prompt token: it never stops a sequence and is never counted
    const int t = a.history[P];
    const int generated = sat_inc(st->generated), window = sat_inc(st->window);

    const int n_ids = min(st->n_ids, kMaxIds), n_seqs = min(st->n_seqs, kMaxSeqs);
    const unsigned long long id_hit = __ballot(lane < n_ids && st->ids[lane < kMaxIds ? lane : 0] == t);

    // lane 4 s + q: entries 8 q .. 8 q + 7 of sequence s against history[P - L + 1 + j]; a quarter beyond the length agrees
    const int s = lane >> 2, q = lane & 3;
    const int L = s < n_seqs ? st->seq_len[s] : 0;
    bool agree = L >= 1 && L <= kMaxLen && L <= window;
    if (agree) {
        const int first = P - L + 1;
        for (int j = 8 * q; j < 8 * q + 8 && j < L; ++j) {
            const int i = first + j;
            if (i < 0 || i >= cap || a.history[i] != st->seq_tok[s * kMaxLen + j]) {
                agree = false;
                break;
            }
        }
    }
    unsigned long long m = __ballot(agree);
    m &= m >> 1;
    m &= m >> 2;
    m &= 0x1111111111111111ull;  // bit 4 s: all four quarters of sequence s agree

    if (lane != 0) return;
    int reason = BITNET_HIP_STOP_NONE, index = 0;
    if (id_hit)
        reason = BITNET_HIP_STOP_TOKEN, index = __ffsll((long long)id_hit) - 1;
    else if (st->eos_id >= 0 && t == st->eos_id)
        reason = BITNET_HIP_STOP_EOS;
    else if (st->max_tokens > 0 && generated >= st->max_tokens)
        reason = BITNET_HIP_STOP_MAX_TOKENS;
    else if (m)
        reason = BITNET_HIP_STOP_SEQUENCE, index = (__ffsll((long long)m) - 1) >> 2;
    st->generated = generated;
    st->window = window;
    if (reason == BITNET_HIP_STOP_NONE) return;
    st->index = index;
    st->token = t;
    st->position = P;
    st->frozen_steps = 0;
    st->reason = reason;
    *a.n_forced = kFrozenForced;
    if (st->live) atomicSub(st->live, 1);
}

__global__ __launch_bounds__(64) void k_stop(StopArgs a) {
    if (!a.st) return;
    stop_body(a);
}

// Every entry of a device table in one launch, one wave each (blockIdx.x = the slot).  A NULL entry is idle: nothing is read or written.
__global__ __launch_bounds__(64) void k_stop_batch(const StopArgs *__restrict__ table) {
    const StopArgs *e = table + blockIdx.x;
    if (!e->st) return;
    const StopArgs a = *e;
    stop_body(a);
}

// the refusals of a config, before the GPU is touched; fills the device image of the config part
int check_cfg(const bitnet_hip_stop_config *c, StopDev *out, const char *who) {
    if (!c) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null config passed to %s", who);
    if (c->n_stop_ids > (size_t)kMaxIds)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: %zu stop ids, at most %d", who, c->n_stop_ids, kMaxIds);
    if (c->n_seqs > (size_t)kMaxSeqs)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: %zu stop sequences, at most %d", who, c->n_seqs, kMaxSeqs);
    if (c->n_stop_ids && !c->stop_ids) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: null stop_ids with n_stop_ids %zu", who, c->n_stop_ids);
    if (c->n_seqs && (!c->seq_len || !c->seq_tokens))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: null seq_len or seq_tokens with n_seqs %zu", who, c->n_seqs);
    if (c->eos_id < -1) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: eos_id %d (-1 = none)", who, c->eos_id);
    if (c->max_tokens < 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: max_tokens %d (0 = none)", who, c->max_tokens);
    memset((char *)out + kCfgOfs, 0, sizeof(StopDev) - kCfgOfs);
    out->n_ids = (int32_t)c->n_stop_ids, out->eos_id = c->eos_id, out->max_tokens = c->max_tokens, out->n_seqs = (int32_t)c->n_seqs;
    for (size_t i = 0; i < c->n_stop_ids; ++i) {
        if (c->stop_ids[i] < 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: stop id %zu is negative (%d)", who, i, c->stop_ids[i]);
        out->ids[i] = c->stop_ids[i];
    }
    size_t at = 0;
    for (size_t s = 0; s < c->n_seqs; ++s) {
        const int32_t L = c->seq_len[s];
        if (L < 1 || L > kMaxLen) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: stop sequence %zu has length %d, 1..%d", who, s, L, kMaxLen);
        out->seq_len[s] = L;
        for (int32_t j = 0; j < L; ++j) {
            const int32_t t = c->seq_tokens[at + (size_t)j];
            if (t < 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: token %d of stop sequence %zu is negative (%d)", who, j, s, t);
            out->seq_tok[s * kMaxLen + (size_t)j] = t;
        }
        at += (size_t)L;
    }
    return BITNET_HIP_OK;
}

}  // namespace
}  // namespace bitnet_hip

using namespace bitnet_hip;

struct bitnet_hip_stop {
    StopDev *dev = nullptr;
    bitnet_hip_stop_batch *table = nullptr;  // the table that holds it, or null
    int slot = -1;
};

struct bitnet_hip_stop_batch {
    int n_slots = 0;
    StopArgs *table = nullptr;  // device: [n_slots]
    int32_t *live = nullptr;    // device: bound members that have not stopped
    bitnet_hip_stop *bound[BITNET_HIP_STOP_BATCH_MAX] = {};
};

namespace {

int set_live(bitnet_hip_stop *sp, int32_t *live) {
    BH_HIP_TRY(hipMemcpy(&sp->dev->live, &live, sizeof(live), hipMemcpyHostToDevice));
    return BITNET_HIP_OK;
}

// the table's live count from its members' states (set and arm: both synchronous, no launch in flight)
int recount_live(bitnet_hip_stop_batch *t) {
    int32_t n = 0;
    for (int b = 0; b < t->n_slots; ++b)
        if (t->bound[b]) {
            int32_t reason = 0;
            BH_HIP_TRY(hipMemcpy(&reason, &t->bound[b]->dev->reason, 4, hipMemcpyDeviceToHost));
            n += reason == 0;
        }
    BH_HIP_TRY(hipMemcpy(t->live, &n, 4, hipMemcpyHostToDevice));
    return BITNET_HIP_OK;
}

}  // namespace

extern "C" {

int bitnet_hip_stop_create(const bitnet_hip_stop_config *cfg, bitnet_hip_stop **out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to stop_create");
    *out = nullptr;
    StopDev h;
    memset(&h, 0, sizeof(h));
    if (int rc = check_cfg(cfg, &h, "stop_create")) return rc;
    bitnet_hip_stop *sp = new (std::nothrow) bitnet_hip_stop();
    if (!sp) return set_error(BITNET_HIP_ERR_EXECUTION, "stop_create: out of host memory");
    hipError_t e = hipMalloc((void **)&sp->dev, sizeof(StopDev));
    if (e == hipSuccess) e = hipMemcpy(sp->dev, &h, sizeof(h), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (sp->dev) (void)hipFree(sp->dev);
        delete sp;
        return set_error(BITNET_HIP_ERR_GPU, "stop_create: %s", hipGetErrorString(e));
    }
    *out = sp;
    return BITNET_HIP_OK;
}

void bitnet_hip_stop_destroy(bitnet_hip_stop *sp) {
    if (!sp) return;
    if (sp->table && sp->slot >= 0) (void)bitnet_hip_stop_batch_set(sp->table, (size_t)sp->slot, nullptr, nullptr, nullptr, 0, nullptr, nullptr);
    if (sp->dev) (void)hipFree(sp->dev);
    delete sp;
}

int bitnet_hip_stop_configure(bitnet_hip_stop *sp, const bitnet_hip_stop_config *cfg) {
    StopDev h;
    if (int rc = check_cfg(cfg, &h, "stop_configure")) return rc;
    if (!sp) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null stop passed to stop_configure");
    BH_HIP_TRY(hipMemcpy((char *)sp->dev + kCfgOfs, (const char *)&h + kCfgOfs, sizeof(StopDev) - kCfgOfs, hipMemcpyHostToDevice));
    return BITNET_HIP_OK;
}

int bitnet_hip_stop_arm(bitnet_hip_stop *sp, int keep_generated) {
    if (!sp) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null stop passed to stop_arm");
    int32_t st[8] = {};
    if (keep_generated) BH_HIP_TRY(hipMemcpy(&st[4], &sp->dev->generated, 4, hipMemcpyDeviceToHost));
    BH_HIP_TRY(hipMemcpy(sp->dev, st, sizeof(st), hipMemcpyHostToDevice));  // the state and the window; the live pointer and the config stay
    if (sp->table) return recount_live(sp->table);
    return BITNET_HIP_OK;
}

int bitnet_hip_stop_get_state(bitnet_hip_stop *sp, bitnet_hip_stop_state *out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null output passed to stop_get_state");
    if (!sp) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null stop passed to stop_get_state");
    BH_HIP_TRY(hipMemcpy(out, sp->dev, sizeof(*out), hipMemcpyDeviceToHost));
    return BITNET_HIP_OK;
}

static int check_binding(const char *who, const int32_t *pos_dev, const int32_t *history_dev, size_t capacity, const int32_t *n_forced_dev) {
    if (!pos_dev || !history_dev || !n_forced_dev)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to %s (position, history or forced count)", who);
    if (capacity == 0 || capacity > (size_t)0x7fffffff) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "%s: capacity %zu, 1..2^31-1", who, capacity);
    return BITNET_HIP_OK;
}

int bitnet_hip_stop_dev(bitnet_hip_stop *sp, int32_t *pos_dev, const int32_t *history_dev, size_t capacity, int32_t *n_forced_dev, int32_t *token_dev,
                        void *stream) {
    if (int rc = check_binding("stop_dev", pos_dev, history_dev, capacity, n_forced_dev)) return rc;
    if (!sp) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null stop passed to stop_dev");
    const StopArgs a{sp->dev, pos_dev, history_dev, n_forced_dev, token_dev, (int32_t)capacity, 0};
    hipLaunchKernelGGL(k_stop, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

int bitnet_hip_stop_batch_create(size_t n_slots, bitnet_hip_stop_batch **out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to stop_batch_create");
    *out = nullptr;
    if (n_slots == 0 || n_slots > (size_t)BITNET_HIP_STOP_BATCH_MAX)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "stop_batch_create: n_slots must be in 1..%d, got %zu", BITNET_HIP_STOP_BATCH_MAX, n_slots);
    bitnet_hip_stop_batch *t = new (std::nothrow) bitnet_hip_stop_batch();
    if (!t) return set_error(BITNET_HIP_ERR_EXECUTION, "stop_batch_create: out of host memory");
    t->n_slots = (int)n_slots;
    hipError_t e = hipMalloc((void **)&t->table, n_slots * sizeof(StopArgs));
    if (e == hipSuccess) e = hipMemset(t->table, 0, n_slots * sizeof(StopArgs));  // a null st: every entry idle
    if (e == hipSuccess) e = hipMalloc((void **)&t->live, 4);
    if (e == hipSuccess) e = hipMemset(t->live, 0, 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        bitnet_hip_stop_batch_destroy(t);
        return set_error(BITNET_HIP_ERR_GPU, "stop_batch_create: %s", hipGetErrorString(e));
    }
    *out = t;
    return BITNET_HIP_OK;
}

void bitnet_hip_stop_batch_destroy(bitnet_hip_stop_batch *t) {
    if (!t) return;
    for (int b = 0; b < t->n_slots; ++b)
        if (t->bound[b]) (void)set_live(t->bound[b], nullptr), t->bound[b]->table = nullptr, t->bound[b]->slot = -1;
    if (t->table) (void)hipFree(t->table);
    if (t->live) (void)hipFree(t->live);
    delete t;
}

int bitnet_hip_stop_batch_set(bitnet_hip_stop_batch *t, size_t slot, bitnet_hip_stop *sp, int32_t *pos_dev, const int32_t *history_dev, size_t capacity,
                              int32_t *n_forced_dev, int32_t *token_dev) {
    if (slot >= (size_t)BITNET_HIP_STOP_BATCH_MAX || (t && slot >= (size_t)t->n_slots))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "stop_batch_set: slot %zu out of range, the table has %d", slot, t ? t->n_slots : BITNET_HIP_STOP_BATCH_MAX);
    if (!t) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null table passed to stop_batch_set");
    StopArgs a;
    memset(&a, 0, sizeof(a));
    if (sp) {
        if (int rc = check_binding("stop_batch_set", pos_dev, history_dev, capacity, n_forced_dev)) return rc;
        if (sp->table && (sp->table != t || (size_t)sp->slot != slot))
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "stop_batch_set: this stop object is already bound to slot %d%s", sp->slot,
                             sp->table == t ? "" : " of another table");
        a = StopArgs{sp->dev, pos_dev, history_dev, n_forced_dev, token_dev, (int32_t)capacity, 0};
    }
    BH_HIP_TRY(hipMemcpy(t->table + slot, &a, sizeof(a), hipMemcpyHostToDevice));
    if (t->bound[slot] && t->bound[slot] != sp) {
        if (int rc = set_live(t->bound[slot], nullptr)) return rc;
        t->bound[slot]->table = nullptr, t->bound[slot]->slot = -1;
    }
    t->bound[slot] = sp;
    if (sp) {
        if (int rc = set_live(sp, t->live)) return rc;
        sp->table = t, sp->slot = (int)slot;
    }
    return recount_live(t);
}

int bitnet_hip_stop_batch_dev(bitnet_hip_stop_batch *t, void *stream) {
    if (!t) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null table passed to stop_batch_dev");
    hipLaunchKernelGGL(k_stop_batch, dim3(t->n_slots), dim3(64), 0, (hipStream_t)stream, (const StopArgs *)t->table);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

int bitnet_hip_stop_batch_live(bitnet_hip_stop_batch *t, int32_t *out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null output passed to stop_batch_live");
    if (!t) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null table passed to stop_batch_live");
    BH_HIP_TRY(hipMemcpy(out, t->live, 4, hipMemcpyDeviceToHost));
    return BITNET_HIP_OK;
}

}  // extern "C"
