// kernels_beam.hip -- beam search behind the batched decode step (gfx950): the launch that picks the next beams, and the launch that permutes the
// beams' KV caches IN PLACE.  include/bitnet_hip_beam.h states the contract; beam_rule.hpp is the rule, compiled here for the device and in
// tests/host/beam_rule_check.cpp for the host.  Replaces nothing in the reference, whose generation follows one hypothesis per request.
//
// k_beam_select: ONE workgroup.  Thread (b, j) scores candidate (b, j) from beam b's tap record and finds its place in the order by counting the
// candidates before it (the order is total: no sort, no ties to break afterwards); the 2B first are walked by one thread (beam_walk: at most 16
// candidates, the pool, the 8 x 8 div table); then all threads move tokens: pool entries first, from the histories as they still are, then the
// histories to their parents'.  The history move is in place: a thread owns an index in ALL B histories, loads every value it needs and only then
// stores, so no thread reads a word another thread writes.
//
// k_kv_permute: the same ownership rule on the caches.  All caches of a call share max_pos, so a word offset means the same (layer, head, slot,
// element) in each; one thread owns a 16-byte vector offset in all B caches, loads the parent's vector for every beam that moves there and only
// then stores -- at most 8 vectors in registers, no scratch copy, no second launch.  Layouts as kernels_kvfork.hip, from a start slot:
//   K  [kv][C][R][64] words: a vector is 4 neighbouring SLOTS of one row; vectors that straddle from[b] or n are stored dword-wise
//   V  [kv][C * 64][R] words: a vector lies inside one slot; slots [from[b], n) are one contiguous run
// Integer loads and stores on pointers typed global: NaN payloads pass, and f32 / f16 caches differ in R alone.
#include <cstring>
#include <new>

#include "beam_rule.hpp"
#include "common.hpp"

namespace bitnet_hip {
namespace {

using BeamState = bitnet_hip_beam_state;
using BeamMember = bitnet_hip_beam_member;
using LogprobRecord = bitnet_hip_logprob_record;

constexpr int kSelThreads = 256;
constexpr int kStateWords = sizeof(BeamState) / 4;
static_assert(sizeof(BeamState) == 4 * (12 + 4 * 8 + 64 + 6 * 8), "state layout: no padding (tests/beam_ref.py words())");
static_assert(kBeamCands <= kSelThreads && 2 * kBeamMax <= BITNET_HIP_LOGPROB_TOP_MAX && kBeamMax == kBatchMax, "a thread per candidate; the tap holds 2B entries");
static_assert(sizeof(BeamMember) == 32, "member layout");

__global__ __launch_bounds__(kSelThreads) void k_beam_select(BeamState *st, const float *len_weight, int32_t *pool_tok, const BeamMember *members, int B) {
    __shared__ BeamState s;
    __shared__ BeamMember m[kBeamMax];
    __shared__ float cs[kBeamCands], ws[2 * kBeamMax];
    __shared__ int wi[2 * kBeamMax], wt[2 * kBeamMax];
    __shared__ BeamWalkTmp walk_tmp;
    __shared__ int ok;
    const int tid = threadIdx.x;
    for (int i = tid; i < kStateWords; i += kSelThreads) reinterpret_cast<uint32_t *>(&s)[i] = reinterpret_cast<const uint32_t *>(st)[i];
    if (tid < B) m[tid] = members[tid];
    __syncthreads();
    B = min(B, min(s.n_beams, kBeamMax));  // the entry point compared them already

    if (s.done) {  // FROZEN: the queued step is undone by putting the positions back; nothing else moves
        if (tid < B && m[tid].pos_dev) {
            const int q = *m[tid].pos_dev;
            if (q >= 1) *m[tid].pos_dev = q - 1;
        }
        if (tid == 0) {
            st->stepped = 0;
            st->frozen_steps = s.frozen_steps < 0x7fffffff ? s.frozen_steps + 1 : s.frozen_steps;
        }
        return;
    }

    // every index that comes out of device memory, before any use of it
    if (tid == 0) {
        bool good = true;
        int q = 0;
        for (int b = 0; b < B; ++b) good = good && m[b].records_dev && m[b].pos_dev && m[b].history_dev;
        if (good) {
            q = *m[0].pos_dev;
            for (int b = 0; b < B; ++b) good = good && *m[b].pos_dev == q && q >= 1 && (uint32_t)q < m[b].capacity;
            good = good && s.pool_n >= 0 && s.pool_n <= B && s.prompt_pos >= 0 && s.gen_len >= 0 && s.gen_len < s.max_new_tokens && (long long)q - 1 == (long long)s.prompt_pos + s.gen_len;
        }
        ok = good ? q : 0;
    }
    __syncthreads();
    const int q = ok;
    if (q == 0) {
        if (tid == 0) st->done = s.done | BITNET_HIP_BEAM_ERR_RANGE, st->stepped = 0;
        return;
    }
    const int p = q - 1, P = s.prompt_pos, n = 2 * B * B;

    // candidates, then each one's place in the order
    const int cb = tid / (2 * B), cj = tid % (2 * B);
    const LogprobRecord *rec = tid < n ? static_cast<const LogprobRecord *>(m[cb].records_dev) + q : nullptr;
    if (rec) cs[tid] = beam_cand(s.score[cb], rec->top_logit[cj], rec->lse);
    __syncthreads();
    if (rec) {
        const int r = beam_rank(cs, n, tid);
        if (r < 2 * B) ws[r] = cs[tid], wi[r] = tid, wt[r] = rec->top_id[cj];
    }
    __syncthreads();
    if (tid == 0) beam_walk(s, len_weight, ws, wi, wt, p, walk_tmp);
    __syncthreads();

    // the tokens of every pool entry this step wrote: its source beam's generated tokens as the histories still hold them, then its last token
    const int max_new = s.max_new_tokens;
    for (int i = 0; i < s.pool_n; ++i) {
        const int src = s.pool_src[i], len = s.pool_len[i];
        if (src < 0 || src >= B || len < 1 || len > max_new) continue;
        int32_t *out = pool_tok + (size_t)i * max_new;
        const int32_t *h = m[src].history_dev + P + 1;
        for (int k = tid; k < len - 1; k += kSelThreads) out[k] = h[k];  // P + 1 + k <= p
        if (tid == 0) out[len - 1] = s.pool_last[i];
    }
    __syncthreads();  // the histories are read; now they move

    int lo = p + 1;
    for (int b = 0; b < B; ++b)
        if (s.parent[b] != b) lo = min(lo, max(s.from[b], 0));
    for (int i = lo + tid; i <= p; i += kSelThreads) {
        int32_t t[kBeamMax];
#pragma unroll
        for (int b = 0; b < kBeamMax; ++b)
            if (b < B && s.parent[b] != b && i >= s.from[b]) t[b] = m[s.parent[b]].history_dev[i];
#pragma unroll
        for (int b = 0; b < kBeamMax; ++b)
            if (b < B && s.parent[b] != b && i >= s.from[b]) m[b].history_dev[i] = t[b];
    }
    if (tid < B && s.token[tid] >= 0) m[tid].history_dev[q] = s.token[tid];  // over the greedy pick's entry; q < capacity
    for (int i = tid; i < kStateWords; i += kSelThreads) reinterpret_cast<uint32_t *>(st)[i] = reinterpret_cast<const uint32_t *>(&s)[i];
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
__device__ __forceinline__ g_u32x4 *as_global4(const void *p) { return reinterpret_cast<g_u32x4 *>(reinterpret_cast<uintptr_t>(p)); }

struct KvPermuteArgs {
    void *const *k, *const *v;  // [n_beams][n_layers]
    const BeamState *st;
    unsigned n_layers, n_beams, n_kv, rows;  // rows = R above
    unsigned parts, key_bound;               // workgroups per segment; n_slots <= key_bound
    size_t head_words;                       // C * 64 * R
};

constexpr int kPermThreads = 256;
constexpr int kPermVecs = 4;  // vectors a thread owns
constexpr size_t kPermTile = (size_t)kPermThreads * kPermVecs;

__global__ __launch_bounds__(kPermThreads) void k_kv_permute(const KvPermuteArgs a) {
    const BeamState *st = a.st;
    if (!st->stepped) return;  // a frozen step, a range error, a fresh reset: nothing moved
    const int n = min(max(st->n_slots, 0), (int)a.key_bound);
    const unsigned seg = blockIdx.x / a.parts, part = blockIdx.x % a.parts;
    const unsigned is_v = seg & 1u, kv = (seg >> 1) % a.n_kv, layer = (seg >> 1) / a.n_kv;
    const int B = (int)a.n_beams;

    int from[kBeamMax];  // n: this beam does not move
    int fmin = n;
#pragma unroll
    for (int b = 0; b < kBeamMax; ++b) {
        from[b] = n;
        if (b < B) {
            const int par = st->parent[b];
            if (par >= 0 && par < B && par != b) from[b] = min(max(st->from[b], 0), n);
        }
        fmin = min(fmin, from[b]);
    }
    if (fmin >= n) return;

    // this workgroup's vectors of the segment, against the vectors slots [fmin, n) occupy
    const size_t r4 = a.rows / 4, chunk4 = (size_t)a.rows * 16;
    const size_t lo = is_v ? (size_t)fmin * r4 : (size_t)(fmin / 64) * chunk4;
    const size_t hi = is_v ? (size_t)n * r4 : (size_t)((n + 63) / 64) * chunk4;
    const size_t tile = (size_t)part * kPermTile;
    if (tile >= hi || tile + kPermTile <= lo) return;

    const size_t base4 = (size_t)kv * (a.head_words / 4);
    void *const *table = is_v ? a.v : a.k;
    g_u32x4 *src[kBeamMax], *dst[kBeamMax];
#pragma unroll
    for (int b = 0; b < kBeamMax; ++b) {
        src[b] = dst[b] = nullptr;
        if (from[b] < n) {  // implies b < B and a parent inside [0, B)
            src[b] = as_global4(table[(size_t)st->parent[b] * a.n_layers + layer]) + base4;
            dst[b] = as_global4(table[(size_t)b * a.n_layers + layer]) + base4;
        }
    }

    for (int u = 0; u < kPermVecs; ++u) {
        const size_t i = tile + (size_t)u * kPermThreads + threadIdx.x;
        if (i < lo || i >= hi) continue;
        // the slots of this vector's four words: V one slot, K four neighbouring ones
        const int s0 = is_v ? (int)(i / r4) : (int)(i / chunk4) * 64 + (int)(i % 16) * 4;
        const int step = is_v ? 0 : 1;
        unsigned mask[kBeamMax];
        u32x4 t[kBeamMax];
#pragma unroll
        for (int b = 0; b < kBeamMax; ++b) {
            mask[b] = 0;
            if (from[b] < n) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int slot = s0 + w * step;
                    mask[b] |= (slot >= from[b] && slot < n) ? 1u << w : 0u;
                }
                if (mask[b]) t[b] = src[b][i];
            }
        }
        // every load stands before the first store: a parent's vector may be another beam's destination
#pragma unroll
        for (int b = 0; b < kBeamMax; ++b) {
            if (!mask[b]) continue;
            if (mask[b] == 15u) {
                dst[b][i] = t[b];
            } else {
                g_u32 *d = reinterpret_cast<g_u32 *>(dst[b] + i);
                if (mask[b] & 1u) d[0] = t[b].x;
                if (mask[b] & 2u) d[1] = t[b].y;
                if (mask[b] & 4u) d[2] = t[b].z;
                if (mask[b] & 8u) d[3] = t[b].w;
            }
        }
    }
}

}  // namespace
}  // namespace bitnet_hip

using namespace bitnet_hip;

// one device allocation: the state, len_weight[max_new + 1], the pool's tokens [kBeamMax][max_new]
struct bitnet_hip_beam {
    bitnet_hip_beam_state *dev = nullptr;
    float *len_weight = nullptr;
    int32_t *pool_tok = nullptr;
    int n_beams = 0, eos = -1, max_new = 0;
};

namespace {
constexpr size_t kBeamMaxNew = (size_t)1 << 20;

int beam_upload_reset(bitnet_hip_beam *bm, int32_t prompt_pos) {
    bitnet_hip_beam_state h;
    memset(&h, 0, sizeof(h));
    h.n_beams = bm->n_beams, h.eos = bm->eos, h.max_new_tokens = bm->max_new;
    beam_reset(h, prompt_pos);
    BH_HIP_TRY(hipDeviceSynchronize());
    BH_HIP_TRY(hipMemcpy(bm->dev, &h, sizeof(h), hipMemcpyHostToDevice));
    return BITNET_HIP_OK;
}
}  // namespace

extern "C" {

int bitnet_hip_beam_create(size_t n_beams, int32_t eos, size_t max_new_tokens, const float *len_weight, bitnet_hip_beam **out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to beam_create");
    *out = nullptr;
    if (n_beams == 0 || n_beams > BITNET_HIP_BEAM_MAX)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "beam_create: n_beams %zu must be 1..%d", n_beams, BITNET_HIP_BEAM_MAX);
    if (eos < -1) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "beam_create: eos %d (-1 = none)", eos);
    if (max_new_tokens == 0 || max_new_tokens > kBeamMaxNew)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "beam_create: max_new_tokens %zu must be 1..%zu", max_new_tokens, kBeamMaxNew);
    if (!len_weight) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null len_weight passed to beam_create");
    bitnet_hip_beam *bm = new (std::nothrow) bitnet_hip_beam;
    if (!bm) return set_error(BITNET_HIP_ERR_EXECUTION, "beam_create: out of host memory");
    bm->n_beams = (int)n_beams, bm->eos = eos, bm->max_new = (int)max_new_tokens;
    const size_t lw_bytes = (max_new_tokens + 1) * sizeof(float), tok_bytes = (size_t)kBeamMax * max_new_tokens * sizeof(int32_t);
    char *mem = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&mem), sizeof(bitnet_hip_beam_state) + lw_bytes + tok_bytes);
    if (e == hipSuccess) e = hipMemset(mem, 0, sizeof(bitnet_hip_beam_state) + lw_bytes + tok_bytes);
    if (e == hipSuccess) e = hipMemcpy(mem + sizeof(bitnet_hip_beam_state), len_weight, lw_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        delete bm;
        return set_error(BITNET_HIP_ERR_GPU, "beam_create: %s", hipGetErrorString(e));
    }
    bm->dev = reinterpret_cast<bitnet_hip_beam_state *>(mem);
    bm->len_weight = reinterpret_cast<float *>(mem + sizeof(bitnet_hip_beam_state));
    bm->pool_tok = reinterpret_cast<int32_t *>(mem + sizeof(bitnet_hip_beam_state) + lw_bytes);
    if (int rc = beam_upload_reset(bm, 0)) {
        (void)hipFree(mem);
        delete bm;
        return rc;
    }
    *out = bm;
    return BITNET_HIP_OK;
}

void bitnet_hip_beam_destroy(bitnet_hip_beam *bm) {
    if (!bm) return;
    if (bm->dev) (void)hipFree(bm->dev);
    delete bm;
}

int bitnet_hip_beam_reset(bitnet_hip_beam *bm, int32_t prompt_pos) {
    if (!bm) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null beam passed to beam_reset");
    if (prompt_pos < 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "beam_reset: prompt_pos %d is negative", prompt_pos);
    return beam_upload_reset(bm, prompt_pos);
}

int bitnet_hip_beam_read(bitnet_hip_beam *bm, bitnet_hip_beam_state *out, int32_t *pool_tokens) {
    if (!bm) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null beam passed to beam_read");
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null output passed to beam_read");
    BH_HIP_TRY(hipDeviceSynchronize());
    BH_HIP_TRY(hipMemcpy(out, bm->dev, sizeof(*out), hipMemcpyDeviceToHost));
    if (pool_tokens) BH_HIP_TRY(hipMemcpy(pool_tokens, bm->pool_tok, (size_t)kBeamMax * bm->max_new * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BITNET_HIP_OK;
}

int bitnet_hip_beam_done_dev(bitnet_hip_beam *bm, const int32_t **done_dev) {
    if (!bm) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null beam passed to beam_done_dev");
    if (!done_dev) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null output passed to beam_done_dev");
    *done_dev = &bm->dev->done;
    return BITNET_HIP_OK;
}

int bitnet_hip_beam_select_dev(bitnet_hip_beam *bm, const bitnet_hip_beam_member *members_dev, size_t n_beams, void *stream) {
    if (!members_dev) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null member table passed to beam_select_dev");
    if (n_beams == 0 || n_beams > BITNET_HIP_BEAM_MAX)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "beam_select_dev: n_beams %zu must be 1..%d", n_beams, BITNET_HIP_BEAM_MAX);
    if (!bm) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null beam passed to beam_select_dev");
    if ((int)n_beams != bm->n_beams)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "beam_select_dev: n_beams %zu, the state was created for %d", n_beams, bm->n_beams);
    hipLaunchKernelGGL(k_beam_select, dim3(1), dim3(kSelThreads), 0, (hipStream_t)stream, bm->dev, bm->len_weight, bm->pool_tok, members_dev, (int)n_beams);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

int bitnet_hip_kv_permute_dev(void *const *k_ptrs_dev, void *const *v_ptrs_dev, bitnet_hip_beam *bm, size_t n_layers, size_t n_beams, size_t n_kv_heads,
                              size_t head_dim, size_t max_pos, size_t key_bound, int flags, void *stream) {
    if (!k_ptrs_dev || !v_ptrs_dev) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null pointer passed to kv_permute_dev");
    if (n_layers == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "kv_permute_dev: n_layers 0");
    if (n_beams == 0 || n_beams > BITNET_HIP_BEAM_MAX)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "kv_permute_dev: n_beams %zu must be 1..%d", n_beams, BITNET_HIP_BEAM_MAX);
    if (head_dim != 128) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "kv_permute_dev: head_dim %zu unsupported (128)", head_dim);
    if (n_kv_heads == 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "kv_permute_dev: num_key_value_heads 0");
    if (flags & ~BITNET_HIP_ATTN_KV_F16)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "kv_permute_dev: flags 0x%x (0 or BITNET_HIP_ATTN_KV_F16)", flags);
    if (key_bound > max_pos)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "KV cache overflow: key_bound %zu, max_pos %zu", key_bound, max_pos);
    const size_t rows = (flags & BITNET_HIP_ATTN_KV_F16) ? head_dim / 2 : head_dim;
    size_t slots = 0, head_words = 0, cache_bytes = 0, segments = 0, blocks = 0;
    if (max_pos > (size_t)0x7fffffff - 63 || __builtin_add_overflow(max_pos, (size_t)63, &slots) || __builtin_mul_overflow(slots / 64 * 64, rows, &head_words) ||
        __builtin_mul_overflow(head_words, n_kv_heads, &cache_bytes) || __builtin_mul_overflow(cache_bytes, sizeof(uint32_t), &cache_bytes) ||
        __builtin_mul_overflow(n_layers, n_kv_heads, &segments) || __builtin_mul_overflow(segments, (size_t)2, &segments) || segments >= ((size_t)1 << 24) ||
        __builtin_mul_overflow(n_layers, n_beams, &slots))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (kv_permute_dev: n_layers %zu, n_kv_heads %zu, max_pos %zu)",
                         n_layers, n_kv_heads, max_pos);
    // the geometry first, the state last: every refusal above names an argument and needs no state to show it
    if (!bm) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "Null beam passed to kv_permute_dev");
    if ((int)n_beams != bm->n_beams)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "kv_permute_dev: n_beams %zu, the state was created for %d", n_beams, bm->n_beams);
    if (key_bound == 0) return BITNET_HIP_OK;  // no slot can have moved
    // a segment's vectors below key_bound (K's whole chunks bound V's run too), in tiles of one workgroup
    const size_t parts = div_ceil(div_ceil(key_bound, (size_t)64) * rows * 16, kPermTile);
    if (__builtin_mul_overflow(segments, parts, &blocks) || blocks > (size_t)0x7fffffff)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "dimensions too large for this library (kv_permute_dev: %zu segments of %zu workgroups)", segments, parts);
    KvPermuteArgs a;
    a.k = k_ptrs_dev, a.v = v_ptrs_dev, a.st = bm->dev;
    a.n_layers = (unsigned)n_layers, a.n_beams = (unsigned)n_beams, a.n_kv = (unsigned)n_kv_heads, a.rows = (unsigned)rows;
    a.parts = (unsigned)parts, a.key_bound = (unsigned)key_bound, a.head_words = head_words;
    hipLaunchKernelGGL(k_kv_permute, dim3((unsigned)blocks), dim3(kPermThreads), 0, (hipStream_t)stream, a);
    BH_HIP_TRY(hipGetLastError());
    return BITNET_HIP_OK;
}

}  // extern "C"
