// kernels_gramc.hip -- the grammar compiler on the device (include/bitnet_hip_grammar_compile.h): a byte-level DFA and the vocabulary's byte
// strings in, the class-compressed token automaton of the sampler's GRAMMAR stage out (gfx950, wave64).
//
// The numpy compiler (bitnet-rs_amd/grammar.py token_automaton) builds the dense [vocab, states] column array and sorts its rows.  Here that
// array never exists: the tokens are partitioned by EXACT PARTITION REFINEMENT over tiles of kTS states.
//   round r (states [r kTS, r kTS + kTS)), two launches:
//     k_gramc_walk    a lane owns a token: it reads the token's bytes once, in aligned 16-byte pieces, and walks them from the kTS states of the
//                     tile at once -- kTS state words in registers, one gather per state and byte into the DFA table (1 KiB per state, served
//                     from L2; a walk ends early once all kTS states are dead).  vals[token][kTS] goes out as eight 16-byte stores.
//     k_gramc_refine  the key of token t is (class so far, vals[t][0 .. kTS)): 33 words.  An open-addressing table of 2 * vocab (rounded up to a
//                     power of two) int32 slots holds REPRESENTATIVE TOKEN IDS: a lane claims an empty slot with a compare-and-swap (after a plain look), or compares
//                     its key with the representative's, word for word -- the keys were written by earlier launches, so they are stable -- and
//                     on a match takes the SLOT INDEX as its new class; on a mismatch it probes on.  The hash only picks the first slot;
//                     equality is exact.  Between rounds a class id is just a slot index: only equality matters.  Classes are read from one
//                     buffer and written to the other, so no lane reads a class word another lane is writing.
//   after the last round the partition is the partition by whole columns, and
//     k_gramc_cmin    turns each class's slot into the smallest token id of the class (atomic min over the representative it already holds);
//     k_gramc_number  one workgroup scans the leader flags (t is the smallest of its class) in token order, 1024 tokens per step by wave ballots
//                     and a 16-entry LDS exchange: a leader's rank is its class's final id -- classes are numbered by smallest token id,
//                     deterministic whatever the races of the rounds were.  The class count (or the error mark) is the one word the host reads;
//     k_gramc_assign  token_class[t] = rank of t's leader, uint16;
//     k_gramc_next    one walk per (class leader, state): next[state][class], the EOS column and the end-state row included;
//     k_gramc_allow   the per-state class bitmaps from the device table -- the step bitnet_hip_grammar_create shares (grammar_derive_allow).
// Not built: a byte -> byte-class map staged in LDS (it pays when distinct byte columns are few; the table rows the walks touch stay in L2 at
// the sizes measured, EXPERIMENTS.md section 38).
//
// Safety: every loop has a bound known at launch (a walk: the token's length from the offsets, clamped to the upload's total; a probe sequence: the
// table's size -- a lane that exhausts it sets the error word and the host returns ERR_GPU); no lane spins or waits for another, no kernel waits
// for another workgroup; every index read from device memory (offsets, slots, representatives, leaders, states) is range-checked before it
// indexes anything; the global atomics are the ordinary vector ones.
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"
#include "grammar_handle.hpp"

namespace bitnet_hip {
namespace {

constexpr int kTS = 32;                // states per tile: a lane's kTS state words stay in registers
constexpr int kNT = 256;               // threads per workgroup of the per-token and per-cell kernels
constexpr int kNumberNT = 1024;        // k_gramc_number: one workgroup, 16 waves
constexpr int kMaxClasses = BITNET_HIP_GRAMMAR_MAX_CLASSES;
constexpr size_t kMaxVocab = (size_t)1 << 20, kMaxCells = (size_t)1 << 24, kMaxBytes = 0x7fffffffu;
constexpr uint32_t kCountError = 0xffffffffu;  // the count word when a refine lane found no slot
static_assert(kTS % 4 == 0, "vals rows go out in 16-byte stores");

// what every walk reads; nothing in it changes during a compile
struct GcIn {
    const uint8_t *bytes;  // the vocabulary's bytes; the allocation ends on a 16-byte piece
    const uint32_t *off;   // [vocab + 1]
    const int32_t *dfa;    // [n][256], entries in [-1, n) (checked on the host)
    const uint8_t *acc;    // [n]
    int vocab, n, eos;     // n: the DFA's states (the end state is n); eos: -1 for none
    uint32_t total;        // bytes in the upload
};

// cur[j] = where token t's bytes lead from state s0 + j of the token automaton (n + 1 states; beyond them: -1)
template <int TS>
__device__ __forceinline__ void walk_cols(const GcIn &a, int t, int s0, int (&cur)[TS]) {
    uint32_t lo = a.off[t], hi = a.off[t + 1];
    hi = hi > a.total ? a.total : hi;
    lo = lo > hi ? hi : lo;
    const bool eos = t == a.eos;
#pragma unroll
    for (int j = 0; j < TS; ++j) {
        const int s = s0 + j;
        int c = -1;
        if (eos) {
            if (s < a.n) c = a.acc[s] ? a.n : -1;
            else if (s == a.n) c = a.n;
        } else if (s < a.n && hi > lo) {
            c = s;
        }
        cur[j] = c;
    }
    if (eos) return;
    uint4 piece = {0u, 0u, 0u, 0u};
    for (uint32_t p = lo; p < hi; ++p) {
        const uint32_t k = p & 15u;
        if (p == lo || k == 0) piece = *reinterpret_cast<const uint4 *>(a.bytes + (p - k));
        const uint32_t w = k < 8 ? (k < 4 ? piece.x : piece.y) : (k < 12 ? piece.z : piece.w);
        const int b = (int)((w >> ((k & 3u) * 8u)) & 255u);
        int all = -1;
#pragma unroll
        for (int j = 0; j < TS; ++j) {
            const int c = cur[j];
            cur[j] = (unsigned)c < (unsigned)a.n ? a.dfa[c * 256 + b] : -1;
            all &= cur[j];
        }
        if (all == -1) break;  // every state of the tile is dead: -1 is absorbing
    }
}

__global__ __launch_bounds__(kNT) void k_gramc_fill(int32_t *__restrict__ p, uint32_t n, int32_t v) {
    const uint32_t i = blockIdx.x * kNT + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(kNT) void k_gramc_walk(GcIn a, int s0, int32_t *__restrict__ vals) {
    const int t = (int)(blockIdx.x * kNT + threadIdx.x);
    if (t >= a.vocab) return;
    int cur[kTS];
    walk_cols<kTS>(a, t, s0, cur);
    int4 *o = reinterpret_cast<int4 *>(vals + (size_t)t * kTS);
#pragma unroll
    for (int j = 0; j < kTS / 4; ++j) o[j] = int4{cur[4 * j], cur[4 * j + 1], cur[4 * j + 2], cur[4 * j + 3]};
}

__device__ __forceinline__ uint32_t mix(uint32_t h, uint32_t w) {
    h = (h ^ w) * 0x9e3779b1u;
    return h ^ (h >> 15);
}

__global__ __launch_bounds__(kNT) void k_gramc_refine(const int32_t *__restrict__ vals, const int32_t *__restrict__ cls_in, int32_t *__restrict__ cls_out,
                                                      int32_t *table, uint32_t mask, int vocab, uint32_t *err) {
    const int t = (int)(blockIdx.x * kNT + threadIdx.x);
    if (t >= vocab) return;
    const int c0 = cls_in[t];
    int4 key[kTS / 4];
    uint32_t h = mix(0x811c9dc5u, (uint32_t)c0);
#pragma unroll
    for (int j = 0; j < kTS / 4; ++j) {
        key[j] = reinterpret_cast<const int4 *>(vals + (size_t)t * kTS)[j];
        h = mix(mix(mix(mix(h, (uint32_t)key[j].x), (uint32_t)key[j].y), (uint32_t)key[j].z), (uint32_t)key[j].w);
    }
    h = mix(h, h >> 7);
    uint32_t slot = h & mask;
    int found = -1;
    for (uint32_t probe = 0; probe <= mask; ++probe) {  // at most one pass over the table
        // a plain look first: slots never change once taken, and the tokens of a large class (the dead column's) would otherwise queue
        // up on one address with a compare-and-swap each
        int r = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (r == -1) r = atomicCAS(&table[slot], -1, t);
        if (r == -1 || r == t) {
            found = (int)slot;
            break;
        }
        if ((unsigned)r < (unsigned)vocab && cls_in[r] == c0) {
            bool same = true;
#pragma unroll
            for (int j = 0; j < kTS / 4; ++j) {
                const int4 q = reinterpret_cast<const int4 *>(vals + (size_t)r * kTS)[j];
                same = same && q.x == key[j].x && q.y == key[j].y && q.z == key[j].z && q.w == key[j].w;
            }
            if (same) {
                found = (int)slot;
                break;
            }
        }
        slot = (slot + 1) & mask;
    }
    if (found < 0) {
        atomicOr(err, 1u);
        found = 0;
    }
    cls_out[t] = found;
}

// table[slot of a class] = the smallest token id of the class (it holds a member already)
__global__ __launch_bounds__(kNT) void k_gramc_cmin(const int32_t *__restrict__ cls, int32_t *table, uint32_t mask, int vocab) {
    const int t = (int)(blockIdx.x * kNT + threadIdx.x);
    if (t >= vocab) return;
    const uint32_t c = (uint32_t)cls[t];
    if (c <= mask && __hip_atomic_load(&table[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > t) atomicMin(&table[c], t);  // the look spares most atomics
}

// One workgroup: rank[leader] = leaders before it in token order = the class's final id; leaders[id] = the leader (ids below kMaxClasses only);
// *count = the number of classes, or kCountError.
__global__ __launch_bounds__(kNumberNT) void k_gramc_number(const int32_t *__restrict__ cls, const int32_t *__restrict__ table, uint32_t mask, int vocab,
                                                            int32_t *__restrict__ rank, int32_t *__restrict__ leaders, const uint32_t *__restrict__ err,
                                                            uint32_t *__restrict__ count) {
    __shared__ uint32_t wsum[kNumberNT / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t base = 0;
    for (int t0 = 0; t0 < vocab; t0 += kNumberNT) {
        const int t = t0 + tid;
        bool lead = false;
        if (t < vocab) {
            const uint32_t c = (uint32_t)cls[t];
            lead = c <= mask && table[c] == t;
        }
        const unsigned long long m = __ballot(lead);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kNumberNT / 64; ++w) {
            const uint32_t v = wsum[w];
            tot += v;
            before += w < wave ? v : 0u;
        }
        if (lead) {
            const uint32_t r = base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            rank[t] = (int32_t)r;
            if (r < (uint32_t)kMaxClasses) leaders[r] = t;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) *count = *err ? kCountError : base;
}

__global__ __launch_bounds__(kNT) void k_gramc_assign(const int32_t *__restrict__ cls, const int32_t *__restrict__ table, uint32_t mask, int vocab,
                                                      const int32_t *__restrict__ rank, int n_classes, uint16_t *__restrict__ token_class) {
    const int t = (int)(blockIdx.x * kNT + threadIdx.x);
    if (t >= vocab) return;
    const uint32_t c = (uint32_t)cls[t];
    const int l = c <= mask ? table[c] : -1;
    const int r = (unsigned)l < (unsigned)vocab ? rank[l] : 0;
    token_class[t] = (uint16_t)((unsigned)r < (unsigned)n_classes ? r : 0);
}

__global__ __launch_bounds__(kNT) void k_gramc_next(GcIn a, const int32_t *__restrict__ leaders, int n_classes, uint32_t cells, int32_t *__restrict__ next) {
    const uint32_t i = blockIdx.x * kNT + threadIdx.x;
    if (i >= cells) return;
    const int s = (int)(i / (uint32_t)n_classes), c = (int)(i % (uint32_t)n_classes);
    const int t = leaders[c];
    int cur[1] = {-1};
    if ((unsigned)t < (unsigned)a.vocab) walk_cols<1>(a, t, s, cur);
    next[i] = cur[0];
}

__global__ __launch_bounds__(kNT) void k_gramc_allow(const int32_t *__restrict__ next, uint32_t n_classes, uint32_t row_words, uint32_t words,
                                                     uint32_t *__restrict__ allow) {
    const uint32_t i = blockIdx.x * kNT + threadIdx.x;
    if (i >= words) return;
    const uint32_t s = i / row_words, c0 = (i % row_words) * 32u;
    const int32_t *row = next + (size_t)s * n_classes;
    uint32_t bits = 0;
    for (uint32_t b = 0; b < 32u; ++b)
        if (c0 + b < n_classes && row[c0 + b] >= 0) bits |= 1u << b;
    allow[i] = bits;
}

inline unsigned blocks_for(size_t n) { return (unsigned)div_ceil(n, (size_t)kNT); }

// the compile's temporaries: freed on every way out
struct DevTmp {
    std::vector<void *> all;
    ~DevTmp() {
        for (void *p : all) (void)hipFree(p);
    }
    template <class T>
    hipError_t get(T **p, size_t bytes) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) all.push_back(q);
        *p = static_cast<T *>(q);
        return e;
    }
};

}  // namespace

hipError_t grammar_derive_allow(const int32_t *next_dev, size_t n_states, size_t n_classes, uint32_t *allow_dev) {
    const size_t cw = (n_classes + 31) / 32, words = n_states * cw;  // at most 2^24 cells: every count fits 32 bits
    hipLaunchKernelGGL(k_gramc_allow, dim3(blocks_for(words)), dim3(kNT), 0, nullptr, next_dev, (uint32_t)n_classes, (uint32_t)cw, (uint32_t)words, allow_dev);
    return hipGetLastError();
}

}  // namespace bitnet_hip

using namespace bitnet_hip;

struct bitnet_hip_vocab {
    uint8_t *bytes = nullptr;  // device: the byte strings, then padding to the end of a 16-byte piece
    uint32_t *off = nullptr;   // device [vocab + 1]
    size_t vocab = 0, total = 0;
};

extern "C" {

int bitnet_hip_vocab_create(const uint8_t *bytes, const uint64_t *offsets, size_t vocab, bitnet_hip_vocab **out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: out is NULL");
    *out = nullptr;
    if (!bytes) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: bytes is NULL");
    if (!offsets) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: offsets is NULL");
    if (vocab < 1 || vocab > kMaxVocab) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: vocab must be in 1..%zu, got %zu", kMaxVocab, vocab);
    if (offsets[0] != 0) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: offsets[0] must be 0, got %llu", (unsigned long long)offsets[0]);
    for (size_t t = 0; t < vocab; ++t)
        if (offsets[t + 1] < offsets[t])
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: offsets[%zu] = %llu is below offsets[%zu] = %llu", t + 1,
                             (unsigned long long)offsets[t + 1], t, (unsigned long long)offsets[t]);
    if (offsets[vocab] > kMaxBytes)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "vocab_create: the total offsets[vocab] = %llu is above %zu bytes", (unsigned long long)offsets[vocab],
                         kMaxBytes);
    std::vector<uint32_t> off;
    bitnet_hip_vocab *v = new (std::nothrow) bitnet_hip_vocab();
    try {
        off.assign(offsets, offsets + vocab + 1);  // every entry fits: the offsets rise to a total below 2^31
    } catch (const std::bad_alloc &) {
        delete v;
        v = nullptr;
    }
    if (!v) return set_error(BITNET_HIP_ERR_EXECUTION, "vocab_create: out of host memory");
    v->vocab = vocab;
    v->total = (size_t)offsets[vocab];
    hipError_t e = hipMalloc((void **)&v->bytes, ((v->total + 15) & ~(size_t)15) + 16);
    if (e == hipSuccess) e = hipMalloc((void **)&v->off, off.size() * sizeof(uint32_t));
    if (e == hipSuccess && v->total) e = hipMemcpy(v->bytes, bytes, v->total, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(v->off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        bitnet_hip_vocab_destroy(v);
        return set_error(BITNET_HIP_ERR_GPU, "vocab_create: %s", hipGetErrorString(e));
    }
    *out = v;
    return BITNET_HIP_OK;
}

void bitnet_hip_vocab_destroy(bitnet_hip_vocab *v) {
    if (!v) return;
    if (v->bytes) (void)hipFree(v->bytes);
    if (v->off) (void)hipFree(v->off);
    delete v;
}

int bitnet_hip_grammar_compile(const bitnet_hip_vocab *v, const bitnet_hip_dfa_desc *dfa, int32_t eos_id, bitnet_hip_grammar **out) {
    if (!out) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: out is NULL");
    *out = nullptr;
    if (!dfa) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: dfa is NULL");
    if (!dfa->next) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: next is NULL");
    if (!dfa->accepting) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: accepting is NULL");
    const size_t n = dfa->n_states;
    if (n < 1 || n > (size_t)BITNET_HIP_GRAMMAR_MAX_STATES - 1)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: n_states must be in 1..%d (the end state is added), got %zu",
                         BITNET_HIP_GRAMMAR_MAX_STATES - 1, n);
    if (dfa->start < 0 || (size_t)dfa->start >= n)
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: start %d is outside [0, n_states = %zu)", dfa->start, n);
    for (size_t i = 0; i < n * 256; ++i)
        if (dfa->next[i] < -1 || dfa->next[i] >= (int32_t)n)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: next[%zu][%zu] is %d, outside [-1, n_states = %zu)", i / 256, i % 256,
                             dfa->next[i], n);
    if (!v) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: vocab handle is NULL");
    const size_t V = v->vocab;
    if (eos_id < -1 || (eos_id >= 0 && (size_t)eos_id >= V))
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: eos_id %d is outside [-1, vocab = %zu)", eos_id, V);

    const size_t S = n + 1, rounds = div_ceil(S, (size_t)kTS);
    size_t slots = 64;
    while (slots < 2 * V) slots *= 2;  // at most 2^21
    const uint32_t mask = (uint32_t)(slots - 1);
    Grammar *g = new (std::nothrow) Grammar();
    if (!g) return set_error(BITNET_HIP_ERR_EXECUTION, "grammar_compile: out of host memory");
    g->vocab = (int)V;
    g->n_states = (int)S;
    DevTmp tmp;
    int32_t *d_dfa = nullptr, *vals = nullptr, *cls_a = nullptr, *cls_b = nullptr, *table = nullptr, *leaders = nullptr;
    uint8_t *d_acc = nullptr;
    uint32_t *words = nullptr;  // [0] the error word, [1] the class count
    hipError_t e = tmp.get(&d_dfa, n * 256 * sizeof(int32_t));
    if (e == hipSuccess) e = tmp.get(&d_acc, n);
    if (e == hipSuccess) e = tmp.get(&vals, V * kTS * sizeof(int32_t));
    if (e == hipSuccess) e = tmp.get(&cls_a, V * sizeof(int32_t));
    if (e == hipSuccess) e = tmp.get(&cls_b, V * sizeof(int32_t));
    if (e == hipSuccess) e = tmp.get(&table, slots * sizeof(int32_t));
    if (e == hipSuccess) e = tmp.get(&leaders, (size_t)kMaxClasses * sizeof(int32_t));
    if (e == hipSuccess) e = tmp.get(&words, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&g->cls, V * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(d_dfa, dfa->next, n * 256 * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_acc, dfa->accepting, n, hipMemcpyHostToDevice);
    const GcIn in{v->bytes, v->off, d_dfa, d_acc, (int)V, (int)n, (int)eos_id, (uint32_t)v->total};
    const dim3 tok_grid(blocks_for(V)), nt(kNT);
    auto launched = [&e]() { return e == hipSuccess && (e = hipGetLastError()) == hipSuccess; };
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gramc_fill, tok_grid, nt, 0, nullptr, cls_a, (uint32_t)V, 0);
        if (launched()) hipLaunchKernelGGL(k_gramc_fill, dim3(1), nt, 0, nullptr, reinterpret_cast<int32_t *>(words), 2u, 0);
    }
    int32_t *cls_in = cls_a, *cls_out = cls_b;
    for (size_t r = 0; r < rounds && launched(); ++r) {
        hipLaunchKernelGGL(k_gramc_fill, dim3(blocks_for(slots)), nt, 0, nullptr, table, (uint32_t)slots, -1);
        if (launched()) hipLaunchKernelGGL(k_gramc_walk, tok_grid, nt, 0, nullptr, in, (int)(r * kTS), vals);
        if (launched()) hipLaunchKernelGGL(k_gramc_refine, tok_grid, nt, 0, nullptr, vals, cls_in, cls_out, table, mask, (int)V, words);
        std::swap(cls_in, cls_out);  // cls_in: the partition so far; cls_out: free, the ranks go there after the last round
    }
    if (launched()) hipLaunchKernelGGL(k_gramc_cmin, tok_grid, nt, 0, nullptr, cls_in, table, mask, (int)V);
    if (launched()) hipLaunchKernelGGL(k_gramc_number, dim3(1), dim3(kNumberNT), 0, nullptr, cls_in, table, mask, (int)V, cls_out, leaders, words, words + 1);
    uint32_t count = 0;
    if (launched()) e = hipMemcpy(&count, words + 1, sizeof(count), hipMemcpyDeviceToHost);  // the one read; it waits for the launches above
    if (e != hipSuccess || count == kCountError || count == 0) {
        free_grammar(g);
        if (e != hipSuccess) return set_error(BITNET_HIP_ERR_GPU, "grammar_compile: %s", hipGetErrorString(e));
        return set_error(BITNET_HIP_ERR_GPU, "grammar_compile: the class table of %zu slots gave a lane no slot (vocab %zu)", slots, V);
    }
    const size_t NC = count;
    if (NC > (size_t)kMaxClasses || S * NC > kMaxCells) {
        free_grammar(g);
        if (NC > (size_t)kMaxClasses)
            return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: %zu token classes, the limit is %d", NC, kMaxClasses);
        return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_compile: %zu states * %zu classes exceed %zu table entries", S, NC, kMaxCells);
    }
    g->n_classes = (int)NC;
    const size_t cells = S * NC;
    e = hipMalloc((void **)&g->next, cells * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&g->allow, S * ((NC + 31) / 32) * sizeof(uint32_t));
    if (e == hipSuccess) hipLaunchKernelGGL(k_gramc_assign, tok_grid, nt, 0, nullptr, cls_in, table, mask, (int)V, cls_out, (int)NC, g->cls);
    if (launched()) hipLaunchKernelGGL(k_gramc_next, dim3(blocks_for(cells)), nt, 0, nullptr, in, leaders, (int)NC, (uint32_t)cells, g->next);
    if (launched()) e = grammar_derive_allow(g->next, S, NC, g->allow);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    bitnet_hip_grammar *h = e == hipSuccess ? new (std::nothrow) bitnet_hip_grammar{g} : nullptr;
    if (!h) {
        free_grammar(g);
        if (e != hipSuccess) return set_error(BITNET_HIP_ERR_GPU, "grammar_compile: %s", hipGetErrorString(e));
        return set_error(BITNET_HIP_ERR_EXECUTION, "grammar_compile: out of host memory");
    }
    *out = h;
    return BITNET_HIP_OK;
}

int bitnet_hip_grammar_info(const bitnet_hip_grammar *gp, size_t *vocab, size_t *n_states, size_t *n_classes) {
    if (!gp) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_info: grammar is NULL");
    if (vocab) *vocab = (size_t)gp->g->vocab;
    if (n_states) *n_states = (size_t)gp->g->n_states;
    if (n_classes) *n_classes = (size_t)gp->g->n_classes;
    return BITNET_HIP_OK;
}

int bitnet_hip_grammar_read(const bitnet_hip_grammar *gp, uint16_t *token_class, int32_t *next) {
    if (!gp) return set_error(BITNET_HIP_ERR_INVALID_ARGUMENT, "grammar_read: grammar is NULL");
    const Grammar *g = gp->g;
    if (token_class) BH_HIP_TRY(hipMemcpy(token_class, g->cls, (size_t)g->vocab * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (next) BH_HIP_TRY(hipMemcpy(next, g->next, (size_t)g->n_states * (size_t)g->n_classes * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BITNET_HIP_OK;
}

}  // extern "C"
