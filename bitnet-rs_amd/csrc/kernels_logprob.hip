// kernels_logprob.hip -- the generation path's logits tap on the device: per position the chosen token, its raw logit, the row's
// log-sum-exp and the top-N (id, logit) pairs (GenerationConfig::{logits_tap_steps, logits_topk, logits_cb}, crates/bitnet-inference/src/
// config.rs:87-93, called after sampling: engine.rs:1182-1210; the CLI's LogitStep records and their ordering rule, crates/bitnet-cli/src/
// main.rs:1337-1373).
//
// One launch after the pick, in the shape of the sampler's S path (kernels_sample.hip): every workgroup reads its slice of the row once
// (16-byte loads), keeps the slice as order-preserving keys in LDS, and leaves a partial -- the slice maximum, sum exp(l - maximum) and its
// stable top-n_top candidates -- in the entry's scratch; the last workgroup to arrive (select.hpp) merges the partials in workgroup-index
// order, selects and orders the final n_top, reads l[token] and writes the record.  No workgroup waits for another.
//
// The key puts the CLI's "finite first" into the order: a finite logit keeps the sampler's key (fkey: -0.0 and +0.0 merge, as partial_cmp
// compares them equal), every non-finite one gets key 0, below every finite key; block_select / block_keep keep array order among equal keys
// (= ascending id), and the final rank is (key descending, id ascending).  The record's logits are read back from the row, so their bits are
// the row's.  The partition (slice width, workgroup count) depends on the vocabulary alone: k_logprob and k_logprob_batch run one body on
// one partition and leave the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "select.hpp"

namespace bitnet_hip {
namespace {

using LogprobArgs = bitnet_hip_logprob_args;
using LogprobRecord = bitnet_hip_logprob_record;

constexpr int kTop = BITNET_HIP_LOGPROB_TOP_MAX;
constexpr int kMaxWG = 128;        // workgroups per entry, at most
constexpr int kMinSlice = 1024;    // entries per workgroup, at least ...
constexpr int kMaxSlice = 8192;    // ... and at most: (1 << 20) / kMaxWG, 32 KiB of keys in LDS
constexpr int kWantWG = 64;        // workgroups a large vocabulary is cut into (EXPERIMENTS.md 19: 128256 entries -> 64 slices of 2004, fastest of 16 / 32 / 64 / 128)
constexpr int kMaxVocab = 1 << 20;
static_assert(kMaxSlice * kMaxWG >= kMaxVocab && kMaxSlice % 4 == 0 && kMinSlice % 4 == 0, "the slices cover every vocabulary");
static_assert(sizeof(LogprobRecord) == 176 && kTop <= 32, "record layout");

// scratch of one entry: the ticket (16 bytes), the partials [kMaxWG] of 16 bytes, the candidates [kMaxWG][kTop] (key, id)
struct Partial {
    float mx, sum;   // slice maximum (NaN read as -inf) and sum exp(l - mx) over the slice (0 unless mx is finite)
    uint32_t cnt;    // candidates left: min(n_top, entries of the slice)
    uint32_t pad;
};
constexpr size_t kPartialOfs = 16, kCandOfs = kPartialOfs + (size_t)kMaxWG * sizeof(Partial);
constexpr size_t kScratchBytes = kCandOfs + (size_t)kMaxWG * kTop * 8;

// finite first: every non-finite logit ranks below every finite one (fkey of a finite value is >= 0x00800000)
__device__ __forceinline__ uint32_t lkey(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0u : fkey(v); }

// LDS (u32 words): hdr[64]; phase 1: hist[256] | tmp[64] | ... | keys[slice] from word 512; phase 2 (kP2Words): below
constexpr int kP2Ofs = 0, kP2Cnt = kMaxWG + 1, kP2Hist = 320, kP2Tmp = 576, kP2Ck = 640, kP2Ci = kP2Ck + kMaxWG * kTop, kP2Sk = kP2Ci + kMaxWG * kTop,
              kP2Si = kP2Sk + 32, kP2Perm = kP2Si + 32, kP2Words = kP2Perm + 32;
static_assert(kP2Cnt + kMaxWG <= kP2Hist, "phase 2 layout");

// One entry's launch: workgroup blockIdx.x of nwg.  The body of both entry points below, so the two cannot drift apart.
__device__ __forceinline__ void logprob_body(const LogprobArgs &a, int V, int slice, int nwg) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *hdr = lds;        // [0]: last arriver, [8..9]: block_select's broadcast, [16..]: wave partials
    uint32_t *work = lds + 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w = blockIdx.x;
    const int ntop = (int)min(a.top_n, (uint32_t)kTop);
    char *scr = static_cast<char *>(a.scratch_dev);
    Partial *parts = reinterpret_cast<Partial *>(scr + kPartialOfs);
    uint32_t *cand = reinterpret_cast<uint32_t *>(scr + kCandOfs);
    const float *l = a.logits_dev;
    const int lo = w * slice, hi = min(V, lo + slice), n = max(0, hi - lo);

    // ---- phase 1: this workgroup's slice, read once -------------------------------------------------------------------------
    {
        uint32_t *hist = work, *tmp = work + 256, *keys = work + 512;
        float *wv = reinterpret_cast<float *>(hdr + 16);
        float mx = -INFINITY;
        auto take = [&](int i, float v) {
            keys[i] = lkey(v);
            mx = fmaxf(mx, v);  // fmaxf drops a NaN operand: NaN reads as -inf
        };
        const int n4 = (reinterpret_cast<uintptr_t>(l) & 15u) == 0 ? n >> 2 : 0;  // lo is a multiple of 4
        const float4 *l4 = reinterpret_cast<const float4 *>(l + lo);
        for (int i = tid; i < n4; i += kNT) {
            const float4 v = l4[i];
            take(4 * i, v.x), take(4 * i + 1, v.y), take(4 * i + 2, v.z), take(4 * i + 3, v.w);
        }
        for (int i = 4 * n4 + tid; i < n; i += kNT) take(i, l[lo + i]);  // the tail of the row (vocab % 4), or a row off 16-byte alignment
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        if (lane == 0) wv[wave] = mx;
        __syncthreads();  // the keys and the wave maxima are in LDS
        mx = wv[0];
        for (int j = 1; j < kNT / 64; ++j) mx = fmaxf(mx, wv[j]);
        // sum exp(l - mx) from the keys: a finite key gives its value back (+0.0 for either zero), a non-finite entry adds nothing here
        // (NaN and -inf weigh 0; with a +inf in the slice mx is +inf and the sum is not used).  Fixed order: per-thread run, wave tree, waves.
        float sum = 0.0f;
        if (mx > -INFINITY && mx < INFINITY)
            for (int i = tid; i < n; i += kNT) {
                const uint32_t k = keys[i];
                if (k) sum += expf(kval(k) - mx);
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        __syncthreads();  // wv is read
        if (lane == 0) wv[wave] = sum;
        __syncthreads();
        const int kk = min(ntop, n);
        if (tid == 0) {
            float s = wv[0];
            for (int j = 1; j < kNT / 64; ++j) s += wv[j];
            Partial p;
            p.mx = mx, p.sum = s, p.cnt = (uint32_t)kk, p.pad = 0;
            parts[w] = p;
        }
        if (kk > 0) {
            uint32_t Tk = 0;
            int rk = n;
            if (kk < n) block_select(keys, n, kk, hist, hdr + 8, &Tk, &rk);
            uint32_t *out = cand + (size_t)w * 2 * kTop;
            block_keep(keys, n, Tk, rk, tmp, [&](int i, uint32_t slot) {
                out[2 * slot] = keys[i];
                out[2 * slot + 1] = (uint32_t)(lo + i);
            });
        }
    }

    // ---- hand-over: the last workgroup to arrive finishes (select.hpp) --------------------------------------------------------
    if (!last_arriver(reinterpret_cast<uint32_t *>(scr), nwg, hdr)) return;

    // ---- phase 2: merge the partials, order the top list, write the record -----------------------------------------------------
    const int q = *a.pos_dev;
    if (q < 0 || (uint32_t)q >= a.capacity) return;  // nothing to write: the ticket is re-armed already
    LogprobRecord *rec = a.records_dev + q;
    uint32_t *ofs = work + kP2Ofs, *cnts = work + kP2Cnt, *hist = work + kP2Hist, *tmp = work + kP2Tmp, *ck = work + kP2Ck, *ci = work + kP2Ci;
    uint32_t *sk = work + kP2Sk, *si = work + kP2Si, *perm = work + kP2Perm;
    if (tid < nwg) cnts[tid] = parts[tid].cnt;
    if (tid < 64) {
        // M, then S = sum_w sum_w * exp(mx_w - M) in workgroup-index order: lane j takes workgroups j and j + 64, then the wave tree
        float m0 = -INFINITY, m1 = -INFINITY, s0 = 0.0f, s1 = 0.0f;
        if (lane < nwg) m0 = parts[lane].mx, s0 = parts[lane].sum;
        if (lane + 64 < nwg) m1 = parts[lane + 64].mx, s1 = parts[lane + 64].sum;
        float M = fmaxf(m0, m1);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
        float S = 0.0f;
        if (M > -INFINITY && M < INFINITY) {  // a slice whose maximum is -inf holds no mass: inf - inf is never evaluated
            if (m0 > -INFINITY) S += s0 * expf(m0 - M);
            if (m1 > -INFINITY) S += s1 * expf(m1 - M);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) S += __shfl_xor(S, off, 64);
        if (lane == 0) {
            const int t = a.history_dev[q];
            float lt = __uint_as_float(0x7fc00000u);
            if (t >= 0 && t < V) {
                lt = l[t];
                if (lt != lt) lt = -INFINITY;
            }
            rec->token = t;
            rec->n_top = min(ntop, V);
            rec->logit = lt;
            rec->lse = (M > -INFINITY && M < INFINITY) ? M + logf(S) : M;
        }
    }
    const int K = min(ntop, V);
    if (K == 0) return;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (int j = 0; j < nwg; ++j) {
            ofs[j] = s;
            s += cnts[j];
        }
        ofs[nwg] = s;
    }
    __syncthreads();
    const int ntot = (int)ofs[nwg];  // >= K: every slice left min(n_top, its entries)
    for (int c = tid; c < nwg * kTop; c += kNT) {  // the candidates in workgroup order (= id order); every slot at once: the loads overlap
        const int j = c / kTop, r = c - j * kTop;
        if (r < (int)cnts[j]) {
            const uint32_t *src = cand + (size_t)j * 2 * kTop;
            ck[ofs[j] + r] = src[2 * r];
            ci[ofs[j] + r] = src[2 * r + 1];
        }
    }
    __syncthreads();
    uint32_t Tk = 0;
    int rk = ntot;
    if (K < ntot) block_select(ck, ntot, K, hist, hdr + 8, &Tk, &rk);
    block_keep(ck, ntot, Tk, rk, tmp, [&](int i, uint32_t slot) {
        sk[slot] = ck[i];
        si[slot] = ci[i];
    });
    __syncthreads();
    if (tid < K) {  // rank among the K survivors (id order): key descending, then id ascending
        const uint32_t k = sk[tid];
        int r = 0;
        for (int j = 0; j < K; ++j) r += sk[j] > k || (sk[j] == k && j < tid);
        perm[r] = (uint32_t)tid;
    }
    __syncthreads();
    if (tid < K) {
        const uint32_t id = si[perm[tid]];
        rec->top_id[tid] = (int32_t)id;
        reinterpret_cast<uint32_t *>(rec->top_logit)[tid] = reinterpret_cast<const uint32_t *>(l)[id];  // the row's bits
    }
}

__global__ __launch_bounds__(kNT) void k_logprob(LogprobArgs a, int vocab, int slice) {
    if (!a.records_dev) return;
    logprob_body(a, vocab, slice, (int)gridDim.x);
}

// Every entry of a batch in one launch: grid (nwg, n_slots), blockIdx.y = the slot, whose LogprobArgs come from a device table (uniform
// loads: they stay in scalar registers).  An entry with null records is empty: its workgroups return before the first barrier and touch
// nothing.  Per slot everything is k_logprob's -- slices, the ticket in that entry's own scratch, the last arriver finishing.
// n_slots: 1..8 through bitnet_hip_logprob_batch_dev, 1..64 through bitnet_hip_logprob_rows_dev; no workgroup waits for another, so the
// larger grid need not be co-resident.
__global__ __launch_bounds__(kNT) void k_logprob_batch(const LogprobArgs *__restrict__ table, int vocab, int slice) {
    const LogprobArgs *e = table + blockIdx.y;
    if (!e->records_dev) return;
    const LogprobArgs a = *e;
    logprob_body(a, vocab, slice, (int)gridDim.x);
}

// the partition of a vocabulary: one formula for both entry points.  BITNET_HIP_LOGPROB_WGS (a tuning knob, read once) replaces kWantWG.
void geometry(size_t vocab, int *nwg, int *slice, size_t *lds) {
    static const int want = [] {
        const char *e = getenv("BITNET_HIP_LOGPROB_WGS");
        const int v = e ? atoi(e) : 0;
        return v >= 1 && v <= kMaxWG ? v : kWantWG;
    }();
    size_t s = (div_ceil(vocab, (size_t)want) + 3) / 4 * 4;
    s = std::min<size_t>(std::max<size_t>(s, kMinSlice), kMaxSlice);
    *slice = (int)s;
    *nwg = (int)div_ceil(vocab, s);
    *lds = (64 + std::max<size_t>(512 + s, kP2Words)) * 4;
}

}  // namespace

size_t logprob_scratch_bytes() { return kScratchBytes; }

hipError_t launch_logprob(const bitnet_hip_logprob_args &a, size_t vocab, hipStream_t stream) {
    int nwg, slice;
    size_t lds;
    geometry(vocab, &nwg, &slice, &lds);
    hipLaunchKernelGGL(k_logprob, dim3(nwg), dim3(kNT), lds, stream, a, (int)vocab, slice);
    return hipGetLastError();
}

hipError_t launch_logprob_batch(const bitnet_hip_logprob_args *table, size_t n_slots, size_t vocab, hipStream_t stream) {
    int nwg, slice;
    size_t lds;
    geometry(vocab, &nwg, &slice, &lds);
    hipLaunchKernelGGL(k_logprob_batch, dim3(nwg, (unsigned)n_slots), dim3(kNT), lds, stream, table, (int)vocab, slice);
    return hipGetLastError();
}

}  // namespace bitnet_hip
