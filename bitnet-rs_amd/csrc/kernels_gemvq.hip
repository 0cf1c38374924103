// kernels_gemvq.hip -- the I2_S / QK256 GEMV of the decode step on PRE-QUANTISED activations (qact.hpp).
//
// Same matrix-core formulation as k_gemv_mfma (kernels_mfma.hip: the vector ALUs only expand 2-bit codes to int8,
// v_mfma_i32_16x16x64_i8 does every multiply-add), with the three fixed costs round 1's profile charged to every
// wave removed (VERDICT r1 "what's weak" 5: ~650 VALU instructions per wave, 218 of them quantising activations,
// 120 LayerNorm statistics; 176 KB of loads per workgroup through a 64 B/clk vector-memory path):
//
//  * activations arrive as int8 digit planes + one power-of-two scale per 16 elements, written by the PRODUCING
//    kernel's epilogue (the previous GEMV, the attention combine, the embedding gather).  A wave copies its K range
//    (576 B per 256 columns) into LDS with two or three flat 16-byte loads -- no conversion, no row maximum;
//  * LayerNorm (applied after the product, bitnet_hip_weights_bind_ln) takes its row statistics from one
//    (sum, sum of squares) pair per producer tile instead of re-reading the row in every wave;
//  * the MFMA operands are swapped: the WEIGHTS are the B operand (16 output rows = the 16 columns of D), the
//    activations the A operand, whose 16 rows are (k-group kg, digit d, block half h) selectors -- row 4 kg + 2 d + h
//    holds digit plane d for the lanes of k-group kg in the MFMAs of parity h and zeros elsewhere.  One lane of D
//    then holds, for ONE weight row and ONE 32-weight block, the four exact integer sums (d, h) in its four
//    accumulator registers: digits recombine in integer arithmetic (v_lshl_add_u32), and the 32-block's weight scale
//    is applied once per lane: 7 VALU instructions per 32-block and lane instead of 12, one f16 scale load per
//    (row, block) instead of four.
//
// Per 1-KiB weight tile (16 rows x 256 columns) a wave issues 4 MFMAs, 44 VALU for the code expansion, 14 for
// digits + scales, 5 LDS reads.  Numerics: every 16-element partial sum is an exact integer; the activation is
// held to 2^-15 of its 16-group's maximum (qact.hpp); f32 accumulation in a fixed order (bit-reproducible).
// Reference semantics: Q/i2s_qk256.rs:196-274 (QK256), K/cpu/quantized_matmul.rs:57-96 (ternary x block scale),
// T:67-100 (LayerNorm), T:756-781 (silu(gate) * up), T:1073 / T:1125 (residual).
#include <cstdlib>

#include "common.hpp"
#include "gemvq_stages.hpp"
#include "qact.hpp"
#include "wave.hpp"

namespace bitnet_hip {

namespace {

constexpr int kMaxGroupQ = 4;  // query heads per KV head in an attention chunk record (kAttnRecFloats = 2 * 4 + 4 * 128)
// In-kernel time stamps (s_memrealtime, 100 MHz): diagnostic build only (-DBH_STAMPS), 16 x u64 per workgroup.
#ifdef BH_STAMPS
#define BH_QSTAMP(i)                                                                                           \
    do {                                                                                                       \
        if (p.stamps && lane == 0 && (wave == 0 || wave == NW - 1))                                            \
            p.stamps[(size_t)blockIdx.x * 16 + (wave ? 8 : 0) + (i)] = __builtin_amdgcn_s_memrealtime();      \
    } while (0)
#else
#define BH_QSTAMP(i) \
    do {             \
    } while (0)
#endif

// Two floats at a WAVE-UNIFORM address that no launch in flight writes (another kernel's finished output): read through the
// constant address space, i.e. the scalar cache -- one s_load_dwordx2 into SGPRs instead of a 64-lane request for 8 bytes.
__device__ __forceinline__ v2f load_uniform2(const void *p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) v2f *>(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ int load_uniform_i(const int *p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) int *>(reinterpret_cast<uintptr_t>(p));
}

struct GemvQArgs : GemvQPrefix {  // tiles .. stats_out: common.hpp
    // MRG: the activation vector is the decode attention's output, assembled HERE from its per-chunk records
    // (launch_attn_decode(..., combine = false): (m, l)[4] + un-normalised P.V [4][128] per KV head and 64-position chunk)
    const float *attn_rec;
    const int *attn_pos;     // *attn_pos + 1 keys
    int attn_chunks_max, attn_group_log2, attn_chunk_log2;  // records per KV head, log2 heads per KV head, log2 positions per record (6 / 7)
    unsigned long long *stamps;  // diagnostic builds only
};
static_assert(sizeof(GemvQArgs) == 176, "the layout k_gemv_q was compiled for: the prefix, then these members");

// NW waves per workgroup; RING = 256-column blocks per wave, all in flight at once; SC = weight scales per 32-block:
// 0 none (QK256), 1 f32, 2 f16; LN = LayerNorm after the product; NCP = 8-KiB passes of the cooperative QAct copy.
//
// Where a launch's time goes (in-kernel stamps, tools/stamp_gemvq.py, 2B-4T shapes): a CU's vector-memory path takes
// 64 B of requests per clock, so WHAT A WORKGROUP ASKS FOR is its start-up time -- with every wave fetching its own K
// range of the activations and its own copy of the statistics the last wave's weight loads were only requested 1.1 us
// after the kernel began (99 KB per workgroup, half of it duplicates).  Hence: the workgroup copies the activation
// vector into LDS ONCE (each thread 16 B), the statistics pairs likewise, and the per-row operands of the epilogue
// (g_r, residual, the next LayerNorm's gamma) are requested up front too -- behind the barrier they were dependent
// L2 / HBM round trips (0.7-0.8 us of a 2.5 us kernel).
// Every global load is unconditional and sits ahead of a scheduling fence (kernels_mfma.hip explains why).
// MRG = NE > 0: contexts of at most NR chunk records (NR = 4 or 8): instead of copying QAct records the workgroup merges the
// attention's chunk records itself: softmax merge of the NR records, then the 16-element group quantisation of qact.hpp straight
// into the LDS image.  One launch (k_attn_combine) and one global round trip of the vector less per layer.  Every workgroup reads
// all NR records, so the fetch asks for each o value ONCE and for nothing else (the rule above): thread t takes NE float4 slots
// (elements 4 (t + NT i) .. + 3: a quad of lanes = one 16-element group) and, for the columns past 4 NT NE, NE1 single floats
// (element 4 NT NE + t: a DPP row of 16 lanes = one group), so 2560 columns are 2048 + 512 with no clamped duplicate; a wave's
// slot lies in two heads (float4) or one (tail), wave-uniform, whose (m, l) pairs come by scalar loads -- no vector request.
// 4 records x 2560 columns: 41 KB per workgroup (the clamped two-slot mapping with per-lane (m, l) loads asked for 98 KB);
// 8 records: 82 KB, which is why the decoder takes the 8-record form up to Decoder::form_at's bound only.
template <int NW, int RING, int SC, int LN, int NCP, int NE = 0, int NE1 = 0, int NR = 4>
__global__ __launch_bounds__(NW * 64) void k_gemv_q(GemvQArgs p) {
    constexpr int NT = NW * 64;
    constexpr bool MRG = NE > 0;
    constexpr int ZB = RING * kQRec;  // zero bytes the dead A lanes read (no masking instructions)
    // every kernel argument in ONE scalar-load round: left alone hipcc fetches some of them where they are first used,
    // each a dependent round trip on the path to the first vector load
    asm volatile("" ::"s"(p.tiles), "s"(p.stiles), "s"(p.rows), "s"(p.nblk), "s"(p.lut), "s"(p.ks_log2), "s"(p.qin), "s"(p.stats_in), "s"(p.n_stats),
                 "s"(p.ln_g), "s"(p.residual), "s"(p.y), "s"(p.silu_mul), "s"(p.qout), "s"(p.gamma_out), "s"(p.stats_out));
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint8_t *zq = lds;                                // [ZB]
    uint8_t *cq = lds + ZB;                           // [NCP * 16 * NT] the whole QAct vector (padded)
    uint8_t *cs = cq + NCP * 16 * NT;                 // [NT * 16] statistics pairs (LN)
    float *part = reinterpret_cast<float *>(cs + (LN ? NT * 16 : 0));  // [NW][16] partial sums by (tile, K part)
    BH_QSTAMP(0);
    if (16 * tid < ZB) *reinterpret_cast<v4u *>(zq + 16 * tid) = v4u{0u, 0u, 0u, 0u};

    // ---- wave -> (row tile, K range of at most RING blocks), as k_gemv_mfma ------------------------------------
    const int ksplit = 1 << p.ks_log2;
    const int tiles_per_wg = NW >> p.ks_log2;
    const int n_tiles = p.rows >> 4;  // rows % 16 == 0 (launcher)
    int tile = blockIdx.x * tiles_per_wg + (wave >> p.ks_log2);
    tile = tile < n_tiles ? tile : n_tiles - 1;  // surplus waves redo the last tile; never stored
    int kpart = wave & (ksplit - 1);
    if (NW == 8 && p.ks_log2 == 3 && wave >= 4) kpart = 11 - wave;  // at most one long range per SIMD (kernels_mfma.hip)
    const int b0 = (kpart * p.nblk) >> p.ks_log2, b1 = ((kpart + 1) * p.nblk) >> p.ks_log2;

    // ---- 1. the activation vector (L2-resident, every workgroup reads it), statistics pairs, epilogue operands ----
    const uint32_t q_last = (uint32_t)kQRec * (uint32_t)p.nblk - 16u;
    v4u qa[NCP];  // native vectors: arrays of HIP's uint4 struct went through scratch memory at the scheduling fence
    float4 mo[MRG ? NE : 1][NR];      // MRG: un-normalised P.V values of this thread's NE float4 slots, records 0..NR-1,
    float mt[NE1 ? NE1 : 1][NR];      //      of its NE1 tail elements,
    v2f sml[MRG ? NE : 1][2][NR];     //      and the (m, l) pairs of a wave's two heads per float4 slot / one head per tail slot:
    v2f smt[NE1 ? NE1 : 1][NR];       //      wave-uniform addresses -> scalar loads (load_uniform2)
    int mpos = 0;                     //      and the position, likewise
    if (!MRG) {
#pragma unroll
        for (int i = 0; i < NCP; ++i) qa[i] = *reinterpret_cast<const v4u *>(p.qin + umin32(16u * (uint32_t)(tid + NT * i), q_last));
    } else {
        // records 0..NR-1 are requested before the position (hence the live record count) is known; dead records hold zeros or
        // an earlier token's finite values: only their m is masked below.
        // Byte offsets in 32 bits from the one uniform base (the launcher bounds the buffer): one add per request.
        const int gl = p.attn_group_log2, gm = (1 << gl) - 1, h_last = (p.cols >> 7) - 1;
        const uint32_t kv_stride = (uint32_t)p.attn_chunks_max * (kAttnRecFloats * 4u);
        const char *rbase = reinterpret_cast<const char *>(p.attn_rec);
        uint32_t ro[NR];
#pragma unroll
        for (int c = 0; c < NR; ++c) ro[c] = (uint32_t)(c < p.attn_chunks_max ? c : p.attn_chunks_max - 1) * (kAttnRecFloats * 4u);
        mpos = load_uniform_i(p.attn_pos);
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            int e = 4 * (tid + NT * i);
            e = e < p.cols ? e : p.cols - 4;
            const int h = e >> 7, d = e & 127;
            const uint32_t vo = (uint32_t)(h >> gl) * kv_stride + 4u * (uint32_t)(2 * kMaxGroupQ + (h & gm) * 128 + d);
#pragma unroll
            for (int c = 0; c < NR; ++c) mo[i][c] = *reinterpret_cast<const float4 *>(rbase + (vo + ro[c]));
        }
#pragma unroll
        for (int i = 0; i < NE1; ++i) {
            int e = 4 * NT * NE + tid + NT * i;
            e = e < p.cols ? e : p.cols - 1;
            const int h = e >> 7, d = e & 127;
            const uint32_t vo = (uint32_t)(h >> gl) * kv_stride + 4u * (uint32_t)(2 * kMaxGroupQ + (h & gm) * 128 + d);
#pragma unroll
            for (int c = 0; c < NR; ++c) mt[i][c] = *reinterpret_cast<const float *>(rbase + (vo + ro[c]));
        }
#pragma unroll
        for (int i = 0; i < NE; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) {  // lanes 0..31 / 32..63 of this wave's slot
                int hs = 2 * (wave + NW * i) + s;
                hs = hs < h_last ? hs : h_last;
                const uint32_t so = (uint32_t)(hs >> gl) * kv_stride + 8u * (uint32_t)(hs & gm);
#pragma unroll
                for (int c = 0; c < NR; ++c) sml[i][s][c] = load_uniform2(rbase + (so + ro[c]));
            }
#pragma unroll
        for (int i = 0; i < NE1; ++i) {
            int hs = ((4 * NT * NE + NT * i) >> 7) + (wave >> 1);
            hs = hs < h_last ? hs : h_last;
            const uint32_t so = (uint32_t)(hs >> gl) * kv_stride + 8u * (uint32_t)(hs & gm);
#pragma unroll
            for (int c = 0; c < NR; ++c) smt[i][c] = load_uniform2(rbase + (so + ro[c]));
        }
    }
    v4u st = {0u, 0u, 0u, 0u};
    if (LN) st = *reinterpret_cast<const v4u *>(p.stats_in + 2 * (size_t)(tid < p.n_stats ? tid : p.n_stats - 1));
    // the storing thread's row(s); other threads request clamped, valid addresses and drop the values
    const int e_tl = tid >> 4, e_r = tid & 15;
    int e_row, e_g0 = 0, e_g1 = 0;
    if (!p.silu_mul) {
        e_row = 16 * (blockIdx.x * tiles_per_wg + e_tl) + e_r;
        e_row = e_row < p.rows ? e_row : p.rows - 1;
        e_g0 = e_row;
    } else {
        const int half_rows = p.rows >> 1;
        const int pg = blockIdx.x * (tiles_per_wg >> 1) + e_tl;
        e_row = 16 * pg + e_r;
        e_row = e_row < half_rows ? e_row : half_rows - 1;
        e_g0 = 32 * (e_row >> 4) + e_r;
        e_g1 = e_g0 + 16;
    }
    float e_lg0 = 0.0f, e_lg1 = 0.0f;
    if (LN) {
        e_lg0 = p.ln_g[e_g0];
        e_lg1 = p.ln_g[e_g1];
    }
    // nullable operands: a valid dummy address instead of a branch around the load (a load under a branch costs a full wait)
    const float e_res = (p.residual ? p.residual : reinterpret_cast<const float *>(p.qin))[p.residual ? e_row : 0];
    const float e_gam = (p.gamma_out ? p.gamma_out : reinterpret_cast<const float *>(p.qin))[p.gamma_out ? e_row : 0];
    // vmcnt retires in order: the activations must be REQUESTED ahead of the weight stream, or their arrival only
    // counts once every weight tile has landed
    __builtin_amdgcn_sched_barrier(0);
    // ---- 2. weight tiles (+ their scale tiles): read once by this wave only -> non-temporal -------------------
    const size_t tb0 = (size_t)tile * p.nblk;
    const uint8_t *wbase = p.tiles + (tb0 * 64 + lane) * 16;
    v4u wt[RING];
    uint32_t sh[SC == 2 ? RING : 1];
    float2 sf[SC == 1 ? RING : 1];
#pragma unroll
    for (int j = 0; j < RING; ++j) {
        const int blk = ring_block(b0, b1, j);
        wt[j] = load_nt16v(wbase + (size_t)blk * 1024);
        if (SC == 2) sh[j] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p.stiles) + (tb0 + blk) * 64 + lane);
        if (SC == 1) {
            const float *sp = reinterpret_cast<const float *>(p.stiles) + ((tb0 + blk) * 64 + lane) * 2;
            sf[j] = float2{__builtin_nontemporal_load(sp), __builtin_nontemporal_load(sp + 1)};
        }
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of this wave is requested before anything waits
    BH_QSTAMP(1);

    // ---- 3. QAct records (and statistics pairs) -> LDS, once per workgroup ------------------------------------
    if (!MRG) {
#pragma unroll
        for (int i = 0; i < NCP; ++i) *reinterpret_cast<v4u *>(cq + 16 * (tid + NT * i)) = qa[i];
    } else {
        const int m_chunks = (mpos + (1 << p.attn_chunk_log2)) >> p.attn_chunk_log2;  // live records, 1..NR (the caller switches form beyond that)
        // softmax merge: out = sum_c e^(m_c - M) o_c / sum_c e^(m_c - M) l_c   (k_attn_combine's value); records in ascending order.
        // Every record count gives the bits the two-launch form gives there.  Up to 4 live records that is the 4-record merge
        // (v_exp_f32, one reciprocal).  From 5 records the decoder used to run k_attn_combine, which for at most 8 records is this
        // same two-pass sum -- each of its 8 thread groups holds one record, (m, l, o) unchanged -- with expf and a division per
        // element: the 8-record instance takes those two from 5 live records on (wave-uniform), so a step's numbers do not depend
        // on whether the combine kernel or this prologue merged the records.
        const bool as_combine = NR > 4 && m_chunks > 4;
        constexpr int NS = MRG ? NE + NE1 : 1;
        float ml[NS][NR], xl[NS][NR], wl[NS][NR];  // per slot (float4 slots, then tail slots): l_c, m_c - M, the weights e^(m_c - M)
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            float mc[NR], M = -INFINITY;
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                const float mv = k < NE ? (lane < 32 ? sml[k < NE ? k : 0][0][c].x : sml[k < NE ? k : 0][1][c].x) : smt[k < NE ? 0 : k - NE][c].x;
                ml[k][c] = k < NE ? (lane < 32 ? sml[k < NE ? k : 0][0][c].y : sml[k < NE ? k : 0][1][c].y) : smt[k < NE ? 0 : k - NE][c].y;
                mc[c] = c < m_chunks ? mv : -INFINITY;
                M = fmaxf(M, mc[c]);
            }
#pragma unroll
            for (int c = 0; c < NR; ++c) xl[k][c] = mc[c] - M;
        }
        if constexpr (NR <= 4) {
#pragma unroll
            for (int k = 0; k < NS; ++k)
#pragma unroll
                for (int c = 0; c < NR; ++c) wl[k][c] = __expf(xl[k][c]);
        } else {
            // The weights are wave-uniform per head, and expf is ~12 instructions: lane 8 k + c (32 + 8 k + c for the upper half's
            // head) evaluates the exponential of record c of slot k ONCE and readlane hands the results round -- one evaluation per
            // wave instead of NR per slot and lane (the same function of the same argument: the same bits).
            float tx = 0.0f;
#pragma unroll
            for (int k = 0; k < NS; ++k)
#pragma unroll
                for (int c = 0; c < NR; ++c) tx = (lane & 31) == 8 * k + c ? xl[k][c] : tx;
            const float ex = as_combine ? expf(tx) : __expf(tx);
#pragma unroll
            for (int k = 0; k < NS; ++k)
#pragma unroll
                for (int c = 0; c < NR; ++c) {
                    const float lo = readlane_f(ex, 8 * k + c);
                    wl[k][c] = k < NE ? (lane < 32 ? lo : readlane_f(ex, 32 + 8 * k + c)) : lo;
                }
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = 4 * (tid + NT * i);
            float L = 0.0f;
            float4 a = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                const float w = wl[i][c];  // explicit fused multiply-adds: what the contraction made of `L += w * l` in the 4-record
                L = fmaf(w, ml[i][c], L);  // form and in k_attn_combine, and no packed multiply + add may take their place
                a.x = fmaf(w, mo[i][c].x, a.x), a.y = fmaf(w, mo[i][c].y, a.y), a.z = fmaf(w, mo[i][c].z, a.z), a.w = fmaf(w, mo[i][c].w, a.w);
            }
            const float rl = e < p.cols ? 1.0f / L : 0.0f;
            float v[4] = {a.x * rl, a.y * rl, a.z * rl, a.w * rl};
            if (as_combine && e < p.cols) v[0] = a.x / L, v[1] = a.y / L, v[2] = a.z / L, v[3] = a.w / L;
            // qact_emit's format (qact.hpp) with the 16-element group spread over 4 lanes x 4 elements; destination = the LDS image
            uint32_t u = __float_as_uint(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])))), o;
            o = dpp_u<0xB1>(u), u = o > u ? o : u;  // quad_perm [1,0,3,2]
            o = dpp_u<0x4E>(u), u = o > u ? o : u;  // quad_perm [2,3,0,1]: the maximum over the quad = the 16 elements
            float sc, as;
            qact_scales(u, sc, as);
            uint32_t d0 = 0, d1 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t t = qact_digits(v[j], sc);
                d0 |= (t & 0xffu) << (8 * j);
                d1 |= ((t >> 8) & 0xffu) << (8 * j);
            }
            if (e < p.cols) {
                const int grp = e >> 4, rec = grp >> 4, tp = grp & 15;
                uint8_t *qb = cq + kQRec * rec;
                *reinterpret_cast<uint32_t *>(qb + 16 * tp + (e & 15)) = d0;
                *reinterpret_cast<uint32_t *>(qb + 256 + 16 * tp + (e & 15)) = d1;
                if ((e & 15) == 0) reinterpret_cast<float *>(qb + 512)[4 * (tp >> 2) + 2 * (tp & 1) + ((tp & 3) >> 1)] = as;  // qact_scale_slot (qact.hpp) restated
            }
        }
#pragma unroll
        for (int i = 0; i < NE1; ++i) {
            const int e = 4 * NT * NE + tid + NT * i;  // whole 16-lane rows are live or dead together (cols % 16 == 0)
            float L = 0.0f, a = 0.0f;
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                const float w = wl[NE + i][c];
                L = fmaf(w, ml[NE + i][c], L);
                a = fmaf(w, mt[i][c], a);
            }
            float v = a * (e < p.cols ? 1.0f / L : 0.0f);
            if (as_combine && e < p.cols) v = a / L;
            // qact_emit's format and lane layout (one element per lane, the group = a DPP row); destination = the LDS image
            float sc, as;
            qact_scales(__float_as_uint(row16_max_abs(v)), sc, as);
            const uint32_t t = qact_digits(v, sc);
            if (e < p.cols) {
                const int grp = e >> 4, rec = grp >> 4, tp = grp & 15, r = e & 15;
                uint8_t *qb = cq + kQRec * rec;
                qb[16 * tp + r] = (uint8_t)t;
                qb[256 + 16 * tp + r] = (uint8_t)(t >> 8);
                if (r == 0) reinterpret_cast<float *>(qb + 512)[4 * (tp >> 2) + 2 * (tp & 1) + ((tp & 3) >> 1)] = as;  // qact_scale_slot (qact.hpp) restated
            }
        }
    }
    if (LN) *reinterpret_cast<v4u *>(cs + 16 * tid) = st;
    // raw barrier: __syncthreads() would also wait for the weight loads in flight
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // A-operand lane (k-group g, selector row c = 4 kg + 2 d + h): digit plane d of k-group kg, live in the MFMAs
    // of parity h only; every other (lane, MFMA) reads zeros.  D lane (g, c): selector group g, weight row c.
    const int g = lane >> 4, c = lane & 15;
    const bool mine = (c >> 2) == g;
    const uint8_t *wq = cq + kQRec * b0;  // this wave's K range
    const uint8_t *live = wq + 256 * ((c >> 1) & 1) + 64 * g;
    const uint8_t *ba0 = (mine && (c & 1) == 0) ? live : zq;  // MFMAs 0 and 2 of a block
    const uint8_t *ba1 = (mine && (c & 1) == 1) ? live : zq;  // MFMAs 1 and 3
    const uint8_t *sa = wq + 512 + 16 * g;                    // this lane's four group scales of a record
    BH_QSTAMP(2);

    float facc = 0.0f;
#pragma unroll
    for (int j = 0; j < RING; ++j) {
        if (j > 0 && b0 + j >= b1) continue;  // wave-uniform: a slot past this wave's range
        const float4 as = *reinterpret_cast<const float4 *>(sa + kQRec * j);  // (h0 p0, h0 p1, h1 p0, h1 p1)
        const uint32_t wd[4] = {wt[j][0], wt[j][1], wt[j][2], wt[j][3]};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {  // the lane group's two 32-weight blocks
            v4i acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i *>(ba0 + kQRec * j + 32 * pp),
                                                        decode16(wd[2 * pp], p.lut), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i *>(ba1 + kQRec * j + 32 * pp + 16),
                                                        decode16(wd[2 * pp + 1], p.lut), acc, 0, 0, 0);
            const float t = gemvq_block_value(acc, as, pp);
            if (SC == 2)
                facc = pp ? fma_mix_hi(t, sh[j], facc) : fma_mix_lo(t, sh[j], facc);
            else if (SC == 1)
                facc = fmaf(t, pp ? sf[j].y : sf[j].x, facc);
            else
                facc += t;
        }
    }
    facc = sum_kgroups(facc);
    if (lane < 16) part[(((wave >> p.ks_log2) << p.ks_log2) + kpart) * 16 + lane] = facc;
    BH_QSTAMP(3);

    // ---- 4. epilogue: the storing waves only ------------------------------------------------------------------
    const bool storing = wave * 64 < tiles_per_wg * 16;
    double ln_mean = 0.0, ln_rdenom = 1.0;
    if (LN && storing) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = lane; i < p.n_stats; i += 64) {
            const double2 pr = *reinterpret_cast<const double2 *>(cs + 16 * i);
            s1 += pr.x;
            s2 += pr.y;
        }
        s1 = wave64_sum_d_rows_readlane(s1);
        s2 = wave64_sum_d_rows_readlane(s2);
        ln_from_sums(s1, s2, p.inv_cols, p.ln_eps, &ln_mean, &ln_rdenom);
    }
    __syncthreads();
    BH_QSTAMP(4);
    if (!storing) return;
    const int tl = e_tl, r = e_r;
    if (!p.silu_mul) {
        if (tl >= tiles_per_wg) return;
        const int t_glob = blockIdx.x * tiles_per_wg + tl;
        if (t_glob >= n_tiles) return;  // whole 16-lane rows leave together
        const int row = 16 * t_glob + r;
        float pv[NW];
#pragma unroll
        for (int kp = 0; kp < NW; ++kp) pv[kp] = part[((tl << p.ks_log2) + (kp < ksplit ? kp : 0)) * 16 + r];  // all reads in flight at once
        float v = 0.0f;
#pragma unroll
        for (int kp = 0; kp < NW; ++kp) v += kp < ksplit ? pv[kp] : 0.0f;  // fixed order: K parts 0, 1, ...
        if (LN) v = (float)(((double)v - ln_mean * (double)e_lg0) * ln_rdenom);
        if (p.residual) v += e_res;
        if (p.y) p.y[row] = v;
        if (p.qout) qact_emit(p.qout, p.stats_out, t_glob, r, v, p.gamma_out ? v * e_gam : v);
        BH_QSTAMP(5);
    } else {
        const int pairs_per_wg = tiles_per_wg >> 1;
        if (tl >= pairs_per_wg) return;
        const int p_glob = blockIdx.x * pairs_per_wg + tl;
        if (2 * p_glob >= n_tiles) return;
        const int row = 16 * p_glob + r;  // row of silu(gate) * up
        float pg[NW / 2], pu[NW / 2];  // paired matrices split K over at most NW / 2 waves
#pragma unroll
        for (int kp = 0; kp < NW / 2; ++kp) {
            pg[kp] = part[(((2 * tl) << p.ks_log2) + (kp < ksplit ? kp : 0)) * 16 + r];
            pu[kp] = part[(((2 * tl + 1) << p.ks_log2) + (kp < ksplit ? kp : 0)) * 16 + r];
        }
        float gv = 0.0f, uv = 0.0f;
#pragma unroll
        for (int kp = 0; kp < NW / 2; ++kp) {
            gv += kp < ksplit ? pg[kp] : 0.0f;
            uv += kp < ksplit ? pu[kp] : 0.0f;
        }
        if (LN) {  // stored rows of the paired matrix: (gate tile, up tile)
            gv = (float)(((double)gv - ln_mean * (double)e_lg0) * ln_rdenom);
            uv = (float)(((double)uv - ln_mean * (double)e_lg1) * ln_rdenom);
        }
        // FeedForward::forward T:756-781: silu(g) * u, silu(v) = v / (1 + e^-v); v_exp_f32 / v_rcp_f32 (1 ulp each) instead of the
        // ~40-instruction libm forms: this runs on ONE wave per workgroup, behind the barrier
        const float v = gv * __builtin_amdgcn_rcpf(1.0f + __expf(-gv)) * uv;
        if (p.y) p.y[row] = v;
        if (p.qout) qact_emit(p.qout, p.stats_out, p_glob, r, v, p.gamma_out ? v * e_gam : v);
        BH_QSTAMP(5);
    }
}

// ---- standalone producers: any f32 vector -> QAct (tests, the first layer's input) ----------------------------
__global__ __launch_bounds__(256) void k_quant_act(const float *__restrict__ x, const float *__restrict__ gamma, int n,
                                                   uint8_t *__restrict__ qout, double *__restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // n % 16 == 0: whole 16-lane rows are in or out together
    if (i >= n) return;
    const float v = x[i];
    qact_emit(qout, stats, i >> 4, i & 15, v, gamma ? v * gamma[i] : v);
}

// TransformerModel::embed (T:1390-1426) of ONE token + the first block's QAct (its attention_norm gamma)
__global__ __launch_bounds__(256) void k_embed_q(const _Float16 *__restrict__ table, const int *__restrict__ tokens,
                                                 const int *__restrict__ offset_ptr, int hidden, int vocab, float *__restrict__ x_out,
                                                 const float *__restrict__ gamma, uint8_t *__restrict__ qout, double *__restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hidden) return;
    int tok = tokens[offset_ptr ? *offset_ptr : 0];
    tok = tok < 0 ? 0 : tok >= vocab ? vocab - 1 : tok;  // ids are range-checked on the host (Decoder::feed); never a wild read
    const float v = (float)table[(size_t)tok * hidden + i];
    x_out[i] = v;
    qact_emit(qout, stats, i >> 4, i & 15, v, gamma ? v * gamma[i] : v);
}

}  // namespace

bool gemvq_supported(const Weights &w) {
    if (!mfma_supported(w)) return false;
    if (w.cols % 256 != 0 || w.rows % 16 != 0) return false;   // whole records, whole producer tiles
    if (w.scaled && w.block_size != 32) return false;          // 256-block scales stay on k_gemv_mfma
    return true;
}

hipError_t launch_quant_act(const float *x, const float *gamma, size_t n, void *qout, double *stats, hipStream_t stream) {
    if (n == 0 || n % 16 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_quant_act, dim3((unsigned)div_ceil(n, 256)), dim3(256), 0, stream, x, gamma, (int)n, static_cast<uint8_t *>(qout), stats);
    return hipGetLastError();
}

hipError_t launch_embed_q(const void *table, const int *tokens, const int *offset_ptr, int hidden, int vocab, float *x_out,
                          const float *gamma, void *qout, double *stats, hipStream_t stream) {
    if (hidden <= 0 || hidden % 16 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_embed_q, dim3((unsigned)div_ceil((size_t)hidden, 256)), dim3(256), 0, stream, static_cast<const _Float16 *>(table), tokens,
                       offset_ptr, hidden, vocab, x_out, gamma, static_cast<uint8_t *>(qout), stats);
    return hipGetLastError();
}

hipError_t fill_gemv_q_prefix(GemvQPrefix &a, const Weights &w, const GemvQIo &io, const GemvGeom &g) {
    a.tiles = w.tiles;
    a.stiles = g.sc == 2 ? (const void *)w.scale_tiles_h : g.sc == 1 ? (const void *)w.scale_tiles : nullptr;
    if (g.sc && !a.stiles) return hipErrorInvalidValue;
    a.rows = (int)w.rows;
    a.cols = (int)w.cols;
    a.nblk = g.nblk;
    a.lut = w.lut;
    a.ks_log2 = g.ks_log2;
    a.qin = static_cast<const uint8_t *>(io.qin);
    if (io.ln_gamma && !(w.ln_g && w.ln_gamma_bound == io.ln_gamma && io.stats_in)) return hipErrorInvalidValue;  // LayerNorm only in the after-product form
    a.stats_in = io.stats_in;
    a.n_stats = (int)(w.cols / 16);
    a.ln_g = w.ln_g;
    a.ln_eps = io.ln_eps;
    a.inv_cols = 1.0 / (double)w.cols;
    a.residual = io.residual;
    a.y = io.y;
    a.silu_mul = io.silu_mul ? 1 : 0;
    if (io.silu_mul && (!w.paired || io.residual)) return hipErrorInvalidValue;
    a.qout = static_cast<uint8_t *>(io.qout);
    a.gamma_out = io.gamma_out;
    a.stats_out = io.stats_out;
    return hipSuccess;
}

// Which k_gemv_q instance a launch takes: the K partition (gemv_geometry), the RING that holds a wave's blocks (the first of 2..5 that does),
// the 8-KiB passes of the QAct copy, and for the merging form (the o-projection shape: K = heads * 128, ring <= 2, one copy pass) the slots per
// thread: one float4 (K <= 2048), one float4 + one float (K <= 2560), two float4 (beyond; 4 records only).  launch_gemv_q instantiates exactly
// this; bitnet_hip_gemv_q_geometry reports it without launching.
hipError_t gemv_q_instance(const Weights &w, bool silu_mul, bool ln, int merge_records, GemvQInstance &q) {
    if (!gemvq_supported(w)) return hipErrorInvalidValue;
    // (16-wave workgroups -- 4 waves per SIMD, half the K range each -- measured slower in round 2, gate|up 5.46 vs 5.23 us, and were removed)
    const int nw = 8;
    q.nw = nw;
    q.g = gemv_geometry(w, silu_mul, nw);
    q.ln = ln ? 1 : 0;
    q.ncp = (int)div_ceil((size_t)kQRec * q.g.nblk, (size_t)16 * nw * 64);
    q.ring_inst = q.g.ring < 2 ? 2 : q.g.ring;
    q.ne = q.ne1 = 0;
    q.nr = merge_records;
    if (q.g.ring > 5 || q.ncp > 3 || (ln && w.cols / 16 > (size_t)nw * 64)) return hipErrorInvalidValue;
    if (merge_records) {
        q.ne = w.cols <= 2560 ? 1 : 2;
        q.ne1 = w.cols > 2048 && w.cols <= 2560 ? 1 : 0;
        if (ln || q.g.ring > 2 || q.ncp != 1 || w.cols % 128 != 0 || w.cols > 4096 || (merge_records != 4 && merge_records != 8) ||
            (merge_records == 8 && q.ne == 2))
            return hipErrorInvalidValue;
        q.ring_inst = 2;
    }
    return hipSuccess;
}

hipError_t launch_gemv_q(const Weights &w, const GemvQIo &io, hipStream_t stream) {
    if (!w.tiles || !gemvq_supported(w) || (!io.qin && !io.attn_rec)) return hipErrorInvalidValue;
    const bool ln = io.ln_gamma != nullptr;
    GemvQInstance q;
    const hipError_t eq = gemv_q_instance(w, io.silu_mul, ln, io.attn_rec ? io.attn_records : 0, q);
    if (eq != hipSuccess) return eq;
    const GemvGeom &g = q.g;
    const int nw = q.nw;
    GemvQArgs a;
    const hipError_t ef = fill_gemv_q_prefix(a, w, io, g);
    if (ef != hipSuccess) return ef;
    a.attn_rec = io.attn_rec;
    a.attn_pos = io.attn_pos;
    a.attn_chunks_max = io.attn_chunks_max;
    a.attn_group_log2 = io.attn_group_log2;
    a.attn_chunk_log2 = io.attn_chunk_log2;
    a.stamps = g_mfma_stamps;
    const int ring = q.ring_inst, sc = g.sc, ncp = q.ncp;
    void (*kfn)(GemvQArgs) = nullptr;
#define BH_QPICK2(RINGv, NCPv)                                                                                                        \
    if (!kfn && ring == RINGv && ncp == NCPv)                                                                                         \
        kfn = ln ? (sc == 2 ? k_gemv_q<8, RINGv, 2, 1, NCPv> : sc == 1 ? k_gemv_q<8, RINGv, 1, 1, NCPv> : k_gemv_q<8, RINGv, 0, 1, NCPv>)  \
                 : (sc == 2 ? k_gemv_q<8, RINGv, 2, 0, NCPv> : sc == 1 ? k_gemv_q<8, RINGv, 1, 0, NCPv> : k_gemv_q<8, RINGv, 0, 0, NCPv>);
#define BH_QPICK(RINGv) BH_QPICK2(RINGv, 1) BH_QPICK2(RINGv, 2) BH_QPICK2(RINGv, 3)
    BH_QPICK(2) BH_QPICK(3) BH_QPICK(4) BH_QPICK(5)
#undef BH_QPICK
#undef BH_QPICK2
    if (io.attn_rec) {  // merging form
        const int ne = q.ne, ne1 = q.ne1, nr = q.nr;
        if (nw != 8 || !io.attn_pos || io.attn_chunks_max < 1) return hipErrorInvalidValue;
        // the kernel addresses the records with 32-bit byte offsets
        if (((uint64_t)(w.cols / 128) >> io.attn_group_log2) * (uint64_t)io.attn_chunks_max * kAttnRecFloats * 4u >= (1ull << 32)) return hipErrorInvalidValue;
#define BH_QMRG(NEv, NE1v, NRv)                     \
    if (ne == NEv && ne1 == NE1v && nr == NRv)      \
        kfn = sc == 2 ? k_gemv_q<8, 2, 2, 0, 1, NEv, NE1v, NRv> : sc == 1 ? k_gemv_q<8, 2, 1, 0, 1, NEv, NE1v, NRv> : k_gemv_q<8, 2, 0, 0, 1, NEv, NE1v, NRv>;
        kfn = nullptr;
        BH_QMRG(1, 0, 4) BH_QMRG(1, 1, 4) BH_QMRG(2, 0, 4) BH_QMRG(1, 0, 8) BH_QMRG(1, 1, 8)
#undef BH_QMRG
    }
    if (!kfn) return hipErrorInvalidValue;
    const size_t lds = (size_t)g.ring_t * kQRec + (size_t)ncp * 16 * nw * 64 + (ln ? (size_t)nw * 64 * 16 : 0) + (size_t)nw * 16 * sizeof(float);
    hipLaunchKernelGGL(kfn, dim3(g.grid), dim3(nw * 64), lds, stream, a);
    return hipGetLastError();
}

}  // namespace bitnet_hip
