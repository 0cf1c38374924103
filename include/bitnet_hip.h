/*
 * bitnet_hip.h -- C ABI of libbitnet_hip.so: the MI355X (gfx950) drop-in for the
 * I2_S / QK256 hot path of EffortlessMetrics/BitNet-rs.
 *
 * This is the boundary the reference's `bitnet-kernels` ROCm provider would bind
 * (`extern "C"`, plain pointers and sizes).  Each entry point names the reference
 * interface it replaces (path:line under the reference checkout).  Prefixes:
 *   K/ = crates/bitnet-kernels/src/   Q/ = crates/bitnet-quantization/src/
 *   M/ = crates/bitnet-models/src/    T  = crates/bitnet-transformer/src/lib.rs
 *
 * Conventions (identical to the reference's existing C bridge, K/ffi/bridge.rs:17-39
 * and K/ffi/cpp_bridge.cpp:19-27,76-86,112-118):
 *   - every fallible call returns int: 0 = success, non-zero = error;
 *   - the error text is kept in a thread-local string, valid until the next call
 *     on the same thread, read with bitnet_hip_get_last_error();
 *   - the caller owns every buffer; nothing is retained past return (handles own
 *     their device copies); outputs are fully overwritten;
 *   - no exception crosses the boundary; entry points are re-entrant.
 *
 * Two families:
 *   1. host-pointer drop-ins: argument lists mirror the Rust slices 1:1
 *      (pointer + length), synchronous and self-contained (H2D, launch, D2H),
 *      like the reference GPU provider does per call (K/gpu/cuda.rs:287-336);
 *   2. device-resident API: upload weights once -> opaque handle; activations
 *      and outputs are device pointers; optional hipStream_t (void*).  This is the
 *      measured path.
 *
 * There is NO CPU fallback behind any symbol: without a HIP device every compute
 * entry point fails with BITNET_HIP_ERR_GPU.
 *
 * ONE SKU.  The launch heuristics -- token-tile and row-tile choices of the tiled matmuls, the
 * weight-stationary group size, the grid covers, the attention's key splits, the GEMV's workgroup
 * counts -- are constants tuned for MI355X: 256 CUs in 8 XCDs, 4 MiB of L2 per XCD, 160 KiB of
 * LDS per CU, 512 registers per SIMD lane.  Results do not depend on them (placement and tiling
 * change speed only); on another gfx950 part they would want re-tuning (kGemmCUs, the cover
 * thresholds, gemm_weight_group's 1.5 MiB in kernels_gemm.hip; Decoder::hybrid_applies' 400
 * workgroups in host/decoder.cpp).  Environment switches that steer them: INTEGRATION.md.
 */
#ifndef BITNET_HIP_H
#define BITNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes.  Mapping to crates/bitnet-common/src/error.rs:80-97 KernelError:
 *   INVALID_ARGUMENT -> InvalidArguments, GPU -> GpuError,
 *   UNSUPPORTED -> UnsupportedHardware, EXECUTION -> ExecutionFailed. */
#define BITNET_HIP_OK 0
#define BITNET_HIP_ERR_INVALID_ARGUMENT (-1) /* same value cpp_bridge.cpp returns for null/size errors */
#define BITNET_HIP_ERR_GPU (-2)
#define BITNET_HIP_ERR_UNSUPPORTED (-3)
#define BITNET_HIP_ERR_EXECUTION (-4)

/* QuantizationType ints, K/ffi.rs:40-44 */
#define BITNET_HIP_QTYPE_I2S 0
#define BITNET_HIP_QTYPE_TL1 1
#define BITNET_HIP_QTYPE_TL2 2

/* ------------------------------------------------------------------------- */
/* lifecycle  (K/ffi/bridge.rs:18-20,38: bitnet_cpp_init/cleanup/is_available/ */
/*             get_last_error;  K/rocm/mod.rs:125-137: is_rocm_available,      */
/*             rocm_device_count)                                              */
/* ------------------------------------------------------------------------- */

/* Idempotent.  Selects `device` for the calling thread and creates the library's
 * internal workspace.  device < 0 means "current device". */
int bitnet_hip_init(int device);
void bitnet_hip_cleanup(void);
/* Non-zero iff at least one HIP device is visible.  The BITNET_ENABLE_ROCM=1
 * opt-in (K/rocm/mod.rs:76-81) stays on the host side of the boundary. */
int bitnet_hip_is_available(void);
int bitnet_hip_device_count(void);
/* NULL when no error is recorded on this thread (cpp_bridge.cpp:281-283). */
const char *bitnet_hip_get_last_error(void);

/* K/rocm/mod.rs:33-53 RocmDeviceInfo */
typedef struct bitnet_hip_device_info {
    int32_t device_id;
    char name[128];
    char gcn_arch[64];
    uint64_t total_memory;
    int32_t compute_unit_count;
    int32_t max_wavefront_size;
    uint64_t max_shared_memory_per_workgroup;
    int32_t supports_fp16;
    int32_t supports_bf16;
} bitnet_hip_device_info;
int bitnet_hip_get_device_info(int device, bitnet_hip_device_info *out);

/* ------------------------------------------------------------------------- */
/* 1. host-pointer drop-ins                                                    */
/* ------------------------------------------------------------------------- */

/* gemv_qk256(qs_data:&[u8], x:&[f32], y_out:&mut [f32], rows, cols, row_stride_bytes)
 * Q/i2s_qk256.rs:346-353 (live call sites T:684, T:924,
 * crates/bitnet-inference/src/layers/quantized_linear.rs:572).
 * y[r] = sum_j LUT[code(r,j)] * x[j], LUT {-2,-1,+1,+2}, LSB-first 2-bit codes,
 * a ragged tail (cols % 256 != 0) is summed like the reference's `take(cols)`.  Error text keeps the substrings the reference's tests
 * assert ("y_out length", "x length", "too short"; Q/i2s_qk256.rs:701-739). */
int bitnet_hip_gemv_qk256(const uint8_t *qs_data, size_t qs_len, const float *x, size_t x_len,
                          float *y_out, size_t y_len, size_t rows, size_t cols,
                          size_t row_stride_bytes);

/* i2s_matmul_f32(activations, weights_packed, scales, out, m, n, k, block_size)
 * K/cpu/quantized_matmul.rs:57-66 == i2s_matmul_forward(act,w,scales,out,&I2sMatmulConfig)
 * K/cuda/quantized_matmul.rs:309-326.
 * out[r,c] = sum_blk sum_{i in blk} act[r,i] * (t(code(c,i)) * scales[c*nb+blk]),
 * t: 0->0, 1->+1, 3->-1, 2->0; weights [n, ceil(k/4)] bytes; scales f32 [n, ceil(k/bs)]. */
int bitnet_hip_i2s_matmul_f32(const float *activations, size_t act_len,
                              const uint8_t *weights_packed, size_t w_len, const float *scales,
                              size_t scales_len, float *out, size_t out_len, size_t m, size_t n,
                              size_t k, size_t block_size);

/* qk256_gemv_hip(weights, scales, input, output, m, n, k, &Qk256GemvConfig)
 * K/rocm/qk256_gemv.rs:52-65 -- the stub this library fills.  Semantics are those
 * the CUDA twin documents (K/cuda/qk256_gemv.rs:1-16, K/cuda/quantized_matmul.rs:7-9):
 * ternary codes, one f32 scale per 256-element block: input [m,k], weights
 * [n, k/4], scales [n, k/256], output [m,n].  == i2s_matmul_f32 with block 256. */
int bitnet_hip_qk256_gemv(const uint8_t *weights, size_t w_len, const float *scales,
                          size_t scales_len, const float *input, size_t in_len, float *output,
                          size_t out_len, size_t m, size_t n, size_t k);

/* KernelProvider::matmul_i2s(a:&[i8], b:&[u8], c:&mut [f32], m, n, k)
 * K/lib.rs:44-52; arithmetic of K/cpu/fallback.rs:39-83 (C = A_i8 . B_u8, B is
 * UNPACKED u8 row-major [k,n], no scale); FFI twin bitnet_cpp_matmul_i2s
 * K/ffi/bridge.rs:21-28. */
int bitnet_hip_matmul_i2s(const int8_t *a, size_t a_len, const uint8_t *b, size_t b_len, float *c,
                          size_t c_len, size_t m, size_t n, size_t k);

/* QuantizedLinear::quantized_matmul_i2s(input, provider)  crates/bitnet-inference/src/layers/quantized_linear.rs:704-802 --
 * the composite the alternative layer runs above the trait: input [m, k] f32 -> i8 by clamp(x, -2, 1).round()
 * (quantize_input_i2s :1762-1773); weights_packed = the layer's 2-bit data, unpacked LSB-first to RAW codes 0..3 and handed
 * to matmul_i2s as its u8 [k, n] row-major operand exactly as the reference does (:769-776, :722-731); then every output
 * column times scales[col] (one scale per output feature) or scales[min(col * k / block_size, len - 1)] (:779-802,
 * input_scale = 1).  Lossy by construction in the reference too; restated quirk for quirk (oracle: bo_quantized_matmul_i2s). */
int bitnet_hip_quantized_matmul_i2s(const float *input, size_t in_len, const uint8_t *weights_packed, size_t w_len,
                                    const float *scales, size_t scales_len, size_t block_size, float *output,
                                    size_t out_len, size_t m, size_t n, size_t k);

/* KernelProvider::quantize(input, output, scales, qtype)  K/lib.rs:53-58;
 * I2S arithmetic of K/cpu/fallback.rs:102-159 (block 32, scale = absmax/1.5,
 * >0.5 -> 1, <-0.5 -> 3, else 0, OR-packed LSB-first into `output`, which the
 * caller zeroes); FFI twin bitnet_cpp_quantize K/ffi/bridge.rs:29-37.
 * Only qtype I2S is on the hot path; TL1/TL2 return BITNET_HIP_ERR_UNSUPPORTED. */
int bitnet_hip_quantize(const float *input, size_t input_len, uint8_t *output, size_t output_len,
                        float *scales, size_t scales_len, int qtype);

/* dequantize_to_f32[_transposed][_with_cfg](bytes, shape, cfg)
 * M/quant/i2s.rs:237, :448, :591, :774 -- blocks of ceil(bs/4) code bytes + 2 B LE
 * f16 scale, value = clamp(|f16|[^-1]*k, 1e-3, 1e3) * {-2,-1,+1,+2}[code]; block size
 * inferred from the byte count among {256,128,64,32}.  Unlike the reference's
 * lenient partial-data path, a byte count matching no block size is an error. */
int bitnet_hip_dequant_i2s(const uint8_t *bytes, size_t bytes_len, size_t rows, size_t cols,
                           int inv_scale, float k, int transposed, float *out, size_t out_len);

/* ------------------------------------------------------------------------- */
/* 2. device-resident API                                                      */
/* ------------------------------------------------------------------------- */

typedef uint64_t bitnet_hip_weights_t; /* opaque; 0 is never a valid handle */

/* Kernel selection for the device GEMV/matmul (bitnet_hip_set_kernel). */
#define BITNET_HIP_KERNEL_AUTO 0
#define BITNET_HIP_KERNEL_EXACT 1 /* one thread per output, reference summation order: bit-exact */
#define BITNET_HIP_KERNEL_VALU 2  /* wave-per-row, f32 FMA, shuffle reduction */
#define BITNET_HIP_KERNEL_MFMA 3  /* i8 MFMA on exact fixed-point activation digits, reference row-major codes */
#define BITNET_HIP_KERNEL_MFMA_TILED 4 /* same, codes re-tiled at upload into 1-KiB lane-ordered tiles */
int bitnet_hip_set_kernel(int kernel);
int bitnet_hip_get_kernel(void);

/* I2SQk256NoScale {rows, cols, row_stride_bytes, qs}  Q/i2s_qk256.rs:66-106:
 * accepts qs_len within +-128 B of rows*row_stride (the reference's alignment
 * slack); map {-2,-1,+1,+2}, no scale. */
int bitnet_hip_weights_upload_qk256(const uint8_t *qs_data, size_t qs_len, size_t rows,
                                    size_t cols, size_t row_stride_bytes,
                                    bitnet_hip_weights_t *out);
/* Ternary weights of K/cpu/quantized_matmul.rs:47-56: [n, ceil(k/4)] code bytes +
 * f32 scales [n, ceil(k/block_size)], block_size 32 (BitNet32-F16) or 256. */
int bitnet_hip_weights_upload_i2s(const uint8_t *weights_packed, size_t w_len, const float *scales,
                                  size_t scales_len, size_t n, size_t k, size_t block_size,
                                  bitnet_hip_weights_t *out);
/* Same storage with an explicit 4-entry code map (value of code 0..3), e.g. {-2,-1,0,+1}
 * x f32 block scale = I2SQuantizer::dequantize_tensor, the form the GGUF loader gives the
 * 32-element flavours (Q/utils.rs:76-91, Q/i2s.rs:181-237, M/gguf_simple.rs:1260-1285). */
int bitnet_hip_weights_upload_coded(const uint8_t *weights_packed, size_t w_len, const float *scales,
                                    size_t scales_len, size_t n, size_t k, size_t block_size,
                                    const int8_t *code_map, bitnet_hip_weights_t *out);
/* BitNet32-F16 on-disk blocks: per 32 elements 8 code bytes + 2 bytes LE f16 scale, blocks
 * running row-major over [n, k] (k % 32 == 0).  scale_mode 0: scale = f16 as stored
 * (M/gguf_simple.rs:1217-1233); scale_mode 1: scale = clamp(|f16|, 1e-3, 1e3)
 * (M/quant/i2s.rs:66-100, Sym map, k = 1). */
int bitnet_hip_weights_upload_inline_f16(const uint8_t *blocks, size_t len, size_t n, size_t k,
                                         const int8_t *code_map, int scale_mode, bitnet_hip_weights_t *out);
int bitnet_hip_weights_free(bitnet_hip_weights_t w);
/* rows (n), cols (k), algorithmic bytes one GEMV reads from this handle
 * (code bytes + scale bytes). */
int bitnet_hip_weights_info(bitnet_hip_weights_t w, size_t *rows, size_t *cols,
                            size_t *algorithmic_bytes);

/* Device memory behind a handle.  The streaming layout (1-KiB code tiles + scale tiles) is the only copy kept: the
 * reference-layout copy the reference-order kernels (BITNET_HIP_KERNEL_EXACT / _VALU) and the tiled matmul's 32-element
 * scales read is rebuilt on their first use (exact inverse permutation; that call synchronises its stream once) and stays
 * until bitnet_hip_weights_trim drops it again.  Nothing a host does concurrently on OTHER handles is affected. */
size_t bitnet_hip_weights_device_bytes(bitnet_hip_weights_t w);
int bitnet_hip_weights_trim(bitnet_hip_weights_t w);

/* y_dev[rows] = W . x_dev[cols]   (one activation row: batch-1 decode) */
int bitnet_hip_gemv_dev(bitnet_hip_weights_t w, const float *x_dev, float *y_dev, void *stream);
/* Y_dev[m, rows] = X_dev[m, cols] . W^T   (forward_qk256's per-row loop T:683-691,
 * batched; row-major, leading dimensions cols / rows) */
int bitnet_hip_matmul_dev(bitnet_hip_weights_t w, const float *x_dev, float *y_dev, size_t m,
                          void *stream);
/* The same with the kernel named per call (BITNET_HIP_KERNEL_*) instead of the process-wide default of
 * bitnet_hip_set_kernel: what a multi-threaded host uses (the trait is Send + Sync, K/lib.rs:39), and how
 * bench.py / the tests run an UNFUSED step on the bit-exact reference-order kernel next to the fast one. */
int bitnet_hip_matmul_kernel_dev(bitnet_hip_weights_t w, const float *x_dev, float *y_dev, size_t m,
                                 int kernel, void *stream);
/* Many activation rows at once (prefill; forward_qk256's per-row loop T:683-691 as ONE tiled
 * matmul on the matrix cores).  Same fusions as gemv_fused_dev, per row.  `digits` = base-256
 * fixed-point digits per activation (4: the GEMV's 30 bits; 3: 22 bits; 2: 14 bits -- on BitNet32-F16 matrices (32-element blocks
 * with f16 scales) digits = 2 means f16 activations with one power-of-two scale per row, on the f16 matrix cores).
 * The int8 digit planes live in a caller-owned device workspace.
 * flags (beside BITNET_HIP_FUSE_SILU_MUL), int8 digit form only -- f16 hand-over between the prompt forward's launches:
 *   BITNET_HIP_FUSE_X_F16: x_dev holds f16 rows [m][cols] (the attention's f16 output, the f16 silu * up rows); no LayerNorm with it
 *   BITNET_HIP_FUSE_Y_F16: with FUSE_SILU_MUL, y_dev receives the product as f16 rows [m][rows / 2]
 *   BITNET_HIP_FUSE_INT8_DIGITS: keep the int8 base-256 digit planes at digits = 2 on every matrix (without it BitNet32-F16 matrices
 *     take f16 activations on the f16 matrix cores, above)
 *   BITNET_HIP_FUSE_FP6_DIGITS: digits = 2 on an unscaled matrix (QK256) whose code map lies in -2..2: the SAME 15-bit integer per
 *     activation as three base-32 digits on the block-scaled fp6 x fp4 MFMA (k_gemm_fp6: same products, f32 accumulation of exact
 *     integers -- bit-identical to the int8 form while every partial sum stays below 2^24); also the process default with
 *     BITNET_HIP_GEMM_FP6=1.  Measured: 10-14 % faster per gate|up / down launch under sustained load, its quantiser 9-20 us slower
 *     per launch: about even inside a prompt, hence opt-in (EXPERIMENTS 4.6).  Round 5: the weight operands come from the resident fp4 image
 *     (bitnet_hip_weights_fp4_image, built on first use) unless
 *   BITNET_HIP_FUSE_FP6_EXPAND is set too: the fp6 form expanding the 2-bit streaming tiles in its K loop (no image is built or read) */
#define BITNET_HIP_FUSE_X_F16 2
#define BITNET_HIP_FUSE_Y_F16 4
#define BITNET_HIP_FUSE_INT8_DIGITS 8
#define BITNET_HIP_FUSE_FP6_DIGITS 16
#define BITNET_HIP_FUSE_FP6_EXPAND 32
size_t bitnet_hip_matmul_workspace_bytes(size_t m, size_t k, int digits);
int bitnet_hip_matmul_fused_dev(bitnet_hip_weights_t w, const float *x_dev, float *y_dev, size_t m,
                                const float *ln_gamma_dev, float ln_eps, const float *residual_dev,
                                int flags, int digits, void *workspace_dev, size_t workspace_bytes,
                                void *stream);
/* Which tile form the calling thread's last bitnet_hip_matmul_[fused_]dev launch ran (any pointer may be null): digits,
 * tokens per wave tile (16 / 32 / 64), waves per workgroup (4 / 8), weight-scale mode (0 none, 1 per 256-block, 2 per
 * 32-block on the masked K = 64 MFMA, 3 per 32-block on the K = 32 int8 MFMA with f16 scale tiles, 4 the f16 MFMA with the block
 * scale folded into f16 weights and f16 activations: BitNet32-F16 at digits = 2).  The parity tests assert
 * that the instance bench.py times (2 digits, 64-token tile) is the one they compared with the oracle. */
int bitnet_hip_matmul_last_tile(int *digits, int *wave_tokens, int *waves, int *scale_mode);
/* Output rows per wave of that launch: 64 (four 16-row tiles, 256-row workgroups) or 80 (five: the 320-row workgroups the forms with
 * f32 accumulators take when they need fewer rounds of the chip -- 2560 output rows x 4096 tokens = 512 workgroups, one round);
 * or 128 (the fp6 x fp4 form's 2 x 2 wave arrangement, k_gemm_fp6w: a wave owns 128 rows x 32 tokens of the 256 x 64 workgroup tile);
 * 0 before the thread's first tiled matmul.  scale_mode 5 = the f16 MFMA on an unscaled matrix, 6 = the fp6 x fp4 form (k_gemm_fp6). */
int bitnet_hip_matmul_last_wave_rows(void);
/* 1 when that launch was the fp6 x fp4 form reading its weight operands from the resident fp4 image (below), else 0. */
int bitnet_hip_matmul_last_resident_fp4(void);
/* The resident fp4 image of an unscaled matrix whose code map lies in -2..2 (QK256: every value is exact in fp4 e2m1): 4 bits per
 * weight in the fp6 x fp4 MFMA's A-operand order, kept BESIDE the 2-bit streaming tiles (which remain the decode path's copy:
 * bitnet_hip_weights_device_bytes counts both; QK256 2B-4T: q|k|v + gate|up of 30 layers = 678 MB, all seven projections 1.04 GB --
 * HBM is 288 GB).  With it bitnet_hip_matmul_fused_dev's BITNET_HIP_FUSE_FP6_DIGITS form loads its weight operands directly: no code
 * expansion in the K loop; the integers multiplied are the same, so the results stay bit-identical to the int8 digit planes.
 * enable = 1 builds it (idempotent; an allocation + one kernel, synchronises `stream`), 0 frees it.  Without this call the first
 * fp6-form launch on the handle builds it (not under stream capture); BITNET_HIP_FP4_RESIDENT=0 disables the image altogether.
 * Replaces nothing in the reference: its loader keeps one packed copy (crates/bitnet-quantization/src/i2s_qk256.rs:66-128). */
int bitnet_hip_weights_fp4_image(bitnet_hip_weights_t h, int enable, void *stream);

/* The prompt forward's f16 ACTIVATION CHAIN (north_star: "2-bit weight unpack x f16 activation dot product"; replaces the reference's
 * per-row loop T:683-691 / T:924 over many activation rows, K/cpu/quantized_matmul.rs:57-96 for the scaled format): every projection
 * reads an f16 matrix xh [m_pad][cols] (m_pad = m rounded up to 64; rows >= m are never stored but must be readable) that the kernel
 * which PRODUCED those activations wrote, so no conversion / quantisation launch sits between two projections.
 *   ln_gamma != NULL: LayerNorm (no bias, mean-subtracting, T:67-100) of the INPUT, applied after the product: xh must hold
 *                     f16(gamma * x); stats_in = float2 (sum, sum of squares) partials [n_stats][m_pad] of the exact f32 x over its
 *                     columns; the matrix must be bound to this gamma (bitnet_hip_weights_bind_ln).
 *   y (nullable): f32 rows [m][rows]; residual (nullable, may alias y): y = residual + W x (T:1073, T:1125).
 *   BITNET_HIP_FUSE_SILU_MUL: (gate, up) interleaved handle, outputs have rows / 2 columns (T:756-781).
 *   yh (nullable): the output as f16 rows [m_pad][rows or rows / 2], multiplied by gamma_out[row] first when given (the NEXT
 *                  LayerNorm's weight); stats_out (nullable): float2 [rows / 64][m_pad] partials of the f32 outputs for that LayerNorm:
 *                  (sum, sum of squares) over disjoint row ranges that together cover the row -- one per wave of the producing launch
 *                  (64 rows, or 80 in 320-row workgroups: then the first rows / 80 entries are used and the others are written as zero);
 *                  the consumer adds all rows / 64 entries up (n_stats = rows / 64).
 * bitnet_hip_matmul_f16_supported: rows % 256 == 0, cols % 256 == 0, code map values in -2..2, no scales or f16 32-block scales.
 * bitnet_hip_rows_to_f16_dev: the chain's entry (the embedding rows): xh = f16(gamma * x) (gamma nullable) + stats partial 0. */
/* f16 hand-over rows carry no row scale: a value beyond +-65504 is clamped -- and COUNTED.  Returns the number of lanes (up to four elements each)
 * that clamped a value of a live token since the last reset, in any of the chain's writers (bitnet_hip_rows_to_f16_dev, the yh outputs of
 * bitnet_hip_matmul_f16_dev / _matmul_qb32_dev / FUSE_Y_F16); reset != 0 clears it.  Synchronises the device.  A host that cannot rule such
 * activations out (outlier channels x gamma beyond the f16 range) checks it behind a prompt and repeats the prompt on the row-scaled forms
 * (bitnet_hip_matmul_fused_dev), as Decoder::prefill does. */
unsigned long long bitnet_hip_f16_saturations(int reset);
int bitnet_hip_matmul_f16_supported(bitnet_hip_weights_t w);
int bitnet_hip_rows_to_f16_dev(const float *x_dev, const float *gamma_dev, size_t m, size_t cols, void *xh_dev, float *stats_dev, void *stream);
int bitnet_hip_matmul_f16_dev(bitnet_hip_weights_t w, const void *xh_dev, size_t m, const float *stats_in_dev, size_t n_stats,
                              const float *ln_gamma_dev, float ln_eps, float *y_dev, const float *residual_dev, int flags, void *yh_dev,
                              const float *gamma_out_dev, float *stats_out_dev, void *stream);

/* QB32 ACTIVATIONS (round 5): the producer-quantised input of the fp6 x fp4 prompt matmul -- what QAct is to the decode GEMV.  The digit forms'
 * row quantiser needs the row maximum, which no producing workgroup has, so it stayed a launch of its own (two per layer, 6 % of the QK256
 * prompt).  The block-scaled MFMA takes one E8M0 scale per 32 K-slots of a token, so a QB32 row scales LOCALLY: per 32-column unit, E = exponent
 * of the unit's largest |v|, q = rint(v 2^(13 - E)) as three balanced base-32 fp6 digits (the 15-bit integer class of the 2-digit planes), one
 * exponent byte per unit.  Buffer: records [m_pad][cols / 256] of 592 bytes (576 of digits, the block's 8 exponent bytes, 8 of padding), m_pad = m
 * rounded up to 64 (bitnet_hip_qb32_bytes).  LayerNorm is applied after the product from the producer's statistics partials, as on the f16 chain.
 *   bitnet_hip_rows_to_qb32_dev: f32 rows -> QB32 of gamma * x (gamma nullable) + stats partial 0: the chain's entry (the embedding rows).
 *   bitnet_hip_matmul_f16_dev(..., flags | BITNET_HIP_FUSE_YH_QB32, yh_dev = a QB32 buffer of [m][rows], gamma_out, stats_out): the o- / down-
 *     projection's epilogue leaves gamma_out * y as QB32 rows (64-token tiles: m_pad / 64 * rows / 256 >= 256 workgroups; no FUSE_SILU_MUL).
 *   bitnet_hip_matmul_qb32_dev: bitnet_hip_matmul_f16_dev's arguments with a QB32 buffer as the input: y / residual / FUSE_SILU_MUL / yh (f16
 *     rows) / gamma_out / stats_out as there; matrices: unscaled, code map in -2..2, rows % 256 == 0, cols % 256 == 0 (reads the resident fp4
 *     image, building it on first use).  Replaces the reference's per-row loop T:683-691 / T:924 over many activation rows. */
#define BITNET_HIP_FUSE_YH_QB32 64
size_t bitnet_hip_qb32_bytes(size_t m, size_t cols);
int bitnet_hip_rows_to_qb32_dev(const float *x_dev, const float *gamma_dev, size_t m, size_t cols, void *qb_dev, float *stats_dev, void *stream);
int bitnet_hip_matmul_qb32_supported(bitnet_hip_weights_t w);
int bitnet_hip_matmul_qb32_dev(bitnet_hip_weights_t w, const void *qb_dev, size_t m, const float *stats_in_dev, size_t n_stats,
                               const float *ln_gamma_dev, float ln_eps, float *y_dev, const float *residual_dev, int flags, void *yh_dev,
                               const float *gamma_out_dev, float *stats_out_dev, void *stream);

/* Several uploaded matrices with the same cols / code map / block size as ONE
 * launch: rows concatenated (q|k|v share their input: T:288-290).  interleave16 != 0
 * (exactly two matrices of equal rows % 16 == 0) alternates 16-row tiles a0,b0,a1,b1..
 * so a (gate, up) pair meets in one workgroup (BITNET_HIP_FUSE_SILU_MUL). */
int bitnet_hip_weights_concat(const bitnet_hip_weights_t *parts, size_t n_parts, int interleave16,
                              bitnet_hip_weights_t *out);

/* GEMV with the neighbouring decode-step work fused in (MFMA kernel; a matrix shape that kernel does not take -- e.g. 32-element
 * scales with cols % 256 != 0 -- gets the same result from separate device launches in the reference's op order):
 *   ln_gamma != NULL : x <- LayerNorm(x) first -- no bias, WITH mean subtraction,
 *                      (x-mean)/sqrt(mean((x-mean)^2)+eps)*gamma  (T:67-100, T:1015, T:1104)
 *   residual != NULL : y = residual + W x                        (T:1073, T:1125)
 *   BITNET_HIP_FUSE_SILU_MUL (handle from concat(..., interleave16=1)):
 *                      y[r] = silu(gate[r]) * up[r], y has rows/2   (T:756-781) */
#define BITNET_HIP_FUSE_SILU_MUL 1
int bitnet_hip_gemv_fused_dev(bitnet_hip_weights_t w, const float *x_dev, float *y_dev, size_t m,
                              const float *ln_gamma_dev, float ln_eps, const float *residual_dev,
                              int flags, void *stream);
/* Optional, once per (matrix, LayerNorm weight) pair: precomputes g_r = W[r,:] . gamma so that
 * gemv_fused_dev called with THIS ln_gamma_dev pointer applies the LayerNorm after the product,
 * (W (gamma*x) - mean g) / denom -- same value to f32 rounding, ~1.4 us less per launch (no
 * whole-row pass before the weights can be used).  Re-bind if the gamma buffer's contents change. */
int bitnet_hip_weights_bind_ln(bitnet_hip_weights_t w, const float *ln_gamma_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* 3. decode-step operators (device pointers; K/rocm/rmsnorm.rs, attention.rs) */
/* ------------------------------------------------------------------------- */

/* rmsnorm_hip(input, gamma, output, num_rows, &HipRmsNormConfig{hidden_dim, eps})
 * K/rocm/rmsnorm.rs:50-60, host pointers: out = x / sqrt(mean(x^2)+eps) * gamma. */
int bitnet_hip_rmsnorm(const float *input, size_t in_len, const float *gamma, size_t gamma_len,
                       float *output, size_t out_len, size_t num_rows, size_t hidden_dim, float eps);
/* fused_attention_hip(q, k, v, output, seq_len, &HipAttentionConfig{num_heads, head_dim, causal, scale})
 * K/rocm/attention.rs:54-65: all four tensors [batch, num_heads, seq_len, head_dim] row-major f32
 * (batch = len / (num_heads*seq_len*head_dim)); softmax(scale * q k^T [+ causal mask]) v per head.
 * head_dim 128 (f16 operands on the matrix cores, f32 accumulate and softmax). */
int bitnet_hip_attention(const float *q, size_t q_len, const float *k, size_t k_len, const float *v,
                         size_t v_len, float *output, size_t out_len, size_t seq_len, size_t num_heads,
                         size_t head_dim, int causal, float scale);
/* qk256_gemv_hip_batch(&[GemvBatchItem], &cfg)  K/rocm/qk256_gemv.rs:67-82: items processed in order,
 * each with the arguments of bitnet_hip_qk256_gemv; stops at the first error. */
typedef struct bitnet_hip_gemv_item {
    const uint8_t *weights; size_t weights_len;
    const float *scales;    size_t scales_len;
    const float *input;     size_t input_len;
    float *output;          size_t output_len;
    size_t m, n, k;
} bitnet_hip_gemv_item;
int bitnet_hip_qk256_gemv_batch(const bitnet_hip_gemv_item *items, size_t n_items);
/* Device rows: rms != 0 -> RMSNorm (above); rms == 0 -> the LayerNorm the transformer
 * actually uses (layer_norm_with_optional_bias T:67-100: no bias, mean subtracted). */
int bitnet_hip_norm_rows_dev(const float *x_dev, const float *gamma_dev, float *out_dev, size_t rows,
                             size_t hidden, float eps, int rms, void *stream);
/* TransformerModel::embed (T:1390-1426), row gather from the f16 table [vocab, hidden];
 * tokens_dev: int32[]; reads tokens_dev[*offset_dev + i], i < n (offset_dev NULL = 0), so a
 * captured graph can walk a token history by position. */
int bitnet_hip_embed_f16_dev(const void *table_f16_dev, const int32_t *tokens_dev,
                             const int32_t *offset_dev, size_t n, size_t hidden, size_t vocab,
                             float *out_dev, void *stream);
/* The two elementwise steps of the reference's UNFUSED block (the fast path fuses them into GEMV epilogues):
 * out = a + b (residual add, T:1073, T:1125); out[i] = silu(gate[.]) * up[.] (T:765-781) -- tile == 0: separate
 * vectors; tile > 0: gate_dev is ONE vector of alternating `tile`-row groups (gate, up, gate, ...) as a plain GEMV
 * on a weights_concat(..., interleave16 = 1) handle produces it (tile = 16), up_dev = gate_dev + tile. */
int bitnet_hip_add_dev(const float *a_dev, const float *b_dev, float *out_dev, size_t n, void *stream);
int bitnet_hip_silu_mul_dev(const float *gate_dev, const float *up_dev, float *out_dev, size_t n, size_t tile,
                            void *stream);
/* *pos_dev += 1 (prompt positions whose logits nobody reads). */
int bitnet_hip_advance_pos_dev(int32_t *pos_dev, void *stream);
/* One new token through MultiHeadAttention::forward's core (T:373-540): RoPE on q,k with
 * the split-half layout (T:134-163) at position *pos_dev, append k,v to the f32 cache
 * (T:1171-1202; n_kv*ceil(max_pos/64)*64*head_dim floats each, layout private to this library: K is kept
 * transposed), GQA softmax attention over pos+1 keys.  head_dim 128, n_heads/n_kv <= 4.
 * The caches must be ZERO-FILLED before their first use (hipMemset once after allocation): the kernel
 * reads whole 64-position tiles and gives slots past the context an exact zero weight, which only cancels
 * finite bit patterns (slots left over from an earlier, longer sequence are fine).
 * qkv_dev: [n_heads*D | n_kv*D | n_kv*D] raw projections; out_dev: [n_heads*D].
 * rope_sin/cos_dev: [max_pos, D/2] (crates/bitnet-rope/src/lib.rs:59-93). */
int bitnet_hip_attention_decode_dev(const float *qkv_dev, const float *rope_sin_dev,
                                    const float *rope_cos_dev, float *kcache_dev, float *vcache_dev,
                                    size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                                    const int32_t *pos_dev, float *scratch_dev, float *out_dev,
                                    void *stream);
/* The same operator with workgroups of 512 threads that cover 128 positions each (half as many workgroups and chunk
 * records).  Slower than bitnet_hip_attention_decode_dev while n_kv_heads * ceil((pos + 1) / 64) fits the 256 CUs
 * (+1.5 us per layer at 0.4k..2.5k keys), faster beyond (4k keys, 5 KV heads: 320 -> 160 workgroups, 11.9 -> 10.9 us). */
int bitnet_hip_attention_decode_wide_dev(const float *qkv_dev, const float *rope_sin_dev,
                                         const float *rope_cos_dev, float *kcache_dev, float *vcache_dev,
                                         size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                                         const int32_t *pos_dev, float *scratch_dev, float *out_dev,
                                         void *stream);
/* Short contexts (at most bitnet_hip_attention_merge_max_keys() keys = 4 records of 64 positions): the attention in ONE launch plus an output projection that
 * merges the chunk results itself.  bitnet_hip_attention_decode_partial_dev = the first of the two kernels of
 * bitnet_hip_attention_decode_dev (RoPE, KV append, per-chunk softmax pieces into scratch_dev; same arguments,
 * no out_dev); bitnet_hip_gemv_attn_merge_dev(w, scratch, ...) = bitnet_hip_gemv_fused_dev(w, attention output,
 * y, m = 1, no LayerNorm, residual) with the attention output assembled from those records on the fly (every
 * workgroup of the projection reads every live record, n_chunks x 10 KB -- which is why this is for short
 * contexts only; the caller falls back to bitnet_hip_attention_decode_dev + bitnet_hip_gemv_fused_dev once
 * *pos_dev + 1 exceeds that).  w: cols == n_heads * 128; query group 1, 2 or 4.  scratch_dev must be zero-filled
 * before its first use (records of chunks past the context are read and given zero weight). */
int bitnet_hip_attention_decode_partial_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev,
                                            float *kcache_dev, float *vcache_dev, size_t n_heads, size_t n_kv_heads,
                                            size_t head_dim, size_t max_pos, const int32_t *pos_dev, float *scratch_dev,
                                            void *stream);
size_t bitnet_hip_attention_merge_max_keys(void); /* largest *pos_dev + 1 the merging projection takes (4 records) */
int bitnet_hip_gemv_attn_merge_dev(bitnet_hip_weights_t w, const float *attn_scratch_dev, size_t n_heads,
                                   size_t n_kv_heads, size_t max_pos, const int32_t *pos_dev, float *y_dev,
                                   const float *residual_dev, void *stream);
/* Which kernel bitnet_hip_gemv_dev / bitnet_hip_gemv_fused_dev / a bitnet_hip_matmul_dev row (merge 0) or bitnet_hip_gemv_attn_merge_dev
 * (merge = query heads per KV head: 1, 2 or 4) would launch for this matrix under the current bitnet_hip_set_kernel choice, and, when that is
 * the MFMA GEMV, which of its instances: flags = 0 or BITNET_HIP_FUSE_SILU_MUL, ln_gamma_dev = the LayerNorm weight the launch would pass
 * (NULL: none; the one bound with bitnet_hip_weights_bind_ln selects the LayerNorm-after-product form).  One activation row (m = 1).  Host
 * only: nothing is launched and the device is not touched.  What the launching entry would refuse for the shape is refused here with its
 * message.  kernel != BITNET_HIP_KERNEL_MFMA: the matrix leaves the MFMA GEMV (unfused = the LayerNorm / residual / silu * up around it run
 * as separate launches) and the instance fields are 0. */
typedef struct {
    int kernel;              /* BITNET_HIP_KERNEL_MFMA, _VALU or _EXACT: what run_gemv resolves the choice to */
    int unfused;             /* 1: the fused options run as separate launches around the product (kernel != MFMA only) */
    int k_split;             /* K ranges per 16-row tile = waves sharing a tile: 1, 2, 4 or 8 */
    int blocks;              /* 256-column blocks per row (the last one may be ragged) */
    int blocks_per_wave;     /* the longest K range */
    int ring;                /* blocks per wave the instance holds (2..5, >= blocks_per_wave) */
    int stat_vectors;        /* float4 LayerNorm-statistics vectors per thread the instance holds: 1 without LayerNorm, else 2 or 4 */
    int layernorm;           /* 0 none, 1 prologue on the activations, 2 after the product (the bound gamma) */
    int scale_form;          /* 32-block weight scales: 0 none, 1 f32, 2 f16 */
    int wscale;              /* 1: one f32 scale per (row, 256-block), folded at run time */
    int merge;               /* 1: the activation row is merged from the decode attention's chunk records */
    int tiles_per_workgroup; /* 8 / k_split */
    int grid;                /* workgroups per activation row */
    int lds_bytes;           /* dynamic LDS of the launch */
    int lds_raised;          /* 1: above 64 KiB, the kernel's dynamic LDS limit is raised before the launch */
} bitnet_hip_gemv_geometry_t;
int bitnet_hip_gemv_geometry(bitnet_hip_weights_t w, int flags, const float *ln_gamma_dev, int merge, bitnet_hip_gemv_geometry_t *out);
/* ---- the decode step on activations quantised by their PRODUCER ("QAct") ---------------------------------------
 * north_star's kernel is "2-bit weight unpack x f16 activation dot product".  The f16-class activation of this
 * library is a QAct: per 16 consecutive elements one power-of-two scale and a 15-bit fixed-point value per element
 * (two int8 digit planes), i.e. every element to 2^-15 of its 16-group's maximum; 576 bytes per 256 elements
 * (bitnet_hip_qact_bytes; layout private to the library, csrc/qact.hpp).  The kernel that PRODUCES a vector
 * writes it in this form (16 output rows of a GEMV = one group), so the consuming GEMV feeds the digit planes to the
 * matrix cores without touching them -- in round 1 every wave of every GEMV re-quantised its K range.  Exact f32
 * activations stay available through gemv_dev / gemv_fused_dev.
 * LayerNorm between producer and consumer (T:1015, T:1104) is applied after the product as with weights_bind_ln:
 * the producer multiplies by the consumer's gamma (gamma_out_dev) before quantising and leaves one (sum, sum of
 * squares) f64 pair per 16 rows (stats_out, bitnet_hip_qact_stats_bytes); the consumer passes them as stats_in together
 * with the bound ln_gamma_dev.  Shapes: cols % 256 == 0, rows % 16 == 0, no scales or 32-element block scales
 * (bitnet_hip_gemv_q_supported); everything else stays on gemv_fused_dev. */
size_t bitnet_hip_qact_bytes(size_t cols);
size_t bitnet_hip_qact_stats_bytes(size_t cols);
/* any f32 device vector -> QAct [* gamma] [+ statistics] (what a producing kernel does in its epilogue) */
int bitnet_hip_quantize_act_dev(const float *x_dev, const float *gamma_dev, size_t cols, void *qact_out,
                                double *stats_out, void *stream);
/* bitnet_hip_embed_f16_dev for ONE token, also leaving the first block's QAct (gamma_dev = its attention_norm) */
int bitnet_hip_embed_q_dev(const void *table_f16_dev, const int32_t *tokens_dev, const int32_t *offset_dev,
                           size_t hidden, size_t vocab, float *x_out_dev, const float *gamma_dev, void *qact_out,
                           double *stats_out, void *stream);
int bitnet_hip_gemv_q_supported(bitnet_hip_weights_t w);
/* Which kernel instance bitnet_hip_gemv_q_dev (merge_records 0) or bitnet_hip_gemv_attn_merge[_rec]_q_dev (merge_records 4 or 8) would launch
 * for this matrix: flags = 0 or BITNET_HIP_FUSE_SILU_MUL, layernorm != 0 = with ln_gamma_dev.  Host only: nothing is launched and the device
 * is not touched.  What the launching entry would refuse for the shape is refused here (BITNET_HIP_ERR_UNSUPPORTED / _INVALID_ARGUMENT). */
typedef struct {
    int k_split;             /* K ranges per 16-row tile = waves sharing a tile: 1, 2, 4 or 8 */
    int blocks;              /* 256-column blocks per row */
    int blocks_per_wave;     /* the longest K range */
    int ring;                /* blocks per wave the instance holds (2..5, >= blocks_per_wave) */
    int copy_passes;         /* 8-KiB passes of the activation copy (1..3) */
    int scale_form;          /* 32-block weight scales: 0 none, 1 f32, 2 f16 */
    int layernorm;           /* the LayerNorm-after-product instance */
    int tiles_per_workgroup; /* 8 / k_split */
    int grid;                /* workgroups */
    int merge_slots4, merge_slots1, merge_records; /* merging form: float4 / single-float slots per thread, records; 0 otherwise */
} bitnet_hip_gemv_q_geometry_t;
int bitnet_hip_gemv_q_geometry(bitnet_hip_weights_t w, int flags, int layernorm, size_t merge_records, bitnet_hip_gemv_q_geometry_t *out);
/* bitnet_hip_gemv_fused_dev on a QAct input: y = [residual +] W . act  [LayerNorm: ln_gamma_dev bound + stats_in]
 * [FUSE_SILU_MUL]; outputs: y_dev f32 (nullable) and / or qact_out [* gamma_out_dev] [+ stats_out]. */
int bitnet_hip_gemv_q_dev(bitnet_hip_weights_t w, const void *qact_in, const double *stats_in,
                          const float *ln_gamma_dev, float ln_eps, const float *residual_dev, int flags,
                          float *y_dev, void *qact_out, const float *gamma_out_dev, double *stats_out, void *stream);
/* bitnet_hip_attention_decode[_wide]_dev whose combine step also (or only: out_dev NULL) leaves the QAct of the
 * attention output for the o-projection */
#define BITNET_HIP_ATTN_WIDE 1    /* 128-position workgroups (bitnet_hip_attention_decode_wide_dev) */
#define BITNET_HIP_ATTN_KV_F16 2  /* the caches hold f16: HALF the bytes of the long-context stream.  Opt-in: the reference's cache is f32
                                   * (T:1171-1202); values are rounded once, from the exact f32 k / v, when appended.  Same element
                                   * counts as the f32 caches, half the allocation; zero-fill before first use likewise.  A cache is
                                   * f16 or f32 for its whole life: fill it with bitnet_hip_attention_prefill_kv16_dev / cache_f16 = 1. */
#define BITNET_HIP_ATTN_PARTIAL 4 /* chunk records only (bitnet_hip_attention_decode_partial_dev): out_dev and qact_out unused */
int bitnet_hip_attention_decode_q_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev,
                                      void *kcache_dev, void *vcache_dev, size_t n_heads, size_t n_kv_heads,
                                      size_t head_dim, size_t max_pos, const int32_t *pos_dev, float *scratch_dev,
                                      int flags, float *out_dev, void *qact_out, void *stream);
/* ---- the decode step for SEVERAL sequences per launch ------------------------------------------------------------
 * The reference's forward takes [B, T, H] and KVCache::new(config, batch_size, ..) carries a batch dimension
 * (crates/bitnet-transformer/src/lib.rs:281, :1146-1160, :1215-1245, :1437-1478).  These four entry points are the decode kernels above taking
 * n_seq = 1..BITNET_HIP_BATCH_MAX vectors per launch -- the weight stream (the f16 table) is read once and used for every vector -- and
 * generalise the reference's lock-step batch to sequences at DIFFERENT positions.  Conventions:
 *   - vector b of every batched buffer lies at b times its batch-1 size: bitnet_hip_qact_bytes / bitnet_hip_qact_stats_bytes of the vector's
 *     length, `rows` floats for y / residual (rows / 2 with FUSE_SILU_MUL), hidden floats, n_heads * head_dim floats, the qkv row,
 *     bitnet_hip_attention_scratch_bytes; the head's scratch is n_seq * n_wg * 8 bytes;
 *   - per-sequence state (KV caches, position, history, forced count, logits row) is reached through DEVICE arrays of n_seq device pointers,
 *     so every sequence keeps buffers of its own.  A NULL entry (history for the gather, a cache or the position for the attention, the
 *     logits row for the head) marks an IDLE slot: nothing is read or written for it.  The GEMV has no tables: it computes all n_seq
 *     vectors, an idle slot's vector must hold finite (stale) data and its outputs are ignored;
 *   - EVERY OUTPUT IS BIT-IDENTICAL to the batch-1 entry point called on that vector alone (same K partition, block order and sums);
 *   - asynchronous and capture-safe: no allocation, no synchronisation; n_seq == 0, n_seq > BITNET_HIP_BATCH_MAX and NULL required pointers
 *     return BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches. */
#define BITNET_HIP_BATCH_MAX 8
/* bitnet_hip_embed_q_dev for n_seq tokens: token b = history_ptrs[b][*pos_ptrs[b]] (clamped to the vocabulary as in batch-1) */
int bitnet_hip_embed_q_batch_dev(const void *table_f16_dev, const int32_t *const *history_ptrs_dev, const int32_t *const *pos_ptrs_dev,
                                 size_t n_seq, size_t hidden, size_t vocab, float *x_out_dev, const float *gamma_dev, void *qact_out,
                                 double *stats_out, void *stream);
/* bitnet_hip_gemv_q_dev for n_seq vectors: the same matrices (bitnet_hip_gemv_q_supported) and fusions; ln_gamma_dev / gamma_out_dev are
 * shared by all vectors.  n_seq whole QAct vectors stay in LDS (160 KiB): 8 vectors of up to 8704 columns; beyond: BITNET_HIP_ERR_UNSUPPORTED */
int bitnet_hip_gemv_q_batch_dev(bitnet_hip_weights_t w, size_t n_seq, const void *qact_in, const double *stats_in,
                                const float *ln_gamma_dev, float ln_eps, const float *residual_dev, int flags, float *y_dev,
                                void *qact_out, const float *gamma_out_dev, double *stats_out, void *stream);
/* bitnet_hip_attention_decode_q_dev (64-position records + combine: flags 0 or BITNET_HIP_ATTN_KV_F16) for n_seq sequences in ONE pair of
 * launches: every sequence applies RoPE, appends and attends at its own *pos_ptrs[b] over its own caches; all caches have max_pos slots */
int bitnet_hip_attention_decode_batch_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev,
                                          void *const *kcache_ptrs_dev, void *const *vcache_ptrs_dev,
                                          const int32_t *const *pos_ptrs_dev, size_t n_seq, size_t n_heads, size_t n_kv_heads,
                                          size_t head_dim, size_t max_pos, float *scratch_dev, int flags, float *out_dev,
                                          void *qact_out, void *stream);
/* bitnet_hip_logits_f16_dev for n_seq rows of x_dev: logits row b -> logits_ptrs[b]; then per slot the greedy pick of batch-1 (lowest index
 * on ties, NaN -> -inf): *token_ptrs[b] = token, history_ptrs[b][p + 1] = token unless p + 1 < *n_forced_ptrs[b], *pos_ptrs[b] = p + 1.
 * token_ptrs_dev / pos_ptrs_dev / history_ptrs_dev / n_forced_ptrs_dev may be NULL as a whole or per entry; a slot with neither a token nor
 * a position pointer gets logits only (a sequence that samples).  hidden * n_seq * 4 <= 152 KiB. */
int bitnet_hip_logits_f16_batch_dev(const void *table_f16_dev, const float *x_dev, const float *gamma_dev, float eps, size_t hidden,
                                    size_t vocab, size_t n_seq, float *const *logits_ptrs_dev, void *scratch_dev, size_t n_wg,
                                    int32_t *const *token_ptrs_dev, int32_t *const *pos_ptrs_dev, int32_t *const *history_ptrs_dev,
                                    const int32_t *const *n_forced_ptrs_dev, void *stream);
/* ---- the WIDE decode step: up to BITNET_HIP_WIDE_MAX live sequences as the dense rows of one matrix ---------------------------------
 * Between the batched step above (8 vectors, the batch-1 GEMV restated per vector) and the packed prompt forward (every member's rows on a
 * 64-row boundary) sits the step that puts M <= 64 sequences' current tokens into M dense rows: bitnet_hip_embed_rows_dev gathers them, the
 * many-row matmuls (bitnet_hip_matmul_fused_dev / _f16_dev) read every weight matrix once, bitnet_hip_attention_decode_rows_dev lets each row
 * attend over its own sequence's cache, bitnet_hip_score_f16_dev (targets -1, argmax, logits_rows = M) takes all logits rows from one pass
 * over the table and bitnet_hip_pick_rows_dev hands every row over to its sequence.  Conventions of the batched entries: per-sequence state
 * through DEVICE arrays of n_seq device pointers, a NULL entry = an idle row (nothing is read or written for it); asynchronous and
 * capture-safe (no allocation, no synchronisation).  BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches: n_seq outside
 * 1..BITNET_HIP_WIDE_MAX, a NULL required pointer, head_dim != 128, n_heads % n_kv_heads != 0 or a group larger than 4, unknown flag bits,
 * sizes that overflow. */
#define BITNET_HIP_WIDE_MAX 64
/* Row b of x_out_dev [n_seq, hidden] f32 = the embedding of history_ptrs[b][*pos_ptrs[b]], the token clamped to the vocabulary: bit for bit
 * what bitnet_hip_embed_f16_dev writes for that token.  An idle row (NULL history or position) is ZERO-FILLED: the matmuls read every row.
 * hidden % 8 == 0. */
int bitnet_hip_embed_rows_dev(const void *table_f16_dev, const int32_t *const *history_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq,
                              size_t hidden, size_t vocab, float *x_out_dev, void *stream);
/* bitnet_hip_attention_decode_batch_dev for up to 64 sequences with a ROW output.  qkv_dev: [n_seq, n_heads*D + 2*n_kv*D] dense.  Sequence b,
 * at p = *pos_ptrs[b]: RoPE on q and k at p, k and v appended at slot p of its own caches (exact f32, or rounded once to f16 under
 * BITNET_HIP_ATTN_CACHE_F16), attention over keys 0..p.  out_dev: [n_seq, n_heads*D] f32, or f16 rows under BITNET_HIP_ATTN_OUT_F16 (the
 * input format of bitnet_hip_matmul_f16_dev and of BITNET_HIP_FUSE_X_F16).  The kernels share their bodies with the batched and the batch-1
 * 64-position-record form: a row's f32 output and its cache bytes are BIT FOR BIT theirs; the f16 output is that f32 value rounded once to
 * nearest-even.
 * key_bound, 1..max_pos: the caller promises *pos_ptrs[b] < key_bound for every bound sequence, and the record grid covers
 * ceil(key_bound / 64) records instead of max_pos / 64 (64 sequences x 5 KV heads x 64 records are 20480 workgroups per layer, most of
 * which would leave at once).  A sequence that breaks the promise is treated as IDLE for the launch: its caches, its records and its output
 * row keep their bytes.  Any key_bound that covers every position gives the same bits.
 * scratch_dev: n_seq areas of bitnet_hip_attention_scratch_bytes(n_kv_heads, max_pos), zero-filled once before first use. */
int bitnet_hip_attention_decode_rows_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev, void *const *kcache_ptrs_dev,
                                         void *const *vcache_ptrs_dev, const int32_t *const *pos_ptrs_dev, size_t n_seq, size_t n_heads,
                                         size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t key_bound, float *scratch_dev, int flags,
                                         void *out_dev, void *stream);
/* The hand-over behind the head, one launch.  logits_dev: the head's [n_seq, vocab] f32 matrix; argmax_dev: its per-row argmax (lowest index
 * on ties, NaN = -inf: what bitnet_hip_score_f16_dev leaves; clamped to the vocabulary).  Row b: the logits row is copied to logits_ptrs[b]
 * (NULL: idle row); where token_ptrs[b] / pos_ptrs[b] are given, the greedy hand-over of bitnet_hip_logits_f16_dev with p = *pos_ptrs[b]:
 * *token_ptrs[b] = argmax, history_ptrs[b][p + 1] = token unless p + 1 < *n_forced_ptrs[b], *pos_ptrs[b] = p + 1.  A row with a logits
 * pointer but neither a token nor a position pointer gets logits only (a sequence that samples).  token / pos / history / n_forced tables may
 * be NULL as a whole or per entry. */
int bitnet_hip_pick_rows_dev(const float *logits_dev, const int32_t *argmax_dev, size_t n_seq, size_t vocab, float *const *logits_ptrs_dev,
                             int32_t *const *token_ptrs_dev, int32_t *const *pos_ptrs_dev, int32_t *const *history_ptrs_dev,
                             const int32_t *const *n_forced_ptrs_dev, void *stream);
/* ---- fork of a live sequence: the KV state of a prompt prefix, copied on the device ------------------------------------
 * The reference caches prompt prefixes on the host (crates/bitnet-inference/src/prefix_cache.rs: lookup, :173, returns the longest cached
 * prefix and its opaque `cached_state` bytes; insert, :212, stores one).  This entry replaces those host-side bytes with a device-to-device
 * copy: in every layer, KV head and destination, cache slots 0 .. n_positions - 1 of K and V become the source's, BIT FOR BIT (integer
 * loads and stores: NaN payloads and denormals pass through), in ONE launch that loads every source vector once and stores it n_dst times.
 * Every other byte of every destination cache keeps its value; the source is only read.
 *   - src_k_ptrs_dev / src_v_ptrs_dev: DEVICE arrays of n_layers cache pointers; dst_k_ptrs_dev / dst_v_ptrs_dev: DEVICE arrays
 *     [n_dst][n_layers] (destination d, layer l at d * n_layers + l), n_dst = 1..BITNET_HIP_BATCH_MAX;
 *   - flags: 0 (f32 caches) or BITNET_HIP_ATTN_KV_F16; every cache of one call has the same type (there is no conversion), the same
 *     max_pos and n_kv_heads, head_dim 128, and is 16-byte aligned;
 *   - source and destination buffers are DISTINCT: no destination cache may be (or overlap) a source cache or another destination's;
 *   - asynchronous and capture-safe: no allocation, no synchronisation.  n_positions == 0 is valid and launches nothing.  NULL tables,
 *     n_layers == 0, n_dst outside 1..BITNET_HIP_BATCH_MAX, head_dim != 128, n_kv_heads == 0, n_positions > max_pos ("KV cache
 *     overflow"), unknown flag bits and sizes that overflow return BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches. */
int bitnet_hip_kv_fork_dev(const void *const *src_k_ptrs_dev, const void *const *src_v_ptrs_dev, void *const *dst_k_ptrs_dev,
                           void *const *dst_v_ptrs_dev, size_t n_layers, size_t n_dst, size_t n_kv_heads, size_t head_dim,
                           size_t max_pos, size_t n_positions, int flags, void *stream);
/* ---- compact snapshots of a live sequence: bitnet_hip_kv_snapshot_bytes, bitnet_hip_kv_save_dev, bitnet_hip_kv_restore_dev -- the KV state of a
 * prompt prefix WITHOUT the cache around it, in a public position-major layout: declared in bitnet_hip_kvsnap.h, included at the end of this
 * header. */
/* ---- context shift of a live sequence: drop positions from the middle of the KV state, on the device -------------------
 * The reference has the pieces on the host: KvCacheBuffer::rotate_kv and truncate (crates/bitnet-kernels/src/cuda/kv_cache.rs:305-348) and
 * WindowedKVCache (crates/bitnet-gpu-hal/src/sliding_window.rs:161-235): keep the first `keep` positions (the attention sinks), discard the
 * next `discard`, slide the rest down.  This entry does that IN PLACE on the private device layouts, in ONE launch: in every layer and KV
 * head, for every j in [keep, n_positions - discard),
 *   - V slot j takes V slot j + discard, BIT FOR BIT (integer loads and stores);
 *   - K slot j takes the key of slot j + discard RE-ROTATED (K is cached after RoPE).  For every RoPE pair (x0, x1) = dims (i, i + 64), with
 *     (sa, ca) = table row j + discard and (sb, cb) = table row j, in f32, unfused, in this order:
 *         c = ca*cb + sa*sb;  s = sa*cb - ca*sb;  x0' = x0*c + x1*s;  x1' = x1*c - x0*s
 *     -- the two table rows actually involved, not row `discard`: rows built from f32 angles do not compose to f32 accuracy.  An f16 cache
 *     word is widened exactly, computed in f32 and rounded once (nearest-even) to f16.
 * Every byte outside those slots keeps its value: slots < keep, slots >= n_positions - discard (stale, as after a rewind), the padding
 * slots of the last chunk.  No slot is read after it was overwritten although the ranges overlap (kernels_kvshift.hip states the argument).
 *   - k_ptrs_dev / v_ptrs_dev: DEVICE arrays of n_layers cache pointers; rope_sin_dev / rope_cos_dev: [max_pos, 64] f32;
 *   - flags: 0 (f32 caches) or BITNET_HIP_ATTN_KV_F16; every cache has the same type, max_pos and n_kv_heads, head_dim 128, and is
 *     16-byte aligned;
 *   - asynchronous and capture-safe: no allocation, no synchronisation, no workspace.  n_positions - keep - discard == 0 is valid and
 *     launches nothing.  NULL tables or RoPE pointers, n_layers == 0, n_kv_heads == 0, head_dim != 128, discard == 0,
 *     keep + discard > n_positions, n_positions > max_pos ("KV cache overflow"), unknown flag bits and sizes that overflow return
 *     BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches. */
int bitnet_hip_kv_shift_dev(void *const *k_ptrs_dev, void *const *v_ptrs_dev, const float *rope_sin_dev, const float *rope_cos_dev,
                            size_t n_layers, size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t keep, size_t discard,
                            size_t n_positions, int flags, void *stream);
/* bitnet_hip_attention_prefill_dev filling f16 decode caches */
int bitnet_hip_attention_prefill_kv16_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev,
                                          void *kcache_f16_dev, void *vcache_f16_dev, size_t n_heads, size_t n_kv_heads,
                                          size_t head_dim, size_t max_pos, size_t seq_len, void *workspace_dev,
                                          size_t workspace_bytes, float *out_dev, void *stream);
/* The same call with a flag word: BITNET_HIP_ATTN_CACHE_F16 = the f16 caches of _kv16_dev; BITNET_HIP_ATTN_OUT_F16 = `out` receives
 * f16 rows [seq_len][n_heads * head_dim] (the input format of bitnet_hip_matmul_f16_dev: the o-projection reads them as they are). */
#define BITNET_HIP_ATTN_CACHE_F16 1
#define BITNET_HIP_ATTN_OUT_F16 2
int bitnet_hip_attention_prefill_flags_dev(const float *qkv, const float *rope_sin, const float *rope_cos, void *kcache, void *vcache, size_t n_heads,
                                           size_t n_kv_heads, size_t head_dim, size_t max_pos, size_t seq_len, void *workspace, size_t workspace_bytes,
                                           void *out, int flags, void *stream);
/* Continuing a LIVE sequence: seq_len new tokens at absolute positions past_len .. past_len + seq_len - 1 over caches that already hold
 * positions 0 .. past_len - 1 (filled by any mix of bitnet_hip_attention_prefill*_dev, the decode attention and earlier calls of this
 * operator).  The reference's attention takes seq_len queries over past_len + seq_len keys from its cache, create_causal_mask(q_len,
 * k_len) hiding the keys beyond past_len + i from query i (T:455-470, T:704-719; cache append T:1171-1202).  qkv_dev: [seq_len,
 * n_heads*D + 2*n_kv*D], the raw projections of the NEW tokens.  The call applies RoPE to q and k at the absolute positions, appends
 * the new k, v to the caches (exact f32, or rounded once to f16) and computes causal GQA attention of each new query over keys 0 .. its
 * own position; out_dev: [seq_len, n_heads*D].  flags: BITNET_HIP_ATTN_CACHE_F16 | BITNET_HIP_ATTN_OUT_F16 as above.  past_len may be
 * ANY value in [0, max_pos - seq_len] (not only a multiple of 64), seq_len >= 1, head_dim 128; past_len + seq_len > max_pos fails with
 * "KV cache overflow".  Cache slots at positions >= past_len are never read as keys (they may hold what a longer, rewound sequence left
 * there) and slots < past_len are not written.  Every call re-reads the past from the cache: O(past_len) bytes on top of the attention.
 * The workspace size is 0 for invalid sizes and non-decreasing in both lengths; the call is asynchronous on `stream`. */
size_t bitnet_hip_attention_extend_workspace_bytes(size_t n_heads, size_t n_kv_heads, size_t past_len, size_t seq_len);
int bitnet_hip_attention_extend_dev(const float *qkv_dev, const float *rope_sin_dev, const float *rope_cos_dev,
                                    void *kcache_dev, void *vcache_dev, size_t n_heads, size_t n_kv_heads, size_t head_dim,
                                    size_t max_pos, size_t past_len, size_t seq_len, void *workspace_dev, size_t workspace_bytes,
                                    void *out_dev, int flags, void *stream);
/* SEVERAL sequences' new tokens in ONE prep launch and ONE attention launch: the prompt-side twin of the batched decode step (the
 * reference's forward takes [B, T, H] in lock step, crates/bitnet-transformer/src/lib.rs:1437-1478; here every sequence has its own
 * position and its own number of new tokens).  qkv_dev: [n_rows, n_heads*D + 2*n_kv*D], the raw projections.  Segment s = one sequence
 * owns rows row0[s] .. row0[s] + len[s] - 1; for it the call is bitnet_hip_attention_extend_dev(those rows, past[s], len[s]) on
 * kcache[s] / vcache[s]: RoPE of q and k at positions past[s] .., k / v appended at those slots (exact f32, or rounded once to f16),
 * causal GQA attention of each new query over keys 0 .. its own position OF ITS OWN SEQUENCE.  Slots < past[s] are read and never
 * written, slots >= past[s] + len[s] are neither read nor written; past[s] == 0 reads nothing from the cache.
 *   - row0[s] is a multiple of bitnet_hip_attention_packed_row_align(n_heads, n_kv_heads) -- the attention workgroup's query tile, which
 *     must lie inside one segment: 64 rows when n_heads / n_kv_heads is even, 128 when it is odd (0 for invalid head counts) -- and segments
 *     do not overlap; their order in the table is free.  Rows that belong to no segment are padding: they are not read, nothing is
 *     written to any cache for them, their output rows are unspecified but finite.
 *   - row0, len, past, kcache, vcache are HOST arrays of n_seq = 1..BITNET_HIP_PACK_MAX entries (the cache entries are device pointers); they
 *     travel as kernel arguments, so the call is asynchronous on `stream` without an upload: no allocation, no synchronisation, and the arrays
 *     may be reused as soon as it returns.  All caches have max_pos slots, head_dim 128 and the type flags says.
 *   - out_dev: [n_rows, n_heads*D]; flags: BITNET_HIP_ATTN_CACHE_F16 | BITNET_HIP_ATTN_OUT_F16 as above.
 *   - BITNET_HIP_ERR_INVALID_ARGUMENT before anything launches: n_seq outside 1..BITNET_HIP_PACK_MAX; NULL tables, buffers or caches; len < 1;
 *     past < 0; past + len > max_pos ("KV cache overflow"); a misaligned or overlapping row0; a segment beyond n_rows; head_dim != 128;
 *     n_heads % n_kv_heads != 0; one cache pointer in two places; a workspace that is too small; unknown flag bits.
 * The workspace size is 0 for invalid sizes and non-decreasing in every past[s] and len[s]. */
#define BITNET_HIP_PACK_MAX 64
size_t bitnet_hip_attention_packed_row_align(size_t n_heads, size_t n_kv_heads);
size_t bitnet_hip_attention_packed_workspace_bytes(size_t n_heads, size_t n_kv_heads, size_t n_rows, size_t n_seq, const int32_t *past,
                                                   const int32_t *len);
int bitnet_hip_attention_packed_dev(const float *qkv_dev, size_t n_rows, const float *rope_sin_dev, const float *rope_cos_dev, size_t n_seq,
                                    const int32_t *row0, const int32_t *len, const int32_t *past, void *const *kcache_dev,
                                    void *const *vcache_dev, size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                                    void *workspace_dev, size_t workspace_bytes, void *out_dev, int flags, void *stream);
/* bitnet_hip_gemv_attn_merge_dev (short contexts) with the QAct outputs of gemv_q_dev */
int bitnet_hip_gemv_attn_merge_q_dev(bitnet_hip_weights_t w, const float *attn_scratch_dev, size_t n_heads,
                                     size_t n_kv_heads, size_t max_pos, const int32_t *pos_dev, float *y_dev,
                                     const float *residual_dev, void *qact_out, const float *gamma_out_dev,
                                     double *stats_out, void *stream);
/* The same with the record bound chosen by the caller: max_records = 4 is bitnet_hip_gemv_attn_merge_q_dev itself; 8 merges up to 8 records
 * of 64 positions (*pos_dev + 1 <= bitnet_hip_attention_merge_q_max_keys() = 512) and gives bit-identical y / QAct / statistics while at
 * most 4 records are live.  All max_records records are requested by every workgroup (the request is what the merge costs: 41 KB at 4, 82 KB
 * at 8 records x 2560 columns), so pass the smallest bound that covers the context.  8 records: w takes the QAct form, cols <= 2560. */
size_t bitnet_hip_attention_merge_q_max_keys(void);
int bitnet_hip_gemv_attn_merge_rec_q_dev(bitnet_hip_weights_t w, const float *attn_scratch_dev, size_t n_heads,
                                         size_t n_kv_heads, size_t max_pos, const int32_t *pos_dev, float *y_dev,
                                         const float *residual_dev, void *qact_out, const float *gamma_out_dev,
                                         double *stats_out, size_t max_records, void *stream);
/* The same attention for a whole prompt of seq_len tokens on a FRESH cache (positions
 * 0..seq_len-1): RoPE, cache append, causal GQA softmax attention (T:398-543 with the causal
 * mask T:452-470).  qkv_dev: [seq_len, n_heads*D + 2*n_kv*D]; out_dev: [seq_len, n_heads*D].
 * q, k, v and the probabilities go through the matrix cores in f16 (f32 accumulate); the
 * cache receives the exact f32 k, v.  Semantics of the reference's stub
 * fused_attention_hip(q,k,v,output,seq_len,&cfg{num_heads,head_dim,causal=true,scale=1/sqrt(d)})
 * (K/rocm/attention.rs:54-65) with grouped KV heads. */
size_t bitnet_hip_attention_prefill_workspace_bytes(size_t n_heads, size_t n_kv_heads, size_t seq_len);
int bitnet_hip_attention_prefill_dev(const float *qkv_dev, const float *rope_sin_dev,
                                     const float *rope_cos_dev, float *kcache_dev, float *vcache_dev,
                                     size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_pos,
                                     size_t seq_len, void *workspace_dev, size_t workspace_bytes,
                                     float *out_dev, void *stream);
/* Token-parallel form of the call above (long prompts split over several GPUs): this GPU holds
 * n_q of the prompt's query rows, q_dev [n_q, ld_q] (head h at columns [128 h, 128 h+128)), in
 * 64-row blocks whose absolute first positions are q_block_pos_dev[b] (multiples of 64; only
 * the last block may be partial), and the raw k|v rows of the WHOLE context gathered from all
 * ranks in absolute order, kv_dev [n_ctx, ld_kv] (k heads, then v heads).  Every query attends
 * to positions <= its own; the cache receives all n_ctx positions.  Needs no collective itself:
 * the caller gathers k|v (RCCL all-gather) between the projection and this call. */
size_t bitnet_hip_attention_prefill_sharded_workspace_bytes(size_t n_heads, size_t n_kv_heads, size_t n_q, size_t n_ctx);
int bitnet_hip_attention_prefill_sharded_dev(const float *q_dev, size_t ld_q, const int32_t *q_block_pos_dev,
                                             size_t n_q, const float *kv_dev, size_t ld_kv, size_t n_ctx,
                                             const float *rope_sin_dev, const float *rope_cos_dev,
                                             float *kcache_dev, float *vcache_dev, size_t n_heads,
                                             size_t n_kv_heads, size_t head_dim, size_t max_pos,
                                             void *workspace_dev, size_t workspace_bytes, float *out_dev,
                                             void *stream);
/* The same with the k|v rows exactly as an all-gather over `world` ranks left them: rank r's block holds its two zigzag
 * chunks (chunk c of 2 * world equal chunks belongs to rank c or 2 * world - 1 - c: every rank gets the same amount of
 * causal attention), each row = k heads then v heads, f32 or -- kv_is_f16 -- f16 (half the bytes on the wire; the f32 decode
 * cache then holds the f16-rounded k, v of the prompt).  No scatter pass on the host side: the position -> row map is
 * applied where the rows are read.  n_ctx % (2 * world * 64) == 0.  bitnet_hip_pack_cols_dev builds the send buffer: the
 * columns [col0, col0 + ncols) of `rows` f32 rows, compact, as f32 or f16. */
int bitnet_hip_attention_prefill_gathered_dev(const float *q_dev, size_t ld_q, const int32_t *q_block_pos_dev, size_t n_q,
                                              const void *kv_gathered_dev, size_t n_ctx, size_t world, int kv_is_f16,
                                              const float *rope_sin_dev, const float *rope_cos_dev, void *kcache_dev,
                                              void *vcache_dev, int cache_f16, size_t n_heads, size_t n_kv_heads,
                                              size_t head_dim, size_t max_pos, void *workspace_dev, size_t workspace_bytes,
                                              float *out_dev, void *stream);
/* The same in two steps, so that the all-gather of k|v can run on ANOTHER stream beside the query-side work: phase 1 prepares the
 * query slabs only (RoPE, f16; kv_gathered_dev is not read), phase 2 does the k / v slabs, the cache fill and the attention on
 * the workspace phase 1 left; phase 0 = both (the call above).  cache_f16 is a flag word here: BITNET_HIP_ATTN_CACHE_F16 (bit 0, as
 * above) | BITNET_HIP_ATTN_OUT_F16 (bit 1: out_dev receives f16 rows, the o-projection's FUSE_X_F16 / f16-chain input). */
int bitnet_hip_attention_prefill_gathered_phase_dev(const float *q_dev, size_t ld_q, const int32_t *q_block_pos_dev, size_t n_q,
                                                    const void *kv_gathered_dev, size_t n_ctx, size_t world, int kv_is_f16,
                                                    const float *rope_sin_dev, const float *rope_cos_dev, void *kcache_dev,
                                                    void *vcache_dev, int cache_f16, size_t n_heads, size_t n_kv_heads,
                                                    size_t head_dim, size_t max_pos, void *workspace_dev, size_t workspace_bytes,
                                                    float *out_dev, int phase, void *stream);
int bitnet_hip_pack_cols_dev(const float *src_dev, size_t ld, size_t col0, size_t ncols, size_t rows, void *dst_dev,
                             int as_f16, void *stream);
/* bytes of scratch_dev attention_decode_dev needs (per-chunk softmax partials) */
size_t bitnet_hip_attention_scratch_bytes(size_t n_kv_heads, size_t max_pos);
/* TransformerModel::logits, tied embeddings (T:1599-1630): logits = LN(x) . E^T, E the f16
 * table [vocab, hidden], f32 accumulate; gamma_dev == NULL skips the final norm (T:1589).
 * scratch_dev: >= 8 * n_workgroups bytes (argmax partials); token_dev (nullable) receives
 * the greedy token (argmax, lowest index on ties, NaN -> -inf:
 * crates/bitnet-cli/src/sampling.rs:45-49,189-202); with p = *pos_dev (nullable):
 * history_dev[p+1] = token unless p+1 < *n_forced_dev (a prompt token already sits there),
 * then *pos_dev = p+1. */
int bitnet_hip_logits_f16_dev(const void *table_f16_dev, const float *x_dev, const float *gamma_dev,
                              float eps, size_t hidden, size_t vocab, float *logits_dev,
                              void *scratch_dev, size_t n_workgroups, int32_t *token_dev,
                              int32_t *pos_dev, int32_t *history_dev, const int32_t *n_forced_dev,
                              void *stream);
/* The SCREENED greedy head: the token, history entry and position bitnet_hip_logits_f16_dev would leave, bit for bit (ties, NaN -> -inf and
 * forced tokens included), from about half the bytes -- and NO logits vector.  An int8 screening image of the table (built once per table on
 * the device: per row int8 codes, an f32 scale and an f32 error coefficient; bitnet_hip_head_screen_bytes bytes, 0 = no instance for this
 * hidden size: 512, 1024, 2048, 2560 and 4096 have one) gives every row a proven interval [lb, ub] around the f32 logit the full head would
 * compute; the rows whose ub is not below the largest lb are then computed from the f16 table with the full head's own arithmetic, and the
 * pick is taken among them.  The result never depends on how many rows that is (non-finite input: all of them).
 * ws_dev: bitnet_hip_head_screen_ws_bytes bytes of floats, with V4 = vocab rounded up to 4 and N4 = n_workgroups rounded up to 4:
 *   [0, vocab) ub | [V4, V4 + n_workgroups) per-workgroup maxima of lb | [V4 + N4, + hidden) a copy of x_dev | three uint32 words at
 *   V4 + N4 + hidden: rows this launch rescored, launches so far (+1 per launch), rows rescored by all launches (zero the words once) |
 *   [V4 + N4 + hidden + 4, + vocab) the rescored logits (rows not rescored: untouched).
 * Every other argument is bitnet_hip_logits_f16_dev's. */
size_t bitnet_hip_head_screen_bytes(size_t hidden, size_t vocab);
size_t bitnet_hip_head_screen_ws_bytes(size_t hidden, size_t vocab, size_t n_workgroups);
int bitnet_hip_head_screen_build_dev(const void *table_f16_dev, size_t hidden, size_t vocab, void *image_dev, void *stream);
int bitnet_hip_logits_screen_dev(const void *table_f16_dev, const float *x_dev, const float *gamma_dev,
                                 float eps, size_t hidden, size_t vocab, const void *image_dev, float *ws_dev,
                                 void *scratch_dev, size_t n_workgroups, int32_t *token_dev,
                                 int32_t *pos_dev, int32_t *history_dev, const int32_t *n_forced_dev,
                                 void *stream);
/* argmax over a device vector with the same tie/NaN rules; scratch as above. */
int bitnet_hip_argmax_dev(const float *v_dev, size_t n, void *scratch_dev, size_t n_workgroups,
                          int32_t *token_dev, void *stream);

/* Teacher-forced scoring of prompt rows (score.rs / eval.rs NLL, parity::eval_logits_all_positions).  Row r of x_dev ([n_rows, hidden] f32, the
 * residual stream after the last block): l_r = f16(LN(x_r) * gamma) . E^T, E the f16 table [vocab, hidden], f32 accumulate; non-finite l -> -inf;
 * nll_dev[r] = logsumexp(l_r) - l_r[targets_dev[r]]  (0 where target < 0, NaN where target >= vocab, +inf where the target logit is non-finite,
 * NaN where every logit of the row is);  argmax_dev[r] (nullable): lowest index on ties;  logits_dev (nullable): raw logits of rows [0, logits_rows),
 * f32 [logits_rows, vocab].  Deterministic.  hidden % 64 == 0.
 * gamma_dev == NULL: no norm (l_r = f16(x_r) . E^T).  The workspace holds the f16 rows and one 16-byte partial per (row, 128-entry vocabulary
 * block); bitnet_hip_score_workspace_bytes returns 0 for sizes this library refuses. */
size_t bitnet_hip_score_workspace_bytes(size_t n_rows, size_t hidden, size_t vocab);
int bitnet_hip_score_f16_dev(const void *table_f16_dev, const float *x_dev, const float *gamma_dev, float eps, size_t hidden, size_t vocab,
                             size_t n_rows, const int32_t *targets_dev, float *nll_dev, int32_t *argmax_dev, float *logits_dev,
                             size_t logits_rows, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- sampling on the device: crates/bitnet-cli/src/sampling.rs `Sampler` ---------------------------------------
 * The reference's `Sampler::sample(&logits, &generated_tokens)` in its order: count every entry of the list, repetition
 * penalty (rp^count by compiler-builtins' __powisf2 loop; logit > 0 ? logit / p : logit * p), NaN -> -inf, greedy shortcut
 * (temperature 0, or temperature 1 && top_k 0 && top_p 1: argmax, lowest index on ties, no RNG word), temperature
 * (division), stable top-k, top-p over the stable descending order, softmax draw with u = (next_u32 >> 8) * 2^-24 from
 * ChaCha20Rng::seed_from_u64(seed).  Three paths, one launch each:
 *   greedy (+- penalty): bit-exact;
 *   1 <= top_k <= BITNET_HIP_SAMPLE_SMALL_K (< vocab): top-p and the draw over the k survivors in the reference's order
 *   (equal up to device expf against the host's in the last ulp);
 *   otherwise (top_k 0 or larger, full-vocabulary temperature / top-p): parallel sums, equal except where a deciding
 *   comparison lies within ~2^-12 of its threshold.
 * The state (config, ChaCha20 key, words drawn, per-token counts) lives in device memory: a graph that captured
 * bitnet_hip_sample_dev follows bitnet_hip_sampler_configure.  A sampler serves one stream at a time.
 * Invalid configs: temperature NaN, negative or infinite; top_k < 0; top_p NaN; repetition_penalty <= 0 or NaN.  top_p <= 0
 * keeps the top entry alone, as the reference does. */
#define BITNET_HIP_SAMPLE_SMALL_K 64
typedef struct bitnet_hip_sampling_config {
    float temperature;        /* --temperature (reference default 1.0) */
    int32_t top_k;            /* --top-k (0 = off) */
    float top_p;              /* --top-p (1.0 = off) */
    float repetition_penalty; /* --repetition-penalty (1.0 = off) */
    uint64_t seed;            /* --seed */
} bitnet_hip_sampling_config;
typedef struct bitnet_hip_sampler bitnet_hip_sampler;
/* vocab in 1..2^20.  Allocates device memory (~5 * 4 * vocab bytes); not capture-safe. */
int bitnet_hip_sampler_create(size_t vocab, const bitnet_hip_sampling_config *cfg, bitnet_hip_sampler **out);
void bitnet_hip_sampler_destroy(bitnet_hip_sampler *sampler);
/* New config and seed: the key is re-derived and the word counter restarts at 0; the counts stay.  Synchronous copy:
 * not capture-safe, but graphs captured before it stay valid and follow it. */
int bitnet_hip_sampler_configure(bitnet_hip_sampler *sampler, const bitnet_hip_sampling_config *cfg);
/* The sampler chain: min-p, typical-p and the additive penalties of the reference's serving front ends around the stages above.
 * A stage removes entries (-inf); the next one sees the softmax of the survivors.  The order is fixed:
 *   counts; ADDITIVE PENALTIES; repetition penalty; NaN -> -inf; greedy shortcut; temperature; top-k; top-p; MIN-P; TYPICAL-P;
 *   softmax; draw.
 * Additive penalties (crates/bitnet-sampling/src/strategies.rs RepetitionPenaltyConfig::apply :247-259): for a token with
 *   occurrence count c > 0, x -= frequency_penalty * (float)c, then x -= presence_penalty, two separate f32 operations in front
 *   of the multiplicative penalty.  For bitnet_hip_sample_dev c is how often this sampler chose the token since the last reset (not
 *   the compounding exponent of the repetition penalty); for bitnet_hip_sample_host it is the token's occurrences in that call's
 *   list (ids >= vocab skipped).  Both 0: the stage is skipped.  Negative values are a bonus.
 * Min-p (crates/bitnet-logits/src/lib.rs apply_min_p :299-310, strategies.rs MinPSampler :37-50): with p the softmax of the
 *   survivors, an entry is removed iff p_i < min_p * max_j p_j.  Clamped to [0, 1]; <= 0 off; 1 keeps the entries tied at the maximum.
 * Typical-p (lib.rs apply_typical :337-381, strategies.rs TypicalSampler :73-86): over the survivors with p > 0, H = -sum p ln p,
 *   d_i = |(-ln p_i) - H|; entries are taken by ascending d until the running sum of p first reaches >= typical_p (the entry that
 *   crosses is kept), the rest are removed, and so is a survivor whose probability is 0.  The reference sorts unstably, so it
 *   leaves the order of equal deviations open: here it is ascending token id.  Clamped to [0, 1]; >= 1 off; 0 keeps the single most
 *   typical entry.  With 1 <= top_k <= BITNET_HIP_SAMPLE_SMALL_K the stage runs over the k survivors in one lane in the reference's
 *   order; on the full-vocabulary path it is a radix select over the deviations with fixed-point mass sums (the roundings are listed in
 *   csrc/kernels_sample.hip), equal except where a deciding comparison lies within those roundings of its threshold.
 * The greedy shortcut needs min_p <= 0 and typical_p >= 1 beside temperature 1, top_k 0, top_p 1 (or temperature 0); the additive
 *   penalties apply in front of its argmax, which stays bit-exact and draws no word.
 * On a row with no finite maximum both new stages are no-ops.
 * Invalid beside the base config's: min_p NaN; typical_p NaN; frequency_penalty or presence_penalty NaN or infinite.
 * bitnet_hip_sampler_create / _configure are these two with min_p 0, typical_p 1 and both penalties 0.  configure_ex is
 * synchronous and not capture-safe; graphs captured before it follow it; the counts stay. */
typedef struct bitnet_hip_sampling_config_ex {
    bitnet_hip_sampling_config base;
    float min_p;              /* <= 0: off */
    float typical_p;          /* >= 1: off */
    float frequency_penalty;  /* 0: off */
    float presence_penalty;   /* 0: off */
} bitnet_hip_sampling_config_ex;
int bitnet_hip_sampler_create_ex(size_t vocab, const bitnet_hip_sampling_config_ex *cfg, bitnet_hip_sampler **out);
int bitnet_hip_sampler_configure_ex(bitnet_hip_sampler *sampler, const bitnet_hip_sampling_config_ex *cfg);
/* Mirostat v2 (crates/bitnet-sampling/src/strategies.rs MirostatSampler :109-196, `sample` :131-190): a mode of the sampler that takes
 * the place of the truncation stages.  Order: counts; additive penalties; repetition penalty; NaN -> -inf; temperature (division);
 * MIROSTAT.  There is no greedy shortcut: temperature 1 / top_k 0 / top_p 1 runs Mirostat.  On that row, with state mu (2 * tau at first):
 *   p = softmax_in_place(x) (crates/bitnet-logits/src/lib.rs:180-213; a row with no finite maximum is uniform over all n ids); an entry with
 *   p_i > 0 and -ln p_i > mu is removed; if nothing is left the FALLBACK runs: no random word, the token is the argmax of the row, the
 *   HIGHEST index on ties (the reference's max_by keeps the last), surprise = -ln p_token of the unfiltered p; otherwise q = the rest
 *   renormalised, u = the next word of the sampler's ChaCha20 stream as (w >> 8) * 2^-24 (the reference's type is ChaCha8Rng; the library keeps
 *   its one stream, as the chain stages did), the token is the first id, ascending, with u <= the running sum (vocab - 1 if none), and
 *   surprise = -ln q_token, or tau if q_token is 0.  Then mu -= eta * (surprise - tau), two f32 operations, in device memory.
 * One launch, as every other path: the slice pass of the full-vocabulary path, then three passes of the finishing workgroup.  The filter is
 * g_i > mu - ln S with g_i = max - x_i, no logarithm per entry; sums are fixed-point, so repeated launches and bitnet_hip_sample_batch_dev
 * give the same bits.  Equal to the reference except where a comparison lies within the roundings listed in csrc/kernels_sample.hip.
 * A forced position moves nothing, mu included.  bitnet_hip_sample_host runs the same path on its own counts and shares mu and the stream.
 * set_mirostat: cfg == NULL: off.  Else on: tau, eta stored, mu = 2 * tau (MirostatSampler::new :120-126), fallback count 0.  Synchronous and
 *   not capture-safe; graphs captured before it stay valid and follow it (the mode is read from device memory, like the config).
 *   Invalid, with nothing changed: tau NaN, infinite or <= 0; eta NaN, infinite or negative (both refused before the sampler is looked at);
 *   a sampler whose current config has top_k != 0, top_p < 1, min_p > 0, typical_p < 1 or temperature == 0.  While Mirostat is on,
 *   bitnet_hip_sampler_configure[_ex] refuses exactly those configs in the same way; a config it takes leaves mu alone.
 * mirostat_state: mu and the number of fallback calls since set_mirostat / reset (either pointer may be NULL).  Synchronous. */
typedef struct bitnet_hip_mirostat_config { float tau; float eta; } bitnet_hip_mirostat_config;
int bitnet_hip_sampler_set_mirostat(bitnet_hip_sampler *sampler, const bitnet_hip_mirostat_config *cfg);
int bitnet_hip_sampler_mirostat_state(bitnet_hip_sampler *sampler, float *mu, uint64_t *fallbacks);
/* Logit constraints: a per-token logit_bias (the reference's llama-compatible front end takes one, crates/bitnet-py/src/llama_compat.py:128,
 * 161,207), banned tokens, an allowed set, an EOS hold-off (min_tokens) and no_repeat_ngram_size -- element-wise edits of the row in front of
 * everything else the sampler does, inside the same single launch.  A stage CONSTRAINTS directly behind "counts":
 *   counts; CONSTRAINTS; additive penalties; repetition penalty; NaN -> -inf; then the rest of the chain, or Mirostat, unchanged.
 * For entry i with raw logit x:
 *   bias: x = x + b[i], one f32 addition; b is 0 except at bias_ids, where it is the value of the LAST entry that names the id; -inf bans.
 *   ban:  x = -inf if i is not in a non-empty allowed list, or i is a hold id and g < min_tokens, or i is n-gram-blocked.  A ban always wins:
 *     a +inf logit with a -inf bias is NaN, and NaN -> -inf catches it.
 *   g: the tokens this sampler has chosen, in launches that ran with constraints on, since bitnet_hip_sampler_reset -- a word in device
 *     memory, advanced by the launch.  A forced position (and so a step frozen by the stop criteria) chooses nothing and does not count.
 *     reset zeroes it; configure[_ex], set_mirostat and set_constraints leave it alone.  Launches with constraints off do not count (they run
 *     the bodies that have no such stage): switch constraints on before the first token, with an empty config if need be.
 *   n-gram block: n = no_repeat_ngram, P = *pos_dev, h = history_dev.  For every j with j + n - 1 <= P and h[j .. j+n-2] == h[P-n+2 .. P],
 *     token h[j+n-1] is banned.  n = 1 bans every token of h[0..P]; a history of fewer than n tokens bans nothing.  Prompt tokens take part.
 *     A token id outside [0, vocab) is skipped.  Without pos_dev / history_dev the block is skipped.  Only h[0..P] is read.
 * bitnet_hip_sample_host applies the same stage with g = n_generated and that call's list as the sequence.  A row on which everything is
 * banned behaves as a row of -inf logits does on the path at hand.  bitnet_hip_sample_batch_dev shares the kernel body: per slot the result
 * is bit for bit bitnet_hip_sample_dev's.
 * The logits tap (bitnet_hip_logprob_*) keeps reading the RAW row: its log-probabilities are those of the unconstrained distribution.
 * set_constraints: cfg == NULL: off.  The lists are copied; the caller's arrays are not kept.  Synchronous and not capture-safe; graphs
 *   captured before it stay valid and follow it (bias, bans and the hold list are reached through device memory).  INVALID_ARGUMENT, with
 *   nothing changed, and before the sampler pointer is looked at: a NULL list with a non-zero count; an id outside [0, vocab) (without a
 *   sampler: outside [0, 2^20)); a bias value that is NaN or +inf; n_hold > BITNET_HIP_CONSTRAINT_MAX_HOLD; min_tokens < 0; no_repeat_ngram
 *   outside 0..BITNET_HIP_CONSTRAINT_MAX_NGRAM.
 * constraints_state: g.  Synchronous. */
#define BITNET_HIP_CONSTRAINT_MAX_HOLD 32
#define BITNET_HIP_CONSTRAINT_MAX_NGRAM 8
typedef struct bitnet_hip_constraints {
    const int32_t *bias_ids; const float *bias_values; size_t n_bias;  /* x += value; -inf = banned */
    const int32_t *allowed_ids; size_t n_allowed;   /* n_allowed > 0: every id NOT listed is banned */
    const int32_t *hold_ids; size_t n_hold;         /* banned while fewer than min_tokens tokens were chosen */
    int32_t min_tokens;                             /* 0: no hold-off */
    int32_t no_repeat_ngram;                        /* 0 off; 1..BITNET_HIP_CONSTRAINT_MAX_NGRAM */
} bitnet_hip_constraints;
int bitnet_hip_sampler_set_constraints(bitnet_hip_sampler *sampler, const bitnet_hip_constraints *cfg);
int bitnet_hip_sampler_constraints_state(bitnet_hip_sampler *sampler, uint64_t *chosen);
/* Grammar-constrained decoding (a token automaton whose state moves with every chosen token; bitnet_hip_grammar_*, bitnet_hip_sampler_set_grammar,
 * _set_grammar_state, _grammar_state): declared in bitnet_hip_grammar.h, included at the end of this header. */
/* Clears the counts (a new generation), the word counter and the constraints' count of chosen tokens, and re-arms the launch hand-over (a
 * launch cut short leaves it unbalanced).  With Mirostat on: mu = 2 * tau (MirostatSampler::reset, strategies.rs:192-195) and the fallback count 0.
 * With a grammar bound: the state word goes back to the bound start state, steps and violations to 0.
 * Synchronous; call it with no sample_dev / sample_host in flight.  Not capture-safe. */
int bitnet_hip_sampler_reset(bitnet_hip_sampler *sampler);
/* ChaCha20 words consumed since create / configure / reset (one per non-greedy call; none for a call that took Mirostat's fallback).
 * Synchronous; not capture-safe. */
int bitnet_hip_sampler_draws(bitnet_hip_sampler *sampler, uint64_t *draws);
/* One sampling step on the device, capture-safe (one kernel, no host work).  "Generated" = the tokens this sampler
 * chose since the last reset: the exponent of token t at call c is sum_{i<c, g_i = t} (c - i), the reference's count when
 * its caller passes the growing list each step.  token_dev (nullable) receives the token; pos / history / n_forced as
 * bitnet_hip_logits_f16_dev: with p = *pos_dev, history_dev[p+1] = token, then *pos_dev = p+1.  At a forced position
 * (p+1 < *n_forced_dev: a prompt token sits there) nothing is sampled or counted, token_dev receives the prompt token. */
int bitnet_hip_sample_dev(bitnet_hip_sampler *sampler, const float *logits_dev, size_t vocab, int32_t *token_dev,
                          int32_t *pos_dev, int32_t *history_dev, const int32_t *n_forced_dev, void *stream);
/* Drop-in of Sampler::sample(&logits, &generated_tokens) with host pointers: the whole generated list on every call,
 * counted as the reference counts it (ids >= vocab are skipped).  Synchronous; not capture-safe.  Keeps its counts
 * apart from those of bitnet_hip_sample_dev; both share the RNG stream. */
int bitnet_hip_sample_host(bitnet_hip_sampler *sampler, const float *logits, size_t vocab, const uint32_t *generated,
                           size_t n_generated, uint32_t *token);

/* ---- batched sampling: every sampling member of a batch in one launch -------------------------------------------
 * The reference's `Sampler::sample` (crates/bitnet-cli/src/sampling.rs) called once per sequence of a `[B, T, H]` batch: here a
 * table of n_slots = 1..BITNET_HIP_BATCH_MAX entries, each binding one bitnet_hip_sampler and the pointers bitnet_hip_sample_dev
 * would take, and ONE kernel launch that serves every bound entry -- grid (workgroups per sampler, n_slots), the entries read from
 * device memory, so a captured graph follows every later bitnet_hip_sample_batch_set.  Per bound slot the token, the history
 * entry, the position, the forced-position rule, the counts, the ChaCha20 word counter and the re-armed hand-over are bit for bit
 * what bitnet_hip_sample_dev on that sampler alone would have left (one kernel body serves both); for an empty slot nothing is read
 * or written.  No workgroup waits for another: the slots finish side by side.
 *   create: vocab in 1..2^20 (every sampler bound later must be made for it), n_slots in 1..BITNET_HIP_BATCH_MAX; anything else is
 *     INVALID_ARGUMENT before the GPU is touched.  Allocates the device table, every entry empty.  Not capture-safe.
 *   set: binds `sampler` and its pointers to `slot`; sampler == NULL empties the slot.  One synchronous copy of one entry: not
 *     capture-safe, but graphs captured before it stay valid and follow it.  Call it with no launch on the table in flight.  Refuses,
 *     with nothing changed: a slot out of range, a NULL logits_dev with a sampler, a sampler made for another vocabulary, a sampler
 *     already bound to another slot of this table.  A sampler serves one table or bitnet_hip_sample_dev at a time; empty its slot
 *     before bitnet_hip_sampler_destroy.
 *   dev: exactly one kernel launch, asynchronous and capture-safe (no allocation, copy or synchronisation); it launches even when
 *     every slot is empty.  A NULL table is INVALID_ARGUMENT. */
typedef struct bitnet_hip_sample_batch bitnet_hip_sample_batch;
int bitnet_hip_sample_batch_create(size_t vocab, size_t n_slots, bitnet_hip_sample_batch **out);
void bitnet_hip_sample_batch_destroy(bitnet_hip_sample_batch *table);
int bitnet_hip_sample_batch_set(bitnet_hip_sample_batch *table, size_t slot, bitnet_hip_sampler *sampler, const float *logits_dev,
                                int32_t *token_dev, int32_t *pos_dev, int32_t *history_dev, const int32_t *n_forced_dev);
int bitnet_hip_sample_batch_dev(bitnet_hip_sample_batch *table, void *stream);

/* ---- per-token log-probabilities and top-N logits: the generation path's logits tap -------------------------------
 * The reference's GenerationConfig::{logits_tap_steps, logits_topk, logits_cb} (crates/bitnet-inference/src/config.rs:87-93), called after
 * sampling with (step, topk [(id, raw logit)], chosen) (crates/bitnet-inference/src/engine.rs:1182-1210), and the CLI's
 * --dump-logit-steps N --logits-topk K `LogitStep` records (crates/bitnet-cli/src/main.rs:1337-1373) -- on the device, after the pick, with
 * no host round trip per token.  One launch AFTER bitnet_hip_logits_f16_dev's greedy pick or bitnet_hip_sample_dev: by then *pos_dev is
 * p + 1 and history_dev[p + 1] holds the chosen (or forced) token.  With q = *pos_dev and t = history_dev[q] the launch writes
 * records_dev[q] when 0 <= q < capacity, and nothing otherwise (its hand-over is re-armed either way).  l = logits_dev, the raw f32 row
 * the sampler reads: no penalty, no temperature (the reference passes &logits to its tap).
 *   top list: the CLI's rule (main.rs:1344-1350): finite entries first, by descending logit (-0.0 == +0.0), then ascending id; every
 *     non-finite entry (NaN, +inf, -inf) after every finite one, by ascending id.  Comparisons only: the list is exact.  Entries
 *     j >= n_top of the record keep their bytes.
 *   lse: M = max_i l_i with NaN read as -inf; lse = M + log(sum_i exp(l_i - M)); +inf if M is +inf, -inf if M is -inf.  Deterministic:
 *     per-workgroup (max, sum) partials are merged in workgroup-index order, and the partition depends on vocab alone, so repeated
 *     launches and the two entry points give the same bits.
 *   log-probability of the token: logit - lse, formed by the host in f32.
 * scratch_dev: bitnet_hip_logprob_scratch_bytes(vocab) bytes (0 for a vocabulary this library refuses: 0 or > 2^20), this entry's own,
 * 16-byte aligned, zeroed once by the caller; history_dev holds at least `capacity` entries.
 * bitnet_hip_logprob_dev: one sequence, args on the host.  bitnet_hip_logprob_batch_dev: n_slots = 1..BITNET_HIP_BATCH_MAX entries read from
 * a DEVICE table by the kernel (a captured graph follows later writes to it); an entry with records_dev == NULL is empty: nothing is read
 * or written for it; top_n beyond the maximum is clamped.  Per bound slot the record and the re-armed scratch are bit for bit what
 * bitnet_hip_logprob_dev on that entry alone leaves (one kernel body serves both).  Both are exactly one kernel launch, asynchronous and
 * capture-safe (no allocation, copy or synchronisation); the batched entry launches even when every entry is empty.  INVALID_ARGUMENT
 * before anything launches and before the GPU is touched: NULL args_host / table_dev; vocab 0 or > 2^20; n_slots outside
 * 1..BITNET_HIP_BATCH_MAX; for bitnet_hip_logprob_dev top_n > BITNET_HIP_LOGPROB_TOP_MAX, or a NULL logits_dev, pos_dev, history_dev or
 * scratch_dev together with a non-NULL records_dev. */
#define BITNET_HIP_LOGPROB_TOP_MAX 20
typedef struct bitnet_hip_logprob_record {
    int32_t token;      /* history[q]; -1 = never written (records are cleared to 0xFF bytes) */
    int32_t n_top;      /* min(top_n, vocab) */
    float   logit;      /* raw l[token], NaN read as -inf; NaN if token is outside [0, vocab) */
    float   lse;        /* log sum_i exp(l_i), NaN read as -inf */
    int32_t top_id[BITNET_HIP_LOGPROB_TOP_MAX];
    float   top_logit[BITNET_HIP_LOGPROB_TOP_MAX];   /* raw bits of l[top_id[j]] */
} bitnet_hip_logprob_record;
typedef struct bitnet_hip_logprob_args {
    const float *logits_dev; const int32_t *pos_dev; const int32_t *history_dev;
    bitnet_hip_logprob_record *records_dev;   /* NULL: empty entry */
    void *scratch_dev;                        /* bitnet_hip_logprob_scratch_bytes(vocab), this entry's own, zeroed once by the caller */
    uint32_t capacity, top_n;                 /* records in records_dev; 0..BITNET_HIP_LOGPROB_TOP_MAX */
} bitnet_hip_logprob_args;
size_t bitnet_hip_logprob_scratch_bytes(size_t vocab);
int bitnet_hip_logprob_dev(const bitnet_hip_logprob_args *args_host, size_t vocab, void *stream);
int bitnet_hip_logprob_batch_dev(const bitnet_hip_logprob_args *table_dev, size_t n_slots, size_t vocab, void *stream);

/* ---- stop criteria on the device: stop token ids, EOS, a token budget, stop sequences of token ids -----------------
 * The reference's StopCriteria / StopReason / check_stop (crates/bitnet-generation/src/lib.rs:119-144), InferenceEngine::should_stop
 * (crates/bitnet-inference/src/engine.rs:1315-1348) and GenerationConfig's stop fields (crates/bitnet-inference/src/config.rs:67-85) as
 * ONE small launch behind the pick (bitnet_hip_logits_f16_dev's greedy pick, bitnet_hip_sample_dev, and the logits tap if there is one),
 * inside a captured step: it decides whether the token just placed ends the sequence, and from then on keeps the sequence FROZEN through
 * every step that is already queued, so a host can queue a chunk of steps and read the state once.
 * With P = *pos_dev after the pick and t = history_dev[P], one launch does exactly one of:
 *   ALREADY STOPPED: *pos_dev = the stop position, *token_dev = the stop token, frozen_steps += 1; nothing else.
 *   NOT STOPPED and P < *n_forced_dev (a prompt token), or P outside [1, capacity): nothing.  Prompt tokens never stop a sequence and are
 *     never counted.  (A forced position does not clear the window either: a caller that feeds tokens into a running generation arms again,
 *     as bitnet_host's feed does.)
 *   OTHERWISE: generated += 1, window += 1, then the first condition that holds, in check_stop's order, sets the reason:
 *     1. t is one of stop_ids: BITNET_HIP_STOP_TOKEN, index = the lowest matching entry (so an id that is also eos_id reports here);
 *     2. t == eos_id: BITNET_HIP_STOP_EOS;
 *     3. max_tokens > 0 and generated >= max_tokens: BITNET_HIP_STOP_MAX_TOKENS.  The current token counts: a budget of n yields n tokens,
 *        the n-th being the stop token.  The reference's callers differ here -- check_stop compares the length of the list its caller
 *        hands it, which some callers extend before the call and some after; the engine's own loop bounds its step count instead;
 *     4. some sequence s of length L <= window with history_dev[P - L + 1 .. P] == s: BITNET_HIP_STOP_SEQUENCE, index = the LOWEST such s,
 *        not the longest.  window counts the tokens counted since the last arm, so a match never reaches back into prompt tokens or across
 *        an arm.
 *     On a stop: reason, index, token = t, position = P, generated are recorded, frozen_steps = 0, 0x7fffffff is stored to *n_forced_dev
 *     -- every later pick then treats its position as forced: it writes no history entry, and the sampler samples nothing, counts
 *     nothing, draws no word and leaves Mirostat's mu alone -- and the table's live count, if a table holds the object, goes down by one.
 * The freeze: a frozen step starts at the stop position again, consumes the stop token there and rewrites that one cache slot with the
 * same bytes; history entries and cache slots beyond the stop position keep whatever they held.  Every history index is checked against
 * `capacity` before it is read: a garbage position is a no-op, never a fault.  Stop strings stay with the owner of the tokenizer: the
 * device takes token-id sequences, and a string that spans a token boundary differently from its own tokenisation needs the host's check.
 *   create: validates the config, allocates the device state (armed, nothing counted).  Not capture-safe.
 *   configure: a new config, the state untouched.  Synchronous; graphs captured earlier stay valid and follow it (the config is read from
 *     device memory).
 *   arm(stop, keep_generated): reason, index, token, position, frozen_steps and window = 0; generated = 0 unless keep_generated.  It does
 *     NOT touch *n_forced_dev, which is the caller's word: a caller that goes on after a stop writes its own forced count back.
 *     Synchronous; no launch on the object in flight.
 *   get_state: synchronous read-back, no launch on the object in flight.
 *   stop_dev: exactly one launch, asynchronous and capture-safe.  token_dev may be NULL.
 *   batch_create / _destroy / _set: a device table of n_slots = 1..BITNET_HIP_STOP_BATCH_MAX entries, each binding one bitnet_hip_stop and
 *     the pointers stop_dev would take; stop == NULL empties the slot.  set is one synchronous copy of one entry: graphs captured before it
 *     stay valid and follow it.  An object serves one table slot or stop_dev at a time; destroying it empties its slot.
 *   batch_dev: exactly one launch, one wave per slot, even when every slot is empty; per bound slot it leaves, bit for bit, what stop_dev on
 *     that object alone leaves (one kernel body serves both).
 *   batch_live: synchronous count of bound slots that have not stopped (kept on the device by the launches, recounted by set and arm).
 * INVALID_ARGUMENT before the GPU is touched: a NULL config or output pointer; n_stop_ids > BITNET_HIP_STOP_MAX_IDS; n_seqs >
 * BITNET_HIP_STOP_MAX_SEQS; a sequence of length 0 or above BITNET_HIP_STOP_MAX_SEQ_LEN; a negative id in either list; a NULL list with a
 * non-zero count; eos_id < -1; max_tokens < 0; a table slot out of range; an object already bound to another slot; NULL pos_dev, history_dev
 * or n_forced_dev; capacity 0 or above 2^31 - 1.  An empty config is valid: it counts tokens and never stops. */
#define BITNET_HIP_STOP_MAX_IDS 32
#define BITNET_HIP_STOP_MAX_SEQS 16
#define BITNET_HIP_STOP_MAX_SEQ_LEN 32
#define BITNET_HIP_STOP_BATCH_MAX 64
#define BITNET_HIP_STOP_NONE 0
#define BITNET_HIP_STOP_TOKEN 1        /* StopReason::StopTokenId(stop_ids[index]) */
#define BITNET_HIP_STOP_EOS 2          /* StopReason::EosToken */
#define BITNET_HIP_STOP_MAX_TOKENS 3   /* StopReason::MaxTokens */
#define BITNET_HIP_STOP_SEQUENCE 4     /* StopReason::StopString, as the token ids of sequence `index` */
typedef struct bitnet_hip_stop_config {
    const int32_t *stop_ids; size_t n_stop_ids;   /* StopCriteria::stop_token_ids */
    int32_t eos_id;                               /* StopCriteria::eos_token_id; -1: none */
    int32_t max_tokens;                           /* StopCriteria::max_tokens; 0: none */
    const int32_t *seq_tokens;                    /* the sequences' token ids, concatenated */
    const int32_t *seq_len;                       /* [n_seqs], each 1..BITNET_HIP_STOP_MAX_SEQ_LEN */
    size_t n_seqs;
} bitnet_hip_stop_config;
typedef struct bitnet_hip_stop_state {
    int32_t reason;        /* BITNET_HIP_STOP_*; NONE: still running */
    int32_t index;         /* of the stop id or sequence that matched */
    int32_t token;         /* the stop token */
    int32_t position;      /* its history slot */
    int32_t generated;     /* tokens counted (since the last arm that did not keep the count), the stop token included */
    int32_t frozen_steps;  /* launches since the stop: the steps that were queued for nothing */
} bitnet_hip_stop_state;
typedef struct bitnet_hip_stop bitnet_hip_stop;
typedef struct bitnet_hip_stop_batch bitnet_hip_stop_batch;
int bitnet_hip_stop_create(const bitnet_hip_stop_config *cfg, bitnet_hip_stop **out);
void bitnet_hip_stop_destroy(bitnet_hip_stop *stop);
int bitnet_hip_stop_configure(bitnet_hip_stop *stop, const bitnet_hip_stop_config *cfg);
int bitnet_hip_stop_arm(bitnet_hip_stop *stop, int keep_generated);
int bitnet_hip_stop_get_state(bitnet_hip_stop *stop, bitnet_hip_stop_state *out);
int bitnet_hip_stop_dev(bitnet_hip_stop *stop, int32_t *pos_dev, const int32_t *history_dev, size_t capacity, int32_t *n_forced_dev,
                        int32_t *token_dev, void *stream);
int bitnet_hip_stop_batch_create(size_t n_slots, bitnet_hip_stop_batch **out);
void bitnet_hip_stop_batch_destroy(bitnet_hip_stop_batch *table);
int bitnet_hip_stop_batch_set(bitnet_hip_stop_batch *table, size_t slot, bitnet_hip_stop *stop, int32_t *pos_dev, const int32_t *history_dev,
                              size_t capacity, int32_t *n_forced_dev, int32_t *token_dev);
int bitnet_hip_stop_batch_dev(bitnet_hip_stop_batch *table, void *stream);
int bitnet_hip_stop_batch_live(bitnet_hip_stop_batch *table, int32_t *live);

/* ---- measurement aid -------------------------------------------------------
 * Measured HBM read ceiling of the device (quote the roofline fraction against the vendor
 * figure AND a measured stream ceiling): a read-only streaming kernel (non-temporal 16-byte loads, one
 * workgroup round per 2 MiB) over `bytes` of freshly written device memory (bytes >= 1 GiB keeps L2 and
 * the 256 MB MALL out of it), `iters` timed passes with HIP events on the given stream.  Writes the
 * best pass in GB/s (1e9 B/s) to *best_gbs and the mean to *mean_gbs.  Allocates and frees its buffer. */
int bitnet_hip_hbm_read_ceiling(size_t bytes, int iters, double *best_gbs, double *mean_gbs, void *stream);

#ifdef __cplusplus
}
#endif

#include "bitnet_hip_grammar.h" /* the sampler's grammar stage: six more entry points of this ABI */
#include "bitnet_hip_kvsnap.h"  /* compact KV snapshots: three more */
#include "bitnet_hip_widetail.h" /* the wide step's tail: the sampler and tap tables at 64 entries, two more */
#include "bitnet_hip_beam.h"    /* beam search: the select launch, the in-place KV permute and their state object, seven more */

#endif /* BITNET_HIP_H */
