"""bitnet-rs_amd -- MI355X (gfx950) drop-in for the BitNet-rs I2_S / QK256 hot path.

The product is libbitnet_hip.so (hand-written HIP behind the C ABI in
include/bitnet_hip.h).  This module is the thin ctypes binding the tests and
bench.py drive it through; it contains no arithmetic and NO fallback: if the
library is missing or there is no GPU, calls raise.

The directory name carries a hyphen (as the project is named), so import it with
    importlib.import_module("bitnet-rs_amd")
"""
from __future__ import annotations

import collections
import ctypes as C
import importlib.util
import os
import sys
import time

import numpy as np

from . import cproto

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libbitnet_hip.so")
HEADER_PATH = os.path.join(ROOT, "include", "bitnet_hip.h")
GRAMMAR_HEADER_PATH = os.path.join(ROOT, "include", "bitnet_hip_grammar.h")  # included by HEADER_PATH: the grammar stage's six entry points
KVSNAP_HEADER_PATH = os.path.join(ROOT, "include", "bitnet_hip_kvsnap.h")  # included by HEADER_PATH: the KV snapshot's three entry points
BEAM_HEADER_PATH = os.path.join(ROOT, "include", "bitnet_hip_beam.h")  # included by HEADER_PATH: beam search, the select and permute launches and their state
WIDETAIL_HEADER_PATH = os.path.join(ROOT, "include", "bitnet_hip_widetail.h")  # included by HEADER_PATH: the wide step's 64-entry tail tables, two

OK = 0
ERR_INVALID_ARGUMENT, ERR_GPU, ERR_UNSUPPORTED, ERR_EXECUTION = -1, -2, -3, -4
KERNEL_AUTO, KERNEL_EXACT, KERNEL_VALU, KERNEL_MFMA, KERNEL_MFMA_TILED = 0, 1, 2, 3, 4
QTYPE_I2S, QTYPE_TL1, QTYPE_TL2 = 0, 1, 2

_u8p = C.POINTER(C.c_uint8)
_i8p = C.POINTER(C.c_int8)
_f32p = C.POINTER(C.c_float)
_sz = C.c_size_t
_vp = C.c_void_p


class BitNetHipError(RuntimeError):
    """Mirrors BitNetError::Kernel(KernelError::*) (crates/bitnet-common/src/error.rs:80-97)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code
        self.kind = {
            ERR_INVALID_ARGUMENT: "InvalidArguments",
            ERR_GPU: "GpuError",
            ERR_UNSUPPORTED: "UnsupportedHardware",
            ERR_EXECUTION: "ExecutionFailed",
        }.get(code, "ExecutionFailed")


def _load_build_module():
    spec = importlib.util.spec_from_file_location("_bitnet_hip_build", os.path.join(HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into libbitnet_hip.so (in-tree)."""
    return _load_build_module().build(force=force, verbose=verbose)


class DeviceInfo(C.Structure):
    _fields_ = [
        ("device_id", C.c_int32),
        ("name", C.c_char * 128),
        ("gcn_arch", C.c_char * 64),
        ("total_memory", C.c_uint64),
        ("compute_unit_count", C.c_int32),
        ("max_wavefront_size", C.c_int32),
        ("max_shared_memory_per_workgroup", C.c_uint64),
        ("supports_fp16", C.c_int32),
        ("supports_bf16", C.c_int32),
    ]


class GemvQGeometry(C.Structure):
    """bitnet_hip_gemv_q_geometry_t"""
    _fields_ = [(n, C.c_int) for n in ("k_split", "blocks", "blocks_per_wave", "ring", "copy_passes", "scale_form", "layernorm", "tiles_per_workgroup",
                                       "grid", "merge_slots4", "merge_slots1", "merge_records")]


class GemvGeometry(C.Structure):
    """bitnet_hip_gemv_geometry_t"""
    _fields_ = [(n, C.c_int) for n in ("kernel", "unfused", "k_split", "blocks", "blocks_per_wave", "ring", "stat_vectors", "layernorm", "scale_form",
                                       "wscale", "merge", "tiles_per_workgroup", "grid", "lds_bytes", "lds_raised")]


def _np(a, dtype):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(t):
    """Device pointer of a torch tensor (or a raw int)."""
    return _vp(t if isinstance(t, int) else t.data_ptr())


def _optr(t):
    """Nullable device pointer."""
    return None if t is None else _ptr(t)


class HipLib:
    """ctypes view of libbitnet_hip.so.  One method per exported symbol."""

    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: build it with __graft_entry__.build() -- there is no fallback path"
            )
        self.path = path
        self.c = C.CDLL(path)
        cproto.bind(self.c, cproto.prototypes(open(HEADER_PATH).read(), "bitnet_hip_"), C_STRUCTS)
        cproto.bind(self.c, grammar_prototypes(), C_STRUCTS)
        cproto.bind(self.c, kvsnap_prototypes(), C_STRUCTS)
        cproto.bind(self.c, widetail_prototypes(), C_STRUCTS)
        cproto.bind(self.c, beam_prototypes(), C_STRUCTS)

    # -- helpers ---------------------------------------------------------
    def last_error(self) -> str:
        e = self.c.bitnet_hip_get_last_error()
        return e.decode() if e else ""

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BitNetHipError(rc, self.last_error() or f"bitnet_hip rc={rc}")

    # -- lifecycle -------------------------------------------------------
    def init(self, device: int = -1) -> None:
        self._check(self.c.bitnet_hip_init(device))

    def cleanup(self) -> None:
        self.c.bitnet_hip_cleanup()

    def is_available(self) -> bool:
        return bool(self.c.bitnet_hip_is_available())

    def device_count(self) -> int:
        return int(self.c.bitnet_hip_device_count())

    def device_info(self, device: int = 0) -> DeviceInfo:
        info = DeviceInfo()
        self._check(self.c.bitnet_hip_get_device_info(device, C.byref(info)))
        return info

    def set_kernel(self, kernel: int) -> None:
        self._check(self.c.bitnet_hip_set_kernel(kernel))

    def get_kernel(self) -> int:
        return int(self.c.bitnet_hip_get_kernel())

    # -- host-pointer drop-ins --------------------------------------------
    def gemv_qk256(self, qs, x, rows, cols, row_stride_bytes, y_len=None) -> np.ndarray:
        q, xa = _np(qs, np.uint8), _np(x, np.float32)
        y = np.zeros(rows if y_len is None else y_len, np.float32)
        self._check(
            self.c.bitnet_hip_gemv_qk256(
                q.ctypes.data_as(_u8p), q.size, xa.ctypes.data_as(_f32p), xa.size, y.ctypes.data_as(_f32p), y.size,
                rows, cols, row_stride_bytes,
            )
        )
        return y

    def i2s_matmul_f32(self, act, w, scales, m, n, k, block_size, out_len=None) -> np.ndarray:
        a, wq, s = _np(act, np.float32), _np(w, np.uint8), _np(scales, np.float32)
        out = np.zeros(m * n if out_len is None else out_len, np.float32)
        self._check(
            self.c.bitnet_hip_i2s_matmul_f32(
                a.ctypes.data_as(_f32p), a.size, wq.ctypes.data_as(_u8p), wq.size, s.ctypes.data_as(_f32p), s.size,
                out.ctypes.data_as(_f32p), out.size, m, n, k, block_size,
            )
        )
        return out

    def qk256_gemv(self, weights, scales, inp, m, n, k) -> np.ndarray:
        wq, s, a = _np(weights, np.uint8), _np(scales, np.float32), _np(inp, np.float32)
        out = np.zeros(m * n, np.float32)
        self._check(
            self.c.bitnet_hip_qk256_gemv(
                wq.ctypes.data_as(_u8p), wq.size, s.ctypes.data_as(_f32p), s.size, a.ctypes.data_as(_f32p), a.size,
                out.ctypes.data_as(_f32p), out.size, m, n, k,
            )
        )
        return out

    def matmul_i2s(self, a, b, m, n, k, c_len=None) -> np.ndarray:
        aa, bb = _np(a, np.int8), _np(b, np.uint8)
        c = np.zeros(m * n if c_len is None else c_len, np.float32)
        self._check(
            self.c.bitnet_hip_matmul_i2s(
                aa.ctypes.data_as(_i8p), aa.size, bb.ctypes.data_as(_u8p), bb.size, c.ctypes.data_as(_f32p), c.size, m, n, k
            )
        )
        return c

    def quantized_matmul_i2s(self, x, packed, scales, block_size: int, m: int, n: int, k: int) -> np.ndarray:
        xa, pa, sa = _np(x, np.float32), _np(packed, np.uint8), _np(scales, np.float32)
        out = np.zeros(m * n, np.float32)
        self._check(self.c.bitnet_hip_quantized_matmul_i2s(xa.ctypes.data_as(_f32p), xa.size, pa.ctypes.data_as(_u8p), pa.size, sa.ctypes.data_as(_f32p), sa.size,
                                                           block_size, out.ctypes.data_as(_f32p), out.size, m, n, k))
        return out

    def quantize(self, x, qtype=QTYPE_I2S, out_len=None, scales_len=None, out_init=None):
        xa = _np(x, np.float32)
        out = np.zeros(xa.size // 4 if out_len is None else out_len, np.uint8) if out_init is None else _np(out_init, np.uint8).copy()
        scales = np.zeros((xa.size + 31) // 32 if scales_len is None else scales_len, np.float32)
        self._check(
            self.c.bitnet_hip_quantize(
                xa.ctypes.data_as(_f32p), xa.size, out.ctypes.data_as(_u8p), out.size, scales.ctypes.data_as(_f32p), scales.size, qtype
            )
        )
        return out, scales

    def dequant_i2s(self, data, rows, cols, inv=False, k=1.0, transposed=False) -> np.ndarray:
        d = _np(data, np.uint8)
        out = np.zeros(rows * cols, np.float32)
        self._check(
            self.c.bitnet_hip_dequant_i2s(d.ctypes.data_as(_u8p), d.size, rows, cols, int(inv), k, int(transposed), out.ctypes.data_as(_f32p), out.size)
        )
        return out

    def attention(self, q, k, v, seq_len: int, num_heads: int, head_dim: int, causal: bool = True, scale: float | None = None) -> np.ndarray:
        qa, ka, va = _np(q, np.float32).reshape(-1), _np(k, np.float32).reshape(-1), _np(v, np.float32).reshape(-1)
        out = np.zeros(qa.size, np.float32)
        sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(head_dim))
        self._check(self.c.bitnet_hip_attention(qa.ctypes.data_as(_f32p), qa.size, ka.ctypes.data_as(_f32p), ka.size, va.ctypes.data_as(_f32p), va.size,
                                                out.ctypes.data_as(_f32p), out.size, seq_len, num_heads, head_dim, int(causal), sc))
        return out

    def qk256_gemv_batch(self, items) -> list:
        """items: (weights u8, scales f32, input f32, m, n, k) tuples -> list of outputs [m*n]."""
        class Item(C.Structure):
            _fields_ = [("weights", _u8p), ("weights_len", _sz), ("scales", _f32p), ("scales_len", _sz), ("input", _f32p), ("input_len", _sz),
                        ("output", _f32p), ("output_len", _sz), ("m", _sz), ("n", _sz), ("k", _sz)]
        keep, arr = [], (Item * len(items))()
        for i, (w, s, x, m, n, k) in enumerate(items):
            wa, sa, xa, ya = _np(w, np.uint8), _np(s, np.float32), _np(x, np.float32), np.zeros(m * n, np.float32)
            keep.append((wa, sa, xa, ya))
            arr[i] = Item(wa.ctypes.data_as(_u8p), wa.size, sa.ctypes.data_as(_f32p), sa.size, xa.ctypes.data_as(_f32p), xa.size,
                          ya.ctypes.data_as(_f32p), ya.size, m, n, k)
        self._check(self.c.bitnet_hip_qk256_gemv_batch(C.cast(arr, C.c_void_p), len(items)))
        return [kp[3] for kp in keep]

    # -- device-resident API ------------------------------------------------
    def weights_upload_qk256(self, qs, rows, cols, row_stride_bytes) -> int:
        q = _np(qs, np.uint8)
        h = C.c_uint64(0)
        self._check(self.c.bitnet_hip_weights_upload_qk256(q.ctypes.data_as(_u8p), q.size, rows, cols, row_stride_bytes, C.byref(h)))
        return h.value

    def weights_upload_i2s(self, w, scales, n, k, block_size) -> int:
        wq, s = _np(w, np.uint8), _np(scales, np.float32)
        h = C.c_uint64(0)
        self._check(self.c.bitnet_hip_weights_upload_i2s(wq.ctypes.data_as(_u8p), wq.size, s.ctypes.data_as(_f32p), s.size, n, k, block_size, C.byref(h)))
        return h.value

    def weights_upload_coded(self, w, scales, n, k, block_size, code_map) -> int:
        wq, s, cm = _np(w, np.uint8), _np(scales, np.float32), _np(code_map, np.int8)
        h = C.c_uint64(0)
        self._check(self.c.bitnet_hip_weights_upload_coded(wq.ctypes.data_as(_u8p), wq.size, s.ctypes.data_as(_f32p), s.size, n, k, block_size, cm.ctypes.data_as(_i8p), C.byref(h)))
        return h.value

    def weights_upload_inline_f16(self, blocks, n, k, code_map, scale_mode: int = 0) -> int:
        b, cm = _np(blocks, np.uint8), _np(code_map, np.int8)
        h = C.c_uint64(0)
        self._check(self.c.bitnet_hip_weights_upload_inline_f16(b.ctypes.data_as(_u8p), b.size, n, k, cm.ctypes.data_as(_i8p), scale_mode, C.byref(h)))
        return h.value

    def matmul_workspace_bytes(self, m: int, k: int, digits: int = 4) -> int:
        return int(self.c.bitnet_hip_matmul_workspace_bytes(m, k, digits))

    def matmul_fused_dev(self, h: int, x, y, m: int, workspace, workspace_bytes: int, ln_gamma=None, ln_eps: float = 0.0, residual=None,
                         flags: int = 0, digits: int = 4, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_matmul_fused_dev(h, _ptr(x), _ptr(y), m, _ptr(ln_gamma) if ln_gamma is not None else None, ln_eps,
                                                       _ptr(residual) if residual is not None else None, flags, digits, _ptr(workspace),
                                                       workspace_bytes, _vp(stream)))

    # -- the prompt forward's f16 activation chain (include/bitnet_hip.h) --------------------------------------------------------
    def matmul_f16_supported(self, h: int) -> bool:
        return bool(self.c.bitnet_hip_matmul_f16_supported(h))

    def rows_to_f16_dev(self, x, gamma, m: int, cols: int, xh, stats, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_rows_to_f16_dev(_ptr(x), _optr(gamma), m, cols, _ptr(xh), _optr(stats), _vp(stream)))

    def matmul_f16_dev(self, h: int, xh, m: int, stats_in=None, n_stats: int = 0, ln_gamma=None, ln_eps: float = 0.0, y=None, residual=None,
                       flags: int = 0, yh=None, gamma_out=None, stats_out=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_matmul_f16_dev(h, _ptr(xh), m, _optr(stats_in), n_stats, _optr(ln_gamma), ln_eps, _optr(y), _optr(residual), flags,
                                                     _optr(yh), _optr(gamma_out), _optr(stats_out), _vp(stream)))

    def f16_saturations(self, reset: bool = True) -> int:
        return int(self.c.bitnet_hip_f16_saturations(1 if reset else 0))

    # ---- QB32: producer-quantised rows for the fp6 x fp4 prompt matmul (include/bitnet_hip.h) ----
    def qb32_bytes(self, m: int, cols: int) -> int:
        return int(self.c.bitnet_hip_qb32_bytes(m, cols))

    def rows_to_qb32_dev(self, x, gamma, m: int, cols: int, qb, stats, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_rows_to_qb32_dev(_ptr(x), _optr(gamma), m, cols, _ptr(qb), _optr(stats), _vp(stream)))

    def matmul_qb32_supported(self, h: int) -> bool:
        return bool(self.c.bitnet_hip_matmul_qb32_supported(h))

    def matmul_qb32_dev(self, h: int, qb, m: int, stats_in=None, n_stats: int = 0, ln_gamma=None, ln_eps: float = 0.0, y=None, residual=None,
                        flags: int = 0, yh=None, gamma_out=None, stats_out=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_matmul_qb32_dev(h, _ptr(qb), m, _optr(stats_in), n_stats, _optr(ln_gamma), ln_eps, _optr(y), _optr(residual), flags,
                                                      _optr(yh), _optr(gamma_out), _optr(stats_out), _vp(stream)))

    def attention_prefill_flags_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, seq_len, workspace, workspace_bytes,
                                    out, flags: int, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_prefill_flags_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv,
                                                                  head_dim, max_pos, seq_len, _ptr(workspace), workspace_bytes, _ptr(out), flags, _vp(stream)))

    def matmul_last_tile(self) -> dict:
        """The tile form this thread's last tiled matmul ran: {digits, wave_tokens, waves, scale_mode}."""
        v = [C.c_int() for _ in range(4)]
        self._check(self.c.bitnet_hip_matmul_last_tile(*[C.byref(x) for x in v]))
        return dict(zip(("digits", "wave_tokens", "waves", "scale_mode"), (x.value for x in v)))

    def matmul_last_wave_rows(self) -> int:
        """Output rows per wave of this thread's last tiled matmul: 64, or 80 (320-row workgroups)."""
        return int(self.c.bitnet_hip_matmul_last_wave_rows())

    def matmul_last_resident_fp4(self) -> bool:
        return bool(self.c.bitnet_hip_matmul_last_resident_fp4())

    def attention_prefill_workspace_bytes(self, n_heads: int, n_kv: int, seq_len: int) -> int:
        return int(self.c.bitnet_hip_attention_prefill_workspace_bytes(n_heads, n_kv, seq_len))

    def attention_prefill_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, seq_len, workspace,
                              workspace_bytes, out, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_prefill_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv,
                                                            head_dim, max_pos, seq_len, _ptr(workspace), workspace_bytes, _ptr(out), _vp(stream)))

    def attention_extend_workspace_bytes(self, n_heads: int, n_kv: int, past_len: int, seq_len: int) -> int:
        """Workspace of attention_extend_dev; 0 for sizes it refuses, non-decreasing in both lengths."""
        return int(self.c.bitnet_hip_attention_extend_workspace_bytes(n_heads, n_kv, past_len, seq_len))

    def attention_extend_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, past_len, seq_len, workspace,
                             workspace_bytes, out, flags: int = 0, stream: int = 0) -> None:
        """seq_len new tokens at positions past_len .. past_len + seq_len - 1 over caches that hold 0 .. past_len - 1: RoPE, cache append,
        causal GQA attention over keys 0 .. own position.  flags: ATTN_CACHE_F16 (1) | ATTN_OUT_F16 (2)."""
        self._check(self.c.bitnet_hip_attention_extend_dev(_optr(qkv), _optr(rope_sin), _optr(rope_cos), _optr(kcache), _optr(vcache), n_heads, n_kv,
                                                           head_dim, max_pos, past_len, seq_len, _optr(workspace), workspace_bytes, _optr(out), flags,
                                                           _vp(stream)))

    def attention_packed_row_align(self, n_heads: int, n_kv: int) -> int:
        """Row alignment of a segment's first row in attention_packed_dev: the attention workgroup's query tile, 64 rows for an even
        n_heads / n_kv, 128 for an odd one; 0 for head counts it refuses."""
        return int(self.c.bitnet_hip_attention_packed_row_align(n_heads, n_kv))

    @staticmethod
    def _i32_table(a):
        """host int32 array (or None) -> (keep-alive array, ctypes pointer)"""
        if a is None:
            return None, None
        t = _np(a, np.int32)
        return t, t.ctypes.data_as(C.POINTER(C.c_int32))

    def attention_packed_workspace_bytes(self, n_heads: int, n_kv: int, n_rows: int, past, len_) -> int:
        """Workspace of attention_packed_dev for segments (past[s], len_[s]) inside n_rows packed rows; 0 for sizes it refuses,
        non-decreasing in every past[s] and len_[s]."""
        pa, pp = self._i32_table(past)
        la, lp = self._i32_table(len_)
        n_seq = 0 if pa is None else pa.size
        return int(self.c.bitnet_hip_attention_packed_workspace_bytes(n_heads, n_kv, n_rows, n_seq, pp, lp))

    def attention_packed_dev(self, qkv, n_rows, rope_sin, rope_cos, row0, len_, past, kcaches, vcaches, n_heads, n_kv, head_dim, max_pos, workspace,
                             workspace_bytes, out, flags: int = 0, stream: int = 0, n_seq: int | None = None) -> None:
        """attention_extend_dev for SEVERAL sequences in one prep + one attention launch: segment s owns packed rows row0[s] .. row0[s] +
        len_[s] - 1 (row0 a multiple of attention_packed_row_align), its tokens sit at positions past[s] .. over kcaches[s] / vcaches[s]
        (tensors or raw device pointers), and its queries see its own keys only.  row0 / len_ / past are host arrays; rows outside every
        segment are padding (finite outputs, no cache traffic).  flags: ATTN_CACHE_F16 (1) | ATTN_OUT_F16 (2)."""
        ra, rp = self._i32_table(row0)
        la, lp = self._i32_table(len_)
        pa, pp = self._i32_table(past)

        def table(caches):
            if caches is None:
                return None
            vals = [None if c is None else (c if isinstance(c, int) else c.data_ptr()) for c in caches]
            return (_vp * max(len(vals), 1))(*vals)

        n = (ra.size if ra is not None else 0) if n_seq is None else n_seq
        self._check(self.c.bitnet_hip_attention_packed_dev(_optr(qkv), n_rows, _optr(rope_sin), _optr(rope_cos), n, rp, lp, pp, table(kcaches), table(vcaches),
                                                           n_heads, n_kv, head_dim, max_pos, _optr(workspace), workspace_bytes, _optr(out), flags, _vp(stream)))

    def attention_prefill_sharded_workspace_bytes(self, n_heads: int, n_kv: int, n_q: int, n_ctx: int) -> int:
        return int(self.c.bitnet_hip_attention_prefill_sharded_workspace_bytes(n_heads, n_kv, n_q, n_ctx))

    def attention_prefill_sharded_dev(self, q, ld_q, q_block_pos, n_q, kv, ld_kv, n_ctx, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv,
                                      head_dim, max_pos, workspace, workspace_bytes, out, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_prefill_sharded_dev(_ptr(q), ld_q, _ptr(q_block_pos), n_q, _ptr(kv), ld_kv, n_ctx, _ptr(rope_sin),
                                                                    _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv, head_dim, max_pos,
                                                                    _ptr(workspace), workspace_bytes, _ptr(out), _vp(stream)))

    def attention_prefill_gathered_dev(self, q, ld_q, q_block_pos, n_q, kv_gathered, n_ctx, world, kv_is_f16, rope_sin, rope_cos, kcache, vcache,
                                       cache_f16, n_heads, n_kv, head_dim, max_pos, workspace, workspace_bytes, out, stream: int = 0) -> None:
        """the k|v rows exactly as an all-gather over `world` ranks left them (rank-major zigzag chunks, f32 or f16)"""
        self._check(self.c.bitnet_hip_attention_prefill_gathered_dev(_ptr(q), ld_q, _ptr(q_block_pos), n_q, _ptr(kv_gathered), n_ctx, world,
                                                                     int(kv_is_f16), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache),
                                                                     int(cache_f16), n_heads, n_kv, head_dim, max_pos, _ptr(workspace), workspace_bytes,
                                                                     _ptr(out), _vp(stream)))

    def weights_bind_ln(self, h: int, ln_gamma, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_weights_bind_ln(h, _ptr(ln_gamma), _vp(stream)))

    def weights_free(self, h: int) -> None:
        self._check(self.c.bitnet_hip_weights_free(h))

    def weights_info(self, h: int):
        r, c, b = _sz(0), _sz(0), _sz(0)
        self._check(self.c.bitnet_hip_weights_info(h, C.byref(r), C.byref(c), C.byref(b)))
        return r.value, c.value, b.value

    def gemv_dev(self, h: int, x, y, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_gemv_dev(h, _ptr(x), _ptr(y), _vp(stream)))

    def matmul_dev(self, h: int, x, y, m: int, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_matmul_dev(h, _ptr(x), _ptr(y), m, _vp(stream)))

    def matmul_kernel_dev(self, h: int, x, y, m: int, kernel: int, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_matmul_kernel_dev(h, _ptr(x), _ptr(y), m, kernel, _vp(stream)))

    def add_dev(self, a, b, out, n: int, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_add_dev(_ptr(a), _ptr(b), _ptr(out), n, _vp(stream)))

    def silu_mul_dev(self, gate, up, out, n: int, tile: int = 0, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_silu_mul_dev(_ptr(gate), _ptr(up), _ptr(out), n, tile, _vp(stream)))

    def weights_device_bytes(self, h: int) -> int:
        return int(self.c.bitnet_hip_weights_device_bytes(h))

    def weights_fp4_image(self, h: int, enable: bool = True, stream: int = 0) -> None:
        """Build (or free) the resident fp4 image the fp6 x fp4 prompt matmul reads (include/bitnet_hip.h)."""
        self._check(self.c.bitnet_hip_weights_fp4_image(h, 1 if enable else 0, stream))

    def weights_trim(self, h: int) -> None:
        self._check(self.c.bitnet_hip_weights_trim(h))

    # ---- QAct: activations quantised by their producer (csrc/qact.hpp) ----
    def qact_bytes(self, cols: int) -> int:
        return int(self.c.bitnet_hip_qact_bytes(cols))

    def qact_stats_bytes(self, cols: int) -> int:
        return int(self.c.bitnet_hip_qact_stats_bytes(cols))

    def quantize_act_dev(self, x, gamma, cols: int, qact_out, stats_out=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_quantize_act_dev(_ptr(x), _optr(gamma), cols, _ptr(qact_out), _optr(stats_out), _vp(stream)))

    def embed_q_dev(self, table, tokens, x_out, hidden: int, vocab: int, gamma, qact_out, stats_out=None, offset=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_embed_q_dev(_ptr(table), _ptr(tokens), _optr(offset), hidden, vocab, _ptr(x_out), _optr(gamma), _ptr(qact_out),
                                                  _optr(stats_out), _vp(stream)))

    def gemv_q_supported(self, h: int) -> bool:
        return bool(self.c.bitnet_hip_gemv_q_supported(h))

    def gemv_geometry(self, h: int, flags: int = 0, ln_gamma=None, merge: int = 0) -> dict:
        """the kernel (and k_gemv_mfma instance) gemv_dev / gemv_fused_dev (merge 0) or gemv_attn_merge_dev (merge = query group) would launch; host only"""
        g = GemvGeometry()
        self._check(self.c.bitnet_hip_gemv_geometry(h, flags, _optr(ln_gamma), merge, C.byref(g)))
        return {n: getattr(g, n) for n, _ in GemvGeometry._fields_}

    def gemv_q_geometry(self, h: int, flags: int = 0, layernorm: bool = False, merge_records: int = 0) -> dict:
        """the k_gemv_q instance gemv_q_dev (merge_records 0) / gemv_attn_merge[_rec]_q_dev (4 or 8) would launch; host only"""
        g = GemvQGeometry()
        self._check(self.c.bitnet_hip_gemv_q_geometry(h, flags, int(layernorm), merge_records, C.byref(g)))
        return {n: getattr(g, n) for n, _ in GemvQGeometry._fields_}

    def gemv_q_dev(self, h: int, qact_in, y=None, stats_in=None, ln_gamma=None, ln_eps: float = 0.0, residual=None, flags: int = 0, qact_out=None,
                   gamma_out=None, stats_out=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_gemv_q_dev(h, _ptr(qact_in), _optr(stats_in), _optr(ln_gamma), ln_eps, _optr(residual), flags, _optr(y),
                                                 _optr(qact_out), _optr(gamma_out), _optr(stats_out), _vp(stream)))

    def attention_decode_q_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, pos, scratch, out, qact_out,
                               wide: bool = False, kv_f16: bool = False, stream: int = 0, partial: bool = False) -> None:
        flags = (1 if wide else 0) | (2 if kv_f16 else 0) | (4 if partial else 0)  # BITNET_HIP_ATTN_WIDE / _KV_F16 / _PARTIAL
        self._check(self.c.bitnet_hip_attention_decode_q_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv,
                                                             head_dim, max_pos, _ptr(pos), _ptr(scratch), flags, _optr(out), _optr(qact_out), _vp(stream)))

    # ---- several sequences per launch: vector b at b times its batch-1 size; *_ptrs = int64 device tensors of n_seq device pointers (0 = idle) ----
    def embed_q_batch_dev(self, table, history_ptrs, pos_ptrs, n_seq: int, hidden: int, vocab: int, x_out, gamma, qact_out, stats_out=None,
                          stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_embed_q_batch_dev(_ptr(table), _ptr(history_ptrs), _ptr(pos_ptrs), n_seq, hidden, vocab, _ptr(x_out), _optr(gamma),
                                                        _ptr(qact_out), _optr(stats_out), _vp(stream)))

    def gemv_q_batch_dev(self, h: int, n_seq: int, qact_in, y=None, stats_in=None, ln_gamma=None, ln_eps: float = 0.0, residual=None, flags: int = 0,
                         qact_out=None, gamma_out=None, stats_out=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_gemv_q_batch_dev(h, n_seq, _ptr(qact_in), _optr(stats_in), _optr(ln_gamma), ln_eps, _optr(residual), flags, _optr(y),
                                                       _optr(qact_out), _optr(gamma_out), _optr(stats_out), _vp(stream)))

    def attention_decode_batch_dev(self, qkv, rope_sin, rope_cos, kcache_ptrs, vcache_ptrs, pos_ptrs, n_seq: int, n_heads, n_kv, head_dim, max_pos, scratch,
                                   out, qact_out, kv_f16: bool = False, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_decode_batch_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache_ptrs), _ptr(vcache_ptrs),
                                                                 _ptr(pos_ptrs), n_seq, n_heads, n_kv, head_dim, max_pos, _ptr(scratch),
                                                                 2 if kv_f16 else 0, _optr(out), _optr(qact_out), _vp(stream)))

    def logits_f16_batch_dev(self, table, x, gamma, eps, hidden, vocab, n_seq: int, logits_ptrs, scratch, n_wg, token_ptrs=None, pos_ptrs=None,
                             history_ptrs=None, n_forced_ptrs=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_logits_f16_batch_dev(_ptr(table), _ptr(x), _optr(gamma), eps, hidden, vocab, n_seq, _ptr(logits_ptrs), _ptr(scratch),
                                                           n_wg, _optr(token_ptrs), _optr(pos_ptrs), _optr(history_ptrs), _optr(n_forced_ptrs), _vp(stream)))

    # ---- the wide decode step: n_seq <= 64 sequences as dense rows; *_ptrs = int64 device tensors of n_seq device pointers (0 = idle row) ----
    def embed_rows_dev(self, table, history_ptrs, pos_ptrs, n_seq: int, hidden: int, vocab: int, x_out, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_embed_rows_dev(_ptr(table), _ptr(history_ptrs), _ptr(pos_ptrs), n_seq, hidden, vocab, _ptr(x_out), _vp(stream)))

    def attention_decode_rows_dev(self, qkv, rope_sin, rope_cos, kcache_ptrs, vcache_ptrs, pos_ptrs, n_seq: int, n_heads, n_kv, head_dim, max_pos, key_bound,
                                  scratch, out, kv_f16: bool = False, out_f16: bool = False, stream: int = 0) -> None:
        flags = (1 if kv_f16 else 0) | (2 if out_f16 else 0)  # BITNET_HIP_ATTN_CACHE_F16 | BITNET_HIP_ATTN_OUT_F16
        self._check(self.c.bitnet_hip_attention_decode_rows_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache_ptrs), _ptr(vcache_ptrs), _ptr(pos_ptrs),
                                                                n_seq, n_heads, n_kv, head_dim, max_pos, key_bound, _ptr(scratch), flags, _ptr(out), _vp(stream)))

    def pick_rows_dev(self, logits, argmax, n_seq: int, vocab: int, logits_ptrs, token_ptrs=None, pos_ptrs=None, history_ptrs=None, n_forced_ptrs=None,
                      stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_pick_rows_dev(_ptr(logits), _ptr(argmax), n_seq, vocab, _ptr(logits_ptrs), _optr(token_ptrs), _optr(pos_ptrs),
                                                    _optr(history_ptrs), _optr(n_forced_ptrs), _vp(stream)))

    def kv_fork_dev(self, src_k_ptrs, src_v_ptrs, dst_k_ptrs, dst_v_ptrs, n_layers: int, n_dst: int, n_kv: int, head_dim: int, max_pos: int,
                    n_positions: int, kv_f16: bool = False, stream: int = 0) -> None:
        """Cache slots [0, n_positions) of every layer's K and V of one source into n_dst destinations, bit for bit, in one launch.  *_ptrs: int64
        device tensors of device pointers, the source's [n_layers], the destinations' [n_dst][n_layers]; buffers distinct, 16-byte aligned."""
        self._check(self.c.bitnet_hip_kv_fork_dev(_ptr(src_k_ptrs), _ptr(src_v_ptrs), _ptr(dst_k_ptrs), _ptr(dst_v_ptrs), n_layers, n_dst, n_kv, head_dim,
                                                  max_pos, n_positions, 2 if kv_f16 else 0, _vp(stream)))

    def kv_permute_dev(self, k_ptrs, v_ptrs, beam: "Beam", n_layers: int, n_beams: int, n_kv: int, head_dim: int, max_pos: int, key_bound: int,
                       kv_f16: bool = False, stream: int = 0) -> None:
        """In place, in one launch: for every beam b whose parent (read from the beam state on the device) is another beam, cache slots
        [from[b], n_slots) of every layer's K and V of cache b take the bits of the parent's.  *_ptrs: int64 device tensors [n_beams][n_layers]."""
        self._check(self.c.bitnet_hip_kv_permute_dev(_ptr(k_ptrs), _ptr(v_ptrs), beam.h, n_layers, n_beams, n_kv, head_dim, max_pos, key_bound,
                                                     2 if kv_f16 else 0, _vp(stream)))

    def kv_snapshot_bytes(self, n_layers: int, n_kv: int, head_dim: int, n_positions: int, kv_f16: bool = False) -> int:
        """Bytes of a snapshot of n_positions: K [n_layers][n_kv][n_positions][128] then V the same, in the cache's element type; 0 for a
        geometry kv_save_dev / kv_restore_dev refuse."""
        return int(self.c.bitnet_hip_kv_snapshot_bytes(n_layers, n_kv, head_dim, n_positions, 2 if kv_f16 else 0))

    def kv_save_dev(self, k_ptrs, v_ptrs, n_layers: int, n_kv: int, head_dim: int, max_pos: int, n_positions: int, snapshot, kv_f16: bool = False,
                    stream: int = 0) -> None:
        """Cache slots [0, n_positions) of every layer's K and V of one sequence into `snapshot` (kv_snapshot_bytes, 16-byte aligned), position-major,
        bit for bit, in one launch.  *_ptrs: int64 device tensors of n_layers device pointers."""
        self._check(self.c.bitnet_hip_kv_save_dev(_ptr(k_ptrs), _ptr(v_ptrs), n_layers, n_kv, head_dim, max_pos, n_positions, 2 if kv_f16 else 0,
                                                  _ptr(snapshot), _vp(stream)))

    def kv_restore_dev(self, snapshot, snapshot_positions: int, dst_k_ptrs, dst_v_ptrs, n_layers: int, n_dst: int, n_kv: int, head_dim: int,
                       max_pos: int, n_positions: int, kv_f16: bool = False, stream: int = 0) -> None:
        """Positions [0, n_positions) of a snapshot of snapshot_positions into cache slots [0, n_positions) of n_dst destinations, bit for bit, in
        one launch; every other cache byte stays.  dst_*_ptrs: int64 device tensors [n_dst][n_layers] of device pointers, as kv_fork_dev takes."""
        self._check(self.c.bitnet_hip_kv_restore_dev(_ptr(snapshot), snapshot_positions, _ptr(dst_k_ptrs), _ptr(dst_v_ptrs), n_layers, n_dst, n_kv,
                                                     head_dim, max_pos, n_positions, 2 if kv_f16 else 0, _vp(stream)))

    def kv_shift_dev(self, k_ptrs, v_ptrs, rope_sin, rope_cos, n_layers: int, n_kv: int, head_dim: int, max_pos: int, keep: int, discard: int,
                     n_positions: int, kv_f16: bool = False, stream: int = 0) -> None:
        """In place, in one launch: cache slot j of every layer's K and V takes slot j + discard for j in [keep, n_positions - discard), V bit for
        bit, K re-rotated between RoPE table rows j + discard and j.  *_ptrs: int64 device tensors of n_layers device pointers; rope_sin /
        rope_cos: [max_pos, 64] f32 on the device."""
        self._check(self.c.bitnet_hip_kv_shift_dev(_ptr(k_ptrs), _ptr(v_ptrs), _ptr(rope_sin), _ptr(rope_cos), n_layers, n_kv, head_dim, max_pos, keep,
                                                   discard, n_positions, 2 if kv_f16 else 0, _vp(stream)))

    def attention_merge_q_max_keys(self) -> int:
        return int(self.c.bitnet_hip_attention_merge_q_max_keys())

    def gemv_attn_merge_rec_q_dev(self, h: int, scratch, n_heads, n_kv, max_pos, pos, y, qact_out, max_records: int, residual=None, gamma_out=None,
                                  stats_out=None, stream: int = 0) -> None:
        """gemv_attn_merge_q_dev with the record bound chosen by the caller (4 or 8 records of 64 positions)"""
        self._check(self.c.bitnet_hip_gemv_attn_merge_rec_q_dev(h, _ptr(scratch), n_heads, n_kv, max_pos, _ptr(pos), _ptr(y), _optr(residual),
                                                                _ptr(qact_out), _optr(gamma_out), _optr(stats_out), max_records, _vp(stream)))

    def gemv_attn_merge_q_dev(self, h: int, scratch, n_heads, n_kv, max_pos, pos, y, qact_out, residual=None, gamma_out=None, stats_out=None,
                              stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_gemv_attn_merge_q_dev(h, _ptr(scratch), n_heads, n_kv, max_pos, _ptr(pos), _ptr(y), _optr(residual),
                                                            _ptr(qact_out), _optr(gamma_out), _optr(stats_out), _vp(stream)))

    def weights_concat(self, parts, interleave16: bool = False) -> int:
        arr = (C.c_uint64 * len(parts))(*parts)
        h = C.c_uint64(0)
        self._check(self.c.bitnet_hip_weights_concat(arr, len(parts), int(interleave16), C.byref(h)))
        return h.value

    def gemv_fused_dev(self, h: int, x, y, m: int = 1, ln_gamma=None, ln_eps: float = 0.0, residual=None, flags: int = 0, stream: int = 0) -> None:
        self._check(
            self.c.bitnet_hip_gemv_fused_dev(h, _ptr(x), _ptr(y), m, _ptr(ln_gamma) if ln_gamma is not None else None, ln_eps,
                                             _ptr(residual) if residual is not None else None, flags, _vp(stream))
        )

    # -- decode-step operators ------------------------------------------------
    def rmsnorm(self, x, gamma, num_rows: int, hidden: int, eps: float = 1e-6) -> np.ndarray:
        xa, ga = _np(x, np.float32), _np(gamma, np.float32)
        out = np.zeros(num_rows * hidden, np.float32)
        self._check(self.c.bitnet_hip_rmsnorm(xa.ctypes.data_as(_f32p), xa.size, ga.ctypes.data_as(_f32p), ga.size, out.ctypes.data_as(_f32p), out.size, num_rows, hidden, eps))
        return out

    def norm_rows_dev(self, x, gamma, out, rows: int, hidden: int, eps: float, rms: bool, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_norm_rows_dev(_ptr(x), _ptr(gamma), _ptr(out), rows, hidden, eps, int(rms), _vp(stream)))

    def embed_f16_dev(self, table, tokens, out, n: int, hidden: int, vocab: int, offset=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_embed_f16_dev(_ptr(table), _ptr(tokens), _ptr(offset) if offset is not None else None, n, hidden, vocab, _ptr(out), _vp(stream)))

    def attention_decode_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, pos, scratch, out, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_decode_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv, head_dim, max_pos, _ptr(pos), _ptr(scratch), _ptr(out), _vp(stream)))

    def attention_decode_wide_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, pos, scratch, out, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_decode_wide_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv, head_dim, max_pos, _ptr(pos), _ptr(scratch), _ptr(out), _vp(stream)))

    def attention_decode_partial_dev(self, qkv, rope_sin, rope_cos, kcache, vcache, n_heads, n_kv, head_dim, max_pos, pos, scratch, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_attention_decode_partial_dev(_ptr(qkv), _ptr(rope_sin), _ptr(rope_cos), _ptr(kcache), _ptr(vcache), n_heads, n_kv, head_dim, max_pos, _ptr(pos), _ptr(scratch), _vp(stream)))

    def gemv_attn_merge_dev(self, h: int, scratch, n_heads: int, n_kv: int, max_pos: int, pos, y, residual=None, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_gemv_attn_merge_dev(h, _ptr(scratch), n_heads, n_kv, max_pos, _ptr(pos), _ptr(y), _ptr(residual) if residual is not None else None, _vp(stream)))

    def logits_f16_dev(self, table, x, gamma, eps, hidden, vocab, logits, scratch, n_wg, token=None, pos=None, history=None, n_forced=None, stream: int = 0) -> None:
        opt = lambda t: _ptr(t) if t is not None else None
        self._check(self.c.bitnet_hip_logits_f16_dev(_ptr(table), _ptr(x), opt(gamma), eps, hidden, vocab, _ptr(logits), _ptr(scratch), n_wg, opt(token), opt(pos), opt(history), opt(n_forced), _vp(stream)))

    def score_workspace_bytes(self, n_rows: int, hidden: int, vocab: int) -> int:
        """Workspace of score_f16_dev; 0 for sizes the library refuses."""
        return int(self.c.bitnet_hip_score_workspace_bytes(n_rows, hidden, vocab))

    def score_f16_dev(self, table, x, gamma, eps: float, hidden: int, vocab: int, n_rows: int, targets, nll, argmax=None, logits=None,
                      logits_rows: int = 0, workspace=None, workspace_bytes: int = 0, stream: int = 0) -> None:
        """Teacher-forced scoring of n_rows residual rows against the tied f16 table (include/bitnet_hip.h bitnet_hip_score_f16_dev):
        nll[r] = logsumexp(l_r) - l_r[targets[r]], argmax[r], and the raw logits of rows < logits_rows.  Device pointers / tensors."""
        self._check(self.c.bitnet_hip_score_f16_dev(_optr(table), _optr(x), _optr(gamma), eps, hidden, vocab, n_rows, _optr(targets), _optr(nll),
                                                    _optr(argmax), _optr(logits), logits_rows, _optr(workspace), workspace_bytes, _vp(stream)))

    def head_screen_bytes(self, hidden: int, vocab: int) -> int:
        """bytes of the screening image of a [vocab, hidden] f16 table; 0: no screened head for this hidden size"""
        return int(self.c.bitnet_hip_head_screen_bytes(hidden, vocab))

    def head_screen_ws_bytes(self, hidden: int, vocab: int, n_wg: int) -> int:
        return int(self.c.bitnet_hip_head_screen_ws_bytes(hidden, vocab, n_wg))

    def head_screen_build_dev(self, table, hidden: int, vocab: int, image, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_head_screen_build_dev(_ptr(table), hidden, vocab, _ptr(image), _vp(stream)))

    def logits_screen_dev(self, table, x, gamma, eps, hidden, vocab, image, ws, scratch, n_wg, token=None, pos=None, history=None, n_forced=None, stream: int = 0) -> None:
        """bitnet_hip_logits_f16_dev's greedy pick without the logits: the int8 screen, then the surviving rows from the f16 table"""
        opt = lambda t: _ptr(t) if t is not None else None
        self._check(self.c.bitnet_hip_logits_screen_dev(_ptr(table), _ptr(x), opt(gamma), eps, hidden, vocab, _ptr(image), _ptr(ws), _ptr(scratch), n_wg, opt(token), opt(pos), opt(history), opt(n_forced), _vp(stream)))

    def argmax_dev(self, v, n: int, scratch, n_wg: int, token, stream: int = 0) -> None:
        self._check(self.c.bitnet_hip_argmax_dev(_ptr(v), n, _ptr(scratch), n_wg, _ptr(token), _vp(stream)))

    def sampler(self, vocab: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0,
                seed: int | None = None, *, min_p: float = 0.0, typical_p: float = 1.0, frequency_penalty: float = 0.0,
                presence_penalty: float = 0.0) -> "Sampler":
        """A device sampler (bitnet_hip_sampler_*): the reference's Sampler::new(temperature, top_k, top_p, repetition_penalty, seed), with
        the chain stages of bitnet_hip_sampling_config_ex (min-p, typical-p, frequency / presence penalty; the defaults switch them off)."""
        return Sampler(self, vocab, SamplingConfigEx.make(temperature, top_k, top_p, repetition_penalty, seed, min_p, typical_p,
                                                          frequency_penalty, presence_penalty))

    def grammar(self, token_class, next_table) -> "Grammar":
        """A token automaton on the device (bitnet_hip_grammar_*): token_class [vocab], next [n_states, n_classes]; grammar.token_automaton
        compiles one from a byte-level DFA and the vocabulary's byte strings."""
        return Grammar(self, token_class, next_table)

    def sample_batch(self, vocab: int, n_slots: int, wide: bool = False) -> "SampleBatch":
        """A table of n_slots sampler bindings served by one launch (bitnet_hip_sample_batch_*): 1..8 slots, or with wide=True 1..64
        (bitnet_hip_sample_batch_create_wide, the wide step's tail)."""
        return SampleBatch(self, vocab, n_slots, wide)

    def logprob_scratch_bytes(self, vocab: int) -> int:
        """Bytes of the scratch one bitnet_hip_logprob_args entry needs (zeroed once by the caller); 0 for a vocabulary the library refuses."""
        return int(self.c.bitnet_hip_logprob_scratch_bytes(vocab))

    def logprob_dev(self, args: "LogprobArgs", vocab: int, stream: int = 0) -> None:
        """One launch after the pick: record [*pos] of the entry -- token, its raw logit, the row's log-sum-exp, the top_n (id, logit) pairs."""
        self._check(self.c.bitnet_hip_logprob_dev(C.byref(args) if args is not None else None, vocab, _vp(stream)))

    def logprob_batch_dev(self, table, n_slots: int, vocab: int, stream: int = 0) -> None:
        """The same for n_slots entries read from a DEVICE table of LogprobArgs (a uint8 tensor holding them, or a raw pointer), one launch."""
        self._check(self.c.bitnet_hip_logprob_batch_dev(C.cast(_optr(table), C.POINTER(LogprobArgs)), n_slots, vocab, _vp(stream)))

    def logprob_rows_dev(self, table, n_slots: int, vocab: int, stream: int = 0) -> None:
        """logprob_batch_dev for n_slots = 1..64 entries (bitnet_hip_logprob_rows_dev, the wide step's tail), one launch."""
        self._check(self.c.bitnet_hip_logprob_rows_dev(C.cast(_optr(table), C.POINTER(LogprobArgs)), n_slots, vocab, _vp(stream)))

    def hbm_read_ceiling(self, nbytes: int = 2 << 30, iters: int = 10, stream: int = 0):
        """Measured read-only stream ceiling of the device: (best, mean) GB/s."""
        best, mean = C.c_double(0.0), C.c_double(0.0)
        self._check(self.c.bitnet_hip_hbm_read_ceiling(nbytes, iters, C.byref(best), C.byref(mean), _vp(stream)))
        return best.value, mean.value


LOGPROB_TOP_MAX = 20


class LogprobRecord(C.Structure):
    """bitnet_hip_logprob_record (176 bytes)"""
    _fields_ = [("token", C.c_int32), ("n_top", C.c_int32), ("logit", C.c_float), ("lse", C.c_float), ("top_id", C.c_int32 * LOGPROB_TOP_MAX),
                ("top_logit", C.c_float * LOGPROB_TOP_MAX)]


# the same layout for numpy: records read back as one structured array
LOGPROB_DTYPE = np.dtype([("token", "<i4"), ("n_top", "<i4"), ("logit", "<f4"), ("lse", "<f4"), ("top_id", "<i4", (LOGPROB_TOP_MAX,)),
                          ("top_logit", "<f4", (LOGPROB_TOP_MAX,))])


class LogprobArgs(C.Structure):
    """bitnet_hip_logprob_args: device pointers as integers (0 = NULL; records_dev 0 = an empty entry)"""
    _fields_ = [("logits_dev", C.c_void_p), ("pos_dev", C.c_void_p), ("history_dev", C.c_void_p), ("records_dev", C.c_void_p),
                ("scratch_dev", C.c_void_p), ("capacity", C.c_uint32), ("top_n", C.c_uint32)]

    @classmethod
    def make(cls, logits=None, pos=None, history=None, records=None, scratch=None, capacity: int = 0, top_n: int = 0) -> "LogprobArgs":
        p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        return cls(p(logits), p(pos), p(history), p(records), p(scratch), int(capacity), int(top_n))


Logprobs = collections.namedtuple("Logprobs", "token logit lse logprob top_ids top_logits")


class SamplingConfig(C.Structure):
    """bitnet_hip_sampling_config"""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repetition_penalty", C.c_float), ("seed", C.c_uint64)]

    @classmethod
    def make(cls, temperature: float, top_k: int, top_p: float, repetition_penalty: float, seed: int | None = None) -> "SamplingConfig":
        if seed is None:  # the reference seeds from entropy when --seed is absent
            seed = int.from_bytes(os.urandom(8), "little")
        return cls(float(temperature), int(top_k), float(top_p), float(repetition_penalty), int(seed) & 0xFFFFFFFFFFFFFFFF)


class SamplingConfigEx(C.Structure):
    """bitnet_hip_sampling_config_ex"""
    _fields_ = [("base", SamplingConfig), ("min_p", C.c_float), ("typical_p", C.c_float), ("frequency_penalty", C.c_float),
                ("presence_penalty", C.c_float)]

    @classmethod
    def make(cls, temperature: float, top_k: int, top_p: float, repetition_penalty: float, seed: int | None = None, min_p: float = 0.0,
             typical_p: float = 1.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0) -> "SamplingConfigEx":
        return cls(SamplingConfig.make(temperature, top_k, top_p, repetition_penalty, seed), float(min_p), float(typical_p),
                   float(frequency_penalty), float(presence_penalty))


class MirostatConfig(C.Structure):
    """bitnet_hip_mirostat_config"""
    _fields_ = [("tau", C.c_float), ("eta", C.c_float)]


CONSTRAINT_MAX_HOLD, CONSTRAINT_MAX_NGRAM = 32, 8


class Constraints(C.Structure):
    """bitnet_hip_constraints.  make() keeps the arrays the pointers refer to alive on the object."""
    _fields_ = [("bias_ids", C.POINTER(C.c_int32)), ("bias_values", _f32p), ("n_bias", _sz), ("allowed_ids", C.POINTER(C.c_int32)),
                ("n_allowed", _sz), ("hold_ids", C.POINTER(C.c_int32)), ("n_hold", _sz), ("min_tokens", C.c_int32), ("no_repeat_ngram", C.c_int32)]

    @classmethod
    def make(cls, bias=None, allowed=None, hold=(), min_tokens: int = 0, no_repeat_ngram: int = 0) -> "Constraints":
        """bias: {id: value} or (id, value) pairs, in order (the last entry of a duplicate id wins; -inf bans); allowed: ids, every other id is
        banned (None or empty: no allowed list); hold: ids banned while fewer than min_tokens tokens were chosen; no_repeat_ngram: 0 = off."""
        pairs = list(bias.items()) if isinstance(bias, dict) else list(bias if bias is not None else ())

        def i32(xs):  # ids as int32, refused rather than wrapped when they do not fit
            a = np.asarray(list(xs), dtype=np.int64).reshape(-1)
            if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
                raise ValueError(f"constraints: token id outside the int32 range: {int(a.min())} .. {int(a.max())}")
            return _np(a.astype(np.int32), np.int32)

        bi, bv = i32(p[0] for p in pairs), _np(np.asarray([p[1] for p in pairs], dtype=np.float32), np.float32)
        al, ho = i32(allowed if allowed is not None else ()), i32(hold)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None
        cfg = cls(p(bi), bv.ctypes.data_as(_f32p) if bv.size else None, bi.size, p(al), al.size, p(ho), ho.size, int(min_tokens), int(no_repeat_ngram))
        cfg._keep = (bi, bv, al, ho)
        return cfg

    @classmethod
    def from_args(cls, bias, allowed, hold, min_tokens, no_repeat_ngram, off, on=False) -> "Constraints | None":
        """None (= off) for off=True, or for a call that names nothing unless on=True (an empty config: it edits nothing, and the chosen
        tokens are counted from then on); else make(...)."""
        n = lambda v: 0 if v is None else len(v)
        hold = list(hold)
        allowed = None if allowed is None else list(allowed)
        nothing = not n(bias) and not n(allowed) and not hold and not min_tokens and not no_repeat_ngram
        return None if off or (nothing and not on) else cls.make(bias, allowed, hold, min_tokens, no_repeat_ngram)


GRAMMAR_MAX_STATES, GRAMMAR_MAX_CLASSES = 65536, 16384


class GrammarDesc(C.Structure):
    """bitnet_hip_grammar_desc.  make() keeps the arrays the pointers refer to alive on the object."""
    _fields_ = [("token_class", C.POINTER(C.c_uint16)), ("vocab", _sz), ("next", C.POINTER(C.c_int32)), ("n_states", _sz), ("n_classes", _sz)]

    @classmethod
    def make(cls, token_class, next_table) -> "GrammarDesc":
        """token_class: [vocab] class ids; next_table: [n_states, n_classes] next states, -1 = the class is not allowed in the state."""
        tc = np.asarray(token_class)
        if tc.ndim != 1 or (tc.size and (tc.min() < 0 or tc.max() > 0xffff)):
            raise ValueError("grammar: token_class must be one-dimensional with every class id in 0..65535")
        nx = np.asarray(next_table)
        if nx.ndim != 2:
            raise ValueError(f"grammar: next must be [n_states, n_classes], got shape {nx.shape}")
        if nx.size and (nx.min() < -(1 << 31) or nx.max() >= (1 << 31)):
            raise ValueError("grammar: a next entry is outside the int32 range")
        tc, nx = _np(tc, np.uint16), _np(nx, np.int32)
        d = cls(tc.ctypes.data_as(C.POINTER(C.c_uint16)), tc.size, nx.ctypes.data_as(C.POINTER(C.c_int32)), nx.shape[0], nx.shape[1])
        d._keep = (tc, nx)
        return d


class Grammar:
    """One bitnet_hip_grammar: a token automaton on the device (token_class [vocab], next [n_states, n_classes]), bound to any number of
    samplers with Sampler.set_grammar (a decoder's sampler: Decoder::set_grammar, host/grammar_host.hpp).  Keeps the descriptor, so walk() -- host only -- works for its whole life,
    after close() too.  close() on a bound grammar takes effect when the last sampler lets go of it."""

    def __init__(self, lib: HipLib, token_class, next_table):
        self.lib = lib
        self.h = None
        self.desc = GrammarDesc.make(token_class, next_table)
        self.vocab, self.n_states, self.n_classes = int(self.desc.vocab), int(self.desc.n_states), int(self.desc.n_classes)
        h = _vp()
        lib._check(lib.c.bitnet_hip_grammar_create(C.byref(self.desc), C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.c.bitnet_hip_grammar_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def walk(self, state: int, tokens) -> tuple[int, int]:
        """(state reached, tokens taken) from `state`: stops in front of the first token that is not allowed or not in the vocabulary."""
        return grammar_walk(self.lib, self.desc, state, tokens)


def grammar_walk(lib: HipLib, desc: GrammarDesc, state: int, tokens) -> tuple[int, int]:
    """bitnet_hip_grammar_walk on a descriptor: host only, no GPU."""
    t = np.asarray(list(tokens), dtype=np.int64).reshape(-1)
    if t.size and (t.min() < -(1 << 31) or t.max() >= (1 << 31)):
        raise ValueError("grammar: token id outside the int32 range")
    t = _np(t.astype(np.int32), np.int32)
    out, taken = C.c_int32(-1), _sz(0)
    lib._check(lib.c.bitnet_hip_grammar_walk(C.byref(desc), int(state), t.ctypes.data_as(_vp) if t.size else None, t.size, C.byref(out), C.byref(taken)))
    return int(out.value), int(taken.value)


class Sampler:
    """One bitnet_hip_sampler: state (config, ChaCha20 key, word counter, token counts) in device memory."""

    def __init__(self, lib: HipLib, vocab: int, cfg: "SamplingConfig | SamplingConfigEx"):
        self.lib, self.vocab = lib, int(vocab)
        h = _vp()
        if isinstance(cfg, SamplingConfigEx):
            lib._check(lib.c.bitnet_hip_sampler_create_ex(vocab, C.byref(cfg), C.byref(h)))
        else:
            lib._check(lib.c.bitnet_hip_sampler_create(vocab, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.c.bitnet_hip_sampler_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def configure(self, temperature: float, top_k: int, top_p: float, repetition_penalty: float, seed: int | None = None, *,
                  min_p: float = 0.0, typical_p: float = 1.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0) -> None:
        cfg = SamplingConfigEx.make(temperature, top_k, top_p, repetition_penalty, seed, min_p, typical_p, frequency_penalty, presence_penalty)
        self.lib._check(self.lib.c.bitnet_hip_sampler_configure_ex(self.h, C.byref(cfg)))

    def reset(self) -> None:
        self.lib._check(self.lib.c.bitnet_hip_sampler_reset(self.h))

    def draws(self) -> int:
        d = C.c_uint64(0)
        self.lib._check(self.lib.c.bitnet_hip_sampler_draws(self.h, C.byref(d)))
        return int(d.value)

    def set_mirostat(self, tau: float | None, eta: float = 0.1) -> None:
        """MirostatSampler::new(tau, eta, ..) in place of the truncation stages: mu = 2 * tau, updated on the device by every sampling
        launch.  set_mirostat(None): off.  Graphs that captured sample_dev follow it."""
        if tau is None:
            self.lib._check(self.lib.c.bitnet_hip_sampler_set_mirostat(self.h, None))
            return
        cfg = MirostatConfig(float(tau), float(eta))
        self.lib._check(self.lib.c.bitnet_hip_sampler_set_mirostat(self.h, C.byref(cfg)))

    def mirostat_state(self) -> tuple[float, int]:
        """(mu as the f32 the device holds, fallback calls since set_mirostat / reset).  Synchronous."""
        mu, fb = C.c_float(0.0), C.c_uint64(0)
        self.lib._check(self.lib.c.bitnet_hip_sampler_mirostat_state(self.h, C.byref(mu), C.byref(fb)))
        return float(mu.value), int(fb.value)

    def set_constraints(self, bias=None, allowed=None, hold=(), min_tokens: int = 0, no_repeat_ngram: int = 0, *, off: bool = False, on: bool = False) -> None:
        """Logit constraints in front of every other stage, inside the same launch (bitnet_hip_sampler_set_constraints): bias {id: value}
        (-inf bans), allowed ids (every other id banned), hold ids banned until min_tokens tokens were chosen, no_repeat_ngram.  With no
        arguments, or off=True: constraints off; on=True with no arguments: an empty config, which edits nothing and lets chosen() count every
        token from then on.  Graphs that captured sample_dev follow it; chosen() stays."""
        cfg = Constraints.from_args(bias, allowed, hold, min_tokens, no_repeat_ngram, off, on)
        self.lib._check(self.lib.c.bitnet_hip_sampler_set_constraints(self.h, C.byref(cfg) if cfg is not None else None))

    def chosen(self) -> int:
        """Tokens chosen by launches that ran with constraints on since the last reset (the hold-off's count).  Synchronous."""
        g = C.c_uint64(0)
        self.lib._check(self.lib.c.bitnet_hip_sampler_constraints_state(self.h, C.byref(g)))
        return int(g.value)

    def set_grammar(self, grammar: "Grammar | None", start_state: int = 0) -> None:
        """Bind a token automaton (bitnet_hip_sampler_set_grammar): every launch bans the tokens the state does not allow and moves the state
        with the token it chose, on the device.  None: off.  The state starts at start_state, both counters at 0.  Graphs that captured
        sample_dev follow it."""
        self.lib._check(self.lib.c.bitnet_hip_sampler_set_grammar(self.h, grammar.h if grammar is not None else None, int(start_state)))
        self._grammar = grammar  # the Python object stays alive while bound

    def set_grammar_state(self, state: int) -> None:
        """Overwrite the state word (the counters stay): what a host calls after a rewind, with Grammar.walk's state."""
        self.lib._check(self.lib.c.bitnet_hip_sampler_set_grammar_state(self.h, int(state)))

    def grammar_state(self) -> tuple[int, int, int]:
        """(state, steps, violations) of the bound grammar; (-1, 0, 0) without one.  Synchronous."""
        s, n, v = C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
        self.lib._check(self.lib.c.bitnet_hip_sampler_grammar_state(self.h, C.byref(s), C.byref(n), C.byref(v)))
        return int(s.value), int(n.value), int(v.value)

    def sample_host(self, logits, generated=()) -> int:
        """Sampler::sample(&logits, &generated_tokens): the whole generated list on every call."""
        x = _np(logits, np.float32)
        g = _np(np.asarray(generated, dtype=np.uint32), np.uint32)
        tok = C.c_uint32(0)
        self.lib._check(self.lib.c.bitnet_hip_sample_host(self.h, x.ctypes.data_as(_f32p), x.size, g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size,
                                                          C.byref(tok)))
        return int(tok.value)

    def sample_dev(self, logits, token, pos=None, history=None, n_forced=None, stream: int = 0) -> None:
        """One step on device tensors (torch); counts the tokens it chose since the last reset."""
        self.lib._check(self.lib.c.bitnet_hip_sample_dev(self.h, _ptr(logits), logits.numel(), _optr(token), _optr(pos), _optr(history), _optr(n_forced),
                                                         _vp(stream)))


class SampleBatch:
    """One bitnet_hip_sample_batch: up to 8 slots (up to 64 with wide=True), each binding a Sampler and the device tensors sample_dev would
    take; launch() samples for every bound slot in ONE kernel launch, per slot bit for bit what Sampler.sample_dev alone would have left.
    Keeps the bound samplers and tensors alive."""

    def __init__(self, lib: HipLib, vocab: int, n_slots: int, wide: bool = False):
        self.lib, self.vocab, self.n_slots = lib, int(vocab), int(n_slots)
        h = _vp()
        create = lib.c.bitnet_hip_sample_batch_create_wide if wide else lib.c.bitnet_hip_sample_batch_create
        lib._check(create(vocab, n_slots, C.byref(h)))
        self.h = h
        self._keep = {}

    def close(self) -> None:
        if self.h:
            self.lib.c.bitnet_hip_sample_batch_destroy(self.h)
            self.h = None
            self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def set(self, slot: int, sampler: "Sampler | None", logits=None, token=None, pos=None, history=None, n_forced=None) -> None:
        """Bind `sampler` and its device tensors to `slot`, or empty the slot (sampler None).  Synchronous; no launch may be in flight."""
        if sampler is None:
            self.lib._check(self.lib.c.bitnet_hip_sample_batch_set(self.h, slot, None, None, None, None, None, None))
            self._keep.pop(slot, None)
            return
        self.lib._check(self.lib.c.bitnet_hip_sample_batch_set(self.h, slot, sampler.h, _optr(logits), _optr(token), _optr(pos), _optr(history),
                                                               _optr(n_forced)))
        self._keep[slot] = (sampler, logits, token, pos, history, n_forced)

    def launch(self, stream: int = 0) -> None:
        """One kernel launch for every bound slot (asynchronous, capture-safe)."""
        self.lib._check(self.lib.c.bitnet_hip_sample_batch_dev(self.h, _vp(stream)))


STOP_MAX_IDS, STOP_MAX_SEQS, STOP_MAX_SEQ_LEN, STOP_BATCH_MAX = 32, 16, 32, 64
STOP_NONE, STOP_TOKEN, STOP_EOS, STOP_MAX_TOKENS, STOP_SEQUENCE = 0, 1, 2, 3, 4
STOP_REASONS = ("none", "stop_token", "eos", "max_tokens", "sequence")


class StopConfig(C.Structure):
    """bitnet_hip_stop_config.  make() keeps the arrays the pointers refer to alive on the object."""
    _fields_ = [("stop_ids", C.POINTER(C.c_int32)), ("n_stop_ids", _sz), ("eos_id", C.c_int32), ("max_tokens", C.c_int32),
                ("seq_tokens", C.POINTER(C.c_int32)), ("seq_len", C.POINTER(C.c_int32)), ("n_seqs", _sz)]

    @classmethod
    def make(cls, stop_ids=(), eos=None, max_tokens: int = 0, sequences=()) -> "StopConfig":
        """stop_ids: token ids; eos: an id or None; max_tokens: 0 = no budget; sequences: token-id sequences (stop strings as their own
        tokenisation -- a string the model spells across a token boundary differently from it needs the host's check on the decoded text)."""
        ids = _np(np.asarray(list(stop_ids), dtype=np.int64).astype(np.int32), np.int32)
        seqs = [list(map(int, s)) for s in sequences]
        lens = _np(np.asarray([len(s) for s in seqs], dtype=np.int32), np.int32)
        toks = _np(np.asarray([t for s in seqs for t in s], dtype=np.int64).astype(np.int32), np.int32)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None
        cfg = cls(p(ids), ids.size, -1 if eos is None else int(eos), int(max_tokens), p(toks), p(lens), len(seqs))
        cfg._keep = (ids, lens, toks)
        return cfg


class StopState(C.Structure):
    """bitnet_hip_stop_state (24 bytes)"""
    _fields_ = [(n, C.c_int32) for n in ("reason", "index", "token", "position", "generated", "frozen_steps")]

    @property
    def stopped(self) -> bool:
        return self.reason != STOP_NONE

    @property
    def reason_name(self) -> str:
        return STOP_REASONS[self.reason] if 0 <= self.reason < len(STOP_REASONS) else f"reason {self.reason}"

    def astuple(self) -> tuple:
        return tuple(int(getattr(self, n)) for n, _ in self._fields_)

    def __repr__(self) -> str:
        return "StopState(%s)" % ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_)


class Stop:
    """One bitnet_hip_stop: the criteria and the state of one sequence in device memory; launch() is the one launch behind the pick."""

    def __init__(self, lib: HipLib, cfg: "StopConfig | None" = None, **kw):
        self.lib = lib
        h = _vp()
        cfg = StopConfig.make(**kw) if cfg is None else cfg
        lib._check(lib.c.bitnet_hip_stop_create(C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.c.bitnet_hip_stop_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def configure(self, cfg: "StopConfig | None" = None, **kw) -> None:
        cfg = StopConfig.make(**kw) if cfg is None else cfg
        self.lib._check(self.lib.c.bitnet_hip_stop_configure(self.h, C.byref(cfg)))

    def arm(self, keep_generated: bool = False) -> None:
        self.lib._check(self.lib.c.bitnet_hip_stop_arm(self.h, int(keep_generated)))

    def state(self) -> StopState:
        st = StopState()
        self.lib._check(self.lib.c.bitnet_hip_stop_get_state(self.h, C.byref(st)))
        return st

    def launch(self, pos, history, capacity: int, n_forced, token=None, stream: int = 0) -> None:
        """One launch on device tensors (int32): asynchronous, capture-safe."""
        self.lib._check(self.lib.c.bitnet_hip_stop_dev(self.h, _optr(pos), _optr(history), capacity, _optr(n_forced), _optr(token), _vp(stream)))


class StopBatch:
    """One bitnet_hip_stop_batch: up to 64 slots, each binding a Stop and the device tensors launch() would take; launch() serves every
    bound slot in ONE kernel launch, per slot bit for bit what Stop.launch alone leaves.  Keeps the bound objects and tensors alive."""

    def __init__(self, lib: HipLib, n_slots: int):
        self.lib, self.n_slots = lib, int(n_slots)
        h = _vp()
        lib._check(lib.c.bitnet_hip_stop_batch_create(n_slots, C.byref(h)))
        self.h = h
        self._keep = {}

    def close(self) -> None:
        if self.h:
            self.lib.c.bitnet_hip_stop_batch_destroy(self.h)
            self.h = None
            self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def set(self, slot: int, stop: "Stop | None", pos=None, history=None, capacity: int = 0, n_forced=None, token=None) -> None:
        """Bind `stop` and its device tensors to `slot`, or empty the slot (stop None).  Synchronous; no launch may be in flight."""
        if stop is None:
            self.lib._check(self.lib.c.bitnet_hip_stop_batch_set(self.h, slot, None, None, None, 0, None, None))
            self._keep.pop(slot, None)
            return
        self.lib._check(self.lib.c.bitnet_hip_stop_batch_set(self.h, slot, stop.h, _optr(pos), _optr(history), capacity, _optr(n_forced), _optr(token)))
        self._keep[slot] = (stop, pos, history, n_forced, token)

    def launch(self, stream: int = 0) -> None:
        self.lib._check(self.lib.c.bitnet_hip_stop_batch_dev(self.h, _vp(stream)))

    def live(self) -> int:
        """Bound slots that have not stopped yet.  Synchronous."""
        n = C.c_int32(0)
        self.lib._check(self.lib.c.bitnet_hip_stop_batch_live(self.h, C.byref(n)))
        return int(n.value)


BEAM_MAX = 8
BEAM_DONE_POOL, BEAM_DONE_BUDGET, BEAM_ERR_RANGE, BEAM_ERR_SHORT = 1, 2, 0x100, 0x200


class BeamState(C.Structure):
    """bitnet_hip_beam_state (624 bytes)"""
    _fields_ = ([(n, C.c_int32) for n in ("n_beams", "eos", "max_new_tokens", "prompt_pos", "gen_len", "done", "stepped", "n_slots", "pool_n", "pool_seq",
                                          "frozen_steps", "reserved")]
                + [("score", C.c_float * BEAM_MAX), ("parent", C.c_int32 * BEAM_MAX), ("from_", C.c_int32 * BEAM_MAX), ("token", C.c_int32 * BEAM_MAX),
                   ("div", C.c_int32 * BEAM_MAX * BEAM_MAX), ("pool_score", C.c_float * BEAM_MAX), ("pool_key", C.c_float * BEAM_MAX),
                   ("pool_len", C.c_int32 * BEAM_MAX), ("pool_order", C.c_int32 * BEAM_MAX), ("pool_src", C.c_int32 * BEAM_MAX),
                   ("pool_last", C.c_int32 * BEAM_MAX)])

    def words(self) -> list:
        """every 32-bit word of the state in the struct's order, floats as their bits"""
        raw = bytes(self)
        signed, unsigned = np.frombuffer(raw, np.int32), np.frombuffer(raw, np.uint32)
        is_float = lambda i: 12 <= i < 20 or 108 <= i < 124  # score; pool_score and pool_key
        return [int(unsigned[i]) if is_float(i) else int(signed[i]) for i in range(signed.size)]


class BeamMember(C.Structure):
    """bitnet_hip_beam_member: device pointers as integers"""
    _fields_ = [("records_dev", C.c_void_p), ("pos_dev", C.c_void_p), ("history_dev", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


class Beam:
    """One bitnet_hip_beam: the state of one beam search in device memory.  select() is the launch behind a batched step that picks the next
    beams and rewrites the histories; HipLib.kv_permute_dev is the launch behind it that moves the caches."""

    def __init__(self, lib: HipLib, n_beams: int, eos: int, max_new_tokens: int, len_weight):
        self.lib, self.n_beams, self.max_new_tokens = lib, int(n_beams), int(max_new_tokens)
        w = _np(len_weight, np.float32)
        if w.size != self.max_new_tokens + 1:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, f"Beam: len_weight holds {w.size} entries, max_new_tokens + 1 = {self.max_new_tokens + 1} needed")
        h = _vp()
        lib._check(lib.c.bitnet_hip_beam_create(n_beams, eos, max_new_tokens, w.ctypes.data_as(C.c_void_p), C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.c.bitnet_hip_beam_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def reset(self, prompt_pos: int) -> None:
        self.lib._check(self.lib.c.bitnet_hip_beam_reset(self.h, int(prompt_pos)))

    def read(self) -> "tuple[BeamState, np.ndarray]":
        """(state, pool tokens [8][max_new_tokens]); synchronises the device"""
        st, tok = BeamState(), np.zeros((BEAM_MAX, self.max_new_tokens), np.int32)
        self.lib._check(self.lib.c.bitnet_hip_beam_read(self.h, C.byref(st), tok.ctypes.data_as(C.c_void_p)))
        return st, tok

    def done_ptr(self) -> int:
        """The device address of the state's `done` word (a host loop reads these 4 bytes per chunk of queued steps)."""
        p = _vp()
        self.lib._check(self.lib.c.bitnet_hip_beam_done_dev(self.h, C.byref(p)))
        return int(p.value)

    def select(self, members, stream: int = 0) -> None:
        """One launch; members: a device table of n_beams BeamMember (a uint8 tensor holding them, or a raw pointer)."""
        self.lib._check(self.lib.c.bitnet_hip_beam_select_dev(self.h, _optr(members), self.n_beams, _vp(stream)))


_lib = None


def load() -> HipLib:
    """Load libbitnet_hip.so (building nothing: call build() first)."""
    global _lib
    if _lib is None:
        # torch carries its own copy of the HIP runtime; when both it and /opt/rocm's (which this library links) end up in one
        # process the one loaded SECOND finds no device ("no ROCm-capable device is detected").  Loading torch's first makes this
        # library bind to the runtime that is already there -- these bindings use torch for device memory anyway.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = HipLib()
    return _lib


def grammar_prototypes() -> list:
    """The prototypes of include/bitnet_hip_grammar.h, the header include/bitnet_hip.h includes for the sampler's grammar stage."""
    return cproto.prototypes(open(GRAMMAR_HEADER_PATH).read(), "bitnet_hip_")


def kvsnap_prototypes() -> list:
    """The prototypes of include/bitnet_hip_kvsnap.h, the header include/bitnet_hip.h includes for the compact KV snapshots."""
    return cproto.prototypes(open(KVSNAP_HEADER_PATH).read(), "bitnet_hip_")


def beam_prototypes() -> list:
    """The prototypes of include/bitnet_hip_beam.h, the header include/bitnet_hip.h includes for beam search."""
    return cproto.prototypes(open(BEAM_HEADER_PATH).read(), "bitnet_hip_")


def widetail_prototypes() -> list:
    """The prototypes of include/bitnet_hip_widetail.h, the header include/bitnet_hip.h includes for the wide step's 64-entry tail tables."""
    return cproto.prototypes(open(WIDETAIL_HEADER_PATH).read(), "bitnet_hip_")


def declared_symbols() -> list[str]:
    """Every function include/bitnet_hip.h declares, the headers it includes among them (used by the export test)."""
    return sorted({name for name, _, _ in cproto.prototypes(open(HEADER_PATH).read(), "bitnet_hip_") + grammar_prototypes() + kvsnap_prototypes()
                   + widetail_prototypes() + beam_prototypes()})


# ---------------------------------------------------------------------------
# Host decode loop (C++ above the C ABI: bitnet-rs_amd/host/decoder.{hpp,cpp})
# ---------------------------------------------------------------------------

HOST_LIB_PATH = os.path.join(HERE, "libbitnet_host.so")
HOST_HEADER_PATHS = [os.path.join(HERE, "host", f) for f in ("decoder.hpp", "batch_decoder.hpp", "gguf.hpp")]
HOST_GRAMMAR_HEADER_PATH = os.path.join(HERE, "host", "grammar_host.hpp")  # the decoder's grammar control, bound beside the others
HOST_PREFIX_HEADER_PATH = os.path.join(HERE, "host", "prefix_cache.hpp")  # PrefixCache and Decoder::prefill_cached, bound beside the others
HOST_WIDE_HEADER_PATH = os.path.join(HERE, "host", "wide_batch.hpp")  # WideBatch, bound beside the others
HOST_BEAM_HEADER_PATH = os.path.join(HERE, "host", "beam_search.hpp")  # BeamSearch, bound beside the others
_host_libs = {}


def host_prototypes() -> list:
    """Every bitnet_host_* function the extern "C" tails of the host headers declare."""
    return [p for h in HOST_HEADER_PATHS for p in cproto.prototypes(open(h).read(), "bitnet_host_")]


def host_grammar_prototypes() -> list:
    """The three exports of host/grammar_host.hpp (Decoder::set_grammar, set_grammar_state, grammar_state), typed at load like the rest."""
    return cproto.prototypes(open(HOST_GRAMMAR_HEADER_PATH).read(), "bitnet_host_")


def host_prefix_prototypes() -> list:
    """The exports of host/prefix_cache.hpp (PrefixCache, Decoder::prefill_cached), typed at load like the rest."""
    return cproto.prototypes(open(HOST_PREFIX_HEADER_PATH).read(), "bitnet_host_")


def host_wide_prototypes() -> list:
    """The exports of host/wide_batch.hpp (WideBatch), typed at load like the rest."""
    return cproto.prototypes(open(HOST_WIDE_HEADER_PATH).read(), "bitnet_host_")


def host_beam_prototypes() -> list:
    """The exports of host/beam_search.hpp (BeamSearch), typed at load like the rest."""
    return cproto.prototypes(open(HOST_BEAM_HEADER_PATH).read(), "bitnet_host_")


def _host_lib(path: str = HOST_LIB_PATH) -> C.CDLL:
    """The host library at `path`, loaded and bound from its headers once per process."""
    if path not in _host_libs:
        L = C.CDLL(path)
        cproto.bind(L, host_prototypes(), C_STRUCTS)
        cproto.bind(L, host_grammar_prototypes(), C_STRUCTS)
        cproto.bind(L, host_prefix_prototypes(), C_STRUCTS)
        cproto.bind(L, host_wide_prototypes(), C_STRUCTS)
        cproto.bind(L, host_beam_prototypes(), C_STRUCTS)
        _host_libs[path] = L
    return _host_libs[path]


def blake3_hex(data: bytes) -> str:
    """BLAKE3 as the trace records carry it (host/blake3.hpp)."""
    load()
    L = _host_lib()
    out = C.create_string_buffer(65)
    if L.bitnet_host_blake3_hex(data, len(data), out) != 0:
        raise BitNetHipError(ERR_INVALID_ARGUMENT, "blake3_hex failed")
    return out.value.decode()


def host_device_bytes() -> int:
    """Bytes of device memory the process's host decoders and batches own right now (host/dev_buffer.hpp; the weight handles are not counted)."""
    load()
    L = _host_lib()
    return int(L.bitnet_host_device_bytes())


class PrefixStats(C.Structure):
    """bitnet_host_prefix_stats (host/prefix_cache.hpp): the reference's PrefixCacheStats"""
    _fields_ = [("hit_rate", C.c_double), ("miss_rate", C.c_double), ("avg_prefix_match_length", C.c_double), ("eviction_count", C.c_uint64),
                ("memory_usage", C.c_uint64)]


class HostConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden", "n_layers", "n_heads", "n_kv_heads", "head_dim", "ffn", "vocab", "max_pos")] + [
        ("eps", C.c_float),
        ("rope_theta", C.c_float),
    ]


# the structs that cross the C ABI by pointer, by their C names: cproto.bind types such a parameter as POINTER of the class
C_STRUCTS = {"bitnet_hip_device_info": DeviceInfo, "bitnet_hip_gemv_q_geometry_t": GemvQGeometry, "bitnet_hip_gemv_geometry_t": GemvGeometry, "bitnet_hip_sampling_config": SamplingConfig,
             "bitnet_hip_sampling_config_ex": SamplingConfigEx, "bitnet_hip_mirostat_config": MirostatConfig,
             "bitnet_hip_constraints": Constraints, "bitnet_hip_grammar_desc": GrammarDesc, "bitnet_hip_logprob_args": LogprobArgs, "bitnet_hip_stop_config": StopConfig,
             "bitnet_hip_stop_state": StopState, "bitnet_hip_beam_state": BeamState, "bitnet_host_config": HostConfig, "bitnet_host_prefix_stats": PrefixStats}

FLAVORS = ("BitNet32F16", "Split32WithSibling", "GgmlQk256NoScale")


class GgufFile:
    """ctypes view of the C++ GGUF reader (bitnet-rs_amd/host/gguf.cpp): header / KV / tensor
    records, sizes from offsets, I2_S flavour detection.  Pure host code: usable without a GPU."""

    def __init__(self, path: str | None = None, data: bytes | None = None, lib_path: str = HOST_LIB_PATH):
        if not os.path.exists(lib_path):
            raise FileNotFoundError(f"{lib_path} not found: build it with __graft_entry__.build()")
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not found: build it with __graft_entry__.build()")
        C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        L = self.c = _host_lib(lib_path)
        self.h = None
        if path is not None:
            self.h = L.bitnet_host_gguf_open(path.encode())
        elif data is not None:
            self._buf = np.frombuffer(data, np.uint8).copy()  # must outlive the reader
            self.h = L.bitnet_host_gguf_from_memory(self._buf.ctypes.data_as(_u8p), self._buf.size)
        if (path is not None or data is not None) and not self.h:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, self.error() or "GGUF parse failed")

    def error(self) -> str:
        e = self.c.bitnet_host_gguf_error()
        return e.decode(errors="replace") if e else ""

    def close(self) -> None:
        if self.h:
            self.c.bitnet_host_gguf_close(self.h)
            self.h = None

    @property
    def data_start(self) -> int:
        return int(self.c.bitnet_host_gguf_data_start(self.h))

    def tensors(self) -> list:
        out = []
        for i in range(self.c.bitnet_host_gguf_tensor_count(self.h)):
            name = C.create_string_buffer(512)
            shape = (C.c_uint64 * 8)()
            nd, ty, off, size = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
            rc = self.c.bitnet_host_gguf_tensor_info(self.h, i, name, 512, shape, C.byref(nd), C.byref(ty), C.byref(off), C.byref(size))
            if rc != 0:
                raise BitNetHipError(ERR_INVALID_ARGUMENT, self.error())
            out.append({"name": name.value.decode(), "shape": tuple(int(shape[j]) for j in range(nd.value)), "type": ty.value,
                        "offset": off.value, "size": size.value})
        return out

    def config(self) -> dict:
        cfg, f = (C.c_uint64 * 6)(), (C.c_float * 2)()
        if self.c.bitnet_host_gguf_config(self.h, cfg, f) != 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, self.error())
        keys = ("vocab", "hidden", "n_layers", "n_heads", "n_kv_heads", "ffn")
        d = {k: int(cfg[i]) for i, k in enumerate(keys)}
        d["rope_theta"] = None if f[0] != f[0] else float(f[0])
        d["eps"] = None if f[1] != f[1] else float(f[1])
        return d

    def detect_i2s_flavor(self, available: int, nelems: int, has_scale_sibling: bool, strict: bool = False) -> str:
        rc = self.c.bitnet_host_gguf_detect_i2s_flavor(available, nelems, int(has_scale_sibling), int(strict))
        if rc < 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, self.error())
        return FLAVORS[rc]

    def check_projection(self, idx: int, rows: int, cols: int) -> None:
        """The loader's per-projection step without a device (flavour decision, size / bounds checks, codes + scales
        split); raises with the loader's message when the tensor would be refused."""
        if self.c.bitnet_host_gguf_check_projection(self.h, idx, rows, cols) != 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, self.error())

    def loader_is_qk256(self, shape, available: int) -> bool:
        sh = (C.c_uint64 * len(shape))(*shape)
        return bool(self.c.bitnet_host_gguf_loader_is_qk256(sh, len(shape), available))


ScoreResult = collections.namedtuple("ScoreResult", "nll argmax logits ms")


class HostDecoder:
    """ctypes view of the C++ Decoder (mirror of the reference's Rust-side
    TransformerModel / KVCache / greedy loop).  No arithmetic here."""

    def __init__(self, cfg, path: str = HOST_LIB_PATH, _owner: "HostDecoder | None" = None):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: build it with __graft_entry__.build() -- there is no fallback path")
        load()  # the kernel library must be loadable first
        L = self.c = _host_lib(path)
        self.cfg = cfg
        self._top_n = -1  # set_logprobs
        self._fed = 0  # tokens fed since the last reset (the default n of score)
        hc = HostConfig(**{k: (float(v) if k in ("eps", "rope_theta") else int(v)) for k, v in cfg.asdict().items()})
        self.h = L.bitnet_host_create(C.byref(hc)) if _owner is None else L.bitnet_host_create_shared(_owner.h)
        if not self.h:
            raise BitNetHipError(ERR_GPU, "bitnet_host_create failed (allocation)" if _owner is None else "bitnet_host_create_shared: dead or closed owner")
        err = self.error()
        if err:
            self.close()  # a dead decoder (rejected configuration, failed allocation) is destroyed before the error is raised
            raise BitNetHipError(ERR_GPU, err)

    def error(self) -> str:
        e = self.c.bitnet_host_error(self.h)
        return e.decode() if e else ""

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BitNetHipError(rc, self.error() or f"bitnet_host rc={rc}")

    def close(self) -> None:
        if self.h:
            self.c.bitnet_host_destroy(self.h)
            self.h = None

    def shared(self) -> "HostDecoder":
        """A decoder that BORROWS this one's weights (same handles, norm vectors, embedding table): its own KV caches, history, position,
        sampler and stream.  It refuses set_layer_* / set_globals / load_gguf / set_act_mode, and this decoder refuses set_layer_* /
        set_globals while borrowers live.  close() order is free: the library keeps the owner until its last borrower is gone."""
        return HostDecoder(self.cfg, path=self.c._name, _owner=self)

    def set_attention_form(self, form: int) -> None:
        """-1: the attention form follows the position (default); 0: 64-position records + combine at every position, the form a
        HostBatch step runs -- run() under form 0 gives the bits a batch reproduces."""
        self._check(self.c.bitnet_host_set_attention_form(self.h, form))

    def set_head_screen(self, on: bool) -> None:
        """the screened greedy head (default on, env BITNET_HOST_HEAD_SCREEN): plain greedy steps pick their token through the int8 screen
        of the embedding table; off, every step runs the full f16 head.  Same tokens, same last_logits().  Drops the captured graphs."""
        self._check(self.c.bitnet_host_set_head_screen(self.h, 1 if on else 0))

    def head_screen(self) -> int:
        """1: plain greedy steps take the screened head (switched on AND an image exists); 0: they take the full head"""
        return int(self.c.bitnet_host_head_screen(self.h))

    def head_screen_stats(self) -> tuple[int, int, int]:
        """device counters of this decoder's screened head: (rows the last launch rescored from the f16 table, launches so far, rows
        rescored over all launches); (0, 0, 0) while no image exists.  Synchronises."""
        out = (C.c_uint32 * 3)()
        self._check(self.c.bitnet_host_head_screen_stats(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def load_gguf(self, gguf: "GgufFile") -> None:
        self._check(self.c.bitnet_host_load_gguf(self.h, gguf.h))

    def set_layer_qk256(self, layer: int, w: dict) -> None:
        a = [_np(w["attn_norm"], np.float32), _np(w["ffn_norm"], np.float32)] + [_np(w[k], np.uint8) for k in ("q", "k", "v", "o", "gate", "up", "down")]
        self._check(self.c.bitnet_host_set_layer_qk256(self.h, layer, a[0].ctypes.data_as(_f32p), a[1].ctypes.data_as(_f32p), *[x.ctypes.data_as(_u8p) for x in a[2:]]))

    def set_layer_i2s(self, layer: int, w: dict, block: int) -> None:
        names = ("q", "k", "v", "o", "gate", "up", "down")
        ws = [_np(w[k], np.uint8) for k in names]
        ss = [_np(w[k + "_scales"], np.float32) for k in names]
        wp = (_u8p * 7)(*[x.ctypes.data_as(_u8p) for x in ws])
        sp = (_f32p * 7)(*[x.ctypes.data_as(_f32p) for x in ss])
        an, fn = _np(w["attn_norm"], np.float32), _np(w["ffn_norm"], np.float32)
        self._check(self.c.bitnet_host_set_layer_i2s(self.h, layer, an.ctypes.data_as(_f32p), fn.ctypes.data_as(_f32p), wp, sp, block))

    def set_globals(self, g: dict) -> None:
        e, f = _np(g["embed_f16"], np.uint16), _np(g["final_norm"], np.float32)
        self._check(self.c.bitnet_host_set_globals(self.h, e.ctypes.data_as(C.POINTER(C.c_uint16)), f.ctypes.data_as(_f32p)))

    def reset(self) -> None:
        self._check(self.c.bitnet_host_reset(self.h))
        self._fed = 0

    def set_sampling(self, temperature: float | None, top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0,
                     seed: int | None = None, *, min_p: float = 0.0, typical_p: float = 1.0, frequency_penalty: float = 0.0,
                     presence_penalty: float = 0.0) -> None:
        """The reference's Sampler::new(temperature, top_k, top_p, repetition_penalty, seed) behind every with-logits step, on the
        device and inside the captured graphs, with the chain stages of bitnet_hip_sampling_config_ex (off by default).
        set_sampling(None): greedy argmax, as a decoder that never called this.
        seed None: from os.urandom, as the reference seeds from entropy."""
        if temperature is None:
            self._check(self.c.bitnet_host_set_sampling(self.h, None))
            return
        cfg = SamplingConfigEx.make(temperature, top_k, top_p, repetition_penalty, seed, min_p, typical_p, frequency_penalty, presence_penalty)
        self._check(self.c.bitnet_host_set_sampling_ex(self.h, C.byref(cfg)))

    def set_mirostat(self, tau: float | None, eta: float = 0.1) -> None:
        """Mirostat v2 (MirostatSampler::new(tau, eta, ..)) behind every with-logits step, mu on the device and inside the captured graphs.
        Needs set_sampling first, with the truncation stages off; set_mirostat(None): off.  Drops no graphs."""
        if tau is None:
            self._check(self.c.bitnet_host_set_mirostat(self.h, None))
            return
        cfg = MirostatConfig(float(tau), float(eta))
        self._check(self.c.bitnet_host_set_mirostat(self.h, C.byref(cfg)))

    def mirostat_state(self) -> tuple[float, int]:
        """(mu, fallback calls since set_mirostat / reset) of the decoder's sampler; (0.0, 0) without one.  Synchronises."""
        mu, fb = C.c_float(0.0), C.c_uint64(0)
        self._check(self.c.bitnet_host_mirostat_state(self.h, C.byref(mu), C.byref(fb)))
        return float(mu.value), int(fb.value)

    def set_constraints(self, bias=None, allowed=None, hold=(), min_tokens: int = 0, no_repeat_ngram: int = 0, *, off: bool = False, on: bool = False) -> None:
        """Logit constraints behind every with-logits step, on the device and inside the captured graphs and generate()'s queued chunks:
        bias {id: value} (-inf bans), allowed ids (every other id banned), hold ids banned until min_tokens tokens were chosen (an EOS
        hold-off), no_repeat_ngram.  Needs set_sampling first (temperature 0 is greedy).  No arguments, or off=True: off; on=True with no
        arguments: an empty config (nothing is edited, chosen() counts).  Drops no graphs."""
        cfg = Constraints.from_args(bias, allowed, hold, min_tokens, no_repeat_ngram, off, on)
        self._check(self.c.bitnet_host_set_constraints(self.h, C.byref(cfg) if cfg is not None else None))

    def chosen(self) -> int:
        """Tokens the decoder's sampler chose under constraints since its last reset; 0 without a sampler.  Synchronises."""
        g = C.c_uint64(0)
        self._check(self.c.bitnet_host_constraints_state(self.h, C.byref(g)))
        return int(g.value)

    def set_grammar(self, grammar: "Grammar | None", start_state: int = 0) -> None:
        """Decoder::set_grammar: binds a token automaton (lib.grammar(...)) to this decoder's sampler -- sampling must be on; temperature 0 is
        greedy decoding under the grammar -- with its state at start_state; None switches the stage off.  The handle stays the caller's."""
        self._check(_host_fn(self.c, "bitnet_host_set_grammar")(self.h, None if grammar is None else grammar.h, int(start_state)))
        self._grammar = grammar  # kept alive while bound

    def set_grammar_state(self, state: int) -> None:
        """Decoder::set_grammar_state: after rewind(n), the state bitnet_hip_grammar_walk gives for the generated tokens that remain."""
        self._check(_host_fn(self.c, "bitnet_host_set_grammar_state")(self.h, int(state)))

    def grammar_state(self) -> tuple[int, int, int]:
        """(state, steps taken, violations) of the bound grammar; (-1, 0, 0) without a sampler or a grammar.  Synchronises."""
        st, steps, viol = C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
        self._check(_host_fn(self.c, "bitnet_host_grammar_state")(self.h, C.byref(st), C.byref(steps), C.byref(viol)))
        return int(st.value), int(steps.value), int(viol.value)

    def sampling_draws(self) -> int:
        """ChaCha20 words the decoder's sampler has consumed since its last reset / set_sampling (one per non-greedy token)."""
        d = C.c_uint64(0)
        self._check(self.c.bitnet_host_sampling_draws(self.h, C.byref(d)))
        return int(d.value)

    def set_logprobs(self, top_n: int | None) -> None:
        """The reference's logits tap (GenerationConfig::logits_cb / --dump-logit-steps) on the device, inside the captured graphs: with
        top_n = 0..20 every with-logits step leaves one record at the position of the token it placed (chosen or forced) -- the token, its raw
        logit, the row's log-sum-exp and the top_n (id, logit) pairs.  None (or -1): off, as a decoder that never called this."""
        self._top_n = -1 if top_n is None else int(top_n)
        self._check(self.c.bitnet_host_set_logprobs(self.h, self._top_n))

    def logprob_records(self, first: int, n: int) -> np.ndarray:
        """Records [first, first + n) as a structured array of LOGPROB_DTYPE (the raw bytes of bitnet_hip_logprob_record)."""
        out = np.zeros(max(int(n), 0), LOGPROB_DTYPE)
        self._check(self.c.bitnet_host_logprobs(self.h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out

    def logprobs(self, first: int, n: int) -> "Logprobs":
        """Records [first, first + n): token [n] (-1: never written), logit [n], lse [n], logprob [n] (= logit - lse in f32), top_ids and
        top_logits [n, top] with top = the current top_n (finite logits first by descending value, then ascending id)."""
        r = self.logprob_records(first, n)
        top = max(getattr(self, "_top_n", -1), 0)
        with np.errstate(invalid="ignore"):
            lp = (r["logit"] - r["lse"]).astype(np.float32)
        return Logprobs(r["token"].copy(), r["logit"].copy(), r["lse"].copy(), lp, r["top_id"][:, :top].copy(), r["top_logit"][:, :top].copy())

    def set_stop(self, stop_ids=(), eos=None, max_tokens: int = 0, sequences=(), *, off: bool = False) -> None:
        """Stop criteria on the device, behind every with-logits step and inside the captured graphs (the reference's StopCriteria /
        check_stop): stop token ids, an EOS id, a token budget (0 = none; the token that reaches it counts and is the stop token) and stop
        sequences of TOKEN IDS.  The first that holds, in that order, stops the sequence; from then on every step already queued leaves it
        frozen -- position, history, cache slots below the stop position, sampler counts, ChaCha20 counter and Mirostat's mu are those of
        a run that ended on the stop token -- and stop_state() says why and where.  Arms for a new request, as feed() and reset() do.
        Stop STRINGS stay with whoever owns the tokenizer: pass each string as its own tokenisation; a string the model spells across a
        token boundary differently from that tokenisation is not seen here and needs the host's check on the decoded text.
        set_stop(off=True): no criteria, the launch sequence of a decoder that never called this.  An all-default call is the empty config:
        it counts tokens and never stops.  Switching on or off drops the captured graphs; a new config on top of an old one does not."""
        if off:
            self._check(self.c.bitnet_host_set_stop(self.h, None))
            return
        cfg = StopConfig.make(stop_ids, eos, max_tokens, sequences)
        self._check(self.c.bitnet_host_set_stop(self.h, C.byref(cfg)))

    def stop_state(self) -> "StopState":
        """(reason, index, token, position, generated, frozen_steps) of the decoder's criteria.  Synchronises."""
        st = StopState()
        self._check(self.c.bitnet_host_stop_state(self.h, C.byref(st)))
        return st

    def resume(self) -> None:
        """Go on after a stop: the criteria are armed again with the token count kept, the next run() consumes the stop token and generates
        behind it -- the tokens an uninterrupted run would have produced."""
        self._check(self.c.bitnet_host_resume(self.h))

    def generate(self, max_steps: int, chunk: int = 16) -> tuple[int, float]:
        """run(chunk) until the criteria stop the sequence or max_steps steps are queued, with ONE 24-byte state read per chunk instead of a
        token read per step; returns (steps up to and including the stopping one -- max_steps if nothing stopped --, milliseconds).  Up to
        chunk - 1 queued steps run frozen behind the stop (stop_state().frozen_steps)."""
        steps, ms = C.c_int(0), C.c_float(0)
        self._check(self.c.bitnet_host_run_until_stop(self.h, int(max_steps), int(chunk), C.byref(steps), C.byref(ms)))
        return int(steps.value), float(ms.value)

    def graph_nodes(self, with_logits: bool = True) -> int:
        """Kernel nodes of the step graph run() would launch at the current position (captured if need be)."""
        n = int(self.c.bitnet_host_graph_nodes(self.h, int(with_logits)))
        if n < 0:
            raise BitNetHipError(n, self.error() or f"bitnet_host_graph_nodes rc={n}")
        return n

    def feed(self, tokens) -> None:
        t = _np(tokens, np.int32)
        self._check(self.c.bitnet_host_feed(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size))
        self._fed += int(t.size)

    def run(self, n: int, with_logits: bool = True, use_graph: bool = True) -> float:
        ms = C.c_float(0)
        self._check(self.c.bitnet_host_run(self.h, n, int(with_logits), int(use_graph), C.byref(ms)))
        return ms.value

    def set_kv_f16(self, on: bool) -> None:
        """Opt-in f16 KV cache (fresh sequence only)."""
        self._check(self.c.bitnet_host_set_kv_f16(self.h, int(on)))

    def set_act_mode(self, mode: int) -> None:
        """1 (default): activations quantised once by their producer (QAct); 0: exact f32 activations."""
        self._check(self.c.bitnet_host_set_act_mode(self.h, mode))

    def act_mode(self) -> int:
        return int(self.c.bitnet_host_act_mode(self.h))

    def trace_step(self, directory: str, with_logits: bool = True) -> None:
        """One eager step leaving the reference's per-tensor trace records (crates/bitnet-trace) in `directory`."""
        os.makedirs(directory, exist_ok=True)
        self._check(self.c.bitnet_host_trace_step(self.h, directory.encode(), int(with_logits)))

    def prepare_graphs(self, with_logits: bool = True) -> None:
        """capture + instantiate the step graph of every attention form a sequence can reach, ahead of time (nothing executes)"""
        self._check(self.c.bitnet_host_prepare_graphs(self.h, int(with_logits)))

    def run_reference(self, n: int, with_logits: bool = True) -> None:
        """n UNFUSED steps on the bit-exact reference-order kernels (the checker of the fast step; slow)."""
        self._check(self.c.bitnet_host_run_reference(self.h, n, int(with_logits)))

    GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

    def prefill_sharded(self, n: int, rank: int, world: int, gather=None, with_logits: bool = True, digits: int = 3, wire_f16: bool = True,
                        rccl_comm: int | None = None) -> float:
        """Token-parallel prefill of the first n fed tokens: this process is `rank` of `world` (one process per GPU).
        gather(send_ptr, recv_ptr, bytes_per_rank, stream) -> 0 is the all-gather the host supplies (torch.distributed in the
        tests, see prefill_parallel.torch_gather); rccl_comm (an ncclComm_t as int) takes the C entry
        bitnet_host_rccl_allgather instead: the path a Rust host would use, no Python per layer."""
        L = self.c
        ms = C.c_float(0)
        if rccl_comm is not None:
            fn = C.cast(L.bitnet_host_rccl_allgather, C.c_void_p)
            self._check(L.bitnet_host_prefill_sharded(self.h, n, rank, world, fn, C.c_void_p(rccl_comm), int(with_logits), digits, int(wire_f16), C.byref(ms)))
            return ms.value
        cb = None
        if gather is not None:
            def _cb(ctx, send, recv, nbytes, stream):
                try:
                    return int(gather(send, recv, nbytes, stream) or 0)
                except Exception as e:  # noqa: BLE001 -- nothing may propagate through the C frames
                    sys.stderr.write(f"gather callback failed: {e!r}\n")
                    return -1
            cb = self.GATHER_FN(_cb)
        self._check(L.bitnet_host_prefill_sharded(self.h, n, rank, world, C.cast(cb, C.c_void_p) if cb else None, None, int(with_logits), digits,
                                                  int(wire_f16), C.byref(ms)))
        return ms.value

    def set_phase_timing(self, on: bool) -> None:
        """per-phase event timing of the next prefill_sharded calls (8 event records per layer)"""
        self._check(self.c.bitnet_host_set_phase_timing(self.h, int(on)))

    def phase_times(self) -> dict:
        """medians over the layers of the last timed prefill_sharded call, microseconds per layer"""
        out = (C.c_float * 4)()
        self._check(self.c.bitnet_host_phase_times(self.h, out))
        return {"matmul_us": round(out[0], 1), "attention_us": round(out[1], 1), "gather_wait_us": round(out[2], 1), "gather_us": round(out[3], 1)}

    def prefill(self, n: int, with_logits: bool = True, digits: int = 4) -> float:
        ms = C.c_float(0)
        self._check(self.c.bitnet_host_prefill(self.h, n, int(with_logits), digits, C.byref(ms)))
        return ms.value

    def extend(self, n: int, with_logits: bool = True, digits: int = 2) -> float:
        """Prompt forward on a LIVE sequence: history tokens [position, position + n) as [n, *] matrices over the cached positions, at
        prefill speed; ends as prefill ends (position + n, with_logits picks the next token).  At position 0 it is prefill.  After a
        with-logits step the picked token sits unconsumed at history[position()] and feed() writes onto that slot: feed it again in
        front of the new tokens to keep it in the context."""
        ms = C.c_float(0)
        self._check(self.c.bitnet_host_extend(self.h, n, int(with_logits), digits, C.byref(ms)))
        return ms.value

    def prefill_packed(self, members, ns, with_logits: bool = True, digits: int = 2) -> float:
        """ONE prompt forward for up to 64 sequences (this decoder's owner or borrowers of the same weights, the same cache type), member i at
        its own position p_i -- fresh or live -- with ns[i] fed tokens to take in: history tokens [p_i, p_i + ns[i]) of all members go
        through every layer as the rows of one matrix, the attention keeps every member to its own keys and caches, and every member ends as
        its own extend(ns[i], with_logits, digits) would leave it (position p_i + ns[i]; with_logits picks its next token with its own
        argmax or sampler, and its logprob record when on).  This decoder is the driver (its stream, its prompt buffers, its error text, its
        saturation_fallbacks()): `members` starts with it, or it is put in front.  Members may sit in HostBatch slots; run(), extend(),
        fork_into() and the batch step go on afterwards.  Carry-on rule as for extend: after a with-logits pack every member's picked token
        sits unconsumed at history[position()] and feed() writes onto that slot -- feed it again in front of the new tokens to keep it."""
        members = list(members)
        if not members or members[0] is not self:
            members = [self] + members
        ns = _np(ns, np.int32)
        if ns.size != len(members):
            raise BitNetHipError(ERR_INVALID_ARGUMENT, f"prefill_packed: {len(members)} members (the driver included), {ns.size} lengths")
        arr = (C.c_void_p * len(members))(*[m.h if m is not None else None for m in members])
        ms = C.c_float(0)
        self._check(self.c.bitnet_host_prefill_packed(arr, ns.ctypes.data_as(C.POINTER(C.c_int32)), len(members), int(with_logits), digits, C.byref(ms)))
        return ms.value

    def step_wide(self, members, n: int = 1, digits: int = 2) -> float:
        """n decode steps for up to 64 live sequences (this decoder's owner or borrowers of the same weights, the same cache type) through ONE
        matrix forward per step: the members' current tokens are the dense rows of one matrix, every weight matrix is read once on the
        many-row matmuls, each row attends over its own cache, one pass over the embedding table gives every member's logits.  Every member
        ends as its own n x extend(1, True, digits) would leave it (same arithmetic class, not the same bits): position + n, last_logits(),
        its own greedy pick or sampler draw, its logprob records.  This decoder is the driver (its stream, its prompt buffers, its error
        text, its saturation_fallbacks()): `members` starts with it, or it is put in front.  Members may sit in HostBatch slots."""
        members = list(members)
        if not members or members[0] is not self:
            members = [self] + members
        arr = (C.c_void_p * len(members))(*[m.h if m is not None else None for m in members])
        ms = C.c_float(0)
        self._check(self.c.bitnet_host_step_wide(arr, len(members), n, digits, C.byref(ms)))
        return ms.value

    def rewind(self, n: int) -> None:
        """Keep the first n positions (0 <= n <= position()): the next feed() writes at n.  The cache bytes and the sampler state stay."""
        self._check(self.c.bitnet_host_rewind(self.h, n))
        self._fed = min(self._fed, int(n))

    def shift(self, keep: int, discard: int) -> None:
        """Context shift: keep the first `keep` positions, discard the next `discard`, slide the rest down (keep >= 0, discard >= 1,
        keep + discard <= position()).  One launch moves every layer's cache slots in place -- V bit for bit, K re-rotated to its new
        position -- and the position, history, forced count and log-probability records follow; the sampler state, last_logits() and the
        captured graphs stay.  A sequence at the end of its cache goes on after shift(4, position() // 2) instead of reset() + a prompt
        forward over what it wants to keep.  Never automatic: the overflow refusals stay."""
        self._check(self.c.bitnet_host_shift(self.h, int(keep), int(discard)))
        f, k, d = self._fed, int(keep), int(discard)
        self._fed = f if f <= k else k if f <= k + d else f - d

    def fork_into(self, dsts, n: int) -> None:
        """Every decoder of `dsts` (1..8 of them: this decoder's owner or borrowers of the same weights, the same cache type, in no batch
        slot) takes over the first n positions, 0 <= n <= position(): it ends as this decoder would after rewind(n) -- position, forced
        count, history[0 .. n], cache slots < n (one copy launch for all destinations), sampler reset -- and this decoder is untouched.
        Best of n: prefill(P) here, fork_into(dsts, P - 1), every destination run(1) under its own seed; with set_logprobs on, best of n
        ranks the candidates by logprobs(P, k).logprob.sum().  Prefix hit: fork at
        cached_prefix(prompt), feed() the rest (it writes at slot n) and extend() over it.  A destination's last_logits() / last_hidden()
        are unspecified until its next with-logits step."""
        dsts = list(dsts)
        arr = (C.c_void_p * max(len(dsts), 1))(*[d.h if d is not None else None for d in dsts])
        self._check(self.c.bitnet_host_fork(self.h, arr, len(dsts), int(n)))
        for d in dsts:
            d._fed = min(self._fed, int(n))

    def fork_from(self, src: "HostDecoder", n: int) -> None:
        """src.fork_into([self], n)"""
        src.fork_into([self], n)

    def prefill_cached(self, cache: "PrefixCache", n: int, with_logits: bool = True, digits: int = 4) -> int:
        """prefill(n) through a PrefixCache, on a fresh sequence: with a hit of length m the entry's first min(m, n - 1) positions are restored
        into this decoder (one launch) and extend() runs over the rest of the prompt -- fork at m, feed, extend, bit for bit; without a hit it
        is prefill(n, with_logits, digits).  Returns the positions restored (0: no hit).  Never inserts: cache.insert(self, n) does.
        A hit is a fork: it also resets this decoder's sampler, clears its logprob records and zeroes tokens fed beyond n, which a miss
        does not (host/decoder.hpp, prefill_cached): feed exactly n tokens and set the sampler up afterwards for one outcome."""
        hit, ms = C.c_int(0), C.c_float(0)
        self._check(_prefix_fn(self.c, "bitnet_host_prefill_cached")(self.h, cache.h, int(n), int(with_logits), int(digits), C.byref(hit), C.byref(ms)))
        return int(hit.value)

    def cached_prefix(self, tokens) -> int:
        """Length of the longest common prefix of `tokens` and this sequence's consumed history (the reference's PrefixCache lookup)."""
        t = _np(tokens, np.int32)
        n = int(self.c.bitnet_host_cached_prefix(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size))
        if n < 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, self.error() or "bitnet_host_cached_prefix failed")
        return n

    def score(self, n: int | None = None, digits: int = 2, logits_rows: int = 0) -> "ScoreResult":
        """Teacher-forced scoring of the first n fed tokens (default: all of them) in one prompt forward: prefill(n, True, digits) as
        it stands -- the decoder ends exactly where that call leaves it -- then the tied head over every row.  nll[r] (f32, n - 1) is
        -log p(token r + 1 | tokens 0..r); argmax (i32, n) the f16 head's greedy token per row (entry n - 1 may differ from the token
        prefill picked in a near-tie); logits: f32 [logits_rows, vocab] or None; ms: prefill + head.  digits = 2 is the prompt forward
        bench.py times."""
        n = self._fed if n is None else int(n)
        nll = np.zeros(max(n - 1, 0), np.float32)
        am = np.zeros(max(n, 0), np.int32)
        lg = np.zeros((logits_rows, self.cfg.vocab), np.float32) if logits_rows > 0 else None
        ms = C.c_float(0)
        self._check(self.c.bitnet_host_score(self.h, n, digits, nll.ctypes.data_as(_f32p), am.ctypes.data_as(C.POINTER(C.c_int32)),
                                             lg.ctypes.data_as(_f32p) if lg is not None else None, logits_rows, C.byref(ms)))
        return ScoreResult(nll, am, lg, ms.value)

    def last_prefill_path(self) -> int:
        """What the last prefill() ran: 0 digit planes (+ f16 hand-over / hybrid o / down), 1 the f16 chain, 2 the QB32 chain."""
        return int(self.c.bitnet_host_last_prefill_path(self.h))

    def saturation_fallbacks(self) -> int:
        """Prompts this decoder repeated on the row-scaled forms because an f16 hand-over value was clamped (bitnet_hip_f16_saturations)."""
        return int(self.c.bitnet_host_saturation_fallbacks(self.h))

    def position(self) -> int:
        return int(self.c.bitnet_host_position(self.h))

    def form_at(self, pos: int) -> int:
        """attention form of a step at `pos`: 0 records + combine, 1 / 3 the o-projection merges 4 / 8 records, 2 128-position records"""
        return int(self.c.bitnet_host_form_at(self.h, pos))

    def history(self, n: int) -> np.ndarray:
        out = np.zeros(n, np.int32)
        self._check(self.c.bitnet_host_history(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return out

    def last_logits(self) -> np.ndarray:
        out = np.zeros(self.cfg.vocab, np.float32)
        self._check(self.c.bitnet_host_last_logits(self.h, out.ctypes.data_as(_f32p)))
        return out

    def last_hidden(self) -> np.ndarray:
        out = np.zeros(self.cfg.hidden, np.float32)
        self._check(self.c.bitnet_host_last_hidden(self.h, out.ctypes.data_as(_f32p)))
        return out

    def probe_gateup(self, reps: int):
        us, b = C.c_float(0), C.c_double(0)
        self._check(self.c.bitnet_host_probe_gateup(self.h, reps, C.byref(us), C.byref(b)))
        return us.value, b.value

    def probe_kernel(self, kind: int, reps: int):
        us, b = C.c_float(0), C.c_double(0)
        self._check(self.c.bitnet_host_probe_kernel(self.h, kind, reps, C.byref(us), C.byref(b)))
        return us.value, b.value

    def weight_bytes(self) -> int:
        return int(self.c.bitnet_host_weight_bytes(self.h))


def _host_fn(host: C.CDLL, name: str):
    """An export of host/grammar_host.hpp, host/wide_batch.hpp or host/beam_search.hpp on the bound host library.  By name, as _prefix_fn:
    these are typed from THOSE headers at load (host_grammar_prototypes, host_wide_prototypes, host_beam_prototypes), not from the three
    headers host_prototypes() reads."""
    return getattr(host, name)


def _prefix_fn(host: C.CDLL, name: str):
    """An export of host/prefix_cache.hpp on the bound host library.  By name: these are typed from THAT header at load (host_prefix_prototypes),
    not from the three headers host_prototypes() reads."""
    return getattr(host, name)


class PrefixCache:
    """ctypes view of the C++ PrefixCache (host/prefix_cache.hpp): the reference's prompt prefix cache (crates/bitnet-inference/src/
    prefix_cache.rs: trie, longest-prefix lookup, LRU / LFU / FIFO / TTL eviction under an entry limit and a byte limit, statistics) with each
    cached state ONE compact device snapshot -- the first n positions of every layer's K and V, nothing of max_pos -- instead of host bytes.
    insert() saves a prefix of a live decoder (one launch), lookup() is host only, restore() puts an entry into up to 8 decoders (one launch),
    each left as fork_into from the source at insert time would have left it.  The defaults are the reference's.  No arithmetic here."""

    POLICIES = {"lru": 0, "lfu": 1, "fifo": 2, "ttl": 3}

    def __init__(self, max_entries: int = 1024, max_memory_bytes: int = 512 * 1024 * 1024, policy: str = "lru", min_prefix_length: int = 4,
                 ttl_seconds: int = 3600, path: str = HOST_LIB_PATH):
        load()
        self.c = _host_lib(path)
        if policy not in self.POLICIES:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, f"PrefixCache: policy must be one of {sorted(self.POLICIES)}, got {policy!r}")
        self.h = self._f("create")(int(max_entries), int(max_memory_bytes), self.POLICIES[policy], int(min_prefix_length), int(ttl_seconds))
        if not self.h:
            raise BitNetHipError(ERR_GPU, "bitnet_host_prefix_cache_create failed")

    def _f(self, name: str):
        return _prefix_fn(self.c, "bitnet_host_prefix_cache_" + name)

    def error(self) -> str:
        e = self._f("error")(self.h)
        return e.decode() if e else ""

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BitNetHipError(rc, self.error() or f"bitnet_host_prefix_cache rc={rc}")

    def close(self) -> None:
        if self.h:
            self._f("destroy")(self.h)
            self.h = None

    def insert(self, dec: "HostDecoder", n: int, now: int | None = None) -> int:
        """Caches the first n positions of `dec` (0 < n <= position()) under its first n tokens: one save launch into a snapshot of
        lib.kv_snapshot_bytes.  Evicts by the policy until both limits hold.  now: a monotonic clock in seconds for the TTL policy
        (default time.monotonic()).  Returns the entry's id."""
        out = C.c_uint64(0)
        self._check(self._f("insert")(self.h, dec.h, int(n), int(time.monotonic() if now is None else now), C.byref(out)))
        return int(out.value)

    def lookup(self, tokens) -> "tuple[int, int] | None":
        """(matched length, id) of the longest entry whose whole key is a prefix of `tokens`, or None.  Host only."""
        t = _np(tokens, np.int32)
        m, i = C.c_int(0), C.c_uint64(0)
        rc = int(self._f("lookup")(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, C.byref(m), C.byref(i)))
        if rc < 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, "bitnet_host_prefix_cache_lookup failed")
        return (int(m.value), int(i.value)) if rc else None

    def restore(self, id: int, dsts, n: int | None = None) -> None:
        """The first n positions of entry `id` (default: all of them) into every decoder of `dsts` (1..8; the refusals are fork_into's): one
        restore launch; each ends as fork_into(dsts, n) from the source at insert time would have left it."""
        dsts = list(dsts)
        arr = (C.c_void_p * max(len(dsts), 1))(*[d.h if d is not None else None for d in dsts])
        self._check(self._f("restore")(self.h, int(id), arr, len(dsts), -1 if n is None else int(n)))
        forced = C.c_int(0)
        self._f("entry")(self.h, int(id), None, None, C.byref(forced))  # the forced count the entry carries, as the host layer keeps it
        for d in dsts:
            d._fed = int(forced.value) if n is None else min(int(forced.value), int(n))

    def entry(self, id: int) -> "tuple[int, int]":
        """(positions, snapshot bytes) of entry `id`; raises for an id the cache does not hold"""
        n, b = C.c_int(0), C.c_uint64(0)
        if self._f("entry")(self.h, int(id), C.byref(n), C.byref(b), None) != 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, f"PrefixCache: no entry {id}")
        return int(n.value), int(b.value)

    def invalidate(self, tokens) -> bool:
        t = _np(tokens, np.int32)
        rc = int(self._f("invalidate")(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size))
        if rc < 0:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, "bitnet_host_prefix_cache_invalidate failed")
        return bool(rc)

    def clear(self) -> None:
        self._check(self._f("clear")(self.h))

    def stats(self) -> dict:
        s = PrefixStats()
        self._check(self._f("stats")(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in PrefixStats._fields_}

    def __len__(self) -> int:
        return int(self._f("len")(self.h))


class HostBatch:
    """ctypes view of the C++ BatchDecoder (host/batch_decoder.hpp): up to 8 slots, each holding a HostDecoder -- an owner or decoders from
    owner.shared() -- that take decode steps TOGETHER through one launch chain, each at its own position.  After step(n) every member is
    where its own run(n) under set_attention_form(0) would have left it, bit for bit.  set_slot() between steps is the scheduler."""

    def __init__(self, n_slots: int, path: str = HOST_LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: build it with __graft_entry__.build() -- there is no fallback path")
        load()
        L = self.c = _host_lib(path)
        self.n_slots = n_slots
        self.h = L.bitnet_host_batch_create(n_slots)
        if not self.h:
            raise BitNetHipError(ERR_GPU, "bitnet_host_batch_create failed")
        err = self.error()
        if err:
            self.close()
            raise BitNetHipError(ERR_INVALID_ARGUMENT, err)

    def error(self) -> str:
        e = self.c.bitnet_host_batch_error(self.h)
        return e.decode() if e else ""

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BitNetHipError(rc, self.error() or f"bitnet_host_batch rc={rc}")

    def close(self) -> None:
        if self.h:
            self.c.bitnet_host_batch_destroy(self.h)
            self.h = None

    def set_slot(self, b: int, decoder: "HostDecoder | None") -> None:
        self._check(self.c.bitnet_host_batch_set_slot(self.h, b, None if decoder is None else decoder.h))

    def step(self, n: int = 1, use_graph: bool = True) -> float:
        """n with-logits decode steps for every occupied slot; returns the elapsed milliseconds (HIP events)."""
        ms = C.c_float(0.0)
        self._check(self.c.bitnet_host_batch_step(self.h, n, int(use_graph), C.byref(ms)))
        return float(ms.value)

    def live(self) -> int:
        """Members with stop criteria (HostDecoder.set_stop) that have not stopped yet.  Synchronises."""
        n = int(self.c.bitnet_host_batch_live(self.h))
        if n < 0:
            raise BitNetHipError(n, self.error() or f"bitnet_host_batch_live rc={n}")
        return n

    def step_until(self, max_steps: int, chunk: int = 16) -> tuple[int, float]:
        """step(chunk) until no member with stop criteria is live or max_steps steps are queued; one 4-byte read per chunk.  A stopped member
        stays frozen in its slot.  Returns (steps queued, milliseconds)."""
        steps, ms = C.c_int(0), C.c_float(0.0)
        self._check(self.c.bitnet_host_batch_step_until(self.h, int(max_steps), int(chunk), C.byref(steps), C.byref(ms)))
        return int(steps.value), float(ms.value)

    def captures(self) -> int:
        """Graph captures so far: one for a batch's life, two if its first sampling member arrived after an all-greedy capture."""
        return int(self.c.bitnet_host_batch_captures(self.h))

    def graph_nodes(self) -> int:
        """Kernel nodes of the captured chain, 0 if none is held."""
        return int(self.c.bitnet_host_batch_graph_nodes(self.h))


class HostBeamSearch:
    """ctypes view of the C++ BeamSearch (host/beam_search.hpp): beam search over the first n_beams slots of a HostBatch -- plain greedy members
    of one owner, brought to one position with identical prefixes (prefill one, fork_into the others).  Per token: the batched step, one select
    launch (the rule of include/bitnet_hip_beam.h) and one launch that moves the beams' caches in place; the host reads 4 bytes per chunk.
    After run() the live beams are live sequences: HostBatch.step, run and fork_into go on from them.  No arithmetic here."""

    def __init__(self, batch: "HostBatch", n_beams: int, eos: int, max_new_tokens: int, alpha: float = 0.0):
        load()
        self.c, self.batch = batch.c, batch
        self.n_beams, self.max_new_tokens = int(n_beams), int(max_new_tokens)
        self.h = self._b("create")(batch.h, int(n_beams), int(eos), int(max_new_tokens), float(alpha))
        if not self.h:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, "bitnet_host_beam_create failed")
        err = self.error()
        if err:
            self.close()
            raise BitNetHipError(ERR_INVALID_ARGUMENT, err)

    def _b(self, name: str):
        return _host_fn(self.c, "bitnet_host_beam_" + name)

    def error(self) -> str:
        e = self._b("error")(self.h)
        return e.decode() if e else ""

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BitNetHipError(rc, self.error() or f"bitnet_host_beam rc={rc}")

    def close(self) -> None:
        if self.h:
            self._b("destroy")(self.h)
            self.h = None

    def start(self) -> None:
        """A new search from the members' common position; refuses members at different positions or with different prefixes."""
        self._check(self._b("start")(self.h))

    def run(self, chunk: int = 8) -> "tuple[int, float]":
        """Queues chunk x {step, select, permute} and reads `done`, until the search is done.  Returns (steps queued, milliseconds of the steps)."""
        steps, ms = C.c_int(0), C.c_float(0.0)
        self._check(self._b("run")(self.h, int(chunk), C.byref(steps), C.byref(ms)))
        return int(steps.value), float(ms.value)

    def state(self) -> BeamState:
        st = BeamState()
        self._check(self._b("state")(self.h, C.byref(st)))
        return st

    def hypotheses(self) -> list:
        """The pool by descending key, then insertion order: [(tokens, score, key)], score and key as numpy float32."""
        n = C.c_int(0)
        lens, tok = np.zeros(BEAM_MAX, np.int32), np.zeros((BEAM_MAX, self.max_new_tokens), np.int32)
        scores, keys = np.zeros(BEAM_MAX, np.float32), np.zeros(BEAM_MAX, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._b("hypotheses")(self.h, C.byref(n), p(lens), p(tok), p(scores), p(keys)))
        return [([int(t) for t in tok[i, :lens[i]]], scores[i], keys[i]) for i in range(int(n.value))]

    def len_weights(self) -> np.ndarray:
        """The length weights the search passes to the device: [max_new_tokens + 1] float32, len ** -alpha."""
        out = np.zeros(self.max_new_tokens + 1, np.float32)
        self._check(self._b("len_weights")(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out


class HostWideBatch:
    """ctypes view of the C++ WideBatch (host/wide_batch.hpp): up to 64 slots, each holding a HostDecoder -- an owner or decoders from
    owner.shared() -- stepped TOGETHER through the wide forward (one matrix forward per step) with at most one sampling, one tap and one stop
    launch per step.  After step(n) every member is bit for bit what HostDecoder.step_wide of the occupied, un-parked slots in slot order
    leaves on twins.  set_slot() between steps is the scheduler; step_until() parks the members it finds stopped.  Admission: feed() the
    prompt, ONE prefill_packed of n - 1 tokens without logits over the newcomers, set_slot() -- the next step picks the first token."""

    def __init__(self, n_slots: int, path: str = HOST_LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: build it with __graft_entry__.build() -- there is no fallback path")
        load()
        self.c = _host_lib(path)
        self.n_slots = int(n_slots)
        self.h = self._w("create")(self.n_slots)
        if not self.h:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, f"bitnet_host_wide_batch_create: n_slots must be in 1..64, got {n_slots}")

    def _w(self, name: str):
        return _host_fn(self.c, "bitnet_host_wide_batch_" + name)

    def error(self) -> str:
        e = self._w("error")(self.h)
        return e.decode() if e else ""

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BitNetHipError(rc, self.error() or f"bitnet_host_wide_batch rc={rc}")

    def close(self) -> None:
        if self.h:
            self._w("destroy")(self.h)
            self.h = None

    def set_slot(self, b: int, decoder: "HostDecoder | None") -> None:
        """Put `decoder` into slot b or clear it (None); clears the slot's parked mark.  A closed decoder is refused (its handle is gone)."""
        if decoder is not None and not decoder.h:
            raise BitNetHipError(ERR_INVALID_ARGUMENT, "wide batch: null member (a closed decoder)")
        self._check(self._w("set_slot")(self.h, int(b), None if decoder is None else decoder.h))

    def step(self, n: int = 1, digits: int = 2) -> float:
        """n wide steps for the occupied, un-parked slots; returns the elapsed milliseconds (HIP events)."""
        ms = C.c_float(0.0)
        self._check(self._w("step")(self.h, int(n), int(digits), C.byref(ms)))
        return float(ms.value)

    def live(self) -> int:
        """Un-parked members with stop criteria (HostDecoder.set_stop) that have not stopped yet.  Synchronises."""
        n = int(self._w("live")(self.h))
        if n < 0:
            raise BitNetHipError(n, self.error() or f"bitnet_host_wide_batch_live rc={n}")
        return n

    def step_until(self, max_steps: int, chunk: int = 16, digits: int = 2) -> tuple[int, float]:
        """step(chunk) until no un-parked member with stop criteria is live or max_steps steps are queued; the members' stop states are read
        once per chunk and a member found stopped is parked: frozen in its slot, no row in later chunks.  Returns (steps queued, ms)."""
        steps, ms = C.c_int(0), C.c_float(0.0)
        self._check(self._w("step_until")(self.h, int(max_steps), int(chunk), int(digits), C.byref(steps), C.byref(ms)))
        return int(steps.value), float(ms.value)

    def tail_launches(self) -> tuple[int, int, int]:
        """(sampling, tap, stop) launches the last step() call issued."""
        out = (C.c_int * 3)()
        self._check(self._w("tail_launches")(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def table_writes(self) -> int:
        """Uploads of a tail table or the pointer tables since creation: a step with nothing changed adds none."""
        return int(self._w("table_writes")(self.h))
