"""Read a Decoder's KV cache back from the device (tests only: no library entry is added for it).

caches(dec, cfg, layer) -> (k [slots, kv, D], v [slots, kv, D]) in the cache's own dtype, slots = ceil(max_pos / 64) * 64: the pointers from
bitnet_host_layer_objects (ptrs[2] / ptrs[3]), a device-to-host hipMemcpy through the HIP runtime, and the private layouts decoded by
tests/extend_ref.py.  Each buffer is n_kv * slots * D elements of 4 bytes; an f16 cache uses the first half (Decoder::set_kv_f16).
Every decoder call in question returns synchronised; the device is synchronised here once more before the copy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import extend_ref as er

_rt = None


def runtime():
    global _rt
    if _rt is None:
        _rt = C.CDLL("libamdhip64.so")
        _rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _rt.hipMemcpy.restype = C.c_int
        _rt.hipDeviceSynchronize.restype = C.c_int
    return _rt


def slots(cfg) -> int:
    return er.chunks(cfg.max_pos) * 64


def raw(dec, cfg, layer, f16):
    """-> (flat K, flat V) as the cache's own dtype, in the device's layout"""
    L = dec.c
    L.bitnet_host_layer_objects.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
    L.bitnet_host_layer_objects.restype = None
    hs, ps = (C.c_uint64 * 4)(), (C.c_void_p * 4)()
    L.bitnet_host_layer_objects(dec.h, layer, hs, ps)
    assert ps[2] and ps[3], f"layer {layer}: no cache"
    rt = runtime()
    assert rt.hipDeviceSynchronize() == 0
    elems = cfg.n_kv_heads * slots(cfg) * cfg.head_dim
    out = []
    for p in (ps[2], ps[3]):
        host = np.empty(elems, np.float16 if f16 else np.float32)
        rc = rt.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(p), host.nbytes, 2)  # hipMemcpyDeviceToHost
        assert rc == 0, f"hipMemcpy rc={rc}"
        out.append(host)
    return out[0], out[1]


def caches(dec, cfg, layer, f16=False):
    k, v = raw(dec, cfg, layer, f16)
    return er.decode_k(k, cfg.n_kv_heads, cfg.max_pos, f16), er.decode_v(v, cfg.n_kv_heads, cfg.max_pos, f16)


def all_layers(dec, cfg, f16=False):
    """-> [(k, v)] per layer"""
    return [caches(dec, cfg, l, f16) for l in range(cfg.n_layers)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)
