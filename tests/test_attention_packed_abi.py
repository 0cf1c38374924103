"""CPU: the packed continuation attention (bitnet_hip_attention_packed_dev, its workspace size and its row alignment) and the host
layer's prefill_packed shim are exported, declared and bound, refuse bad arguments before anything touches a device, and size their
workspace monotonically.  No GPU compute here."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

ENTRIES = ("bitnet_hip_attention_packed_row_align", "bitnet_hip_attention_packed_workspace_bytes", "bitnet_hip_attention_packed_dev")
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
PACK_MAX = 64
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_declared_and_typed(pkg, lib):
    have = exported(lib.path)
    for name in ENTRIES:
        assert name in set(pkg.declared_symbols()) and name in have, name
        assert getattr(lib.c, name).argtypes is not None, name
    assert len(lib.c.bitnet_hip_attention_packed_dev.argtypes) == 19 and lib.c.bitnet_hip_attention_packed_dev.restype is C.c_int
    header = open(pkg.HEADER_PATH).read()
    assert re.search(r"#define BITNET_HIP_PACK_MAX 64\b", header)
    assert "bitnet_host_prefill_packed" in exported(pkg.HOST_LIB_PATH)
    fn = pkg._host_lib().bitnet_host_prefill_packed  # typed from host/decoder.hpp when the host library is loaded, never on first use
    assert fn.argtypes is not None and len(fn.argtypes) == 6 and fn.restype is C.c_int
    assert hasattr(pkg.HostDecoder, "prefill_packed")


def test_row_align(lib):
    assert lib.attention_packed_row_align(4, 2) == 64 and lib.attention_packed_row_align(20, 5) == 64
    assert lib.attention_packed_row_align(3, 3) == 128 and lib.attention_packed_row_align(5, 5) == 128
    assert lib.attention_packed_row_align(6, 2) == 128 and lib.attention_packed_row_align(8, 2) == 64
    assert lib.attention_packed_row_align(5, 2) == 0 and lib.attention_packed_row_align(0, 1) == 0 and lib.attention_packed_row_align(4, 0) == 0


def test_workspace_is_monotone_in_every_past_and_len_and_zero_for_invalid_sizes(lib):
    ws = lib.attention_packed_workspace_bytes
    for n_heads, n_kv in ((4, 2), (3, 3), (20, 5)):
        n_rows = 1024
        grid = (0, 1, 63, 64, 65, 200)
        for other in ((0, 1), (100, 64)):
            prev_p = 0
            for past in grid:
                prev_l = 0
                for ln in (1, 2, 63, 64, 65, 130):
                    b = ws(n_heads, n_kv, n_rows, [past, other[0]], [ln, other[1]])
                    assert b > 0 and b >= prev_l, (n_heads, n_kv, past, ln)
                    assert b == ws(n_heads, n_kv, n_rows, [other[0], past], [other[1], ln])  # the table order does not matter
                    prev_l = b
                b = ws(n_heads, n_kv, n_rows, [past, other[0]], [64, other[1]])
                assert b >= prev_p
                prev_p = b
        assert ws(n_heads, n_kv, 2048, [0], [5]) >= ws(n_heads, n_kv, 1024, [0], [5])  # and in the row count
    assert ws(4, 2, 64, [0], [0]) == 0 and ws(4, 2, 64, [-1], [5]) == 0 and ws(4, 2, 0, [0], [5]) == 0
    assert ws(5, 2, 64, [0], [5]) == 0 and ws(0, 2, 64, [0], [5]) == 0 and ws(4, 0, 64, [0], [5]) == 0
    assert ws(4, 2, 64, [1 << 24], [5]) == 0 and ws(4, 2, 1 << 24, [0], [5]) == 0
    assert ws(4, 2, 8192, [0] * (PACK_MAX + 1), [1] * (PACK_MAX + 1)) == 0 and ws(4, 2, 8192, [0] * PACK_MAX, [1] * PACK_MAX) > 0
    assert ws(4, 2, 64, None, None) == 0
    c = lib.c.bitnet_hip_attention_packed_workspace_bytes
    one = (C.c_int32 * 1)(5)
    assert c(4, 2, 64, 1, None, one) == 0 and c(4, 2, 64, 1, one, None) == 0 and c(4, 2, 64, 0, one, one) == 0


def test_packed_attention_refuses_bad_arguments_without_a_device(lib):
    fn = lib.c.bitnet_hip_attention_packed_dev
    err = lib.last_error
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    caches = [C.c_void_p(p.value + 64 * i) for i in range(2 * PACK_MAX + 4)]

    def i32(a):
        return np.ascontiguousarray(a, np.int32).ctypes.data_as(I32P)

    def call(n_seq=2, row0=(0, 64), ln=(5, 64), past=(0, 10), heads=(4, 2), head_dim=128, max_pos=300, n_rows=128, ws_bytes=1 << 40, flags=0, kc=None, vc=None, holes=()):
        kc = [caches[2 * i] for i in range(max(n_seq, 1))] if kc is None else kc
        vc = [caches[2 * i + 1] for i in range(max(n_seq, 1))] if vc is None else vc
        kt, vt = (C.c_void_p * len(kc))(*kc), (C.c_void_p * len(vc))(*vc)
        args = {"qkv": p, "sin": p, "cos": p, "row0": i32(row0), "len": i32(ln), "past": i32(past), "kc": kt, "vc": vt, "ws": p, "out": p}
        for h in holes:
            args[h] = None
        return fn(args["qkv"], n_rows, args["sin"], args["cos"], n_seq, args["row0"], args["len"], args["past"], args["kc"], args["vc"], heads[0], heads[1], head_dim,
                  max_pos, args["ws"], ws_bytes, args["out"], flags, None)

    # every refusal below returns before the workspace size is compared, except the last: a valid table with a huge workspace would launch
    for n_seq in (0, PACK_MAX + 1):
        assert call(n_seq=n_seq, row0=[0] * 65, ln=[1] * 65, past=[0] * 65) == INVALID and "n_seq" in err(), n_seq
    for hole in ("qkv", "sin", "cos", "row0", "len", "past", "kc", "vc", "ws", "out"):
        assert call(holes=(hole,)) == INVALID and "Null pointer" in err(), hole
    assert call(kc=[caches[0], None]) == INVALID and "null cache" in err()
    assert call(vc=[None, caches[3]]) == INVALID and "null cache" in err()
    for ln in ((0, 64), (5, -1)):
        assert call(ln=ln) == INVALID and "len must be at least 1" in err(), ln
    assert call(past=(0, -1)) == INVALID and "negative past" in err()
    assert call(past=(0, 237)) == INVALID and "KV cache overflow" in err()  # 237 + 64 > 300
    assert call(past=(296, 0)) == INVALID and "KV cache overflow" in err()
    for row0 in ((0, 32), (1, 64), (0, -64)):
        assert call(row0=row0) == INVALID and "row alignment" in err(), row0
    assert call(row0=(0, 64), heads=(3, 3)) == INVALID and "row alignment" in err()  # odd groups: 128-row tiles
    assert call(row0=(0, 0)) == INVALID and "overlap" in err()
    assert call(row0=(64, 0), ln=(5, 65)) == INVALID and "overlap" in err()
    assert call(n_rows=127) == INVALID and "beyond n_rows" in err()
    assert call(n_rows=0) == INVALID
    for head_dim in (0, 64, 256):
        assert call(head_dim=head_dim) == INVALID and "head_dim" in err(), head_dim
    for heads in ((5, 2), (4, 0), (0, 2)):
        assert call(heads=heads) == INVALID and "num_key_value_heads" in err(), heads
    assert call(kc=[caches[0], caches[0]]) == INVALID and "share a cache" in err()
    assert call(vc=[caches[1], caches[1]]) == INVALID and "share a cache" in err()
    assert call(kc=[caches[0], caches[1]]) == INVALID and "share a cache" in err()  # segment 1's k cache is segment 0's v cache
    assert call(kc=[caches[0], caches[2]], vc=[caches[0], caches[3]]) == INVALID and "one cache for k and v" in err()
    for flags in (4, 8, -1, 1 | 4):
        assert call(flags=flags) == INVALID and "unknown flag bits" in err(), flags
    need = lib.attention_packed_workspace_bytes(4, 2, 128, [0, 10], [5, 64])
    assert need > 0
    assert call(ws_bytes=need - 1) == INVALID and "workspace too small" in err()
    assert call(ws_bytes=0) == INVALID and "workspace too small" in err()


def test_host_shim_refuses_a_null_driver(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    fn = c.bitnet_host_prefill_packed
    fn.argtypes = [C.POINTER(C.c_void_p), I32P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    fn.restype = C.c_int
    n = (C.c_int32 * 1)(4)
    assert fn(None, n, 1, 1, 2, None) == INVALID
    assert fn((C.c_void_p * 1)(None), n, 1, 1, 2, None) == INVALID
