"""CPU: the KV fork entry point (bitnet_hip_kv_fork_dev) and the host layer's fork / cached_prefix shims are exported, declared and bound, and
refuse bad arguments before anything touches a device.  No GPU compute here."""
import ctypes as C
import re
import subprocess

import pytest

ENTRY = "bitnet_hip_kv_fork_dev"
HOST_ENTRIES = ("bitnet_host_fork", "bitnet_host_cached_prefix")
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
KV_F16 = 2    # BITNET_HIP_ATTN_KV_F16


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_and_declared(pkg, lib):
    assert ENTRY in set(pkg.declared_symbols()) and ENTRY in exported(lib.path)
    header = open(pkg.HEADER_PATH).read()
    doc = header[:header.index("int " + ENTRY)][-3000:]
    assert "prefix_cache.rs" in doc and ":173" in doc and ":212" in doc and "cached_state" in doc  # what it replaces in the reference
    assert "DISTINCT" in doc  # source and destination buffers
    host = exported(pkg.HOST_LIB_PATH)
    for name in HOST_ENTRIES:
        assert name in host, name


def test_every_new_binding_is_typed_at_load(pkg, lib):
    """argtypes / restype are set when the library is loaded (or the wrapper constructed), never on first use"""
    fn = getattr(lib.c, ENTRY)
    assert fn.argtypes is not None and len(fn.argtypes) == 12 and fn.restype is C.c_int
    for name, n_args in zip(HOST_ENTRIES, (4, 3)):  # typed from host/decoder.hpp when the host library is loaded
        fn = getattr(pkg._host_lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args and fn.restype is C.c_int, name
    for method in ("fork_into", "fork_from", "cached_prefix"):
        assert hasattr(pkg.HostDecoder, method), method


def test_kv_fork_refuses_bad_arguments_without_a_device(lib):
    c = lib.c
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.last_error()
    fork = c.bitnet_hip_kv_fork_dev
    # (src_k, src_v, dst_k, dst_v, n_layers, n_dst, n_kv_heads, head_dim, max_pos, n_positions, flags, stream)
    for hole in range(4):
        tables = [p, p, p, p]
        tables[hole] = None
        assert fork(*tables, 3, 2, 2, 128, 640, 10, 0, None) == INVALID and "Null pointer" in err(), hole
    assert fork(p, p, p, p, 0, 2, 2, 128, 640, 10, 0, None) == INVALID and "n_layers" in err()
    for n_dst in (0, 9):
        assert fork(p, p, p, p, 3, n_dst, 2, 128, 640, 10, 0, None) == INVALID and "n_dst" in err(), n_dst
    for head_dim in (0, 64, 256):
        assert fork(p, p, p, p, 3, 2, 2, head_dim, 640, 10, 0, None) == INVALID and "head_dim" in err(), head_dim
    assert fork(p, p, p, p, 3, 2, 0, 128, 640, 10, 0, None) == INVALID and "num_key_value_heads" in err()
    assert fork(p, p, p, p, 3, 2, 2, 128, 640, 641, 0, None) == INVALID and "KV cache overflow" in err()
    assert fork(p, p, p, p, 3, 2, 2, 128, 0, 1, KV_F16, None) == INVALID and "KV cache overflow" in err()
    for flags in (1, 4, KV_F16 | 1, -1):
        assert fork(p, p, p, p, 3, 2, 2, 128, 640, 10, flags, None) == INVALID and "flags" in err(), flags
    # sizes whose products wrap size_t (or pass the grid's range) are refused, not multiplied
    big = (1 << 64) - 1
    assert fork(p, p, p, p, 3, 2, 2, 128, big, 10, 0, None) == INVALID and "too large" in err()
    assert fork(p, p, p, p, 3, 2, 1 << 60, 128, 1 << 20, 10, 0, None) == INVALID and "too large" in err()
    assert fork(p, p, p, p, 1 << 40, 2, 1 << 40, 128, 640, 10, 0, None) == INVALID and "too large" in err()
    assert fork(p, p, p, p, 1 << 30, 2, 2, 128, 640, 10, 0, None) == INVALID and "too large" in err()


def test_host_fork_shims_refuse_a_null_decoder(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_fork.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int]
    c.bitnet_host_fork.restype = C.c_int
    c.bitnet_host_cached_prefix.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    c.bitnet_host_cached_prefix.restype = C.c_int
    dsts = (C.c_void_p * 2)()
    toks = (C.c_int32 * 4)(1, 2, 3, 4)
    assert c.bitnet_host_fork(None, dsts, 2, 0) != 0
    assert c.bitnet_host_fork(None, None, 0, 0) != 0
    assert c.bitnet_host_cached_prefix(None, toks, 4) == -1
    assert c.bitnet_host_cached_prefix(None, None, 0) == -1
