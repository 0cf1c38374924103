"""CPU: the context-shift entry point (bitnet_hip_kv_shift_dev) and the host layer's shift shim are exported, declared and bound, and refuse bad
arguments before anything touches a device.  No GPU compute here."""
import ctypes as C
import re
import subprocess

import pytest

ENTRY = "bitnet_hip_kv_shift_dev"
HOST_ENTRY = "bitnet_host_shift"
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
    doc = header[:header.index("int " + ENTRY)][-3500:]
    assert "kv_cache.rs:305-348" in doc and "sliding_window.rs:161-235" in doc  # what it replaces in the reference
    assert "c = ca*cb + sa*sb" in doc and "s = sa*cb - ca*sb" in doc and "x0' = x0*c + x1*s" in doc and "x1' = x1*c - x0*s" in doc
    assert "not row `discard`" in doc
    assert HOST_ENTRY in exported(pkg.HOST_LIB_PATH)


def test_every_new_binding_is_typed_at_load(pkg, lib):
    """argtypes / restype are set when the library is loaded (or the wrapper constructed), never on first use"""
    fn = getattr(lib.c, ENTRY)
    assert fn.argtypes is not None and len(fn.argtypes) == 13 and fn.restype is C.c_int
    fn = getattr(pkg._host_lib(), HOST_ENTRY)  # typed from host/decoder.hpp when the host library is loaded
    assert fn.argtypes is not None and len(fn.argtypes) == 3 and fn.restype is C.c_int
    assert hasattr(pkg.HostDecoder, "shift") and hasattr(pkg.HipLib, "kv_shift_dev")


def test_kv_shift_refuses_bad_arguments_without_a_device(lib):
    c = lib.c
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.last_error()
    shift = c.bitnet_hip_kv_shift_dev
    # (k_ptrs, v_ptrs, rope_sin, rope_cos, n_layers, n_kv_heads, head_dim, max_pos, keep, discard, n_positions, flags, stream)
    for hole in range(4):
        ptrs = [p, p, p, p]
        ptrs[hole] = None
        assert shift(*ptrs, 3, 2, 128, 640, 4, 10, 100, 0, None) == INVALID and "Null pointer" in err(), hole
    assert shift(p, p, p, p, 0, 2, 128, 640, 4, 10, 100, 0, None) == INVALID and "n_layers" in err()
    assert shift(p, p, p, p, 3, 0, 128, 640, 4, 10, 100, 0, None) == INVALID and "num_key_value_heads" in err()
    for head_dim in (0, 64, 256):
        assert shift(p, p, p, p, 3, 2, head_dim, 640, 4, 10, 100, 0, None) == INVALID and "head_dim" in err(), head_dim
    assert shift(p, p, p, p, 3, 2, 128, 640, 4, 0, 100, 0, None) == INVALID and "discard 0" in err()
    for keep, discard, n in ((4, 97, 100), (101, 1, 100), (0, 101, 100), (0, 1, 0)):
        assert shift(p, p, p, p, 3, 2, 128, 640, keep, discard, n, 0, None) == INVALID and "exceeds n_positions" in err(), (keep, discard, n)
    assert shift(p, p, p, p, 3, 2, 128, 640, 4, 10, 641, 0, None) == INVALID and "KV cache overflow" in err()
    assert shift(p, p, p, p, 3, 2, 128, 0, 0, 1, 1, KV_F16, None) == INVALID and "KV cache overflow" in err()
    for flags in (1, 4, KV_F16 | 1, -1):
        assert shift(p, p, p, p, 3, 2, 128, 640, 4, 10, 100, flags, None) == INVALID and "flags" in err(), flags
    # sizes whose sums or products wrap size_t (or pass the grid's range) are refused, not computed with
    big = (1 << 64) - 1
    assert shift(p, p, p, p, 3, 2, 128, 640, big, 2, 100, 0, None) == INVALID and "exceeds n_positions" in err()
    assert shift(p, p, p, p, 3, 2, 128, big, 4, 10, 100, 0, None) == INVALID and "too large" in err()
    assert shift(p, p, p, p, 3, 2, 128, 1 << 31, 4, 10, 100, 0, None) == INVALID and "too large" in err()
    assert shift(p, p, p, p, 3, 1 << 60, 128, 1 << 20, 4, 10, 100, 0, None) == INVALID and "too large" in err()
    assert shift(p, p, p, p, 1 << 40, 1 << 40, 128, 640, 4, 10, 100, 0, None) == INVALID and "too large" in err()
    assert shift(p, p, p, p, 1 << 30, 2, 128, 640, 4, 10, 100, 0, None) == INVALID and "too large" in err()


def test_host_shift_shim_refuses_a_null_decoder(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_shift.argtypes = [C.c_void_p, C.c_int, C.c_int]
    c.bitnet_host_shift.restype = C.c_int
    assert c.bitnet_host_shift(None, 4, 10) != 0
    assert c.bitnet_host_shift(None, 0, 0) != 0
