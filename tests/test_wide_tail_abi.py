"""CPU: the wide step's tail -- bitnet_hip_sample_batch_create_wide and bitnet_hip_logprob_rows_dev (include/bitnet_hip_widetail.h), the
sampler and tap tables at 64 entries -- and the host layer's WideBatch shim (host/wide_batch.hpp) are exported, declared and typed at load,
and refuse bad arguments before anything touches a device.  The 8-slot entries keep their own bound (tests/test_sample_batch_abi.py,
tests/test_logprob_abi.py).  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ENTRIES = {"bitnet_hip_sample_batch_create_wide": 3, "bitnet_hip_logprob_rows_dev": 4}
HOST_ENTRIES = {"bitnet_host_wide_batch_create": 1, "bitnet_host_wide_batch_destroy": 1, "bitnet_host_wide_batch_error": 1, "bitnet_host_wide_batch_set_slot": 3,
                "bitnet_host_wide_batch_step": 4, "bitnet_host_wide_batch_live": 1, "bitnet_host_wide_batch_step_until": 6,
                "bitnet_host_wide_batch_tail_launches": 2, "bitnet_host_wide_batch_table_writes": 1}
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg._load_build_module().build()  # by path, as pkg.build() does
    return pkg.load()


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_and_declared_in_the_included_header(pkg, lib):
    declared, have = set(pkg.declared_symbols()), exported(lib.path)
    assert sorted(p[0] for p in pkg.widetail_prototypes()) == sorted(ENTRIES)
    for name in ENTRIES:
        assert name in declared and name in have, name
    main = open(pkg.HEADER_PATH).read()
    assert re.search(r'^#include "bitnet_hip_widetail\.h"', main, re.M)
    assert not [n for n in ENTRIES if re.search(rf"\b{n}\s*\(", re.sub(r"/\*.*?\*/", " ", main, flags=re.S))]  # declared there, and only there
    host = exported(pkg.HOST_LIB_PATH)
    assert sorted(p[0] for p in pkg.host_wide_prototypes()) == sorted(HOST_ENTRIES)
    for name in HOST_ENTRIES:
        assert name in host, name


def test_every_new_binding_is_typed_at_load(pkg, lib):
    for name, n in ENTRIES.items():
        fn = getattr(lib.c, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n and fn.restype is C.c_int, name
    assert lib.c.bitnet_hip_logprob_rows_dev.argtypes == [C.POINTER(pkg.LogprobArgs), C.c_size_t, C.c_size_t, C.c_void_p]
    host = pkg._host_lib()
    for name, n in HOST_ENTRIES.items():
        fn = getattr(host, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    assert host.bitnet_host_wide_batch_create.restype is C.c_void_p and host.bitnet_host_wide_batch_error.restype is C.c_char_p
    assert host.bitnet_host_wide_batch_destroy.restype is None and host.bitnet_host_wide_batch_table_writes.restype is C.c_int64
    for method in ("set_slot", "step", "live", "step_until", "tail_launches", "table_writes", "close"):
        assert callable(getattr(pkg.HostWideBatch, method)), method
    for method in ("set_grammar", "set_grammar_state", "grammar_state"):
        assert callable(getattr(pkg.HostDecoder, method)), method
    assert hasattr(pkg.HipLib, "logprob_rows_dev") and "wide" in pkg.HipLib.sample_batch.__code__.co_varnames


def test_create_wide_refuses_bad_arguments_without_a_device(lib):
    c, err = lib.c, lib.last_error
    out = C.c_void_p(0x1234)
    assert c.bitnet_hip_sample_batch_create_wide(1000, 4, None) == INVALID and "Null pointer" in err()
    for vocab in (0, (1 << 20) + 1):
        assert c.bitnet_hip_sample_batch_create_wide(vocab, 4, C.byref(out)) == INVALID and "vocab must be in 1..1048576" in err(), vocab
        assert out.value is None  # *out is cleared on every refusal
    for n_slots in (0, 65):
        out = C.c_void_p(0x1234)
        assert c.bitnet_hip_sample_batch_create_wide(1000, n_slots, C.byref(out)) == INVALID, n_slots
        assert "n_slots" in err() and "64" in err() and out.value is None, (n_slots, err())


def test_nine_and_sixty_four_slots_pass_the_argument_checks(lib):
    """whatever a box without a device answers (a table with one), it is not the n_slots refusal; the 8-slot entry still refuses 9"""
    c = lib.c
    for n_slots in (9, 64):
        out = C.c_void_p()
        rc = c.bitnet_hip_sample_batch_create_wide(1000, n_slots, C.byref(out))
        assert rc != INVALID and (rc != 0 or out.value), (n_slots, rc, lib.last_error())
        assert rc == 0 or "n_slots" not in lib.last_error(), lib.last_error()
        if rc == 0:
            c.bitnet_hip_sample_batch_destroy(out)
    out = C.c_void_p()
    assert c.bitnet_hip_sample_batch_create(1000, 9, C.byref(out)) == INVALID and "n_slots must be in 1..8" in lib.last_error()


def test_logprob_rows_dev_refuses_bad_arguments_without_a_device(pkg, lib):
    c, err = lib.c, lib.last_error
    table = (pkg.LogprobArgs * 64)()  # host memory: every refusal below comes before the table is looked at
    assert c.bitnet_hip_logprob_rows_dev(None, 4, 1000, None) == INVALID and "Null table" in err()
    for n_slots in (0, 65):
        assert c.bitnet_hip_logprob_rows_dev(table, n_slots, 1000, None) == INVALID, n_slots
        assert "n_slots" in err() and "64" in err(), (n_slots, err())
    for vocab in (0, (1 << 20) + 1):
        assert c.bitnet_hip_logprob_rows_dev(table, 4, vocab, None) == INVALID and "vocab must be in 1..1048576" in err(), vocab
    assert c.bitnet_hip_logprob_batch_dev(table, 9, 1000, None) == INVALID and "1..8" in err()  # the 8-slot entry keeps its bound


def test_host_shim_refuses_bad_slot_counts_and_null_handles(pkg):
    host = pkg._host_lib()
    for n_slots in (0, 65, -1):
        assert not host.bitnet_host_wide_batch_create(n_slots), n_slots
    with pytest.raises(pkg.BitNetHipError, match="n_slots") as e:
        pkg.HostWideBatch(65)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT
    ms, steps, out3 = C.c_float(0), C.c_int(0), (C.c_int * 3)()
    assert host.bitnet_host_wide_batch_set_slot(None, 0, None) == INVALID
    assert host.bitnet_host_wide_batch_step(None, 1, 2, C.byref(ms)) == INVALID
    assert host.bitnet_host_wide_batch_live(None) == INVALID
    assert host.bitnet_host_wide_batch_step_until(None, 4, 2, 2, C.byref(steps), C.byref(ms)) == INVALID
    assert host.bitnet_host_wide_batch_tail_launches(None, out3) == INVALID
    assert host.bitnet_host_wide_batch_table_writes(None) == -1
    assert host.bitnet_host_wide_batch_error(None) == b"null wide batch"
    host.bitnet_host_wide_batch_destroy(None)  # a no-op
    b = host.bitnet_host_wide_batch_create(64)  # a live, empty batch needs no device
    assert b and host.bitnet_host_wide_batch_table_writes(b) == 0
    assert host.bitnet_host_wide_batch_tail_launches(b, None) == INVALID
    assert host.bitnet_host_wide_batch_set_slot(b, 64, None) == INVALID and b"out of range" in host.bitnet_host_wide_batch_error(b)
    assert host.bitnet_host_wide_batch_step(b, 0, 2, None) == INVALID and b"n_steps" in host.bitnet_host_wide_batch_error(b)
    assert host.bitnet_host_wide_batch_step(b, 1, 2, None) == INVALID and b"empty" in host.bitnet_host_wide_batch_error(b)
    assert host.bitnet_host_wide_batch_step_until(b, 4, 2, 2, None, None) == INVALID and b"criteria" in host.bitnet_host_wide_batch_error(b)
    assert host.bitnet_host_wide_batch_live(b) == 0
    host.bitnet_host_wide_batch_destroy(b)
