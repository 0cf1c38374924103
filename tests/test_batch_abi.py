"""CPU: the batched decode entry points (bitnet_hip_*_batch_dev) and the host layer's batch shim are exported, declared and bound, and refuse
bad arguments before anything touches a device.  No GPU compute here."""
import ctypes as C
import re
import subprocess

import pytest

BATCH_ENTRIES = ("bitnet_hip_embed_q_batch_dev", "bitnet_hip_gemv_q_batch_dev", "bitnet_hip_attention_decode_batch_dev", "bitnet_hip_logits_f16_batch_dev")
HOST_ENTRIES = ("bitnet_host_create_shared", "bitnet_host_set_attention_form", "bitnet_host_release", "bitnet_host_batch_create", "bitnet_host_batch_destroy",
                "bitnet_host_batch_error", "bitnet_host_batch_set_slot", "bitnet_host_batch_step")
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg.load()


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_and_declared(pkg, lib):
    declared = set(pkg.declared_symbols())
    have = exported(lib.path)
    for name in BATCH_ENTRIES:
        assert name in declared and name in have, name
    header = open(pkg.HEADER_PATH).read()
    assert re.search(r"#define\s+BITNET_HIP_BATCH_MAX\s+8\b", header)
    host = exported(pkg.HOST_LIB_PATH)
    for name in HOST_ENTRIES:
        assert name in host, name


def test_every_new_binding_is_typed_at_load(pkg, lib):
    """argtypes / restype are set when the library is loaded (or the wrapper constructed), never on first use"""
    for name in BATCH_ENTRIES:
        fn = getattr(lib.c, name)
        assert fn.argtypes is not None and len(fn.argtypes) >= 11 and fn.restype is C.c_int, name
    want = {"bitnet_host_create_shared": C.c_void_p, "bitnet_host_batch_create": C.c_void_p, "bitnet_host_batch_error": C.c_char_p,
            "bitnet_host_release": None, "bitnet_host_batch_destroy": None}  # every other entry returns int
    for name in HOST_ENTRIES:  # typed from host/decoder.hpp / host/batch_decoder.hpp when the host library is loaded
        fn = getattr(pkg._host_lib(), name)
        assert fn.argtypes is not None and fn.restype is want.get(name, C.c_int), name


def test_batch_entry_points_refuse_bad_arguments_without_a_device(lib):
    c = lib.c
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.last_error()
    # n_seq 0 and 9
    for n_seq in (0, 9):
        assert c.bitnet_hip_embed_q_batch_dev(p, p, p, n_seq, 512, 100, p, None, p, None, None) == INVALID and "n_seq" in err()
        assert c.bitnet_hip_gemv_q_batch_dev(12345, n_seq, p, None, None, 0.0, None, 0, p, None, None, None, None) == INVALID and "n_seq" in err()
        assert c.bitnet_hip_attention_decode_batch_dev(p, p, p, p, p, p, n_seq, 4, 2, 128, 320, p, 0, p, p, None) == INVALID and "n_seq" in err()
        assert c.bitnet_hip_logits_f16_batch_dev(p, p, None, 1e-5, 512, 100, n_seq, p, p, 8, None, None, None, None, None) == INVALID and "n_seq" in err()
    # null required pointers
    assert c.bitnet_hip_embed_q_batch_dev(p, None, p, 2, 512, 100, p, None, p, None, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_embed_q_batch_dev(p, p, p, 2, 512, 100, None, None, p, None, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_gemv_q_batch_dev(12345, 2, None, None, None, 0.0, None, 0, p, None, None, None, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_gemv_q_batch_dev(12345, 2, p, None, None, 0.0, None, 0, None, None, None, None, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_gemv_q_batch_dev(12345, 2, p, None, None, 0.0, None, 0, p, None, None, None, None) == INVALID and "unknown weights handle" in err()
    assert c.bitnet_hip_attention_decode_batch_dev(p, p, p, None, p, p, 2, 4, 2, 128, 320, p, 0, p, p, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_attention_decode_batch_dev(p, p, p, p, p, p, 2, 4, 2, 128, 320, p, 0, None, None, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_attention_decode_batch_dev(p, p, p, p, p, p, 2, 4, 2, 128, 320, p, 1, p, p, None) == INVALID and "flags" in err()  # no wide form in a batch
    assert c.bitnet_hip_logits_f16_batch_dev(p, p, None, 1e-5, 512, 100, 2, None, p, 8, None, None, None, None, None) == INVALID and "Null pointer" in err()
    assert c.bitnet_hip_logits_f16_batch_dev(p, p, None, 1e-5, 512, 100, 2, p, None, 8, None, None, None, None, None) == INVALID and "Null pointer" in err()


def test_batched_head_refuses_shapes_it_cannot_launch_without_a_device(lib):
    """hidden outside the instances, more vectors than the LDS holds (152 KiB beside the kernel's static arrays) and a workgroup count outside the
    grid's range: all refused before the launch, with the code and the wording a caller can act on."""
    c = lib.c
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    UNSUPPORTED = -3  # BITNET_HIP_ERR_UNSUPPORTED
    head = lambda hidden, n_seq, n_wg=8: c.bitnet_hip_logits_f16_batch_dev(p, p, None, 1e-5, hidden, 100, n_seq, p, p, n_wg, None, None, None, None, None)
    for n_seq, hidden in ((8, 5120), (5, 8192)):   # 160 KiB each; 8 x 4608 (144 KiB) and 4 x 8192 (128 KiB) are the largest that run
        assert head(hidden, n_seq) == UNSUPPORTED and "do not fit the LDS" in lib.last_error(), (n_seq, hidden)
    for hidden in (768, 8704):
        assert head(hidden, 2) == UNSUPPORTED and f"hidden {hidden} must be a multiple of 512, <= 8192" in lib.last_error(), hidden
    assert head(0, 2) == UNSUPPORTED
    for n_wg in (0, 65536):
        assert head(512, 2, n_wg) == INVALID, n_wg


def test_host_batch_shim_refuses_without_a_device(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_batch_create.restype = C.c_void_p
    c.bitnet_host_batch_create.argtypes = [C.c_int]
    c.bitnet_host_batch_error.restype = C.c_char_p
    c.bitnet_host_batch_error.argtypes = [C.c_void_p]
    c.bitnet_host_batch_destroy.argtypes = [C.c_void_p]
    c.bitnet_host_batch_destroy.restype = None
    c.bitnet_host_batch_set_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    c.bitnet_host_batch_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    c.bitnet_host_create_shared.restype = C.c_void_p
    c.bitnet_host_create_shared.argtypes = [C.c_void_p]
    for n in (0, 9):
        b = c.bitnet_host_batch_create(n)
        assert b and b"1..8 slots" in c.bitnet_host_batch_error(b)
        assert c.bitnet_host_batch_set_slot(b, 0, None) != 0 and c.bitnet_host_batch_step(b, 1, 0, None) != 0  # a dead batch refuses everything
        c.bitnet_host_batch_destroy(b)
    assert c.bitnet_host_batch_set_slot(None, 0, None) != 0 and c.bitnet_host_batch_step(None, 1, 0, None) != 0
    assert c.bitnet_host_create_shared(None) is None
