"""CPU-side checks of bitnet_hip_gemv_attn_merge_rec_q_dev (the merging o-projection with the record bound chosen by the
caller): declared where a host looks for it, and its arguments are validated before any device work."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bitnet_hip_gemv_attn_merge_rec_q_dev", "bitnet_hip_attention_merge_q_max_keys")


@pytest.fixture(scope="module")
def c(pkg):
    pkg.build()
    c = C.CDLL(pkg.load().path)
    c.bitnet_hip_get_last_error.restype = C.c_char_p
    c.bitnet_hip_gemv_attn_merge_rec_q_dev.argtypes = [C.c_uint64, C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
    return c


def test_declared_in_the_header_and_in_integration_md(pkg):
    header = open(os.path.join(ROOT, "include", "bitnet_hip.h")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert re.search(r"pub fn " + name + r"\(", text), name
        assert name in pkg.declared_symbols()
    # the environment variable that carries the record bound is documented with its values
    row = [l for l in text.splitlines() if "BITNET_HOST_ATTN_MERGE" in l and l.startswith("|")]
    assert row and "8" in row[0] and "4" in row[0]


def test_queries_need_no_device(c):
    c.bitnet_hip_attention_merge_q_max_keys.restype = C.c_size_t
    c.bitnet_hip_attention_merge_max_keys.restype = C.c_size_t
    assert c.bitnet_hip_attention_merge_q_max_keys() == 512
    assert c.bitnet_hip_attention_merge_max_keys() == 256


def test_refuses_null_pointers_an_unknown_handle_and_other_record_bounds(c):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    # no QAct destination
    assert c.bitnet_hip_gemv_attn_merge_rec_q_dev(12345, p, 8, 2, 512, p, p, None, None, None, None, 8, None) != 0
    assert b"Null pointer passed to gemv_attn_merge_rec_q_dev" in c.bitnet_hip_get_last_error()
    # a record bound that has no kernel
    for bad in (0, 5, 16):
        assert c.bitnet_hip_gemv_attn_merge_rec_q_dev(12345, p, 8, 2, 512, p, p, None, p, None, None, bad, None) != 0
        assert b"max_records must be 4 or 8" in c.bitnet_hip_get_last_error()
    # an unknown handle, as its sibling says it
    for rec in (4, 8):
        assert c.bitnet_hip_gemv_attn_merge_rec_q_dev(12345, p, 8, 2, 512, p, p, None, p, None, None, rec, None) != 0
        assert b"unknown weights handle" in c.bitnet_hip_get_last_error()
    assert c.bitnet_hip_gemv_attn_merge_rec_q_dev(12345, None, 8, 2, 512, None, None, None, p, None, None, 8, None) != 0
    assert b"unknown weights handle" in c.bitnet_hip_get_last_error()


def test_form_at_refuses_a_dead_decoder(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_create.restype = C.c_void_p
    c.bitnet_host_create.argtypes = [C.POINTER(pkg.HostConfig)]
    c.bitnet_host_form_at.argtypes = [C.c_void_p, C.c_int]
    hc = pkg.HostConfig(hidden=100, n_layers=4, n_heads=4, n_kv_heads=2, head_dim=128, ffn=256, vocab=64, max_pos=32, eps=1e-5, rope_theta=1e4)
    d = c.bitnet_host_create(C.byref(hc))
    assert d and c.bitnet_host_form_at(d, 10) == -1
    c.bitnet_host_destroy.argtypes = [C.c_void_p]
    c.bitnet_host_destroy(d)
