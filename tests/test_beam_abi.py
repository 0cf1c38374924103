"""CPU: the beam search entry points (include/bitnet_hip_beam.h) and the host layer's BeamSearch exports (host/beam_search.hpp) are exported,
declared and bound; every refusal of the launches and of the state object comes by message before anything touches a device; INTEGRATION.md
spells the entries out for Rust.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ENTRIES = {"bitnet_hip_beam_create": 5, "bitnet_hip_beam_destroy": 1, "bitnet_hip_beam_reset": 2, "bitnet_hip_beam_read": 3, "bitnet_hip_beam_done_dev": 2,
           "bitnet_hip_beam_select_dev": 4, "bitnet_hip_kv_permute_dev": 11}
HOST_ENTRIES = {"bitnet_host_beam_create": 5, "bitnet_host_beam_destroy": 1, "bitnet_host_beam_error": 1, "bitnet_host_beam_start": 1,
                "bitnet_host_beam_run": 4, "bitnet_host_beam_state": 2, "bitnet_host_beam_hypotheses": 6, "bitnet_host_beam_len_weights": 3}
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
KV_F16 = 2    # BITNET_HIP_ATTN_KV_F16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_declared_and_typed_at_load(pkg, lib):
    have = exported(lib.path)
    assert {p[0]: len(p[2]) for p in pkg.beam_prototypes()} == ENTRIES
    for name in ENTRIES:
        assert name in set(pkg.declared_symbols()) and name in have, name
        assert len(getattr(lib.c, name).argtypes) == ENTRIES[name]
        assert getattr(lib.c, name).restype is (None if name.endswith("destroy") else C.c_int), name
    assert '#include "bitnet_hip_beam.h"' in open(pkg.HEADER_PATH).read()
    doc = open(pkg.BEAM_HEADER_PATH).read()
    assert "IN PLACE" in doc and "descending s, then ascending b, then ascending j" in doc and "FROZEN" in doc
    assert C.sizeof(pkg.BeamState) == 4 * (12 + 4 * 8 + 64 + 6 * 8) and C.sizeof(pkg.BeamMember) == 32
    assert pkg.BeamState.done.offset == 20 and pkg.BeamState.score.offset == 48 and pkg.BeamState.div.offset == 48 + 4 * 32
    assert (pkg.BEAM_MAX, pkg.BEAM_DONE_POOL, pkg.BEAM_DONE_BUDGET, pkg.BEAM_ERR_RANGE, pkg.BEAM_ERR_SHORT) == (8, 1, 2, 0x100, 0x200)
    for macro, value in (("BITNET_HIP_BEAM_MAX", "8"), ("BITNET_HIP_BEAM_DONE_POOL", "1"), ("BITNET_HIP_BEAM_DONE_BUDGET", "2"),
                         ("BITNET_HIP_BEAM_ERR_RANGE", "0x100"), ("BITNET_HIP_BEAM_ERR_SHORT", "0x200")):
        assert re.search(rf"#define {macro}\s+{value}\b", doc), macro
    host, hostlib = exported(pkg.HOST_LIB_PATH), pkg._host_lib()
    assert {p[0]: len(p[2]) for p in pkg.host_beam_prototypes()} == HOST_ENTRIES
    for name, n_args in HOST_ENTRIES.items():  # typed from host/beam_search.hpp when the host library is loaded
        assert name in host, name
        assert len(getattr(hostlib, name).argtypes) == n_args, name
    assert hostlib.bitnet_host_beam_state.argtypes == [C.c_void_p, C.POINTER(pkg.BeamState)]
    assert hostlib.bitnet_host_beam_create.restype is C.c_void_p and hostlib.bitnet_host_beam_error.restype is C.c_char_p
    assert hasattr(pkg.HipLib, "kv_permute_dev") and all(hasattr(pkg.Beam, m) for m in ("reset", "read", "select", "done_ptr"))
    assert all(hasattr(pkg.HostBeamSearch, m) for m in ("start", "run", "state", "hypotheses", "len_weights"))
    src = open(pkg.__file__).read()  # every export the package's HostBeamSearch reaches by name is one the header declares
    body = src[src.index("class HostBeamSearch"):src.index("class HostWideBatch")]
    assert {"bitnet_host_beam_" + m for m in re.findall(r'self\._b\("([a-z_]+)"\)', body)} == set(HOST_ENTRIES)


def test_the_launches_refuse_bad_arguments_without_a_device(lib):
    c = lib.c
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p(C.addressof(buf))
    err = lambda: lib.last_error()
    # permute(k, v, beam, n_layers, n_beams, n_kv_heads, head_dim, max_pos, key_bound, flags, stream)
    P = lambda k=p, v=p, beam=None, layers=3, B=4, kv=2, hd=128, mp=640, kb=100, flags=0: c.bitnet_hip_kv_permute_dev(k, v, beam, layers, B, kv, hd, mp, kb,
                                                                                                                      flags, None)
    for hole in ("k", "v"):
        assert P(**{hole: None}) == INVALID and "Null pointer passed to kv_permute_dev" in err(), hole
    assert P(layers=0) == INVALID and "kv_permute_dev: n_layers 0" in err()
    for B in (0, 9):
        assert P(B=B) == INVALID and f"kv_permute_dev: n_beams {B} must be 1..8" in err(), B
    for head_dim in (0, 64, 256):
        assert P(hd=head_dim) == INVALID and f"kv_permute_dev: head_dim {head_dim} unsupported (128)" in err(), head_dim
    assert P(kv=0) == INVALID and "kv_permute_dev: num_key_value_heads 0" in err()
    for flags in (1, 4, KV_F16 | 1, -1):
        assert P(flags=flags) == INVALID and "kv_permute_dev: flags" in err() and "BITNET_HIP_ATTN_KV_F16" in err(), flags
    assert P(kb=641) == INVALID and "KV cache overflow: key_bound 641, max_pos 640" in err()
    assert P(mp=0, kb=1, flags=KV_F16) == INVALID and "KV cache overflow" in err()
    big = (1 << 64) - 1
    assert P(mp=big, kb=10) == INVALID and "too large" in err() and "kv_permute_dev" in err()
    assert P(kv=1 << 60, mp=1 << 20) == INVALID and "too large" in err()
    assert P(layers=1 << 40, kv=1 << 40) == INVALID and "too large" in err()
    assert P(layers=1 << 30) == INVALID and "too large" in err()
    assert P() == INVALID and "Null beam passed to kv_permute_dev" in err()  # every argument good but the state
    # select(beam, members, n_beams, stream)
    S = c.bitnet_hip_beam_select_dev
    assert S(None, None, 4, None) == INVALID and "Null member table passed to beam_select_dev" in err()
    for B in (0, 9):
        assert S(None, p, B, None) == INVALID and f"beam_select_dev: n_beams {B} must be 1..8" in err(), B
    assert S(None, p, 4, None) == INVALID and "Null beam passed to beam_select_dev" in err()


def test_the_state_object_refuses_bad_arguments_without_a_device(lib, pkg):
    c = lib.c
    err = lambda: lib.last_error()
    w = (C.c_float * 8)(*([1.0] * 8))
    h = C.c_void_p()
    create = lambda B=4, eos=-1, max_new=7, lw=w, out=C.byref(h): c.bitnet_hip_beam_create(B, eos, max_new, lw, out)
    assert create(out=None) == INVALID and "Null pointer passed to beam_create" in err()
    for B in (0, 9):
        assert create(B=B) == INVALID and f"beam_create: n_beams {B} must be 1..8" in err(), B
    assert create(eos=-2) == INVALID and "beam_create: eos -2" in err()
    for max_new in (0, (1 << 20) + 1):
        assert create(max_new=max_new) == INVALID and "beam_create: max_new_tokens" in err(), max_new
    assert create(lw=None) == INVALID and "Null len_weight passed to beam_create" in err()
    assert not h.value  # no refusal left an object behind
    st = pkg.BeamState()
    assert c.bitnet_hip_beam_reset(None, 0) == INVALID and "Null beam passed to beam_reset" in err()
    assert c.bitnet_hip_beam_read(None, C.byref(st), None) == INVALID and "Null beam passed to beam_read" in err()
    assert c.bitnet_hip_beam_done_dev(None, C.byref(h)) == INVALID and "Null beam passed to beam_done_dev" in err()
    c.bitnet_hip_beam_destroy(None)


def test_host_shims_refuse_null_handles(pkg):
    h = pkg._host_lib()
    assert h.bitnet_host_beam_create(None, 2, -1, 4, 0.0) is None
    assert h.bitnet_host_beam_start(None) == INVALID and h.bitnet_host_beam_run(None, 1, None, None) == INVALID
    assert h.bitnet_host_beam_state(None, None) == INVALID and h.bitnet_host_beam_len_weights(None, None, 0) == INVALID
    assert h.bitnet_host_beam_hypotheses(None, None, None, None, None, None) == INVALID
    assert h.bitnet_host_beam_error(None) == b"null beam search"
    h.bitnet_host_beam_destroy(None)


def test_integration_md_declares_the_beam_entries_for_rust():
    """every entry of include/bitnet_hip_beam.h is spelt out in INTEGRATION.md's extern "C" block, with the argument count of the C prototype"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    have = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (bitnet_hip_[a-z0-9_]+)\(([^;]*?)\)\s*(?:->[^;]*)?;", text, re.S)}
    for name, n_args in ENTRIES.items():
        assert name in have, name
        assert (0 if not have[name].strip() else have[name].count(":")) == n_args, name
