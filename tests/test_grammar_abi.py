"""CPU, no GPU: the grammar's entry points are exported and bound; bitnet_hip_grammar_create / _walk refuse every bad descriptor with its field
named before the GPU is touched; bitnet_hip_grammar_walk equals the restatement (tests/grammar_ref.py); set_grammar* refuse a NULL sampler.
The descriptor validation and the walk live in host-only code (csrc/grammar_desc.hpp): tests/host/grammar_desc_check.cpp, a stand-alone
program, runs them under the address and undefined-behaviour sanitizers.  Nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grammar_ref as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg.load()


def test_new_symbols_are_exported_and_bound(lib, pkg):
    names = ["bitnet_hip_grammar_create", "bitnet_hip_grammar_destroy", "bitnet_hip_grammar_walk", "bitnet_hip_sampler_set_grammar",
             "bitnet_hip_sampler_set_grammar_state", "bitnet_hip_sampler_grammar_state"]
    declared = pkg.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in names:
        assert n in declared and n in exported and hasattr(lib.c, n), n
        assert getattr(lib.c, n).argtypes is not None, n
        assert getattr(lib.c, n).restype is (None if n.endswith("destroy") else C.c_int), n
    assert lib.c.bitnet_hip_grammar_create.argtypes == [C.POINTER(pkg.GrammarDesc), C.c_void_p]
    assert lib.c.bitnet_hip_grammar_walk.argtypes == [C.POINTER(pkg.GrammarDesc), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert lib.c.bitnet_hip_sampler_set_grammar.argtypes == [C.c_void_p, C.c_void_p, C.c_int32]
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], text=True)
    host = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"bitnet_host_set_grammar", "bitnet_host_set_grammar_state", "bitnet_host_grammar_state"} <= host
    # the six live in a header of their own that include/bitnet_hip.h includes; the host's three in host/grammar_host.hpp; all nine are typed
    # from those headers when the libraries load
    assert '#include "bitnet_hip_grammar.h"' in open(pkg.HEADER_PATH).read()
    assert sorted(p[0] for p in pkg.grammar_prototypes()) == sorted(names)
    assert sorted(p[0] for p in pkg.host_grammar_prototypes()) == ["bitnet_host_grammar_state", "bitnet_host_set_grammar", "bitnet_host_set_grammar_state"]
    hostlib = pkg._host_lib()
    assert hostlib.bitnet_host_set_grammar.argtypes == [C.c_void_p, C.c_void_p, C.c_int] and hostlib.bitnet_host_set_grammar.restype is C.c_int
    assert hostlib.bitnet_host_set_grammar_state.argtypes == [C.c_void_p, C.c_int]
    assert hostlib.bitnet_host_grammar_state.argtypes == [C.c_void_p] * 4
    header = open(pkg.GRAMMAR_HEADER_PATH).read()
    assert "BITNET_HIP_GRAMMAR_MAX_STATES  65536" in header and "BITNET_HIP_GRAMMAR_MAX_CLASSES 16384" in header
    assert "Replaces nothing in the reference" in header
    assert (pkg.GRAMMAR_MAX_STATES, pkg.GRAMMAR_MAX_CLASSES) == (65536, 16384)
    assert C.sizeof(pkg.GrammarDesc) == 5 * 8
    assert all(hasattr(pkg.Sampler, m) for m in ("set_grammar", "set_grammar_state", "grammar_state"))


def bad_descriptors(pkg):
    """name -> (descriptor, the field the refusal must name)"""
    M = pkg.GrammarDesc.make
    good = M([0, 1, 0], [[0, -1], [1, 1]])

    def edit(**kw):
        d = pkg.GrammarDesc(good.token_class, good.vocab, good.next, good.n_states, good.n_classes)
        d._keep = good._keep
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    return {
        "NULL token_class": (edit(token_class=None), "token_class is NULL"),
        "NULL next": (edit(next=None), "next is NULL"),
        "vocab 0": (edit(vocab=0), "vocab"),
        "vocab past 2^20": (edit(vocab=(1 << 20) + 1), "vocab"),
        "n_states 0": (edit(n_states=0), "n_states"),
        "n_states past the maximum": (edit(n_states=65537), "n_states"),
        "n_classes 0": (edit(n_classes=0), "n_classes"),
        "n_classes past the maximum": (edit(n_classes=16385), "n_classes"),
        "the table past 2^24": (edit(n_states=65536, n_classes=257), "n_states * n_classes"),
        "a class id past n_classes": (M([0, 2, 0], [[0, -1], [1, 1]]), "token_class[1]"),
        "a next entry past n_states": (M([0, 1, 0], [[0, -1], [2, 1]]), "next[1][0]"),
        "a next entry below -1": (M([0, 1, 0], [[0, -2], [1, 1]]), "next[0][1]"),
    }


def test_every_refusal_names_its_field_and_comes_without_a_gpu(lib, pkg):
    for name, (d, field) in bad_descriptors(pkg).items():
        h = C.c_void_p(123)
        assert lib.c.bitnet_hip_grammar_create(C.byref(d), C.byref(h)) == pkg.ERR_INVALID_ARGUMENT, name
        msg = lib.last_error()
        assert msg.startswith("grammar_create:") and field in msg, (name, msg)
        assert not h.value, name
        s, k = C.c_int32(-5), C.c_size_t(77)
        assert lib.c.bitnet_hip_grammar_walk(C.byref(d), 0, None, 0, C.byref(s), C.byref(k)) == pkg.ERR_INVALID_ARGUMENT, name
        msg = lib.last_error()
        assert msg.startswith("grammar_walk:") and field in msg, (name, msg)
        assert (s.value, k.value) == (-5, 77), name
    h = C.c_void_p()
    assert lib.c.bitnet_hip_grammar_create(None, C.byref(h)) == pkg.ERR_INVALID_ARGUMENT and "desc is NULL" in lib.last_error()
    good = pkg.GrammarDesc.make([0, 1, 0], [[0, -1], [1, 1]])
    assert lib.c.bitnet_hip_grammar_create(C.byref(good), None) == pkg.ERR_INVALID_ARGUMENT and "out is NULL" in lib.last_error()
    s, k = C.c_int32(0), C.c_size_t(0)
    for state in (-1, 2):
        assert lib.c.bitnet_hip_grammar_walk(C.byref(good), state, None, 0, C.byref(s), C.byref(k)) == pkg.ERR_INVALID_ARGUMENT
        assert "state" in lib.last_error() and "n_states" in lib.last_error()
    assert lib.c.bitnet_hip_grammar_walk(C.byref(good), 0, None, 3, C.byref(s), C.byref(k)) == pkg.ERR_INVALID_ARGUMENT  # a count with no list
    assert lib.c.bitnet_hip_grammar_walk(C.byref(good), 0, None, 0, None, C.byref(k)) == pkg.ERR_INVALID_ARGUMENT
    lib.c.bitnet_hip_grammar_destroy(None)  # as free(NULL)
    with pytest.raises(ValueError, match="class id"):
        pkg.GrammarDesc.make([0, 70000], [[0]])
    with pytest.raises(ValueError, match="n_states, n_classes"):
        pkg.GrammarDesc.make([0], [0, 1])


def test_walk_through_the_abi_equals_the_restatement(lib, pkg):
    rng = np.random.default_rng(4)
    stops_banned = stops_range = 0
    for case in range(50):
        S, C_, V = int(rng.integers(3, 12)), int(rng.integers(1, 50)), int(rng.integers(2, 400))
        desc, single = gr.random_automaton(rng, S, C_, V, 0.3 * float(rng.random()))
        d = pkg.GrammarDesc.make(*desc)
        for s0 in range(S):
            toks = rng.integers(0, V, size=int(rng.integers(0, 16))).tolist()
            if case % 3 == 1 and toks:
                toks[int(rng.integers(0, len(toks)))] = [-1, V, V + 7, (1 << 31) - 1, -(1 << 31)][case % 5]
            want = gr.walk(desc, s0, toks)
            assert pkg.grammar_walk(lib, d, s0, toks) == want, (case, s0, toks)
            if want[1] < len(toks):
                t = toks[want[1]]
                stops_range += not 0 <= t < V
                stops_banned += 0 <= t < V
        # the state that allows one token, and the empty one
        assert pkg.grammar_walk(lib, d, S - 1, [0, 1]) == (S - 1, 0)
        if C_ >= 2:
            other = (single + 1) % V
            s1, k1 = pkg.grammar_walk(lib, d, S - 2, [single, other])
            assert k1 >= 1 and pkg.grammar_walk(lib, d, S - 2, [other, single]) == (S - 2, 0)
    assert stops_banned > 20 and stops_range > 20  # both kinds of stop were met


def test_set_grammar_with_a_null_sampler_is_refused(lib, pkg):
    assert lib.c.bitnet_hip_sampler_set_grammar(None, None, 0) == pkg.ERR_INVALID_ARGUMENT
    assert "Null sampler passed to sampler_set_grammar" in lib.last_error()
    assert lib.c.bitnet_hip_sampler_set_grammar_state(None, 0) == pkg.ERR_INVALID_ARGUMENT
    assert "Null sampler passed to sampler_set_grammar_state" in lib.last_error()
    s, n, v = C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.c.bitnet_hip_sampler_grammar_state(None, C.byref(s), C.byref(n), C.byref(v)) == pkg.ERR_INVALID_ARGUMENT
    assert "Null sampler passed to sampler_grammar_state" in lib.last_error()


def test_grammar_desc_check_under_sanitizers(tmp_path):
    """the stand-alone program: valid descriptors, every invalid one, random walks -- exit 0 and no sanitizer report"""
    exe = str(tmp_path / "grammar_desc_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'bitnet-rs_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "host", "grammar_desc_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "grammar_desc_check: ok" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
