"""CPU, no GPU: the grammar compiler's entry points (include/bitnet_hip_grammar_compile.h) are exported and bound, and bitnet_hip_vocab_create /
bitnet_hip_grammar_compile refuse every bad argument with its field named before the GPU is touched."""
import ctypes as C
import subprocess

import numpy as np
import pytest

NAMES = ["bitnet_hip_grammar_compile", "bitnet_hip_grammar_info", "bitnet_hip_grammar_read", "bitnet_hip_vocab_create", "bitnet_hip_vocab_destroy"]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg.load()


def test_new_symbols_are_exported_and_bound(lib, pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(p[0] for p in pkg.gramc_prototypes()) == NAMES and set(NAMES) <= exported and set(NAMES) <= set(pkg.declared_symbols())
    assert '#include "bitnet_hip_grammar_compile.h"' in open(pkg.HEADER_PATH).read()
    assert lib.c.bitnet_hip_vocab_create.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert lib.c.bitnet_hip_grammar_compile.argtypes == [C.c_void_p, C.POINTER(pkg.DfaDesc), C.c_int32, C.c_void_p]
    assert lib.c.bitnet_hip_grammar_info.argtypes == [C.c_void_p] * 4 and lib.c.bitnet_hip_grammar_read.argtypes == [C.c_void_p] * 3
    assert lib.c.bitnet_hip_vocab_destroy.restype is None and C.sizeof(pkg.DfaDesc) == 4 * 8
    assert all(hasattr(pkg.Grammar, m) for m in ("info", "tables", "from_handle")) and hasattr(pkg.HipLib, "grammar_compile")
    lib.c.bitnet_hip_vocab_destroy(None)  # as free(NULL)


def u64(*xs):
    return np.array(xs, np.uint64)


VOCAB_REFUSALS = [  # (bytes pointer given, offsets or None, vocab, the field named)
    (False, u64(0, 1), 1, "bytes is NULL"),
    (True, None, 1, "offsets is NULL"),
    (True, u64(0, 1), 0, "vocab must be in"),
    (True, u64(0, 1), (1 << 20) + 1, "vocab must be in"),
    (True, u64(1, 2), 1, "offsets[0]"),
    (True, u64(0, 3, 2), 2, "offsets[2]"),
    (True, u64(0, 1 << 31), 1, "total"),
]


@pytest.mark.parametrize("has_bytes,off,vocab,field", VOCAB_REFUSALS, ids=[r[3] + str(r[2]) for r in VOCAB_REFUSALS])
def test_vocab_create_refusals(lib, pkg, has_bytes, off, vocab, field):
    data, h = (C.c_uint8 * 8)(), C.c_void_p(123)
    rc = lib.c.bitnet_hip_vocab_create(C.cast(data, C.c_void_p) if has_bytes else None, off.ctypes.data if off is not None else None, vocab, C.byref(h))
    assert rc == pkg.ERR_INVALID_ARGUMENT and lib.last_error().startswith("vocab_create:") and field in lib.last_error(), lib.last_error()
    assert not h.value


COMPILE_REFUSALS = [  # (n_states, start, (state, byte, value) written into next or None, the pointer set to NULL or None, the field named)
    (2, 0, None, "next", "next is NULL"),
    (2, 0, None, "accepting", "accepting is NULL"),
    (0, 0, None, None, "n_states must be in 1..65535"),
    (65536, 0, None, None, "n_states must be in 1..65535"),
    (2, 0, (1, 7, 2), None, "next[1][7] is 2"),
    (2, 0, (0, 255, -2), None, "next[0][255] is -2"),
    (2, 2, None, None, "start 2"),
    (2, -1, None, None, "start -1"),
    (2, 0, None, None, "vocab handle is NULL"),  # a valid DFA: the handle is looked at last, eos_id (judged against its size) after it
]


@pytest.mark.parametrize("n,start,edit,null,field", COMPILE_REFUSALS, ids=[r[4] for r in COMPILE_REFUSALS])
def test_grammar_compile_refusals(lib, pkg, n, start, edit, null, field):
    """Every refusal that needs no vocabulary handle (none can exist without a GPU): the DFA is judged first, field by field.  n_states is judged
    before next is read, so the 0- and 65536-state descriptors carry a 2-state table.  eos_id's range is held by the GPU file."""
    nx, acc = np.full((2, 256), -1, np.int32), np.ones(2, np.uint8)
    if edit:
        nx[edit[0], edit[1]] = edit[2]
    d = pkg.DfaDesc(nx.ctypes.data_as(C.POINTER(C.c_int32)), n, start, acc.ctypes.data_as(C.POINTER(C.c_uint8)))
    if null:
        setattr(d, null, None)
    h = C.c_void_p(123)
    assert lib.c.bitnet_hip_grammar_compile(None, C.byref(d), -1, C.byref(h)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.last_error().startswith("grammar_compile:") and field in lib.last_error(), lib.last_error()
    assert not h.value


def test_null_pointers_are_refused(lib, pkg):
    h = C.c_void_p()
    assert lib.c.bitnet_hip_grammar_compile(None, None, -1, C.byref(h)) == pkg.ERR_INVALID_ARGUMENT and "dfa is NULL" in lib.last_error()
    assert lib.c.bitnet_hip_grammar_compile(None, None, -1, None) == pkg.ERR_INVALID_ARGUMENT and "out is NULL" in lib.last_error()
    assert lib.c.bitnet_hip_grammar_info(None, None, None, None) == pkg.ERR_INVALID_ARGUMENT and "grammar is NULL" in lib.last_error()
    assert lib.c.bitnet_hip_grammar_read(None, None, None) == pkg.ERR_INVALID_ARGUMENT and "grammar is NULL" in lib.last_error()
