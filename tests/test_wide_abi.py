"""CPU: the wide decode step's three kernel entries (bitnet_hip_embed_rows_dev, bitnet_hip_attention_decode_rows_dev, bitnet_hip_pick_rows_dev)
and the host layer's step_wide shim are exported, declared and bound, and refuse bad arguments before anything touches a device.  No GPU
compute here."""
import ctypes as C
import re
import subprocess

import pytest

ENTRIES = ("bitnet_hip_embed_rows_dev", "bitnet_hip_attention_decode_rows_dev", "bitnet_hip_pick_rows_dev")
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
WIDE_MAX = 64


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
        assert getattr(lib.c, name).argtypes is not None and getattr(lib.c, name).restype is C.c_int, name
        assert hasattr(lib, name[len("bitnet_hip_"):]), name  # the thin wrapper the kernel tests call
    assert len(lib.c.bitnet_hip_embed_rows_dev.argtypes) == 8
    assert len(lib.c.bitnet_hip_attention_decode_rows_dev.argtypes) == 16
    assert len(lib.c.bitnet_hip_pick_rows_dev.argtypes) == 10
    header = open(pkg.HEADER_PATH).read()
    assert re.search(r"#define BITNET_HIP_WIDE_MAX 64\b", header)
    assert re.search(r"#define BITNET_HIP_BATCH_MAX 8\b", header)  # the batched step keeps its width
    assert "bitnet_host_step_wide" in exported(pkg.HOST_LIB_PATH)
    fn = pkg._host_lib().bitnet_host_step_wide  # typed from host/decoder.hpp when the host library is loaded, never on first use
    assert fn.argtypes is not None and len(fn.argtypes) == 5 and fn.restype is C.c_int
    assert hasattr(pkg.HostDecoder, "step_wide")


@pytest.fixture()
def p():
    buf = (C.c_uint8 * 4096)()
    return C.cast(buf, C.c_void_p), buf  # (the buffer is kept alive by the tuple)


def test_embed_rows_refuses_bad_arguments_without_a_device(lib, p):
    fn, err, p = lib.c.bitnet_hip_embed_rows_dev, lib.last_error, p[0]

    def call(n_seq=3, hidden=512, vocab=1000, holes=()):
        a = {"table": p, "hist": p, "pos": p, "x": p}
        for h in holes:
            a[h] = None
        return fn(a["table"], a["hist"], a["pos"], n_seq, hidden, vocab, a["x"], None)

    for n_seq in (0, WIDE_MAX + 1, 1 << 40):
        assert call(n_seq=n_seq) == INVALID and "n_seq" in err(), n_seq
    for hole in ("table", "hist", "pos", "x"):
        assert call(holes=(hole,)) == INVALID and "Null pointer" in err(), hole
    for hidden in (0, 4, 516):
        assert call(hidden=hidden) == INVALID and "multiple of 8" in err(), hidden
    for hidden, vocab in ((512, 0), (512, 1 << 31), (1 << 31, 1000), (1 << 40, 1 << 30)):
        assert call(hidden=hidden, vocab=vocab) == INVALID and "too large" in err(), (hidden, vocab)


def test_attention_decode_rows_refuses_bad_arguments_without_a_device(lib, p):
    fn, err, p = lib.c.bitnet_hip_attention_decode_rows_dev, lib.last_error, p[0]

    def call(n_seq=3, heads=(4, 2), head_dim=128, max_pos=300, key_bound=65, flags=0, holes=()):
        a = {"qkv": p, "sin": p, "cos": p, "kc": p, "vc": p, "pos": p, "scratch": p, "out": p}
        for h in holes:
            a[h] = None
        return fn(a["qkv"], a["sin"], a["cos"], a["kc"], a["vc"], a["pos"], n_seq, heads[0], heads[1], head_dim, max_pos, key_bound, a["scratch"], flags, a["out"],
                  None)

    for n_seq in (0, WIDE_MAX + 1, 1 << 40):
        assert call(n_seq=n_seq) == INVALID and "n_seq" in err(), n_seq
    for hole in ("qkv", "sin", "cos", "kc", "vc", "pos", "scratch", "out"):
        assert call(holes=(hole,)) == INVALID and "Null pointer" in err(), hole
    for flags in (4, 8, -1, 1 | 4, 2 | 16):
        assert call(flags=flags) == INVALID and "unknown flag bits" in err(), flags
    for heads in ((5, 2), (4, 0), (0, 0), (7, 3)):
        assert call(heads=heads) == INVALID and "num_key_value_heads" in err(), heads
    for heads in ((5, 1), (8, 1), (10, 2)):  # a group larger than 4
        assert call(heads=heads) == INVALID and "group" in err(), heads
    for head_dim in (0, 64, 256):
        assert call(head_dim=head_dim) == INVALID and "head_dim" in err(), head_dim
    for max_pos in (0, (1 << 24) + 1, 1 << 40):
        assert call(max_pos=max_pos, key_bound=1) == INVALID and "too large" in err(), max_pos
    assert call(heads=(4096, 4096), max_pos=1 << 24, key_bound=1) == INVALID and "too large" in err()  # one sequence's records beyond 2^31 floats
    for key_bound in (0, 301, 1 << 40):
        assert call(key_bound=key_bound) == INVALID and "key_bound" in err(), key_bound


def test_pick_rows_refuses_bad_arguments_without_a_device(lib, p):
    fn, err, p = lib.c.bitnet_hip_pick_rows_dev, lib.last_error, p[0]

    def call(n_seq=3, vocab=1000, holes=()):
        a = {"logits": p, "argmax": p, "lt": p}
        for h in holes:
            a[h] = None
        return fn(a["logits"], a["argmax"], n_seq, vocab, a["lt"], None, None, None, None, None)

    for n_seq in (0, WIDE_MAX + 1, 1 << 40):
        assert call(n_seq=n_seq) == INVALID and "n_seq" in err(), n_seq
    for hole in ("logits", "argmax", "lt"):
        assert call(holes=(hole,)) == INVALID and "Null pointer" in err(), hole
    for vocab in (0, 1 << 31, 1 << 40):
        assert call(vocab=vocab) == INVALID and "too large" in err(), vocab


def test_host_shim_refuses_a_null_driver(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    fn = c.bitnet_host_step_wide
    fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    fn.restype = C.c_int
    assert fn(None, 1, 1, 2, None) == INVALID
    assert fn((C.c_void_p * 1)(None), 1, 1, 2, None) == INVALID
