"""CPU: the C-ABI surface of the device stop criteria (bitnet_hip_stop_*, csrc/kernels_stop.hip).  Every new symbol is declared in the
header, exported by the library and bound by the Python package, and every refusal the header lists that can be reached without a device
object returns BITNET_HIP_ERR_INVALID_ARGUMENT with a text, before the GPU is touched (this file runs without one).  The two refusals
that need live objects -- a slot beyond a table's own size, an object bound to two slots -- are in tests/test_stop_gpu.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

SYMBOLS = ["bitnet_hip_stop_" + s for s in ("create", "destroy", "configure", "arm", "get_state", "dev", "batch_create", "batch_destroy",
                                            "batch_set", "batch_dev", "batch_live")]
HOST_SYMBOLS = ["bitnet_host_" + s for s in ("set_stop", "stop_state", "resume", "run_until_stop", "graph_nodes")]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg._load_build_module().build()  # (not pkg.build: a test that imports the build submodule by name leaves the module under that attribute)
    return pkg.load()


def test_every_stop_symbol_is_declared_exported_and_bound(pkg, lib):
    declared = pkg.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in SYMBOLS:
        assert s in declared and s in exported, s
        assert getattr(lib.c, s).argtypes is not None, f"{s}: not bound by HipLib.__init__"
    assert C.sizeof(pkg.StopState) == 24
    assert (pkg.STOP_MAX_IDS, pkg.STOP_MAX_SEQS, pkg.STOP_MAX_SEQ_LEN, pkg.STOP_BATCH_MAX) == (32, 16, 32, 64)
    header = open(pkg.HEADER_PATH).read()
    for name, value in (("MAX_IDS", 32), ("MAX_SEQS", 16), ("MAX_SEQ_LEN", 32), ("BATCH_MAX", 64), ("NONE", 0), ("TOKEN", 1), ("EOS", 2),
                        ("MAX_TOKENS", 3), ("SEQUENCE", 4)):
        assert f"#define BITNET_HIP_STOP_{name} {value}" in header, name


def test_host_layer_exports_the_stop_entry_points(pkg, lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [s for s in HOST_SYMBOLS if s not in exported]


def _refused(lib, pkg, rc, *words):
    assert rc == pkg.ERR_INVALID_ARGUMENT, (rc, lib.last_error())
    text = lib.last_error()
    assert text and all(w in text for w in words), text


def _create(lib, cfg):
    h = C.c_void_p()
    rc = lib.c.bitnet_hip_stop_create(C.byref(cfg) if cfg is not None else None, C.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_config_refusals_come_before_the_gpu(pkg, lib):
    mk = pkg.StopConfig.make
    _refused(lib, pkg, _create(lib, None), "Null config")
    cfg = mk()
    _refused(lib, pkg, lib.c.bitnet_hip_stop_create(C.byref(cfg), None), "Null pointer")
    _refused(lib, pkg, _create(lib, mk(stop_ids=range(33))), "33 stop ids")
    _refused(lib, pkg, _create(lib, mk(sequences=[[1]] * 17)), "17 stop sequences")
    _refused(lib, pkg, _create(lib, mk(sequences=[[1, 2], list(range(33))])), "sequence 1", "length 33")
    zero = mk(sequences=[[1, 2], [3]])
    zero._keep[1][1] = 0  # a sequence of length 0
    _refused(lib, pkg, _create(lib, zero), "sequence 1", "length 0")
    _refused(lib, pkg, _create(lib, mk(stop_ids=[4, -2])), "stop id 1", "negative")
    _refused(lib, pkg, _create(lib, mk(sequences=[[4], [5, -7]])), "sequence 1", "negative")
    null_ids = mk(stop_ids=[1, 2])
    null_ids.stop_ids = None
    _refused(lib, pkg, _create(lib, null_ids), "null stop_ids")
    null_seq = mk(sequences=[[1]])
    null_seq.seq_tokens = None
    _refused(lib, pkg, _create(lib, null_seq), "null seq_len or seq_tokens")
    null_len = mk(sequences=[[1]])
    null_len.seq_len = None
    _refused(lib, pkg, _create(lib, null_len), "null seq_len or seq_tokens")
    _refused(lib, pkg, _create(lib, mk(eos=-2)), "eos_id -2")
    _refused(lib, pkg, _create(lib, mk(max_tokens=-1)), "max_tokens -1")
    # configure checks its config before it looks at the object
    _refused(lib, pkg, lib.c.bitnet_hip_stop_configure(None, None), "Null config")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_configure(None, C.byref(mk(eos=-9))), "eos_id -9")


def test_null_pointers_and_ranges_are_refused_before_the_gpu(pkg, lib):
    buf = np.zeros(16, np.int32)
    p = buf.ctypes.data  # never dereferenced: the refusals come first
    st = pkg.StopState()
    _refused(lib, pkg, lib.c.bitnet_hip_stop_get_state(None, None), "Null output")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_get_state(None, C.byref(st)), "Null stop")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_arm(None, 0), "Null stop")
    for args in ((None, p, 8, p), (p, None, 8, p), (p, p, 8, None)):
        _refused(lib, pkg, lib.c.bitnet_hip_stop_dev(None, args[0], args[1], args[2], args[3], None, None), "Null pointer", "stop_dev")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_dev(None, p, p, 0, p, None, None), "capacity 0")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_dev(None, p, p, 1 << 31, p, None, None), "capacity")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_dev(None, p, p, 8, p, None, None), "Null stop")
    h = C.c_void_p()
    _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_create(4, None), "Null pointer")
    for n in (0, 65):
        _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_create(n, C.byref(h)), "n_slots must be in 1..64")
        assert not h.value
    _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_set(None, 64, None, None, None, 0, None, None), "slot 64 out of range")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_set(None, 0, None, None, None, 0, None, None), "Null table")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_dev(None, None), "Null table")
    n = C.c_int32()
    _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_live(None, None), "Null output")
    _refused(lib, pkg, lib.c.bitnet_hip_stop_batch_live(None, C.byref(n)), "Null table")
    lib.c.bitnet_hip_stop_destroy(None)  # both are no-ops on NULL
    lib.c.bitnet_hip_stop_batch_destroy(None)


def test_an_empty_config_passes_the_checks(pkg, lib):
    """An empty config is valid: create gets past every check -- and without a device fails on the allocation instead."""
    import torch

    h = C.c_void_p()
    cfg = pkg.StopConfig.make()
    rc = lib.c.bitnet_hip_stop_create(C.byref(cfg), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        lib.c.bitnet_hip_stop_destroy(h)
    else:
        assert rc == pkg.ERR_GPU and not h.value


def test_stop_config_make_lays_the_sequences_out_concatenated(pkg):
    cfg = pkg.StopConfig.make(stop_ids=[5, 6], eos=2, max_tokens=9, sequences=[[1, 2, 3], [4]])
    assert (cfg.n_stop_ids, cfg.eos_id, cfg.max_tokens, cfg.n_seqs) == (2, 2, 9, 2)
    assert [cfg.stop_ids[i] for i in range(2)] == [5, 6]
    assert [cfg.seq_len[i] for i in range(2)] == [3, 1] and [cfg.seq_tokens[i] for i in range(4)] == [1, 2, 3, 4]
    none = pkg.StopConfig.make()
    assert (none.n_stop_ids, none.eos_id, none.max_tokens, none.n_seqs) == (0, -1, 0, 0) and not none.stop_ids and not none.seq_len
