"""CPU: the batched sampling entry points (bitnet_hip_sample_batch_*) and the two observability calls of the host layer's batch shim are
exported, declared, spelt out in INTEGRATION.md and bound at load; they refuse bad arguments before anything touches a device; and both
sampling kernels of csrc/kernels_sample.hip compile for gfx950 without scratch.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ENTRIES = ("bitnet_hip_sample_batch_create", "bitnet_hip_sample_batch_destroy", "bitnet_hip_sample_batch_set", "bitnet_hip_sample_batch_dev")
N_ARGS = {"bitnet_hip_sample_batch_create": 3, "bitnet_hip_sample_batch_destroy": 1, "bitnet_hip_sample_batch_set": 8, "bitnet_hip_sample_batch_dev": 2}
HOST_ENTRIES = ("bitnet_host_batch_captures", "bitnet_host_batch_graph_nodes")
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    # build.py loaded by path, as pkg.build() does: another test module may have imported bitnet-rs_amd.build as a submodule,
    # whose attribute then shadows the package's build() function
    pkg._load_build_module().build()
    return pkg.load()


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_declared_and_in_integration_md(pkg, lib):
    declared = set(pkg.declared_symbols())
    have = exported(lib.path)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in declared and name in have, name
        m = re.search(rf"pub fn {name}\(([^;]*?)\)\s*(?:->[^;]*)?;", text, re.S)
        assert m and m.group(1).count(":") == N_ARGS[name], name
    host = exported(pkg.HOST_LIB_PATH)
    for name in HOST_ENTRIES:
        assert name in host, name


def test_every_new_binding_is_typed_at_load(pkg, lib):
    for name in ENTRIES:
        fn = getattr(lib.c, name)
        assert fn.argtypes is not None and len(fn.argtypes) == N_ARGS[name], name
        assert fn.restype is (None if name.endswith("destroy") else C.c_int), name
    src = open(pkg.__file__).read()
    for name in HOST_ENTRIES:  # typed from host/batch_decoder.hpp when the host library is loaded
        fn = getattr(pkg._host_lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == 1 and fn.restype is C.c_int, name
    assert re.search(r"def captures\(self\)", src) and re.search(r"def graph_nodes\(self\)", src)
    assert hasattr(pkg, "SampleBatch") and hasattr(pkg.HipLib, "sample_batch")


def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    c = lib.c
    err = lambda: lib.last_error()
    out = C.c_void_p(0x1234)
    for n_slots in (0, 9):
        assert c.bitnet_hip_sample_batch_create(1000, n_slots, C.byref(out)) == INVALID and "n_slots" in err()
        assert out.value is None  # *out is cleared on every refusal
    for vocab in (0, (1 << 20) + 1):
        assert c.bitnet_hip_sample_batch_create(vocab, 4, C.byref(out)) == INVALID and "vocab must be in 1..1048576" in err()
    assert c.bitnet_hip_sample_batch_create(1000, 4, None) == INVALID and "Null pointer" in err()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert c.bitnet_hip_sample_batch_set(None, 0, None, p, None, None, None, None) == INVALID and "Null table" in err()
    assert c.bitnet_hip_sample_batch_dev(None, None) == INVALID and "Null table" in err()
    c.bitnet_hip_sample_batch_destroy(None)  # a no-op


def test_host_shim_answers_zero_for_a_null_or_dead_batch(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_batch_create.restype = C.c_void_p
    c.bitnet_host_batch_create.argtypes = [C.c_int]
    c.bitnet_host_batch_destroy.argtypes = [C.c_void_p]
    c.bitnet_host_batch_destroy.restype = None
    for name in HOST_ENTRIES:
        getattr(c, name).argtypes = [C.c_void_p]
        getattr(c, name).restype = C.c_int
        assert getattr(c, name)(None) == 0
    b = c.bitnet_host_batch_create(0)  # a dead batch
    assert b and c.bitnet_host_batch_captures(b) == 0 and c.bitnet_host_batch_graph_nodes(b) == 0
    c.bitnet_host_batch_destroy(b)


def test_both_sampling_kernels_compile_without_scratch(pkg, tmp_path):
    """kernels_sample.hip to gfx950 assembly with the build's flags: k_sample and k_sample_batch are there, and no kernel of the file has a
    private segment (EXPERIMENTS.md 9: the F path spills once too much is in flight per thread; reading the arguments from memory must not
    push it over)."""
    build = pkg._load_build_module()  # by path: importing it as a submodule would shadow the package's build() function
    src = "kernels_sample.hip"
    assert "-ffp-contract=off" in build.EXTRA[src]
    asm = tmp_path / "kernels_sample.s"
    cmd = [build.HIPCC, *build.COMMON_FLAGS, *build.EXTRA[src], "--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", str(asm)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    kernels = dict(re.findall(r"\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)", text, re.S))
    names = sorted(kernels)
    assert len(names) == 2, names
    assert any(re.search(r"\d+k_sampleE", n) for n in names), names
    assert any("k_sample_batch" in n for n in names), names
    for n, scratch in kernels.items():
        assert int(scratch) == 0, (n, scratch)
    assert text.count(".amdhsa_private_segment_fixed_size 0") == 2
