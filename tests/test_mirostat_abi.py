"""CPU: Mirostat's surface -- bitnet_hip_sampler_set_mirostat / _mirostat_state and the host layer's bitnet_host_set_mirostat /
_mirostat_state are declared in the header, exported by the libraries, spelt out in INTEGRATION.md and bound at load; every invalid tau or
eta is refused with BITNET_HIP_ERR_INVALID_ARGUMENT and an error text that names the field, before the sampler is looked at and before the
GPU is touched.  (The refusals that need a live sampler -- a config with a truncation stage on -- are in tests/test_mirostat_gpu.py, where
the state is read back unchanged.)  No GPU compute here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NEW = ("bitnet_hip_sampler_set_mirostat", "bitnet_hip_sampler_mirostat_state")
HOST = ("bitnet_host_set_mirostat", "bitnet_host_mirostat_state")


@pytest.fixture(scope="module")
def lib(pkg):
    pkg._load_build_module().build()
    return pkg.load()


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_the_new_symbols_are_declared_exported_and_documented(pkg, lib):
    header = open(os.path.join(ROOT, "include", "bitnet_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    exported, declared = _exports(lib.path), pkg.declared_symbols()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in declared and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", integration), name
    assert "typedef struct bitnet_hip_mirostat_config { float tau; float eta; } bitnet_hip_mirostat_config;" in header
    for cite in ("MirostatSampler :109-196", "`sample` :131-190", "MirostatSampler::new :120-126", "strategies.rs:192-195", "lib.rs:180-213", "ChaCha8Rng"):
        assert cite in header, cite
    host = _exports(pkg.HOST_LIB_PATH)
    for name in HOST:
        assert name in host, name


def test_the_struct_layout_matches_the_header(pkg):
    assert C.sizeof(pkg.MirostatConfig) == 8 and [f[0] for f in pkg.MirostatConfig._fields_] == ["tau", "eta"]
    assert pkg.MirostatConfig.eta.offset == 4


def test_the_python_bindings_bind_the_new_entries_at_load(pkg, lib):
    L = lib.c
    assert L.bitnet_hip_sampler_set_mirostat.argtypes[1]._type_ is pkg.MirostatConfig and L.bitnet_hip_sampler_set_mirostat.restype is C.c_int
    assert len(L.bitnet_hip_sampler_mirostat_state.argtypes) == 3 and L.bitnet_hip_sampler_mirostat_state.restype is C.c_int
    for cls in (pkg.Sampler, pkg.HostDecoder):
        ps = inspect.signature(cls.set_mirostat).parameters
        assert list(ps) == ["self", "tau", "eta"], cls
        assert callable(cls.mirostat_state)


INVALID = [((NAN, 0.1), b"tau"), ((INF, 0.1), b"tau"), ((-INF, 0.1), b"tau"), ((0.0, 0.1), b"tau"), ((-1.0, 0.1), b"tau"),
           ((5.0, NAN), b"eta"), ((5.0, INF), b"eta"), ((5.0, -INF), b"eta"), ((5.0, -0.1), b"eta")]


def test_invalid_values_are_refused_before_the_sampler_is_looked_at(pkg, lib):
    c = C.CDLL(lib.path)
    c.bitnet_hip_get_last_error.restype = C.c_char_p
    c.bitnet_hip_sampler_set_mirostat.argtypes = [C.c_void_p, C.c_void_p]
    for (tau, eta), word in INVALID:
        cfg = pkg.MirostatConfig(tau, eta)
        assert c.bitnet_hip_sampler_set_mirostat(None, C.byref(cfg)) == pkg.ERR_INVALID_ARGUMENT, (tau, eta)
        assert word in c.bitnet_hip_get_last_error(), (tau, eta, c.bitnet_hip_get_last_error())
    # valid values (eta 0 is one): what is refused is the sampler
    for tau, eta in ((5.0, 0.1), (1e-3, 0.0)):
        cfg = pkg.MirostatConfig(tau, eta)
        assert c.bitnet_hip_sampler_set_mirostat(None, C.byref(cfg)) == pkg.ERR_INVALID_ARGUMENT
        assert b"Null sampler" in c.bitnet_hip_get_last_error()
    assert c.bitnet_hip_sampler_set_mirostat(None, None) == pkg.ERR_INVALID_ARGUMENT
    c.bitnet_hip_sampler_mirostat_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    mu = C.c_float(7.0)
    assert c.bitnet_hip_sampler_mirostat_state(None, C.byref(mu), None) == pkg.ERR_INVALID_ARGUMENT and mu.value == 7.0
    assert b"Null sampler" in c.bitnet_hip_get_last_error()


def test_the_host_shims_refuse_a_null_decoder(pkg, lib):
    h = C.CDLL(pkg.HOST_LIB_PATH)
    h.bitnet_host_set_mirostat.argtypes = [C.c_void_p, C.c_void_p]
    h.bitnet_host_mirostat_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    cfg = pkg.MirostatConfig(5.0, 0.1)
    assert h.bitnet_host_set_mirostat(None, C.byref(cfg)) != 0
    assert h.bitnet_host_mirostat_state(None, None, None) != 0
