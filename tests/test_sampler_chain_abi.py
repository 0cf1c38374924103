"""CPU: the sampler chain's entry points (bitnet_hip_sampler_create_ex / _configure_ex, the host layer's bitnet_host_set_sampling_ex) are
exported, declared and bound at load, and refuse every invalid config with BITNET_HIP_ERR_INVALID_ARGUMENT and an error text that names
the field, before the GPU is touched.  No GPU compute here."""
import ctypes as C
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib(pkg):
    pkg._load_build_module().build()
    return pkg.load()


def _ex(pkg, base=(1.0, 0, 1.0, 1.0), min_p=0.0, typical_p=1.0, frequency_penalty=0.0, presence_penalty=0.0):
    return pkg.SamplingConfigEx(pkg.SamplingConfig(*base, 0), min_p, typical_p, frequency_penalty, presence_penalty)


def test_the_new_symbols_are_exported_and_declared(lib):
    c = C.CDLL(lib.path)
    header = open(os.path.join(ROOT, "include", "bitnet_hip.h")).read()
    for name in ("bitnet_hip_sampler_create_ex", "bitnet_hip_sampler_configure_ex"):
        assert getattr(c, name) is not None
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "typedef struct bitnet_hip_sampling_config_ex" in header
    for cite in ("RepetitionPenaltyConfig::apply :247-259", "apply_min_p :299-310", "apply_typical :337-381", "MinPSampler :37-50", "TypicalSampler :73-86"):
        assert cite in header, cite


def test_the_struct_layout_matches_the_header(pkg):
    assert C.sizeof(pkg.SamplingConfig) == 24 and C.sizeof(pkg.SamplingConfigEx) == 40
    assert [f[0] for f in pkg.SamplingConfigEx._fields_] == ["base", "min_p", "typical_p", "frequency_penalty", "presence_penalty"]
    assert pkg.SamplingConfigEx.min_p.offset == 24 and pkg.SamplingConfigEx.presence_penalty.offset == 36
    cfg = pkg.SamplingConfigEx.make(0.8, 40, 0.9, 1.1, 5)
    assert (cfg.min_p, cfg.typical_p, cfg.frequency_penalty, cfg.presence_penalty) == (0.0, 1.0, 0.0, 0.0) and cfg.base.seed == 5


INVALID = [(dict(min_p=NAN), b"min_p"), (dict(typical_p=NAN), b"typical_p"), (dict(frequency_penalty=NAN), b"frequency_penalty"),
           (dict(frequency_penalty=INF), b"frequency_penalty"), (dict(frequency_penalty=-INF), b"frequency_penalty"),
           (dict(presence_penalty=NAN), b"presence_penalty"), (dict(presence_penalty=INF), b"presence_penalty"),
           (dict(presence_penalty=-INF), b"presence_penalty"),
           (dict(base=(NAN, 0, 1.0, 1.0)), b"temperature"), (dict(base=(1.0, -1, 1.0, 1.0)), b"top_k"), (dict(base=(1.0, 0, NAN, 1.0)), b"top_p"),
           (dict(base=(1.0, 0, 1.0, 0.0)), b"repetition_penalty")]


def test_create_ex_refuses_invalid_configs_and_names_the_field(pkg, lib):
    c = C.CDLL(lib.path)
    c.bitnet_hip_get_last_error.restype = C.c_char_p
    c.bitnet_hip_sampler_create_ex.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    h = C.c_void_p()
    for kw, word in INVALID:
        cfg = _ex(pkg, **kw)
        assert c.bitnet_hip_sampler_create_ex(1000, C.byref(cfg), C.byref(h)) == pkg.ERR_INVALID_ARGUMENT, kw
        assert word in c.bitnet_hip_get_last_error() and not h.value, (kw, c.bitnet_hip_get_last_error())
    assert c.bitnet_hip_sampler_create_ex(1000, None, C.byref(h)) == pkg.ERR_INVALID_ARGUMENT
    assert b"Null" in c.bitnet_hip_get_last_error()
    assert c.bitnet_hip_sampler_create_ex(1000, C.byref(_ex(pkg)), None) == pkg.ERR_INVALID_ARGUMENT
    assert b"Null" in c.bitnet_hip_get_last_error()
    assert c.bitnet_hip_sampler_create_ex(0, C.byref(_ex(pkg)), C.byref(h)) == pkg.ERR_INVALID_ARGUMENT
    assert b"vocab" in c.bitnet_hip_get_last_error()
    c.bitnet_hip_sampler_configure_ex.argtypes = [C.c_void_p, C.c_void_p]
    assert c.bitnet_hip_sampler_configure_ex(None, C.byref(_ex(pkg))) == pkg.ERR_INVALID_ARGUMENT
    assert b"Null" in c.bitnet_hip_get_last_error()
    assert math.isnan(_ex(pkg, min_p=NAN).min_p)


def test_the_python_bindings_bind_the_new_entries_at_load(pkg, lib):
    L = lib.c
    assert L.bitnet_hip_sampler_create_ex.argtypes[1]._type_ is pkg.SamplingConfigEx and L.bitnet_hip_sampler_create_ex.restype is C.c_int
    assert L.bitnet_hip_sampler_configure_ex.argtypes[1]._type_ is pkg.SamplingConfigEx and L.bitnet_hip_sampler_configure_ex.restype is C.c_int
    import inspect

    for fn in (type(lib).sampler, pkg.Sampler.configure, pkg.HostDecoder.set_sampling):
        ps = inspect.signature(fn).parameters
        assert [ps[k].default for k in ("min_p", "typical_p", "frequency_penalty", "presence_penalty")] == [0.0, 1.0, 0.0, 0.0], fn
