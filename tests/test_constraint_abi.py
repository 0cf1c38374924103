"""CPU, no GPU: bitnet_hip_sampler_set_constraints validates the config before it looks at the sampler pointer (as set_mirostat does), and
the new entry points are exported, in the library and in the decoder host."""
import ctypes as C
import subprocess

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg.load()


def call(lib, cfg):
    return lib.c.bitnet_hip_sampler_set_constraints(None, C.byref(cfg) if cfg is not None else None)


I32P = C.POINTER(C.c_int32)


def raw(pkg, **kw):
    """a bitnet_hip_constraints with the given fields and nothing else (NULL lists, zero counts)"""
    return pkg.Constraints(**kw)


def test_every_refusal_comes_before_the_sampler_pointer(lib, pkg):
    ids = (C.c_int32 * 40)(*range(40))
    vals = (C.c_float * 4)(0.5, 1.0, -np.inf, 0.0)
    p = C.cast(ids, I32P)
    v = C.cast(vals, C.POINTER(C.c_float))
    M = pkg.Constraints.make
    bad = {
        "NULL bias ids": raw(pkg, bias_values=v, n_bias=2),
        "NULL bias values": raw(pkg, bias_ids=p, n_bias=2),
        "NULL allowed": raw(pkg, n_allowed=3),
        "NULL hold": raw(pkg, n_hold=1, min_tokens=2),
        "negative bias id": M(bias=[(-1, 0.5)]),
        "bias id past every vocabulary": M(bias=[(1 << 20, 0.5)]),
        "negative allowed id": M(allowed=[3, -7]),
        "allowed id past every vocabulary": M(allowed=[1 << 20]),
        "negative hold id": M(hold=[-2], min_tokens=1),
        "hold id past every vocabulary": M(hold=[5, 1 << 21], min_tokens=1),
        "NaN bias": M(bias=[(1, 0.5), (2, float("nan"))]),
        "+inf bias": M(bias=[(1, float("inf"))]),
        "too many hold ids": raw(pkg, hold_ids=p, n_hold=pkg.CONSTRAINT_MAX_HOLD + 1, min_tokens=1),
        "negative min_tokens": M(min_tokens=-1),
        "negative ngram": M(no_repeat_ngram=-1),
        "ngram past the maximum": M(no_repeat_ngram=pkg.CONSTRAINT_MAX_NGRAM + 1),
    }
    for name, cfg in bad.items():
        assert call(lib, cfg) == pkg.ERR_INVALID_ARGUMENT, name
        msg = lib.last_error()
        assert msg.startswith("constraints:") and "Null sampler" not in msg, (name, msg)


def test_a_valid_config_is_refused_as_a_null_sampler(lib, pkg):
    good = [None, pkg.Constraints.make(), pkg.Constraints.make(bias={0: -np.inf, 5: 2.0, (1 << 20) - 1: -1.0}, allowed=[0, 5, 9], hold=list(range(32)),
                                                              min_tokens=7, no_repeat_ngram=pkg.CONSTRAINT_MAX_NGRAM)]
    for cfg in good:
        assert call(lib, cfg) == pkg.ERR_INVALID_ARGUMENT
        assert "Null sampler passed to sampler_set_constraints" in lib.last_error()
    g = C.c_uint64(7)
    assert lib.c.bitnet_hip_sampler_constraints_state(None, C.byref(g)) == pkg.ERR_INVALID_ARGUMENT
    assert "Null pointer passed to sampler_constraints_state" in lib.last_error()


def test_struct_layout_and_limits(pkg):
    assert C.sizeof(pkg.Constraints) == 7 * 8 + 2 * 4  # three (pointer, count) lists, one more pointer, two int32
    assert (pkg.CONSTRAINT_MAX_HOLD, pkg.CONSTRAINT_MAX_NGRAM) == (32, 8)
    cfg = pkg.Constraints.from_args(None, None, (), 0, 0, False)
    assert cfg is None and pkg.Constraints.from_args({1: 2.0}, None, (), 0, 0, True) is None
    cfg = pkg.Constraints.make(bias={3: 1.5, 4: -np.inf}, allowed=[1, 2], hold=[9], min_tokens=2, no_repeat_ngram=3)
    assert (cfg.n_bias, cfg.n_allowed, cfg.n_hold, cfg.min_tokens, cfg.no_repeat_ngram) == (2, 2, 1, 2, 3)
    assert [cfg.bias_ids[i] for i in range(2)] == [3, 4] and cfg.bias_values[1] == -np.inf and cfg.hold_ids[0] == 9


def test_the_binding_builds_off_empty_and_numpy_configs(pkg):
    F = pkg.Constraints.from_args
    assert F(None, None, (), 0, 0, False) is None and F(None, None, (), 0, 0, False, on=True) is not None  # nothing named: off, unless on=True
    empty = F(None, None, (), 0, 0, False, on=True)
    assert (empty.n_bias, empty.n_allowed, empty.n_hold, empty.min_tokens, empty.no_repeat_ngram) == (0, 0, 0, 0, 0)
    assert F({1: 1.0}, None, (), 0, 0, True, on=True) is None  # off wins
    cfg = F(None, np.array([4, 5, 6]), np.array([7, 8]), 2, 0, False)  # arrays with more than one element are no truth values
    assert cfg.n_allowed == 3 and cfg.n_hold == 2 and cfg.allowed_ids[2] == 6
    cfg = F(np.array([[3, 1.5], [4, -2.0]]), None, (), 0, 0, False)
    assert cfg.n_bias == 2 and cfg.bias_ids[1] == 4 and cfg.bias_values[1] == -2.0
    for bad in (dict(bias={1 << 32: 1.0}), dict(allowed=[(1 << 32) + 5]), dict(hold=[-(1 << 31) - 1], min_tokens=1)):
        with pytest.raises(ValueError, match="int32"):  # refused, not wrapped to a valid id
            pkg.Constraints.make(**bad)


def test_new_symbols_are_exported(lib, pkg):
    names = ["bitnet_hip_sampler_set_constraints", "bitnet_hip_sampler_constraints_state"]
    declared = pkg.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in names:
        assert n in declared and n in exported and hasattr(lib.c, n), n
        assert getattr(lib.c, n).argtypes is not None and getattr(lib.c, n).restype is C.c_int, n
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], text=True)
    host = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"bitnet_host_set_constraints", "bitnet_host_constraints_state"} <= host
    header = open(pkg.HEADER_PATH).read()
    assert "BITNET_HIP_CONSTRAINT_MAX_HOLD 32" in header and "BITNET_HIP_CONSTRAINT_MAX_NGRAM 8" in header
