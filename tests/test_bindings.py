"""The ctypes signatures are derived from the C headers (bitnet-rs_amd/cproto.py) and set when a library is loaded: the parser on every
prototype shape the headers hold, the refusal of unknown types, and the loaded libraries against the headers.  No GPU compute here."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

SAMPLE = """
#ifdef __cplusplus
extern "C" {
#endif
#define PFX_MAX 8
#define PFX_CALL(x) \\
    pfx_macro(x);
/* a block comment with a call; pfx_commented(int a); and a ( */
typedef struct pfx_config {
    int32_t hidden, n_layers;
    float eps;
} pfx_config;
typedef int (*pfx_gather_fn)(void *ctx, size_t n);
int pfx_count(void);
const char *pfx_error(void *d);  // int pfx_in_a_line_comment(int a);
void *pfx_create(const pfx_config *cfg);
void pfx_destroy(void *d);
int pfx_times(void *d, float out[4]);
int pfx_tables(void *const *members, const uint8_t *const *w7, const float *const *scales7,
               size_t block_size,
               unsigned long long seed);
size_t pfx_bytes(size_t m, size_t k, int digits);
uint64_t pfx_total(void);
int pfx_create_handle(size_t vocab, pfx_sampler **out);
#ifdef __cplusplus
}
#endif
"""


def test_parser_reads_every_prototype_shape(pkg):
    assert pkg.cproto.prototypes(SAMPLE, "pfx_") == [
        ("pfx_count", "int", []),
        ("pfx_error", "const char *", [("void *", "d")]),
        ("pfx_create", "void *", [("const pfx_config *", "cfg")]),
        ("pfx_destroy", "void", [("void *", "d")]),
        ("pfx_times", "int", [("void *", "d"), ("float *", "out")]),
        ("pfx_tables", "int", [("void *const *", "members"), ("const uint8_t *const *", "w7"), ("const float *const *", "scales7"),
                               ("size_t", "block_size"), ("unsigned long long", "seed")]),
        ("pfx_bytes", "size_t", [("size_t", "m"), ("size_t", "k"), ("int", "digits")]),
        ("pfx_total", "uint64_t", []),
        ("pfx_create_handle", "int", [("size_t", "vocab"), ("pfx_sampler **", "out")]),
    ]


def test_one_rule_from_c_types_to_ctypes(pkg):
    class Config(C.Structure):
        _fields_ = [("hidden", C.c_int32)]

    ctype = lambda c: pkg.cproto.ctype(c, {"pfx_config": Config}, "pfx_f")
    assert ctype("const char *") is C.c_char_p and ctype("char *") is C.c_char_p
    assert ctype("const pfx_config *") is C.POINTER(Config) and ctype("pfx_config *") is C.POINTER(Config)
    for c in ("void *", "const float *", "float *", "void *const *", "const uint8_t *const *", "pfx_sampler *", "pfx_sampler **", "pfx_config **",
              "char **", "bitnet_host_allgather_fn"):
        assert ctype(c) is C.c_void_p, c
    for c, want in (("int", C.c_int), ("size_t", C.c_size_t), ("float", C.c_float), ("double", C.c_double), ("int32_t", C.c_int32),
                    ("uint32_t", C.c_uint32), ("int64_t", C.c_int64), ("uint64_t", C.c_uint64), ("unsigned long long", C.c_ulonglong),
                    ("bitnet_hip_weights_t", C.c_uint64), ("const int", C.c_int)):
        assert ctype(c) is want, c


class _Lib:
    """stands in for a CDLL: any symbol is there"""

    def __getattr__(self, name):
        fn = self.__dict__[name] = type("Fn", (), {})()
        return fn


def test_bind_sets_both_and_refuses_what_is_in_no_table(pkg):
    lib = _Lib()
    pkg.cproto.bind(lib, pkg.cproto.prototypes(SAMPLE, "pfx_"), {})
    assert lib.pfx_count.argtypes == [] and lib.pfx_count.restype is C.c_int
    assert lib.pfx_error.restype is C.c_char_p and lib.pfx_create.restype is C.c_void_p and lib.pfx_destroy.restype is None
    assert lib.pfx_bytes.argtypes == [C.c_size_t, C.c_size_t, C.c_int] and lib.pfx_bytes.restype is C.c_size_t
    assert lib.pfx_times.argtypes == [C.c_void_p, C.c_void_p]
    with pytest.raises(TypeError, match="pfx_scalar.*'long double'"):  # an unknown scalar
        pkg.cproto.bind(_Lib(), pkg.cproto.prototypes("int pfx_scalar(void *d, long double x);", "pfx_"), {})
    with pytest.raises(TypeError, match="pfx_by_value.*'pfx_config'"):  # an unknown struct by value, though its pointer is known
        pkg.cproto.bind(_Lib(), pkg.cproto.prototypes("int pfx_by_value(pfx_config cfg);", "pfx_"), {"pfx_config": C.Structure})
    with pytest.raises(TypeError, match="pfx_returns"):
        pkg.cproto.bind(_Lib(), pkg.cproto.prototypes("pfx_config pfx_returns(void);", "pfx_"), {})
    with pytest.raises(AttributeError):  # a declared symbol the library does not export
        pkg.cproto.bind(object(), pkg.cproto.prototypes("int pfx_missing(void);", "pfx_"), {})


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg.load()


def _held_to_header(pkg, cdll, protos):
    for name, ret, params in protos:
        fn = getattr(cdll, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert list(fn.argtypes) == [pkg.cproto.ctype(t, pkg.C_STRUCTS, name) for t, _ in params], name
        assert fn.restype is (None if ret == "void" else pkg.cproto.ctype(ret, {}, name)), name


def test_kernel_library_is_typed_from_its_header_at_load(pkg, lib):
    protos = pkg.cproto.prototypes(open(pkg.HEADER_PATH).read(), "bitnet_hip_")
    assert len(protos) == 132 and len({p[0] for p in protos}) == 132
    _held_to_header(pkg, lib.c, protos)
    assert isinstance(lib.c, C.CDLL)
    # a few by value: a size_t return, a char pointer return, a struct pointer, an opaque handle pair, a void return
    assert lib.c.bitnet_hip_qb32_bytes.restype is C.c_size_t and lib.c.bitnet_hip_get_last_error.restype is C.c_char_p
    assert lib.c.bitnet_hip_get_device_info.argtypes == [C.c_int, C.POINTER(pkg.DeviceInfo)]
    assert lib.c.bitnet_hip_sampler_create.argtypes == [C.c_size_t, C.POINTER(pkg.SamplingConfig), C.c_void_p]
    assert lib.c.bitnet_hip_cleanup.argtypes == [] and lib.c.bitnet_hip_cleanup.restype is None
    assert lib.c.bitnet_hip_weights_free.argtypes == [C.c_uint64]


def test_host_library_is_typed_from_its_headers_at_load_and_exports_them(pkg, lib):
    # 82 prototypes, and the two the decoder's C tail defined without declaring: bitnet_host_last_prefill_path, bitnet_host_saturation_fallbacks
    protos = pkg.host_prototypes()
    assert len(protos) == 84 and len({p[0] for p in protos}) == 84
    host = pkg._host_lib()
    assert isinstance(host, C.CDLL) and pkg._host_lib(pkg.HOST_LIB_PATH) is host  # one bound library per path
    _held_to_header(pkg, host, protos)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [p[0] for p in protos if p[0] not in exported]
    assert host.bitnet_host_create.argtypes == [C.POINTER(pkg.HostConfig)] and host.bitnet_host_create.restype is C.c_void_p
    assert host.bitnet_host_weight_bytes.restype is C.c_uint64 and host.bitnet_host_gguf_tensor_count.restype is C.c_int64
    assert host.bitnet_host_phase_times.argtypes == [C.c_void_p, C.c_void_p]  # float out[4]
    assert host.bitnet_host_prefill_sharded.argtypes[4] is C.c_void_p  # bitnet_host_allgather_fn
    assert host.bitnet_host_trace_step.argtypes == [C.c_void_p, C.c_char_p, C.c_int]
    assert pkg.GgufFile().c is host  # every wrapper takes the bound library from the one place


def test_every_symbol_the_package_calls_is_declared(pkg):
    declared = set(pkg.declared_symbols()) | {p[0] for p in pkg.host_prototypes()}
    called = set()
    for path in glob.glob(os.path.join(os.path.dirname(pkg.__file__), "*.py")):
        called |= set(re.findall(r"\.(bitnet_(?:hip|host)_[a-z0-9_]+)\b", open(path).read()))
    assert len(called) > 150
    assert not sorted(called - declared)


def test_no_hand_written_signature_remains(pkg):
    src = open(pkg.__file__).read()
    assert not re.findall(r"\.(?:argtypes|restype)\b", src)
