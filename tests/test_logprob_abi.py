"""CPU: the C surface of the logits tap (include/bitnet_hip.h: bitnet_hip_logprob_*) -- the record's layout, the scratch size, and every
refusal the header lists, all before the GPU is touched (this runs on machines without one)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def test_record_and_args_layout(pkg):
    R, A = pkg.LogprobRecord, pkg.LogprobArgs
    assert C.sizeof(R) == 176 and pkg.LOGPROB_DTYPE.itemsize == 176
    assert [getattr(R, f).offset for f in ("token", "n_top", "logit", "lse", "top_id", "top_logit")] == [0, 4, 8, 12, 16, 96]
    assert [pkg.LOGPROB_DTYPE.fields[f][1] for f in ("token", "n_top", "logit", "lse", "top_id", "top_logit")] == [0, 4, 8, 12, 16, 96]
    assert C.sizeof(A) == 48
    assert [getattr(A, f).offset for f in ("logits_dev", "pos_dev", "history_dev", "records_dev", "scratch_dev", "capacity", "top_n")] == [0, 8, 16, 24, 32, 40, 44]
    assert pkg.LOGPROB_TOP_MAX == 20


def test_header_declares_the_struct_as_the_binding_lays_it_out(pkg):
    text = open(pkg.HEADER_PATH).read()
    assert "#define BITNET_HIP_LOGPROB_TOP_MAX 20" in text
    for name in ("bitnet_hip_logprob_scratch_bytes", "bitnet_hip_logprob_dev", "bitnet_hip_logprob_batch_dev"):
        assert name in pkg.declared_symbols()
    for ref_line in ("config.rs:87-93", "engine.rs:1182-1210", "main.rs:1337-1373"):
        assert ref_line in text


def test_scratch_bytes(lib):
    assert lib.logprob_scratch_bytes(0) == 0
    assert lib.logprob_scratch_bytes((1 << 20) + 1) == 0
    sizes = [lib.logprob_scratch_bytes(v) for v in (1, 2, 20, 21, 1023, 1024, 1025, 4099, 65536, 65537, 128256, 1 << 19, 1 << 20)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)  # non-decreasing in the vocabulary


def test_refusals_before_the_gpu_is_touched(pkg, lib):
    E = pkg.ERR_INVALID_ARGUMENT

    def refused(fn, *a):
        with pytest.raises(pkg.BitNetHipError) as e:
            fn(*a)
        assert e.value.code == E, e.value
        return str(e.value)

    ok = dict(logits=0x1000, pos=0x2000, history=0x3000, records=0x4000, scratch=0x5000, capacity=4, top_n=5)
    assert "Null pointer" in refused(lib.logprob_dev, None, 2048)
    for vocab in (0, (1 << 20) + 1):
        assert "vocab" in refused(lib.logprob_dev, pkg.LogprobArgs.make(**ok), vocab)
        assert "vocab" in refused(lib.logprob_batch_dev, 0x6000, 1, vocab)
    assert "top_n" in refused(lib.logprob_dev, pkg.LogprobArgs.make(**dict(ok, top_n=21)), 2048)
    for missing in ("logits", "pos", "history", "scratch"):
        assert "Null pointer" in refused(lib.logprob_dev, pkg.LogprobArgs.make(**dict(ok, **{missing: None})), 2048)
    assert "Null table" in refused(lib.logprob_batch_dev, None, 1, 2048)
    for n_slots in (0, 9):
        assert "n_slots" in refused(lib.logprob_batch_dev, 0x6000, n_slots, 2048)


def test_host_shim_refusals_without_a_device(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_set_logprobs.argtypes = [C.c_void_p, C.c_int]
    c.bitnet_host_logprobs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    buf = (pkg.LogprobRecord * 2)()
    assert c.bitnet_host_set_logprobs(None, 5) == pkg.ERR_INVALID_ARGUMENT
    assert c.bitnet_host_logprobs(None, 0, 1, buf) == pkg.ERR_INVALID_ARGUMENT
    # a dead decoder (a configuration the kernels refuse) refuses both, and nothing is dereferenced
    c.bitnet_host_create.restype = C.c_void_p
    c.bitnet_host_create.argtypes = [C.POINTER(pkg.HostConfig)]
    c.bitnet_host_destroy.argtypes = [C.c_void_p]
    hc = pkg.HostConfig(hidden=100, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=128, ffn=256, vocab=64, max_pos=32, eps=1e-5, rope_theta=1e4)
    d = c.bitnet_host_create(C.byref(hc))
    assert d
    for top_n in (-1, 0, 20, 21):
        assert c.bitnet_host_set_logprobs(d, top_n) == pkg.ERR_INVALID_ARGUMENT
    assert c.bitnet_host_logprobs(d, 0, 1, buf) == pkg.ERR_INVALID_ARGUMENT
    c.bitnet_host_destroy(d)
