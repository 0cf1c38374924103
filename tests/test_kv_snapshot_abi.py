"""CPU: the KV snapshot entry points (bitnet_hip_kv_snapshot_bytes / _kv_save_dev / _kv_restore_dev, include/bitnet_hip_kvsnap.h) and the host
layer's prefix cache exports (host/prefix_cache.hpp) are exported, declared and bound; the launches refuse every bad argument by message before
anything touches a device; bitnet_hip_kv_snapshot_bytes is the layout's formula and 0 for what the launches refuse.  No GPU compute here."""
import ctypes as C
import re
import subprocess

import pytest

ENTRIES = ("bitnet_hip_kv_snapshot_bytes", "bitnet_hip_kv_save_dev", "bitnet_hip_kv_restore_dev")
HOST_ENTRIES = {"bitnet_host_prefix_cache_create": 5, "bitnet_host_prefix_cache_destroy": 1, "bitnet_host_prefix_cache_error": 1,
                "bitnet_host_prefix_cache_insert": 5, "bitnet_host_prefix_cache_lookup": 5, "bitnet_host_prefix_cache_restore": 5,
                "bitnet_host_prefix_cache_invalidate": 3, "bitnet_host_prefix_cache_clear": 1, "bitnet_host_prefix_cache_stats": 2,
                "bitnet_host_prefix_cache_len": 1, "bitnet_host_prefix_cache_entry": 5, "bitnet_host_prefill_cached": 7}
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
KV_F16 = 2    # BITNET_HIP_ATTN_KV_F16
BATCH_MAX = 8


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_exported_declared_and_typed_at_load(pkg, lib):
    have = exported(lib.path)
    for name in ENTRIES:
        assert name in set(pkg.declared_symbols()) and name in have, name
    assert sorted(p[0] for p in pkg.kvsnap_prototypes()) == sorted(ENTRIES)
    assert '#include "bitnet_hip_kvsnap.h"' in open(pkg.HEADER_PATH).read()
    doc = open(pkg.KVSNAP_HEADER_PATH).read()
    assert "prefix_cache.rs:64-77" in doc and "cached_state" in doc  # what the snapshot is in the reference
    assert "K [n_layers][n_kv_heads][S][128]" in doc and "DISTINCT" in doc and "16-byte aligned" in doc
    assert lib.c.bitnet_hip_kv_snapshot_bytes.restype is C.c_size_t and lib.c.bitnet_hip_kv_snapshot_bytes.argtypes == [C.c_size_t] * 4 + [C.c_int]
    assert len(lib.c.bitnet_hip_kv_save_dev.argtypes) == 10 and lib.c.bitnet_hip_kv_save_dev.restype is C.c_int
    assert len(lib.c.bitnet_hip_kv_restore_dev.argtypes) == 12 and lib.c.bitnet_hip_kv_restore_dev.restype is C.c_int
    host, hostlib = exported(pkg.HOST_LIB_PATH), pkg._host_lib()
    assert {p[0]: len(p[2]) for p in pkg.host_prefix_prototypes()} == HOST_ENTRIES
    for name, n_args in HOST_ENTRIES.items():  # typed from host/prefix_cache.hpp when the host library is loaded
        assert name in host, name
        assert len(getattr(hostlib, name).argtypes) == n_args, name
    assert hostlib.bitnet_host_prefix_cache_stats.argtypes == [C.c_void_p, C.POINTER(pkg.PrefixStats)]
    assert hostlib.bitnet_host_prefix_cache_create.restype is C.c_void_p and hostlib.bitnet_host_prefix_cache_error.restype is C.c_char_p
    for method in ("kv_snapshot_bytes", "kv_save_dev", "kv_restore_dev"):
        assert hasattr(pkg.HipLib, method), method
    assert hasattr(pkg.HostDecoder, "prefill_cached")
    for method in ("insert", "lookup", "restore", "invalidate", "clear", "stats", "__len__"):
        assert hasattr(pkg.PrefixCache, method), method
    # every export the package's PrefixCache reaches by name is one the header declares
    src = open(pkg.__file__).read()
    reached = {"bitnet_host_prefix_cache_" + m for m in re.findall(r'self\._f\("([a-z_]+)"\)', src)} | set(re.findall(r'"(bitnet_host_prefill_cached)"', src))
    assert len(reached) == len(HOST_ENTRIES) and reached == set(HOST_ENTRIES)


def test_snapshot_bytes_is_the_layout_formula(lib):
    f = lib.c.bitnet_hip_kv_snapshot_bytes
    for layers, kv, n in ((1, 1, 1), (3, 2, 65), (30, 5, 128), (30, 5, 4096), (2, 5, 0)):
        assert f(layers, kv, 128, n, 0) == 2 * layers * kv * n * 128 * 4
        assert f(layers, kv, 128, n, KV_F16) == 2 * layers * kv * n * 128 * 2
    assert f(30, 5, 128, 1, 0) == 153600 and f(30, 5, 128, 128, 0) == 19660800  # the 2B-4T shape: bytes per position, a 128-token prompt
    # 0 for what the launches refuse
    assert f(0, 5, 128, 10, 0) == 0 and f(3, 0, 128, 10, 0) == 0
    for head_dim in (0, 64, 256):
        assert f(3, 2, head_dim, 10, 0) == 0
    for flags in (1, 4, KV_F16 | 1, -1):
        assert f(3, 2, 128, 10, flags) == 0
    big = (1 << 64) - 1
    assert f(3, 2, 128, big, 0) == 0 and f(1 << 40, 1 << 40, 128, 10, 0) == 0 and f(1 << 30, 2, 128, 10, 0) == 0 and f(3, 2, 128, 1 << 55, 0) == 0


def test_save_and_restore_refuse_bad_arguments_without_a_device(lib):
    c = lib.c
    buf = (C.c_uint8 * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    p = C.c_void_p(base)
    err = lambda: lib.last_error()
    save, restore = c.bitnet_hip_kv_save_dev, c.bitnet_hip_kv_restore_dev
    # save(k, v, n_layers, n_kv_heads, head_dim, max_pos, n_positions, flags, snapshot, stream)
    S = lambda k=p, v=p, layers=3, kv=2, hd=128, mp=640, n=10, flags=0, snap=p: save(k, v, layers, kv, hd, mp, n, flags, snap, None)
    # restore(snapshot, snapshot_positions, dst_k, dst_v, n_layers, n_dst, n_kv_heads, head_dim, max_pos, n_positions, flags, stream)
    R = lambda snap=p, sp=10, k=p, v=p, layers=3, n_dst=2, kv=2, hd=128, mp=640, n=10, flags=0: restore(snap, sp, k, v, layers, n_dst, kv, hd, mp, n, flags, None)
    for hole in ("k", "v", "snap"):
        assert S(**{hole: None}) == INVALID and "Null pointer passed to kv_save_dev" in err(), hole
        assert R(**{hole: None}) == INVALID and "Null pointer passed to kv_restore_dev" in err(), hole
    for call, name in ((S, "kv_save_dev"), (R, "kv_restore_dev")):
        assert call(layers=0) == INVALID and f"{name}: n_layers 0" in err()
        assert call(kv=0) == INVALID and f"{name}: num_key_value_heads 0" in err()
        for head_dim in (0, 64, 256):
            assert call(hd=head_dim) == INVALID and f"{name}: head_dim {head_dim} unsupported (128)" in err(), head_dim
        for flags in (1, 4, KV_F16 | 1, -1):
            assert call(flags=flags) == INVALID and f"{name}: flags" in err() and "BITNET_HIP_ATTN_KV_F16" in err(), flags
        assert call(n=641) == INVALID and "KV cache overflow: n_positions 641, max_pos 640" in err()
        assert call(mp=0, n=1, flags=KV_F16) == INVALID and "KV cache overflow" in err()
        for off in (1, 4, 8):
            assert call(snap=C.c_void_p(base + off)) == INVALID and f"{name}: the snapshot must be 16-byte aligned" in err(), off
        # sizes whose products wrap size_t (or pass the grid's range) are refused, not multiplied
        big = (1 << 64) - 1
        assert call(mp=big) == INVALID and "too large" in err() and name in err()
        assert call(kv=1 << 60, mp=1 << 20) == INVALID and "too large" in err()
        assert call(layers=1 << 40, kv=1 << 40) == INVALID and "too large" in err()
        assert call(layers=1 << 30) == INVALID and "too large" in err()
    for n_dst in (0, BATCH_MAX + 1):
        assert R(n_dst=n_dst) == INVALID and f"kv_restore_dev: n_dst {n_dst} must be 1..{BATCH_MAX}" in err(), n_dst
    assert R(sp=9, n=10) == INVALID and "kv_restore_dev: n_positions 10 exceeds snapshot_positions 9" in err()
    assert R(sp=1 << 62, n=10) == INVALID and "too large" in err()  # the snapshot's own size wraps
    # n_positions == 0 is valid and launches nothing: no device is needed to say so
    assert S(n=0) == 0 and R(n=0) == 0 and R(sp=0, n=0) == 0


def test_host_shims_refuse_null_handles(pkg):
    h = pkg._host_lib()
    toks = (C.c_int32 * 4)(1, 2, 3, 4)
    out = C.c_uint64(0)
    m = C.c_int(0)
    assert h.bitnet_host_prefix_cache_create(4, 1 << 20, 7, 1, 60) is None  # no such policy
    assert h.bitnet_host_prefix_cache_insert(None, None, 4, 0, C.byref(out)) == INVALID
    assert h.bitnet_host_prefix_cache_lookup(None, toks, 4, C.byref(m), C.byref(out)) < 0
    assert h.bitnet_host_prefix_cache_restore(None, 0, None, 1, 0) == INVALID
    assert h.bitnet_host_prefix_cache_invalidate(None, toks, 4) < 0
    assert h.bitnet_host_prefix_cache_clear(None) == INVALID and h.bitnet_host_prefix_cache_stats(None, None) == INVALID
    assert h.bitnet_host_prefix_cache_len(None) < 0 and h.bitnet_host_prefix_cache_entry(None, 0, None, None, None) == INVALID
    assert h.bitnet_host_prefill_cached(None, None, 4, 1, 2, None, None) == INVALID
    h.bitnet_host_prefix_cache_destroy(None)
    # a cache without a device: the index side works, and the refusals that need no decoder are by message
    pc = pkg.PrefixCache(max_entries=2, max_memory_bytes=1 << 20, policy="lfu", min_prefix_length=2, ttl_seconds=60)
    assert len(pc) == 0 and pc.lookup([1, 2, 3]) is None and not pc.invalidate([1, 2])
    s = pc.stats()
    assert s == {"hit_rate": 0.0, "miss_rate": 1.0, "avg_prefix_match_length": 0.0, "eviction_count": 0, "memory_usage": 0}
    with pytest.raises(pkg.BitNetHipError, match="restore: null destination"):
        pc.restore(0, [None])
    with pytest.raises(pkg.BitNetHipError, match="restore: n_dst must be 1..8"):
        pc.restore(0, [])
    pc.clear()
    assert pc.stats()["miss_rate"] == 0.0  # clear resets the statistics
    with pytest.raises(pkg.BitNetHipError, match="policy"):
        pkg.PrefixCache(policy="mru")
    pc.close()
