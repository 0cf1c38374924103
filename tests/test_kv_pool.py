"""CPU: the paged KV cache without a device.  host/kv_pool.hpp through its stand-alone checker (tests/host/kv_pool_check.cpp, its own main, built
with AddressSanitizer and UBSan and run as a program); the refusals of the paged entry points (include/bitnet_hip_paged.h); the split rule's host
function against its stated definition."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()


def test_page_pool_checker_under_sanitizers(tmp_path):
    exe = str(tmp_path / "kv_pool_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", f"-I{os.path.join(ROOT, 'bitnet-rs_amd', 'host')}", os.path.join(ROOT, "tests", "host", "kv_pool_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and "kv_pool_check: ok" in run.stdout


def test_sizes_are_host_queries(lib):
    assert lib.kv_pool_bytes(10, 5, 128, kv_f16=True) == 10 * 5 * 64 * 64 * 4 and lib.kv_pool_bytes(10, 5, 128) == 10 * 5 * 128 * 64 * 4
    for bad in ((0, 5, 128), (10, 0, 128), (10, 5, 64), (1 << 31, 5, 128), (1 << 30, 1 << 40, 128)):
        assert lib.kv_pool_bytes(*bad) == 0, bad
    assert lib.attention_paged_scratch_bytes(3, 2, 4) == 64 * 2 * 4 + 3 * 2 * 4 * 520 * 4
    for bad in ((0, 2, 4), (65, 2, 4), (3, 0, 4), (3, 2, 0), (3, 1 << 62, 4), (64, 5, 1 << 58)):  # (the last: n_seq * n_splits wraps to 0)
        assert lib.attention_paged_scratch_bytes(*bad) == 0, bad


@pytest.mark.parametrize("n_seq,n_kv,key_bound", [(64, 5, 4096), (8, 5, 4096), (8, 5, 512), (1, 2, 64), (1, 1, 1 << 20), (3, 2, 576), (64, 16, 100)])
def test_split_rule_matches_its_definition(lib, n_seq, n_kv, key_bound):
    """n_splits = min(ceil(key_bound / 64), 16, ceil(512 / (n_seq n_kv))), at least 1 (csrc/paged_splits.hpp)"""
    want = max(1, min(-(-key_bound // 64), 16, -(-512 // (n_seq * n_kv))))
    assert lib.attention_paged_splits(n_seq, n_kv, key_bound) == want
    assert lib.attention_paged_splits(0, n_kv, key_bound) == 0 and lib.attention_paged_splits(n_seq, 0, key_bound) == 0 and lib.attention_paged_splits(n_seq, n_kv, 0) == 0


P = "a valid pointer"
MOVE = dict(n_layers=3, n_kv=2, head_dim=128, max_pos=640, n=100, flags=0, stream=None)
GOOD = {  # every entry's arguments in the header's order, all valid
    "attention_decode_paged": dict(qkv=P, sin=P, cos=P, kpool=P, vpool=P, n_pages=8, tables=P, pos=P, n_seq=3, n_heads=8, n_kv=2, head_dim=128, max_pos=640,
                                   key_bound=300, n_splits=2, scratch=P, flags=0, out=P, stream=None),
    "kv_page_in": dict(k=P, v=P, kpool=P, vpool=P, table=P, n_pages=8, **MOVE),
    "kv_page_out": dict(kpool=P, vpool=P, table=P, n_pages=8, k=P, v=P, **MOVE),
    "kv_page_copy": dict(kpool=P, vpool=P, n_pages=8, pairs=(0, 1, 2, 3, 0, 4, 5, 6), n_pairs=4, n_layers=3, n_kv=2, head_dim=128, flags=0, stream=None),
}
MOVER_BAD = [(dict(n_layers=0), "n_layers"), (dict(head_dim=64), "head_dim"), (dict(n_kv=0), "num_key_value_heads"), (dict(n=641), "KV cache overflow"),
             (dict(flags=1), "flags"), (dict(n_pages=0), "n_pages"), (dict(n_layers=1 << 30), "too large"), (dict(n_pages=1 << 31), "too large")]
BAD = [(e, {k: None}, "Null pointer") for e, g in GOOD.items() for k, v in g.items() if v is P or k == "pairs"] + [
    ("attention_decode_paged", kw, word) for kw, word in [
        (dict(n_seq=0), "n_seq"), (dict(n_seq=65), "n_seq"), (dict(head_dim=64), "head_dim"), (dict(n_heads=10), "group"), (dict(n_heads=7), "divisible"),
        (dict(flags=4), "flag"), (dict(flags=-1), "flag"), (dict(n_pages=0), "n_pages"), (dict(n_pages=1 << 40), "too large"),
        (dict(n_kv=1 << 50, n_heads=1 << 50), "too large"), (dict(key_bound=0), "key_bound"), (dict(key_bound=641), "key_bound"),
        (dict(n_splits=6), "n_splits"), (dict(max_pos=1 << 30, key_bound=1 << 30), "too large")]] + [
    (e, kw, word) for e in ("kv_page_in", "kv_page_out") for kw, word in MOVER_BAD] + [
    ("kv_page_copy", kw, word) for kw, word in [
        (dict(n_pairs=0), "n_pairs"), (dict(n_pairs=65), "n_pairs"), (dict(n_pages=6), "outside the pool"), (dict(n_pages=0), "n_pages"), (dict(flags=4), "flags"),
        # dst = src; a dst that is a later / an earlier src; two pairs into one dst
        (dict(pairs=(0, 0), n_pairs=1), "overlaps"), (dict(pairs=(0, 1, 1, 2), n_pairs=2), "overlaps"), (dict(pairs=(0, 1, 2, 1), n_pairs=2), "overlaps"),
        (dict(pairs=(1, 2, 0, 1), n_pairs=2), "overlaps")]]


@pytest.mark.parametrize("entry,bad,word", BAD, ids=lambda x: x if isinstance(x, str) else ",".join(map(str, x)) if isinstance(x, dict) else None)
def test_entries_refuse_bad_arguments_without_a_device(lib, entry, bad, word):
    buf = (C.c_uint32 * 1024)()
    args = {**GOOD[entry], **bad}
    if args.get("pairs") is not None:
        args["pairs"] = C.cast((C.c_uint32 * len(args["pairs"]))(*args["pairs"]), C.c_void_p)
    vals = [C.cast(buf, C.c_void_p) if v is P else v for v in args.values()]
    assert getattr(lib.c, f"bitnet_hip_{entry}_dev")(*vals) == INVALID and word in lib.last_error(), (entry, bad, lib.last_error())
