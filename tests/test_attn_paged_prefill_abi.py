"""CPU: the prompt attention over page tables (bitnet_hip_attention_paged_prefill_dev and its workspace size, include/bitnet_hip_pagedprefill.h)
is exported, declared and bound, refuses bad arguments before anything touches a device, and sizes its workspace from the row count alone (its
signature takes no past).  No GPU compute here."""
import ctypes as C

import numpy as np
import pytest

INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
PACK_MAX = 64
I32P = C.POINTER(C.c_int32)
GOOD = dict(n_seq=2, row0=(0, 64), ln=(5, 64), past=(0, 10), heads=(4, 2), head_dim=128, max_pos=300, n_rows=128, n_pages=8, ws_bytes=1 << 40, flags=0,
            tables=None, holes=())
# (what differs from GOOD, a piece of the message)
REFUSALS = [
    (dict(n_seq=0), "n_seq"), (dict(n_seq=PACK_MAX + 1, row0=[0] * 65, ln=[1] * 65, past=[0] * 65), "n_seq"),
    *[(dict(holes=(h,)), "Null pointer") for h in ("qkv", "sin", "cos", "row0", "len", "past", "tables", "kpool", "vpool", "ws", "out")],
    (dict(tables=(1, None)), "null table"), (dict(tables=(1, 1)), "share a table"),
    (dict(ln=(0, 64)), "len must be at least 1"), (dict(ln=(5, -1)), "len must be at least 1"), (dict(past=(0, -1)), "negative past"),
    (dict(past=(0, 237)), "KV cache overflow"), (dict(past=(296, 0)), "KV cache overflow"),
    (dict(row0=(0, 32)), "row alignment"), (dict(row0=(0, -64)), "row alignment"), (dict(heads=(2, 2)), "row alignment"),  # odd groups: 128-row tiles
    (dict(row0=(0, 0)), "overlap"), (dict(row0=(64, 0), ln=(5, 65)), "overlap"), (dict(n_rows=127), "beyond n_rows"), (dict(n_rows=0), "sizes out of range"),
    (dict(head_dim=64), "head_dim"), (dict(head_dim=256), "head_dim"),
    (dict(heads=(5, 2)), "num_key_value_heads"), (dict(heads=(4, 0)), "num_key_value_heads"), (dict(heads=(0, 2)), "num_key_value_heads"),
    (dict(heads=(10, 2)), "group 5"), (dict(heads=(8, 1)), "group 8"),
    (dict(n_pages=0), "n_pages 0"), (dict(n_pages=1 << 31), "dimensions too large"),
    (dict(flags=4), "unknown flag bits"), (dict(flags=-1), "unknown flag bits"), (dict(flags=1 | 8), "unknown flag bits"),
    (dict(ws_bytes=0), "workspace too small"), (dict(ws_bytes="need - 1"), "workspace too small"),
]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def test_symbols_are_declared_and_typed(pkg, lib):
    for name in ("bitnet_hip_attention_paged_prefill_workspace_bytes", "bitnet_hip_attention_paged_prefill_dev"):
        assert name in set(pkg.declared_symbols()) and getattr(lib.c, name).argtypes is not None, name
    assert len(lib.c.bitnet_hip_attention_paged_prefill_dev.argtypes) == 21 and lib.c.bitnet_hip_attention_paged_prefill_dev.restype is C.c_int


def test_workspace_depends_on_the_rows_alone_and_is_zero_for_invalid_sizes(lib):
    ws = lib.attention_paged_prefill_workspace_bytes
    for n_heads, n_kv in ((8, 2), (4, 2), (2, 2), (3, 3)):
        sizes = [ws(n_heads, n_kv, n) for n in (1, 128, 129, 4096)]
        assert sizes[0] == sizes[1] > 0 and sizes == sorted(sizes) and sizes[2] > sizes[1]
        assert sizes[1] == n_heads * 128 * 256 + 256 + 256  # the f16 query image of 128 rows, two block records rounded up, the alignment slack
    for bad in ((0, 2, 64), (4, 0, 64), (5, 2, 64), (10, 2, 64), (4, 2, 0), (4, 2, 1 << 24), (1 << 24, 1 << 24, 64)):
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("change,text", REFUSALS, ids=[f"{i}-{t.replace(' ', '_')}" for i, (_, t) in enumerate(REFUSALS)])
def test_refusals_come_before_any_launch(lib, change, text):
    a = dict(GOOD, **change)
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    n = max(a["n_seq"], 1)
    tables = a["tables"] or tuple(range(1, n + 1))
    tb = (C.c_void_p * len(tables))(*[None if t is None else p.value + 64 * t for t in tables])
    i32 = lambda x: np.ascontiguousarray(x, np.int32).ctypes.data_as(I32P)
    args = {"qkv": p, "sin": p, "cos": p, "row0": i32(a["row0"]), "len": i32(a["ln"]), "past": i32(a["past"]), "tables": tb, "kpool": p, "vpool": p, "ws": p, "out": p}
    for h in a["holes"]:
        args[h] = None
    ws_bytes = a["ws_bytes"]
    if ws_bytes == "need - 1":
        ws_bytes = lib.attention_paged_prefill_workspace_bytes(*a["heads"], a["n_rows"]) - 1
        assert ws_bytes > 0
    rc = lib.c.bitnet_hip_attention_paged_prefill_dev(args["qkv"], a["n_rows"], args["sin"], args["cos"], a["n_seq"], args["row0"], args["len"], args["past"],
                                                      args["tables"], args["kpool"], args["vpool"], a["n_pages"], a["heads"][0], a["heads"][1], a["head_dim"],
                                                      a["max_pos"], args["ws"], ws_bytes, args["out"], a["flags"], None)
    assert rc == INVALID and text in lib.last_error(), (change, lib.last_error())
