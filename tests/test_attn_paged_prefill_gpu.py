"""GPU: the prompt attention over page tables (bitnet_hip_attention_paged_prefill_dev, csrc/kernels_prefill_paged.hip: k_paged_prefill_prep +
k_prefill_attn_paged<HW, KV16>) by value against the float64 model tests/attn_ref.py -- its operands (the packed path's by definition), its
families, its per-element tolerance tol().

No further tolerance term.  The kernel differs from the modelled loop in moving its reference point in every tile: one more rounding (2^-24
relative) of each output accumulator and of l per key tile, at most 6 tiles here = 6 * 2^-23 of sum_j p_j |v_jd|, inside the factor 2 tol() keeps
over the 2^-11 of the f16 probabilities.  Probabilities are taken relative to the running maximum (<= 1), as the model's are.

Every call carries three segments in non-table row order over permuted, interleaved page tables; table entries past a context hold 0xFFFFFFFF;
every stale slot and every unnamed page holds hostile finite values (f32 pools: 3e38, which f16 would turn into inf).  Checked per call: the
rows; the appended slots, bit for bit, against bitnet_hip_attention_packed_dev on contiguous caches + bitnet_hip_kv_page_in_dev from the same
inputs; every other pool byte against its planted value; every output row up to n_rows finite.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_ref as ar  # noqa: E402
from kv_read import bits  # noqa: E402
from test_attn_paged_gpu import N_KV, N_PAGES, decode_k, encode  # noqa: E402  (the pool's word order, stated once)

pytestmark = pytest.mark.gpu

D, MAX_POS, NOWHERE = 128, 384, 0xFFFFFFFF
ENTRIES = MAX_POS // 64
# (past, len): new rows from position 0 over four pages | starting mid-page and ending exactly on a page end | one row;
# spanning three pages from mid-page | ending on the first page's end | a whole page from a page start;
# two segments that share their first page read-only (a fork) | four pages from mid-page
SETS = {"mixed": [(0, 200), (63, 65), (130, 1)], "edges": [(65, 129), (1, 63), (64, 64)], "forked": [(64, 63), (64, 1), (130, 200)]}
ORDER = (2, 0, 1)  # row order of the segments: not the table's
CASES = {}


@pytest.fixture(scope="module")
def rig(hip, oracle):
    import torch

    sin, cos = oracle.rope_tables(D, MAX_POS, 10000.0)
    sin, cos = np.asarray(sin, np.float32).reshape(MAX_POS, D // 2), np.asarray(cos, np.float32).reshape(MAX_POS, D // 2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(hip=hip, t=torch, sin=sin, cos=cos, sin_d=dev(sin), cos_d=dev(cos), dev=dev)


def case(rig, H, name, set_name, kv16):
    """inputs and the model's rows of one (heads, family, segment set, pool type), computed once"""
    key = (H, name, set_name, kv16)
    if key in CASES:
        return CASES[key]
    sin, cos, dt = rig["sin"], rig["cos"], np.float16 if kv16 else np.float32
    segs = []
    for s, (past, n) in enumerate(SETS[set_name]):
        T, pos = past + n, np.arange(past, past + n)
        q1, k1, v, _ = ar.family(name, np.random.default_rng(ar.seed_of("pagedprefill", H, name, set_name, s)), pos, T, H, N_KV)
        k_c, v_c = k1[:past].astype(dt), v[:past].astype(dt)  # the past as the pool holds it
        if set_name == "forked" and s == 1:
            k_c, v_c = segs[0]["k_c"], segs[0]["v_c"]  # the shared page
        q_in, k_in, v_in = ar.unrope(q1, pos, sin, cos), ar.unrope(k1[past:], pos, sin, cos), v[past:].astype(np.float32)
        kh = np.concatenate([ar.f16(k_c), ar.operands_k(k_in, pos, sin, cos)])
        vh = np.concatenate([ar.f16(v_c), ar.operands_v(v_in)])
        qh = ar.operands_q(q_in, pos, sin, cos)
        segs.append(dict(past=past, n=n, k_c=k_c, v_c=v_c, qkv=np.concatenate([q_in.reshape(n, -1), k_in.reshape(n, -1), v_in.reshape(n, -1)], axis=1),
                         model={o16: ar.model(qh, kh, vh, pos, out_f16=o16)[:2] for o16 in (False, True)}))
    CASES[key] = segs
    return segs


def run(rig, H, kv16, out_f16, name, set_name, idle=None):
    t, hip, dev = rig["t"], rig["hip"], rig["dev"]
    segs = case(rig, H, name, set_name, kv16)
    align = hip.attention_packed_row_align(H, N_KV)
    row0, cursor = [0] * 3, 0
    for s in ORDER:
        row0[s], cursor = cursor, cursor + -(-segs[s]["n"] // align) * align
    n_rows = row0[ORDER[-1]] + segs[ORDER[-1]]["n"]  # the last segment's padding is not part of the call
    lens, pasts = [g["n"] for g in segs], [g["past"] for g in segs]
    perm = np.random.default_rng(ar.seed_of("tables", set_name, H)).permutation(N_PAGES).astype(np.uint32)
    tables = [perm[s::3][:ENTRIES].copy() for s in range(3)]
    if set_name == "forked":
        tables[1][0] = tables[0][0]
    hostile = (6.0e4, -6.0e4) if kv16 else (3.0e38, -3.0e38)
    dt = np.float16 if kv16 else np.float32
    K0, V0 = np.full((N_PAGES, N_KV, 64, D), hostile[0], dt), np.full((N_PAGES, N_KV, 64, D), hostile[1], dt)
    qkv = np.full((n_rows, (H + 2 * N_KV) * D), np.nan, np.float32)
    for g, tbl, r0 in zip(segs, tables, row0):
        for p in range(g["past"]):
            K0[tbl[p // 64], :, p % 64], V0[tbl[p // 64], :, p % 64] = g["k_c"][p], g["v_c"][p]
        qkv[r0:r0 + g["n"]] = g["qkv"]
        tbl[(g["past"] + g["n"] - 1) // 64 + 1:] = NOWHERE
    good = [tb.copy() for tb in tables]
    if idle is not None:
        tables[idle][(pasts[idle] + lens[idle] - 1) // 64 // 2] = N_PAGES  # the first id outside the pool, inside the context
    kflat, vflat = encode(K0, V0, kv16)
    kpool, vpool, qkv_d = dev(kflat), dev(vflat), dev(qkv)
    flags = (1 if kv16 else 0) | (2 if out_f16 else 0)
    wsb = hip.attention_paged_prefill_workspace_bytes(H, N_KV, n_rows)
    ws = t.empty(wsb, dtype=t.uint8, device="cuda")
    out = t.full((n_rows, H * D), float("nan"), dtype=t.float16 if out_f16 else t.float32, device="cuda")
    tab_d = [dev(tb) for tb in tables]
    hip.attention_paged_prefill_dev(qkv_d, n_rows, rig["sin_d"], rig["cos_d"], row0, lens, pasts, tab_d, kpool, vpool, N_PAGES, H, N_KV, D, MAX_POS, ws, wsb, out,
                                    flags=flags)
    # the contiguous path from the same inputs, moved into a second copy of the planted pools
    words = N_KV * ENTRIES * 64 * D
    kc, vc = [t.zeros(words, dtype=t.float32, device="cuda") for _ in segs], [t.zeros(words, dtype=t.float32, device="cuda") for _ in segs]
    wsb2 = hip.attention_packed_workspace_bytes(H, N_KV, n_rows, pasts, lens)
    ws2, out2 = t.empty(wsb2, dtype=t.uint8, device="cuda"), t.empty((n_rows, H * D), dtype=out.dtype, device="cuda")
    hip.attention_packed_dev(qkv_d, n_rows, rig["sin_d"], rig["cos_d"], row0, lens, pasts, kc, vc, H, N_KV, D, MAX_POS, ws2, wsb2, out2, flags=flags)
    kpool2, vpool2 = dev(kflat), dev(vflat)
    ptr = lambda x: t.tensor([x.data_ptr()], dtype=t.int64, device="cuda")
    for g, k_c, v_c, tb in zip(segs, kc, vc, good):
        hip.kv_page_in_dev(ptr(k_c), ptr(v_c), ptr(kpool2), ptr(vpool2), dev(tb), N_PAGES, 1, N_KV, D, MAX_POS, g["past"] + g["n"], kv_f16=kv16)
    t.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "every output row, padding and idle ones too, is finite"
    K1, V1 = decode_k(kpool.cpu().numpy(), kv16), vpool.cpu().numpy().reshape(N_PAGES, N_KV, 64, D)
    K2, V2 = decode_k(kpool2.cpu().numpy(), kv16), vpool2.cpu().numpy().reshape(N_PAGES, N_KV, 64, D)
    may_k, may_v = np.zeros(K1.shape[:3] + (1,), bool), np.zeros(K1.shape[:3] + (1,), bool)
    for s, (g, tb, r0) in enumerate(zip(segs, good, row0)):
        if s == idle:
            continue
        tag = (name, set_name, H, kv16, out_f16, s, idle)
        want, tol = g["model"][out_f16]
        r = float(np.max(np.abs(got[r0:r0 + g["n"]].reshape(g["n"], H, D) - want) / tol))
        print(f"PAGED-PREFILL {tag}: err/tol {r:.4f}")
        assert r <= 1.0, (tag, "rows", r)
        p = np.arange(g["past"], g["past"] + g["n"])
        pg, sl = tb[p // 64].astype(np.int64), p % 64
        assert np.array_equal(bits(K1[pg, :, sl]), bits(K2[pg, :, sl])), (tag, "appended keys differ from the contiguous path's")
        assert np.array_equal(bits(V1[pg, :, sl]), bits(V2[pg, :, sl])), (tag, "appended values differ from the contiguous path's")
        may_k[pg, :, sl], may_v[pg, :, sl] = True, True
    assert not ((bits(K1) != bits(K0)) & ~may_k).any() and not ((bits(V1) != bits(V0)) & ~may_v).any(), "a pool byte outside the appended slots changed"


@pytest.mark.parametrize("out_f16", (False, True), ids=("o32", "o16"))
@pytest.mark.parametrize("set_name", sorted(SETS))
@pytest.mark.parametrize("H", (8, 4, 2), ids=("g4", "g2", "g1"))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_paged_prefill_by_value(rig, kv16, H, set_name, out_f16):
    for name in ("gauss", "sunk", "needle"):
        run(rig, H, kv16, out_f16, name, set_name)


@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_a_segment_with_a_page_id_outside_the_pool_is_idle(rig, kv16):
    """segment 0 (the longest) names page id n_pages inside its range: none of its pages changes (run() holds every pool byte outside the other
    segments' appended slots to its planted value), its rows are finite, and the other two segments are held to the model and the bits as ever"""
    run(rig, 8, kv16, False, "gauss", "mixed", idle=0)
