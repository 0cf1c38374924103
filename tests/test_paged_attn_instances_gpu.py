"""GPU: every instance and walk of the three paged attention entries that their feature tests leave unrun, by value against the float64 models
(tests/attn_decode_ref.py for bitnet_hip_attention_decode_paged_dev and bitnet_hip_attention_decode_paged_shared_dev, tests/attn_ref.py for
bitnet_hip_attention_paged_prefill_dev).  The conditions are the tables of tests/paged_attn_cases.py (tests/test_paged_attn_cases.py holds each
table to the code path it exists for): head group 3, full batches of 64, key_bound < max_pos, walks past the 256 page ids a workgroup keeps in
LDS, one-token prompts, more new page tiles than row blocks, full and uneven MFMA row tiles, idle leaders, dead groups, the broken promise.

Every case keeps the older tests' checks: hostile stale slots and unnamed pages, scattered non-monotone page ids with 0xFFFFFFFF past a context, the
rows by value, the appended key and value, every other pool byte unchanged, the arrival counters back at 0, a second launch with the same bits,
idle rows untouched (NaN fill: decode, shared) or finite (prefill).  Output type: f16 rows go with f16 pools unless a test crosses them.

Tolerances, none new (paged_attn_cases.decode_tol / prefill_case):
  decode   dr.tol + 2^-23 (pages + n_splits) sum_j p_j |v_jd|, pages = pos // 64 + 1 (259 in the id-cap case: the formula's own growth);
  shared   the same with n_shared_splits more records, plus extra_tol on the shared keys;
  prefill  attn_ref.tol + n_tiles 2^-23 sum_j p_j |v_jd|: the per-tile rescale the older test argues into tol()'s factor 2 at 6 tiles, here a
           stated term, so that the 258-tile walk rests on a bound and not on slack.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_decode_ref as dr  # noqa: E402
import attn_ref as ar  # noqa: E402
import paged_attn_cases as pc  # noqa: E402
from kv_read import bits  # noqa: E402
from paged_attn_cases import D, NOWHERE  # noqa: E402

pytestmark = pytest.mark.gpu

REC_FLOATS = 8 + 4 * D
KV = pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))


class Rig:
    def __init__(self, hip, oracle, torch):
        self.hip, self.t, self.oracle, self.ropes = hip, torch, oracle, {}

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def rope(self, max_pos):
        """-> ((sin, cos) [max_pos, D / 2] on the host, sin and cos on the device), once per max_pos"""
        if max_pos not in self.ropes:
            sin, cos = self.oracle.rope_tables(D, max_pos, 10000.0)
            sin, cos = np.asarray(sin, np.float32).reshape(max_pos, D // 2), np.asarray(cos, np.float32).reshape(max_pos, D // 2)
            self.ropes[max_pos] = ((sin, cos), self.dev(sin), self.dev(cos))
        return self.ropes[max_pos]

    def ptrs(self, n, base, stride, null=()):
        """int64 device tensor of the n pointers base + s * stride, 0 where s is in `null`"""
        return self.t.tensor([0 if s in null else base + s * stride for s in range(n)], dtype=self.t.int64, device="cuda")


@pytest.fixture(scope="module")
def rig(hip, oracle):
    import torch

    return Rig(hip, oracle, torch)


def check_appended(ref, gk, gv, kv16, tag):
    """slot pos % 64 of page table[pos // 64]: gk / gv [kv, D] as the pool holds them"""
    gk, kn = gk.astype(np.float64), ref["kn"]
    if kv16:  # the nearest f16 of the float64 rotation or its neighbour; the value's exact rounding
        near = dr.f16(kn)
        ulp = np.maximum(np.spacing(np.abs(near).astype(np.float16)), np.spacing(np.abs(gk).astype(np.float16))).astype(np.float64)
        assert np.all(np.abs(gk - near) <= ulp), (tag, "appended key")
        assert np.array_equal(bits(gv), bits(ref["vn"].astype(np.float16))), (tag, "appended value")
    else:  # three f32 roundings of x0 c -+ x1 s
        pair = np.hypot(kn[:, : D // 2], kn[:, D // 2:])
        assert np.all(np.abs(gk - kn) <= 2.0 ** -22 * np.concatenate([pair, pair], axis=1)), (tag, "appended key")
        assert np.array_equal(bits(gv), bits(ref["vn"])), (tag, "appended value")


def plant(refs, tables, n_pages, n_kv):
    """logical pools [page, kv, 64, D] in the cache's dtype: hostile everywhere (the first row's stale values), then each row's past below its
    position in the pages its table names, its own stale values behind (a page named twice -- a full page of a shared run -- gets the same words twice)"""
    ks0, vs0 = refs[0]["stale"]
    K = np.broadcast_to(ks0[None, :, None, :], (n_pages, n_kv, 64, D)).copy()
    V = np.broadcast_to(vs0[None, :, None, :], (n_pages, n_kv, 64, D)).copy()
    for ref, tb in zip(refs, tables):
        for c in range(pc.pages(ref["pos"])):
            pg, live = int(tb[c]), max(0, min(64, ref["pos"] - 64 * c))
            K[pg], V[pg] = ref["stale"][0][:, None, :], ref["stale"][1][:, None, :]
            K[pg, :, :live], V[pg, :, :live] = ref["kp"][:, 64 * c:64 * c + live], ref["vp"][:, 64 * c:64 * c + live]
    return K, V


# =============================================================== the decode entry ===============================================================
def decode_run(rig, tag, cfg, kv16, out_f16, n_splits, name, positions, idle=None, seed=0):
    """one launch of len(positions) sequences; idle {row: 'table' | 'page'}; rows at or past cfg's key_bound are idle too.  -> worst err / tol"""
    t, hip, idle = rig.t, rig.hip, idle or {}
    H, n_kv, max_pos = cfg["H"], cfg["n_kv"], cfg["max_pos"]
    key_bound, n = cfg.get("key_bound", max_pos), len(positions)
    rope, sin_d, cos_d = rig.rope(max_pos)
    refs = [pc.decode_ref(rope, tag, kv16, H, n_kv, name, p, s, max_pos) for s, p in enumerate(positions)]
    n_pages = sum(pc.pages(p) for p in positions) + 3  # three pages nobody names
    perm = pc.deal(dr.seed_of("inst-pages", tag, seed), n_pages)
    tables = np.full((n, max_pos // 64), NOWHERE, np.uint32)
    for s, p in enumerate(positions):
        tables[s, :pc.pages(p)] = [next(perm) for _ in range(pc.pages(p))]
    K0, V0 = plant(refs, tables, n_pages, n_kv)
    tab_host = tables.copy()
    for s, kind in idle.items():
        if kind == "page":
            tab_host[s, positions[s] // 64 // 2] = n_pages  # the first id outside the pool, inside the context
    live = [s not in idle and p < key_bound for s, p in enumerate(positions)]
    kflat, vflat = pc.encode(K0, V0, kv16)
    kpool, vpool, tab_d = rig.dev(kflat), rig.dev(vflat), rig.dev(tab_host)
    pos_d = t.tensor(positions, dtype=t.int32, device="cuda")
    tp, pp = rig.ptrs(n, tab_d.data_ptr(), 4 * tables.shape[1], {s for s, k in idle.items() if k == "table"}), rig.ptrs(n, pos_d.data_ptr(), 4)
    qkv_d = rig.dev(np.stack([r["qkv"] for r in refs]))
    asked, n_splits = n_splits, n_splits or hip.attention_paged_splits(n, n_kv, key_bound)  # 0: the library's rule, the scratch sized by its report
    sb = hip.attention_paged_scratch_bytes(n, n_kv, n_splits)
    assert sb == 64 * n_kv * 4 + n * n_kv * n_splits * REC_FLOATS * 4
    scratch = t.zeros(sb // 4, dtype=t.float32, device="cuda")
    scratch[64 * n_kv:] = 1.0e6  # hostile records behind the zeroed counters
    odt, view = (t.float16, np.uint16) if out_f16 else (t.float32, np.uint32)
    outs = []
    for _ in range(2):  # the second launch: the same scratch, the same bits
        out = t.full((n, H * D), float("nan"), dtype=odt, device="cuda")
        hip.attention_decode_paged_dev(qkv_d, sin_d, cos_d, kpool, vpool, n_pages, tp, pp, n, H, n_kv, D, max_pos, key_bound, asked, scratch, out,
                                       kv_f16=kv16, out_f16=out_f16)
        t.cuda.synchronize()
        assert int(scratch[: 64 * n_kv].view(t.int32).abs().sum().item()) == 0, "arrival counters not back at 0"
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(view), outs[1].view(view)), "a replay changed the bits"
    K1, V1 = pc.decode_k(kpool.cpu().numpy(), kv16, n_pages, n_kv), vpool.cpu().numpy().reshape(n_pages, n_kv, 64, D)
    changed_k, changed_v = bits(K1) != bits(K0), bits(V1) != bits(V0)
    worst = 0.0
    for s, (ref, pos) in enumerate(zip(refs, positions)):
        tag_s = (tag, name, kv16, out_f16, n_splits, s, pos)
        if not live[s]:
            assert np.isnan(outs[0][s].astype(np.float32)).all(), (tag_s, "output row of an idle sequence")
            continue
        got = outs[0][s].reshape(H, D).astype(np.float64)
        r = dr.ratio(got, ref["out"], pc.decode_tol(ref, n_splits, out_f16))
        assert r <= 1.0, (tag_s, "rows", r)
        worst = max(worst, r)
        if name == "needle" and not out_f16:
            assert np.array_equal(got, ref["vt"]), (tag_s, "needle rows are v[t(h)] to the last bit")
        pg, sl = int(tables[s, pos // 64]), pos % 64
        check_appended(ref, K1[pg, :, sl], V1[pg, :, sl], kv16, tag_s)
        changed_k[pg, :, sl], changed_v[pg, :, sl] = False, False
    assert not changed_k.any() and not changed_v.any(), (tag, "a pool byte outside the appended slots changed")
    print(f"INST decode {tag} {name} kv16={kv16} o16={out_f16} splits={n_splits}: err/tol {worst:.4f}")
    return worst


@pytest.mark.parametrize("out_f16", (False, True), ids=("o32", "o16"))
@pytest.mark.parametrize("n_splits", pc.G3["n_splits"])
@KV
def test_decode_group_3(rig, kv16, n_splits, out_f16):
    """H = 6 over 2 KV heads: wave 3 rotates a clamped head, contributes zeros and writes no row"""
    for pos in pc.G3["positions"]:
        for name in pc.G3["families"]:
            decode_run(rig, "g3", pc.G3, kv16, out_f16, n_splits, name, (pos,) + pc.G3["companions"], seed=pos + 7 * n_splits)


@KV
def test_decode_full_batch(rig, kv16):
    """64 sequences, one arrival counter per (sequence, KV head): all 128 back at 0 (decode_run reads every counter word); rows 5 and 40 idle"""
    for name in pc.FULL["families"]:
        decode_run(rig, "full", pc.FULL, kv16, kv16, pc.FULL["n_splits"], name, pc.FULL["positions"], idle=pc.FULL["idle"])


@pytest.mark.parametrize("n_splits", pc.BOUND["n_splits"])
@KV
def test_decode_key_bound_below_max_pos(rig, kv16, n_splits):
    """key_bound 200 under max_pos 576: the row at 199 is live, the rows at 200 and 575 are idle and untouched; n_splits 0 is the rule's answer
    for the BOUND (4 = ceil(200 / 64), the most the entry takes: tests/test_paged_attn_cases.py has the refusal of 5)"""
    assert rig.hip.attention_paged_splits(len(pc.BOUND["positions"]), pc.BOUND["n_kv"], pc.BOUND["key_bound"]) == 4
    for name in pc.BOUND["families"]:
        decode_run(rig, "bound", pc.BOUND, kv16, kv16, n_splits, name, pc.BOUND["positions"])


@pytest.mark.parametrize("n_splits", pc.IDCAP["n_splits"])
@KV
def test_decode_walk_past_the_id_cap(rig, kv16, n_splits):
    """258 pages: one split reads the ids of pages 256 and 257 from the table again, two splits own 129 each and do not; both hold to the model"""
    for name in pc.IDCAP["families"]:
        decode_run(rig, "idcap", pc.IDCAP, kv16, kv16, n_splits, name, pc.IDCAP["positions"])


# =============================================================== the prefill entry ==============================================================
def prefill_run(rig, H, n_kv, kv16, out_f16, name, set_name, max_pos=384, idle=()):
    """one call over the segment set; idle: segments that name page id n_pages inside their range.  The appended slots are compared bit for bit
    with bitnet_hip_attention_packed_dev on contiguous caches + bitnet_hip_kv_page_in_dev from the same inputs, for every segment of every set
    (the 258-tile one too: its twin caches are 8 MB each)."""
    t, hip, dev = rig.t, rig.hip, rig.dev
    rope, sin_d, cos_d = rig.rope(max_pos)
    segs, order = pc.prefill_case(rope, H, n_kv, name, set_name, kv16), pc.prefill_order(set_name)
    spec, entries = pc.prefill_segs(set_name), max_pos // 64
    align = hip.attention_packed_row_align(H, n_kv)
    row0, n_rows = pc.packed_rows(spec, order, align)
    lens, pasts = [g["n"] for g in segs], [g["past"] for g in segs]
    n_pages = sum(pc.pages(p + n - 1) for p, n in spec) + 3
    perm = pc.deal(ar.seed_of("inst-tables", set_name, H), n_pages)
    tables = []
    for past, n in spec:
        tb = np.full(entries, NOWHERE, np.uint32)
        tb[:pc.pages(past + n - 1)] = [next(perm) for _ in range(pc.pages(past + n - 1))]
        tables.append(tb)
    for a, b in pc.forks_of(set_name):
        tables[b][0] = tables[a][0]
    hostile = (6.0e4, -6.0e4) if kv16 else (3.0e38, -3.0e38)
    dt = np.float16 if kv16 else np.float32
    K0, V0 = np.full((n_pages, n_kv, 64, D), hostile[0], dt), np.full((n_pages, n_kv, 64, D), hostile[1], dt)
    qkv = np.full((n_rows, (H + 2 * n_kv) * D), np.nan, np.float32)
    for g, tbl, r0 in zip(segs, tables, row0):
        p = np.arange(g["past"])
        K0[tbl[p // 64].astype(np.int64), :, p % 64], V0[tbl[p // 64].astype(np.int64), :, p % 64] = g["k_c"], g["v_c"]
        qkv[r0:r0 + g["n"]] = g["qkv"]
    good = [tb.copy() for tb in tables]
    for s in idle:
        tables[s][(pasts[s] + lens[s] - 1) // 64 // 2] = n_pages  # the first id outside the pool, inside the context
    kflat, vflat = pc.encode(K0, V0, kv16)
    kpool, vpool, qkv_d = dev(kflat), dev(vflat), dev(qkv)
    flags = (1 if kv16 else 0) | (2 if out_f16 else 0)
    wsb = hip.attention_paged_prefill_workspace_bytes(H, n_kv, n_rows)
    ws = t.empty(wsb, dtype=t.uint8, device="cuda")
    out = t.full((n_rows, H * D), float("nan"), dtype=t.float16 if out_f16 else t.float32, device="cuda")
    tab_d = [dev(tb) for tb in tables]
    hip.attention_paged_prefill_dev(qkv_d, n_rows, sin_d, cos_d, row0, lens, pasts, tab_d, kpool, vpool, n_pages, H, n_kv, D, max_pos, ws, wsb, out, flags=flags)
    # the contiguous path from the same inputs, moved into a second copy of the planted pools
    words = n_kv * entries * 64 * D
    kc, vc = [t.zeros(words, dtype=t.float32, device="cuda") for _ in segs], [t.zeros(words, dtype=t.float32, device="cuda") for _ in segs]
    wsb2 = hip.attention_packed_workspace_bytes(H, n_kv, n_rows, pasts, lens)
    ws2, out2 = t.empty(wsb2, dtype=t.uint8, device="cuda"), t.empty((n_rows, H * D), dtype=out.dtype, device="cuda")
    hip.attention_packed_dev(qkv_d, n_rows, sin_d, cos_d, row0, lens, pasts, kc, vc, H, n_kv, D, max_pos, ws2, wsb2, out2, flags=flags)
    kpool2, vpool2 = dev(kflat), dev(vflat)
    ptr = lambda x: t.tensor([x.data_ptr()], dtype=t.int64, device="cuda")  # noqa: E731
    for g, k_c, v_c, tb in zip(segs, kc, vc, good):
        hip.kv_page_in_dev(ptr(k_c), ptr(v_c), ptr(kpool2), ptr(vpool2), dev(tb), n_pages, 1, n_kv, D, max_pos, g["past"] + g["n"], kv_f16=kv16)
    t.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "every output row, padding and idle ones too, is finite"
    K1, V1 = pc.decode_k(kpool.cpu().numpy(), kv16, n_pages, n_kv), vpool.cpu().numpy().reshape(n_pages, n_kv, 64, D)
    K2, V2 = pc.decode_k(kpool2.cpu().numpy(), kv16, n_pages, n_kv), vpool2.cpu().numpy().reshape(n_pages, n_kv, 64, D)
    may_k, may_v = np.zeros(K1.shape[:3] + (1,), bool), np.zeros(K1.shape[:3] + (1,), bool)
    worst = 0.0
    for s, (g, tb, r0) in enumerate(zip(segs, good, row0)):
        if s in idle:
            continue
        tag = (name, set_name, H, kv16, out_f16, s)
        want, tol = g["model"][out_f16]
        r = float(np.max(np.abs(got[r0:r0 + g["n"]].reshape(g["n"], H, D) - want) / tol))
        assert r <= 1.0, (tag, "rows", r)
        worst = max(worst, r)
        p = np.arange(g["past"], g["past"] + g["n"])
        pg, sl = tb[p // 64].astype(np.int64), p % 64
        assert np.array_equal(bits(K1[pg, :, sl]), bits(K2[pg, :, sl])), (tag, "appended keys differ from the contiguous path's")
        assert np.array_equal(bits(V1[pg, :, sl]), bits(V2[pg, :, sl])), (tag, "appended values differ from the contiguous path's")
        may_k[pg, :, sl], may_v[pg, :, sl] = True, True
    assert not ((bits(K1) != bits(K0)) & ~may_k).any() and not ((bits(V1) != bits(V0)) & ~may_v).any(), "a pool byte outside the appended slots changed"
    print(f"INST prefill {set_name} H={H} {name} kv16={kv16} o16={out_f16}: err/tol {worst:.4f}")
    return n_rows


PREFILL_FAMILIES = ("gauss", "sunk", "needle")


@pytest.mark.parametrize("set_name", ("edges", "forked", "mixed", "tiny"))
@KV
def test_prefill_group_3(rig, kv16, set_name):
    """H = 6 over 2 KV heads: the HW = 1 instance with kvh = h / 3, 128-row alignment; 'tiny' brings T = 1 and T % 4 = 0 .. 3 past a page's first unit"""
    for name in PREFILL_FAMILIES:
        prefill_run(rig, 6, 2, kv16, kv16, name, set_name)


@pytest.mark.parametrize("H", (8, 4, 2), ids=("g4", "g2", "g1"))
@KV
def test_prefill_tiny_segments(rig, kv16, H):
    for name in PREFILL_FAMILIES:
        prefill_run(rig, H, 2, kv16, kv16, name, "tiny")


@KV
def test_prefill_more_new_tiles_than_row_blocks(rig, kv16):
    """the prep grid's width is the new page tiles, not the 64-row blocks: asserted here from the library's own alignment and the lengths"""
    spec = pc.prefill_segs("straddle")
    for name in PREFILL_FAMILIES:
        n_rows = prefill_run(rig, 8, 2, kv16, kv16, name, "straddle")
        assert rig.hip.attention_packed_row_align(8, 2) == 64 and pc.new_tiles(spec) > -(-n_rows // 128) * 128 // 64


@KV
def test_prefill_64_segments(rig, kv16):
    """BITNET_HIP_PACK_MAX segments, five forked first pages, two idle segments, rows not in table order"""
    for name in PREFILL_FAMILIES:
        prefill_run(rig, 8, 2, kv16, kv16, name, "wide", idle=pc.WIDE["idle"])


@KV
def test_prefill_walk_past_the_id_cap(rig, kv16):
    """key tiles 256 and 257 come through the table; 'steep' puts a third of the mass there"""
    for name in ("gauss", "steep"):
        prefill_run(rig, 2, 1, kv16, kv16, name, "idcap", max_pos=258 * 64)


# =============================================================== the shared entry ===============================================================
def shared_run(rig, cname, kv16, out_f16, name, share=True):
    """one case through the shared entry (share=False: its runs declared as 0) -> (refs, live, out rows, the paged entry's rows on a twin pool)"""
    t, hip, case = rig.t, rig.hip, pc.SHARED[cname]
    H, n_kv, max_pos, key_bound, runs, rows = (case[k] for k in ("H", "n_kv", "max_pos", "key_bound", "runs", "rows"))
    n_splits, nss = case["n_splits"], case["nss"] if share else 0
    rope, sin_d, cos_d = rig.rope(max_pos)
    targets = pc.IDCAP_TARGETS if (cname, name) == ("idcap", "needle") else None
    refs = [pc.decode_ref(rope, ("shared", cname), kv16, H, n_kv, name, pos, r, max_pos, group=gi, S=runs[gi] if gi is not None else 0, targets=targets)
            for r, (gi, pos, _) in enumerate(rows)]
    n, live = len(rows), pc.shared_live(case)
    run_len = lambda gi, pos: 0 if gi is None else min(runs[gi], pos >> 6)  # noqa: E731  (the page that takes the append is never the run's)
    n_pages = sum(runs.values()) + sum(pc.pages(pos) - run_len(gi, pos) for gi, pos, _ in rows) + 3
    perm = pc.deal(dr.seed_of("inst-pages", cname), n_pages)
    run_pages = {gi: [next(perm) for _ in range(S)] for gi, S in runs.items()}
    tables, leader_of, leader, shared = np.full((n, max_pos // 64), NOWHERE, np.uint32), {}, [], []
    for r, (gi, pos, idle) in enumerate(rows):
        leader_of.setdefault(gi, r)
        tables[r, :pc.pages(pos)] = [run_pages[gi][c] if c < run_len(gi, pos) else next(perm) for c in range(pc.pages(pos))]
        leader.append(r if gi is None else leader_of[gi])
        shared.append(runs[gi] if share and gi is not None else 0)
    K0, V0 = plant(refs, tables, n_pages, n_kv)
    tab_host = tables.copy()
    for r, (gi, pos, idle) in enumerate(rows):
        if idle == "page":
            tab_host[r, pos // 64] = n_pages  # in its private tail
    kflat, vflat = pc.encode(K0, V0, kv16)
    tab_d, pos_d = rig.dev(tab_host), t.tensor([pos for _, pos, _ in rows], dtype=t.int32, device="cuda")
    tp = rig.ptrs(n, tab_d.data_ptr(), 4 * tables.shape[1], {r for r, row in enumerate(rows) if row[2] == "table"})
    pp = rig.ptrs(n, pos_d.data_ptr(), 4, {r for r, row in enumerate(rows) if row[2] == "pos"})
    qkv_d = rig.dev(np.stack([ref["qkv"] for ref in refs]))
    scratch = t.zeros(hip.attention_paged_shared_scratch_bytes(n, n_kv, n_splits, nss) // 4, dtype=t.float32, device="cuda")
    scratch[64 * n_kv:] = 1.0e6  # hostile records behind the zeroed counters
    odt, view = (t.float16, np.uint16) if out_f16 else (t.float32, np.uint32)
    pools, outs = [], []
    for twin in (False, True, None):  # the shared entry, the paged entry on a twin pool, the shared entry again on the stepped pool
        kpool, vpool = (rig.dev(kflat), rig.dev(vflat)) if twin is not None else pools[0]
        out = t.full((n + 1, H * D), float("nan"), dtype=odt, device="cuda")  # a guard row behind the output rows
        if twin:
            hip.attention_decode_paged_dev(qkv_d, sin_d, cos_d, kpool, vpool, n_pages, tp, pp, n, H, n_kv, D, max_pos, key_bound, n_splits, scratch, out,
                                           kv_f16=kv16, out_f16=out_f16)
        else:
            hip.attention_decode_paged_shared_dev(qkv_d, sin_d, cos_d, kpool, vpool, n_pages, tp, pp, n, H, n_kv, D, max_pos, key_bound, n_splits, scratch, out,
                                                  leader, shared, nss, kv_f16=kv16, out_f16=out_f16)
        t.cuda.synchronize()
        assert int(scratch[: 64 * n_kv].view(t.int32).abs().sum().item()) == 0, "arrival counters not back at 0"
        pools.append((kpool, vpool))
        outs.append(out.cpu().numpy())
        assert np.isnan(outs[-1][n].astype(np.float32)).all(), "something was written behind the output rows"
    assert np.array_equal(outs[0].view(view), outs[2].view(view)), "a second launch changed the bits"
    k1, v1, k2, v2 = (x.cpu().numpy() for x in pools[0] + pools[1])
    assert np.array_equal(bits(k1), bits(k2)) and np.array_equal(bits(v1), bits(v2)), "the pools differ from the paged entry's twin"
    K1, V1 = pc.decode_k(k1, kv16, n_pages, n_kv), v1.reshape(n_pages, n_kv, 64, D)
    ck, cv = bits(K1) != bits(K0), bits(V1) != bits(V0)
    for r, (ref, (gi, pos, _)) in enumerate(zip(refs, rows)):
        if live[r]:  # slot pos % 64 of page table[pos // 64], and nothing else
            pg, sl = int(tables[r, pos // 64]), pos % 64
            check_appended(ref, K1[pg, :, sl], V1[pg, :, sl], kv16, (cname, name, r))
            ck[pg, :, sl], cv[pg, :, sl] = False, False
    assert not ck.any() and not cv.any(), "a pool byte outside the live rows' appended slots changed"
    return refs, live, outs[0][:n], outs[1][:n]


def shared_case(rig, cname, kv16):
    """every family of a case, rows by value (an unchecked group: only what the header promises, which shared_run has asserted)"""
    case, out_f16 = pc.SHARED[cname], kv16
    for name in case["families"]:
        refs, live, got, _ = shared_run(rig, cname, kv16, out_f16, name)
        worst = 0.0
        for r, (ref, (gi, pos, _)) in enumerate(zip(refs, case["rows"])):
            if not live[r]:
                assert np.isnan(got[r].astype(np.float32)).all(), (cname, name, r, "output row of an idle member")
            elif gi not in case["unchecked"]:
                g64 = got[r].reshape(case["H"], D).astype(np.float64)
                ratio = dr.ratio(g64, ref["out"], pc.decode_tol(ref, case["n_splits"] + case["nss"], out_f16))
                assert ratio <= 1.0, (cname, name, kv16, r, pos, ratio)
                worst = max(worst, ratio)
                if name == "needle" and not out_f16:
                    assert np.array_equal(g64, ref["vt"]), (cname, r, "needle rows are v[t(h)] to the last bit")
        print(f"INST shared {cname} {name} kv16={kv16} o16={out_f16}: err/tol {worst:.4f}")


@pytest.mark.parametrize("cname", [c for c in pc.SHARED if c.startswith("g3-")])
@KV
def test_shared_group_3(rig, kv16, cname):
    """18 and 66 query rows of 3 heads a member: members whose heads lie in two MFMA row tiles"""
    shared_case(rig, cname, kv16)


@pytest.mark.parametrize("cname", [c for c in pc.SHARED if c.startswith("g4-")])
@KV
def test_shared_full_and_uneven_row_tiles(rig, kv16, cname):
    """16, 32 and 48 rows: the last tile has no padding row; 96 and 112 rows: the second tile slot of a wave is active in only some waves"""
    shared_case(rig, cname, kv16)


@pytest.mark.parametrize("cname", [c for c in pc.SHARED if c.startswith("suffix-")])
@KV
def test_shared_suffix_shapes(rig, kv16, cname):
    """the suffix pass with and without arrival counters behind lead merges of 5, 6 and 1 records; with nothing shared it is the paged entry, bit for bit"""
    shared_case(rig, cname, kv16)
    _, _, got, twin = shared_run(rig, cname, kv16, False, "ramp12", share=False)
    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32))


@pytest.mark.parametrize("cname", ("leader-null", "leader-page", "dead-group", "broken", "bound", "idcap"))
@KV
def test_shared_edges(rig, kv16, cname):
    """an idle leader (the run is read through the first LIVE row's table), a group with no live member, the documented broken promise (no pool
    byte, no counter, no row outside the group and nothing behind the rows is off; the group's own values are not looked at), key_bound below
    max_pos with the longest run it allows, 258 shared pages in one split"""
    shared_case(rig, cname, kv16)
