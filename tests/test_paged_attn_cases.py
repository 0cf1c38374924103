"""CPU: the case tables of tests/paged_attn_cases.py held to the code paths they exist for (computed from the case data, so an edit cannot hollow
a case out), the refusals the new shapes sit next to (on the loaded library, no device), and the sensitivity of the new cases: a seeded fault of
the float32 models leaves the case's own tolerance.
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

D, P = 128, 0x1000  # P: a non-null pointer no refusal path reads


@pytest.fixture(scope="module")
def ropes(oracle):
    def rope(max_pos):
        sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
        return np.asarray(sin, np.float32).reshape(max_pos, D // 2), np.asarray(cos, np.float32).reshape(max_pos, D // 2)

    return rope


# ---- the tables against their conditions ------------------------------------------------------------------------------------------------------
def test_decode_tables_reach_their_paths():
    g3 = pc.G3
    assert g3["H"] // g3["n_kv"] == 3 and {0, 63, 64, 130, 300} <= set(g3["positions"]) and max(g3["n_splits"]) == g3["max_pos"] // 64
    assert set(g3["families"]) == {"gauss", "needle", "sunk"}
    full = pc.FULL
    pos = full["positions"]
    assert len(pos) == 64 and {0, 63, 64} <= set(pos) and max(pos) == 320 < full["max_pos"] and full["idle"] == {5: "table", 40: "page"}
    assert full["n_splits"] == 2 and pc.pages(pos[40]) >= 2  # the idle page id sits inside a context of more than one page
    b = pc.BOUND
    assert b["key_bound"] == 200 < b["max_pos"] == 576 and {199, 200, 575} <= set(b["positions"]) and 0 in b["n_splits"]
    cap = pc.IDCAP
    long_pos = cap["positions"][0]
    assert long_pos == 16384 + 64 + 5 and long_pos < cap["max_pos"] and pc.pages(long_pos) == 258
    own = {ns: -(-pc.pages(long_pos) // ns) for ns in cap["n_splits"]}  # pages of split 0, the largest share
    assert own[1] > pc.ID_CAP and own[2] <= pc.ID_CAP, "one split walks past the id cap, two do not"
    assert "gauss" in cap["families"] and set(cap["families"]) & {"ramp12", "fall12"}
    pool_mb = 2 * (sum(pc.pages(p) for p in cap["positions"]) + 3) * cap["n_kv"] * 64 * D * 4 / 2 ** 20
    assert pool_mb < 24


def test_prefill_tables_reach_their_paths():
    tiny = pc.SETS["tiny"]
    assert tiny[:6] == [(0, 1), (0, 64), (0, 65), (127, 2), (63, 2), (190, 5)]
    T = [p + n for p, n in tiny]
    assert [t % 64 for t in T[:6]] == [1, 0, 1, 1, 1, 3]
    assert {t % 4 for t in T if t % 64 >= 4} == {0, 1, 2, 3}, "the 16-byte unit of commit_k that straddles the key count, behind a page's first unit"
    seen = {(p + n) % 64 for s in pc.SETS.values() for p, n in s}
    assert seen > {0, 1, 2, 3, 8, 10, 63}, "key counts T % 64 beyond the older sets'"
    # more new page tiles than 64-row blocks, at the alignment the library reports for an even group (asserted on the GPU as well)
    spec = pc.prefill_segs("straddle")
    assert len(spec) == 4 and all(p % 64 == 63 and 2 <= n <= 3 for p, n in spec)
    row0, n_rows = pc.packed_rows(spec, pc.prefill_order("straddle"), 64)
    assert pc.new_tiles(spec) == 8 > -(-n_rows // 128) * 128 // 64
    wide = pc.WIDE
    assert len(wide["segs"]) == 64 and sorted(wide["order"]) == list(range(64)) and wide["order"] != tuple(range(64))
    assert [n for _, n in wide["segs"][:5]] == [1, 2, 3, 4, 5] and {p for p, _ in wide["segs"]} == set(pc.PASTS64)
    assert len(wide["forks"]) >= 4 and len(wide["idle"]) == 2
    for a, b in wide["forks"]:  # a whole first page of past on both sides, so nobody writes it; no fork partner is idle
        assert a < b and wide["segs"][a][0] >= 64 and wide["segs"][b][0] >= 64 and not {a, b} & set(wide["idle"])
    past, n = pc.PREFILL_IDCAP[0]
    assert (past, n) == (16420, 50) and (past + n - 1) // 64 == 257 >= pc.ID_CAP and past // 64 == 256
    for name in list(pc.SETS) + ["straddle", "wide", "idcap"]:
        order = pc.prefill_order(name)
        assert sorted(order) == list(range(len(pc.prefill_segs(name)))) and order != tuple(range(len(order))), (name, "row order is not table order")


def test_shared_tables_reach_their_paths():
    rows_nt = {name: pc.shared_rows(case, 0) for name, case in pc.SHARED.items()}
    assert [rows_nt[f"g3-{n}m-{s}"] for n in (6, 22) for s in (1, 2)] == [(18, 2), (18, 2), (66, 5), (66, 5)]
    assert pc.straddlers(pc.SHARED["g3-6m-1"], 0) == [5] and len(pc.straddlers(pc.SHARED["g3-22m-1"], 0)) >= 3  # rows 15, 16, 17 are one member's
    assert [rows_nt[f"g4-{n}m"] for n in (4, 8, 12, 24, 28)] == [(16, 1), (32, 2), (48, 3), (96, 6), (112, 7)]
    assert not any(pc.straddlers(pc.SHARED[f"g4-{n}m"], 0) for n in (4, 8, 12, 24, 28))
    older = {2, 3, 4, 5, 6, 8, 10, 12, 17, 20, 34, 64, 68, 128, 256}
    new = {rows for rows, _ in rows_nt.values()} - older
    assert new >= {16, 18, 32, 48, 66, 96, 112} and {nt for rows, nt in rows_nt.values() if rows in new} >= {6, 7}, "row counts and tiles the older test has not run"
    assert {(c["n_splits"], c["nss"]) for n, c in pc.SHARED.items() if n.startswith("suffix-")} == {(1, 5), (1, 6), (3, 5), (2, 1)}
    for name, case in pc.SHARED.items():
        live = pc.shared_live(case)
        for (gi, pos, idle), ok in zip(case["rows"], live):
            assert pos < case["max_pos"]
            if gi is not None and ok and gi not in case["unchecked"]:
                assert case["runs"][gi] <= pos >> 6, (name, "a promise is broken only where the case says so")
        assert max(case["runs"].values()) <= -(-case["key_bound"] // 64) - 1 and case["nss"] <= max(case["runs"].values())
        assert case["n_splits"] <= -(-case["key_bound"] // 64)
    sfx = pc.SHARED["suffix-1-5"]
    assert sfx["max_pos"] == 512 and sfx["runs"] == {0: 6} and all(384 <= p <= 450 for _, p, _ in sfx["rows"])
    for name in ("leader-null", "leader-page"):
        case = pc.SHARED[name]
        assert case["rows"][0][2] in ("table", "page") and pc.shared_live(case) == [False, True, True, True]
    dead = pc.SHARED["dead-group"]
    assert pc.shared_rows(dead, 0) == (0, 0) and pc.shared_rows(dead, 1)[0] > 0 and (None, 77, None) in dead["rows"]
    broken = pc.SHARED["broken"]
    assert broken["runs"][0] == 2 and (0, 100, None) in broken["rows"] and 100 >> 6 < 2 and broken["unchecked"] == (0,)
    bound = pc.SHARED["bound"]
    assert (bound["max_pos"], bound["key_bound"], bound["runs"][0]) == (512, 256, 3) and pc.shared_live(bound) == [True, True, False, True]
    cap = pc.SHARED["idcap"]
    assert cap["runs"][0] == 258 > pc.ID_CAP and cap["nss"] == 1 and [p for _, p, _ in cap["rows"]] == [258 * 64 + 3, 258 * 64 + 40]
    assert all(t // 64 >= pc.ID_CAP for t in pc.IDCAP_TARGETS), "the needle heads look into the pages whose ids come from the table arm"


# ---- the refusals next to the new shapes --------------------------------------------------------------------------------------------------------
def shared_call(hip, n_seq=4, leader=(0, 0, 2, 3), shared=(3, 3, 0, 0), nss=0, key_bound=256, n_splits=1):
    hip.attention_decode_paged_shared_dev(P, P, P, P, P, 32, P, P, n_seq, 8, 2, D, 512, key_bound, n_splits, P, P, leader, shared, nss)


@pytest.mark.parametrize("kw, wording", (
    (dict(n_splits=5), "n_splits 5 above the 4 pages of key_bound 256"),
    (dict(shared=(4, 4, 0, 0)), "at most 3 under key_bound 256"),  # ceil(256 / 64) - 1 = 3 is the bound case's own run
    (dict(nss=4), "n_shared_splits 4 above the longest shared run of 3 pages"),
    (dict(n_seq=65), "n_seq 65 must be 1..64"),
), ids=lambda p: p if isinstance(p, str) else "")
def test_shared_refusals_beside_the_new_shapes(pkg, kw, wording):
    with pytest.raises(pkg.BitNetHipError) as e:
        shared_call(pkg.load(), **kw)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT and wording in str(e.value)


def test_decode_refuses_more_splits_than_the_pages_of_key_bound(pkg):
    """key_bound 200 has ceil(200 / 64) = 4 pages: 5 splits are refused, with the entry's wording; 4 are taken (and run on the GPU as the rule's own answer)"""
    hip = pkg.load()
    assert hip.attention_paged_splits(4, 2, 200) == 4
    for n_seq, n_splits, wording in ((4, 5, "n_splits 5 above the 4 pages of key_bound 200"), (65, 1, "n_seq 65 must be 1..64")):
        with pytest.raises(pkg.BitNetHipError) as e:
            hip.attention_decode_paged_dev(P, P, P, P, P, 32, P, P, n_seq, 8, 2, D, 576, 200, n_splits, P, P)
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT and wording in str(e.value)


# ---- sensitivity: a seeded fault leaves the case's tolerance ---------------------------------------------------------------------------------------
# fault -> the family of the case that shows it (the other families of the case may keep a fault inside the tolerance: sunk hides head_map, ...)
G3_FAULTS = {"head_map": "gauss", "mask_tail": "sunk", "merge_swap": "gauss", "dead_record": "gauss"}


@pytest.mark.parametrize("fault", sorted(G3_FAULTS))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_group_3_decode_case_is_sensitive(ropes, kv16, fault):
    """the group-3 decode case at position 300 (5 records): dr.walk holds its tolerance, and with the fault it does not (the GPU test's ratio)"""
    g3, name, pos = pc.G3, G3_FAULTS[fault], 300
    rope = ropes(g3["max_pos"])
    ref = pc.decode_ref(rope, "g3", kv16, g3["H"], g3["n_kv"], name, pos, 0, g3["max_pos"])
    slots = pc.pages(pos) * 64
    kc, vc = (np.broadcast_to(s[:, None, :], (g3["n_kv"], slots, D)).copy() for s in ref["stale"])
    kc[:, :pos], vc[:, :pos] = ref["kp"][:, :pos], ref["vp"][:, :pos]
    tol = pc.decode_tol(ref, max(g3["n_splits"]), False)
    good, _ = dr.walk(ref["qkv"], kc, vc, pos, *rope, g3["H"], g3["n_kv"], kv16)
    bad, _ = dr.walk(ref["qkv"], kc, vc, pos, *rope, g3["H"], g3["n_kv"], kv16, fault=fault)
    r_good, r_bad = dr.ratio(good, ref["out"], tol), dr.ratio(bad, ref["out"], tol)
    print(f"g3 {name} kv16={kv16} {fault}: err/tol {r_good:.3f} -> {r_bad:.3g}")
    assert r_good <= 1.0 < r_bad


@pytest.mark.parametrize("fault", ("merge_swap", "dead_record"))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_lead_5_merge_case_is_sensitive(ropes, kv16, fault):
    """the suffix case behind 5 lead records, the member at 450, family ramp12 (every later record has the larger maximum).  dr.walk cannot express
    a lead merge -- records of several pages from f16 operands, merged ahead of the row's own -- and is not extended to; what it has is the merge of
    the same keys' 64-position records, and its two merge faults leave this case's tolerance (shared-key terms included)."""
    case, name = pc.SHARED["suffix-1-5"], "ramp12"
    rope = ropes(case["max_pos"])
    r, (gi, pos, _) = 4, case["rows"][4]
    ref = pc.decode_ref(rope, ("shared", "suffix-1-5"), kv16, case["H"], case["n_kv"], name, pos, r, case["max_pos"], group=gi, S=case["runs"][gi])
    kc, vc = (np.broadcast_to(s[:, None, :], (case["n_kv"], pc.pages(pos) * 64, D)).copy() for s in ref["stale"])
    kc[:, :pos], vc[:, :pos] = ref["kp"][:, :pos], ref["vp"][:, :pos]
    tol = pc.decode_tol(ref, case["n_splits"] + case["nss"], False)
    good, _ = dr.walk(ref["qkv"], kc, vc, pos, *rope, case["H"], case["n_kv"], kv16)
    bad, _ = dr.walk(ref["qkv"], kc, vc, pos, *rope, case["H"], case["n_kv"], kv16, fault=fault)
    r_good, r_bad = dr.ratio(good, ref["out"], tol), dr.ratio(bad, ref["out"], tol)
    print(f"lead-5 {name} kv16={kv16} {fault}: err/tol {r_good:.3f} -> {r_bad:.3g}")
    assert r_good <= 1.0 < r_bad


@pytest.mark.parametrize("seg", (0, 3), ids=("T1", "across-a-page-end"))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_tiny_prefill_case_is_sensitive(ropes, kv16, seg):
    """segments (0, 1) and (127, 2) of 'tiny', family sunk (a zero-padded key left unmasked takes the row): ar.walk holds the case's tolerance, with
    fault 'mask' (one key too many) it does not.  ar.walk's other switch for this kernel's paths, merge_m, needs a key split, which the paged kernel
    does not have: left out."""
    H, n_kv, name = 6, 2, "sunk"
    rope = ropes(384)
    g = pc.prefill_case(rope, H, n_kv, name, "tiny", kv16)[seg]
    past, n = g["past"], g["n"]
    pos = np.arange(past, past + n)
    sin, cos = rope
    q_in, k_in, v_in = (g["qkv"][:, a * D:b * D].reshape(n, -1, D) for a, b in ((0, H), (H, H + n_kv), (H + n_kv, H + 2 * n_kv)))
    qh, kh = ar.operands_q(q_in, pos, sin, cos), np.concatenate([ar.f16(g["k_c"]), ar.operands_k(k_in, pos, sin, cos)])
    vh = np.concatenate([ar.f16(g["v_c"]), ar.operands_v(v_in)])
    want, tol = g["model"][False]
    for h in range(H):
        good, _ = ar.walk(qh[:, h], kh[:, h // 3], vh[:, h // 3], pos, qg=128)
        bad, _ = ar.walk(qh[:, h], kh[:, h // 3], vh[:, h // 3], pos, qg=128, fault="mask")
        r_good, r_bad = float(np.max(np.abs(good - want[:, h]) / tol[:, h])), float(np.max(np.abs(bad - want[:, h]) / tol[:, h]))
        print(f"tiny seg {seg} head {h} kv16={kv16}: err/tol {r_good:.3f} -> {r_bad:.3g}")
        assert r_good <= 1.0 < r_bad
