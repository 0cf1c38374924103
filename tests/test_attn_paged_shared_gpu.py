"""GPU: the fork groups' paged decode attention (bitnet_hip_attention_decode_paged_shared_dev: k_attn_paged_shared<KV16> + k_attn_paged's suffix
instance) by value against the float64 model tests/attn_decode_ref.py over the pool contents, its input families and its per-element tolerance.

Tolerance, derived.  Start from tests/test_attn_paged_gpu.py's: dr.tol() + 2^-23 (pages + n_splits + n_shared_splits) sum_j p_j |v_jd| (one fused rescale
per page walked, one merge step per record).  On the SHARED keys j < 64 S the operands of both products are f16:
  * q' (scaled) is rounded to f16 and, on f32 pools, so is k: each moves score j by 2^-11 scale sum_d |q_d k_jd|; below the smallest normal f16 an
    operand moves by at most 2^-25 instead: scale 2^-25 sum_d (|q_d| + |k_jd|).  The record's maximum goes from base 2 to natural log with two f32
    roundings: 2^-23 max_j |s_j|.  All three join ds_j, which enters as sum_j p_j ds_j |v_jd - out_d|;
  * p is rounded to f16 and l sums the rounded weights, so the row moves by 2^-11 sum_j p_j |v_jd - out_d|; a weight below the smallest normal f16
    (relative to the running maximum, itself at most the largest weight) moves by 2^-25 of that: 2^-25 max_j p_j sum_j |v_jd - out_d|;
  * on f32 pools v is rounded to f16: 2^-11 sum_j p_j |v_jd|.
The private keys and the new token carry the paged attention's own arithmetic and nothing is added for them.
Beyond the terms the issue lists: the 2^-25 terms (f16 has a smallest normal; the issue's 2^-11 is relative), the 2^-23 max |s| of the record
maximum's unit change, and the paged test's own 2^-23 per page and record, which that test adds to dr.tol() for the same merge.

Every case: scattered, non-monotone page ids; members of a group name the SAME pages in entries 0 .. S - 1; private tails hold per-member keys and
values.  Checked: the rows; the pools bit for bit against a twin pool that bitnet_hip_attention_decode_paged_dev stepped (the appended key / value)
and, outside the appended slots, against the pools before; idle rows' NaN fill; the counters back at 0; a second launch: the same bits.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_decode_ref as dr  # noqa: E402
from kv_read import bits  # noqa: E402

pytestmark = pytest.mark.gpu

D, N_KV, MAX_POS, N_PAGES, N_SPLITS = 128, 2, 320, 96, 2
FAMILIES = ("fall12", "newtok", "ramp12")  # the mass on the shared keys, on the new token, every later record with the larger maximum
# a case: groups [(S, member positions)], ungrouped positions, idle rows [(kind, group index, position)], n_shared_splits
CASES = {
    "pair": ([(1, (64, 70))], (), (), 1),                       # the suffix is the append page only, once at slot 0
    "five-1": ([(3, (192, 200, 255, 193, 261))], (), (), 1),    # 20 rows at group 4: a ragged second row tile; one member with two further pages
    "five-2": ([(3, (192, 200, 255, 193, 261))], (), (), 2),
    "five-3": ([(3, (192, 200, 255, 193, 261))], (), (), 3),
    "seventeen": ([(2, tuple(128 + 3 * i for i in range(17)))], (), (), 2),       # 68 rows: past one wave's 64
    "sixtyfour": ([(2, tuple(128 + 7 * i % 64 for i in range(64)))], (), (), 0),  # 256 rows, the library's split rule
    "mixed": ([(1, (64, 100, 127)), (2, (130, 140))], (77,), (("table", 0, 90), ("page", 1, 200)), 2),
}
REFS = {}


def member_master(name, gm, S, seed):
    """a member's keys and values: the group's below 64 S, its own behind (the same trend direction w, fresh noise and values)"""
    m = dr.master(name, np.random.default_rng(seed), MAX_POS, N_KV)
    b = dr.trend_of(name, MAX_POS) / (dr.A_W * dr.SCALE)
    m["k"] = m["k"] + b[:, None, None] * (gm["w"] - m["w"])[None]
    m["w"] = gm["w"]
    m["k"][:64 * S], m["v"][:64 * S] = gm["k"][:64 * S], gm["v"][:64 * S]
    return m


def refs_for(case, kv16, H, name, sin, cos):
    """the rows of a case -> [dict(pos, S, group, idle, qkv, ex, kp, vp, tol_extra)], computed once"""
    key = (case, kv16, H, name)
    if key in REFS:
        return REFS[key]
    groups, singles, idles, _ = CASES[case]
    dt, plan = dr.cache_dtype(kv16), [(p, 0, None, None) for p in singles[:1]]  # an ungrouped row first: no leader is row 0
    for gi, (S, poss) in enumerate(groups):
        plan += [(p, S, gi, None) for p in poss] + [(p, S, gi, kind) for kind, g, p in idles if g == gi]
    plan += [(p, 0, None, None) for p in singles[1:]]
    gms = [dr.master(name, np.random.default_rng(dr.seed_of("shared", name, gi)), MAX_POS, N_KV) for gi in range(max(len(groups), 1))]
    rows = []
    for r, (pos, S, gi, idle) in enumerate(plan):
        m = member_master(name, gms[gi or 0], S, dr.seed_of("shared", name, case, r))
        q1, kn1, vn, _ = dr.token(m, np.random.default_rng(dr.seed_of("shared", H, name, case, r)), pos, H)
        qkv = dr.raw_qkv(q1, kn1, vn, pos, sin, cos)
        kp, vp = m["k"].astype(dt).transpose(1, 0, 2), m["v"].astype(dt).transpose(1, 0, 2)
        ex = dr.exact(qkv, kp, vp, pos, sin, cos, H, N_KV, kv16, recs=())
        rows.append(dict(pos=pos, S=S, group=gi, idle=idle, qkv=qkv, ex=ex, kp=kp, vp=vp, extra=extra_tol(ex, 64 * S, kv16),
                         pav=np.einsum("hj,hjd->hd", ex["p"], ex["aV"][np.arange(H) // (H // N_KV), :pos + 1]), stale=dr.stale(name, q1, N_KV, kv16)))
    REFS[key] = rows
    return rows


def extra_tol(ex, n_sh, kv16):
    """[H, D]: what the f16 operands of the shared keys 0 .. n_sh - 1 add to dr.tol (module docstring)"""
    t = np.zeros_like(ex["out"])
    for h in range(t.shape[0]):
        g, p, o, q = h // ex["group"], ex["p"][h], ex["out"][h], np.abs(ex["q"][h])
        if n_sh == 0:
            continue
        aK, V = np.abs(ex["K"][g, :n_sh]), ex["V"][g, :n_sh]
        ds = (2.0 ** -11 * (1 if kv16 else 2) * dr.SCALE * (aK @ q) + dr.SCALE * 2.0 ** -25 * (q.sum() + aK.sum(axis=1))
              + 2.0 ** -23 * np.abs(ex["s"][h, :n_sh]).max())
        dev = np.abs(V - o[None])
        t[h] = (p[:n_sh] * ds) @ dev + 2.0 ** -11 * (p[:n_sh] @ dev) + 2.0 ** -25 * p.max() * dev.sum(axis=0)
        if not kv16:
            t[h] += 2.0 ** -11 * (p[:n_sh] @ np.abs(V))
    return t


def encode(K, V, kv16):
    """logical [page, kv, 64, D] -> the pool's words: K [page][kv][R][64] (f16: dim pairs), V [page][kv][64][R]"""
    Kd = K.reshape(N_PAGES, N_KV, 64, D // 2, 2).transpose(0, 1, 3, 2, 4) if kv16 else K.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(Kd).reshape(-1), np.ascontiguousarray(V).reshape(-1)


@pytest.fixture(scope="module")
def rope(oracle):
    sin, cos = oracle.rope_tables(D, MAX_POS, 10000.0)
    return sin.reshape(MAX_POS, D // 2), cos.reshape(MAX_POS, D // 2)


def run_case(hip, rope, case, kv16, H, name, share=True):
    """one case through the shared entry (share=False: its runs declared as 0) -> (rows, outs [n, H * D] f32, leader, shared)"""
    import torch as t

    sin, cos = rope
    rows = refs_for(case, kv16, H, name, sin, cos)
    n, nss = len(rows), CASES[case][3]
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    # pages: a permutation dealt out; a group's run once, every member's tail its own
    perm = iter(np.random.default_rng(dr.seed_of("pages", case)).permutation(N_PAGES).astype(np.uint32))
    runs, leader_of, tables, leader, shared = {}, {}, [], [], []
    ks0, vs0 = rows[0]["stale"]
    K0 = np.broadcast_to(ks0[None, :, None, :], (N_PAGES, N_KV, 64, D)).copy()
    V0 = np.broadcast_to(vs0[None, :, None, :], (N_PAGES, N_KV, 64, D)).copy()
    for r, row in enumerate(rows):
        gi, S, pos = row["group"], row["S"], row["pos"]
        if gi is not None and gi not in runs:
            runs[gi], leader_of[gi] = [next(perm) for _ in range(S)], r
        tb = np.full(MAX_POS // 64, 0xFFFFFFFF, np.uint32)
        for c in range(pos // 64 + 1):
            pg = int(runs[gi][c]) if gi is not None and c < S else int(next(perm))
            tb[c], lo, live = pg, c * 64, max(0, min(64, pos - c * 64))
            K0[pg, :, :live], V0[pg, :, :live] = row["kp"][:, lo:lo + live], row["vp"][:, lo:lo + live]
        if row["idle"] == "page":
            tb[pos // 64] = N_PAGES  # in its private tail
        tables.append(tb)
        leader.append(leader_of[gi] if gi is not None else r)
        shared.append(S if share else 0)
    kflat, vflat = encode(K0, V0, kv16)
    tab_d = [dev(tb) for tb in tables]
    pos_d = [t.tensor([row["pos"]], dtype=t.int32, device="cuda") for row in rows]
    tp = t.tensor([0 if row["idle"] == "table" else tab_d[r].data_ptr() for r, row in enumerate(rows)], dtype=t.int64, device="cuda")
    pp = t.tensor([p.data_ptr() for p in pos_d], dtype=t.int64, device="cuda")
    qkv_d, sin_d, cos_d = dev(np.stack([row["qkv"] for row in rows])), dev(np.asarray(sin, np.float32)), dev(np.asarray(cos, np.float32))
    nss_r = (nss or hip.attention_paged_shared_splits(len(runs), N_KV, max(shared))) if share else 0
    scratch = t.zeros(hip.attention_paged_shared_scratch_bytes(n, N_KV, N_SPLITS, nss_r) // 4, dtype=t.float32, device="cuda")
    scratch[64 * N_KV:] = 1.0e6  # hostile records behind the zeroed counters
    pools, outs = [], []
    for twin in (False, True, None):  # the shared entry, the paged entry on a twin pool, the shared entry again on the stepped pool
        kpool, vpool = (dev(kflat), dev(vflat)) if twin is not None else pools[0]
        out = t.full((n, H * D), float("nan"), dtype=t.float32, device="cuda")
        if twin:
            hip.attention_decode_paged_dev(qkv_d, sin_d, cos_d, kpool, vpool, N_PAGES, tp, pp, n, H, N_KV, D, MAX_POS, MAX_POS, N_SPLITS, scratch, out, kv_f16=kv16)
        else:
            hip.attention_decode_paged_shared_dev(qkv_d, sin_d, cos_d, kpool, vpool, N_PAGES, tp, pp, n, H, N_KV, D, MAX_POS, MAX_POS, N_SPLITS, scratch, out,
                                                  leader, shared, nss if share else 0, kv_f16=kv16)
        t.cuda.synchronize()
        assert int(scratch[: 64 * N_KV].view(t.int32).abs().sum().item()) == 0, "arrival counters not back at 0"
        pools.append((kpool, vpool))
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32)), "a second launch changed the bits"
    k1, v1, k2, v2 = (x.cpu().numpy() for x in pools[0] + pools[1])
    assert np.array_equal(bits(k1), bits(k2)) and np.array_equal(bits(v1), bits(v2)), "the pools differ from the paged entry's twin"
    # independent of the twin: only slot pos % 64 of page table[pos // 64] of a live row may differ from the pools before
    ck = (bits(k1) != bits(kflat)).reshape(N_PAGES, N_KV, -1, 64, 2 if kv16 else 1)  # [.., dim pair | dim, position, half]
    cv = (bits(v1) != bits(vflat)).reshape(N_PAGES, N_KV, 64, D)
    for row, tb in zip(rows, tables):
        if row["idle"] is None:
            ck[int(tb[row["pos"] // 64]), :, :, row["pos"] % 64] = False
            cv[int(tb[row["pos"] // 64]), :, row["pos"] % 64] = False
    assert not ck.any() and not cv.any(), "a pool byte outside the appended slots changed"
    return rows, outs[0], outs[1], nss_r


@pytest.mark.parametrize("H", (8, 4, 2), ids=("g4", "g2", "g1"))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
@pytest.mark.parametrize("case", tuple(CASES))
def test_shared_attention_by_value(hip, rope, case, kv16, H):
    for name in FAMILIES:
        rows, got, _, nss = run_case(hip, rope, case, kv16, H, name)
        for r, row in enumerate(rows):
            if row["idle"]:
                assert np.isnan(got[r]).all(), (case, name, r, "output row of an idle member")
                continue
            tol = dr.tol(row["ex"]) + 2.0 ** -23 * (row["pos"] // 64 + 1 + N_SPLITS + nss) * row["pav"] + row["extra"]
            ratio = dr.ratio(got[r].reshape(H, D), row["ex"]["out"], tol)
            print(f"SHARED {case} {name} kv16={kv16} H={H} row {r} pos {row['pos']} S {row['S']}: err/tol {ratio:.4f}")
            assert ratio <= 1.0, (case, name, kv16, H, r, ratio)


@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_nothing_shared_is_the_paged_entry(hip, rope, kv16):
    _, got, twin, _ = run_case(hip, rope, "mixed", kv16, 8, "ramp12", share=False)
    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32))
