"""GPU: the paged decode attention (bitnet_hip_attention_decode_paged_dev, csrc/kernels_kvpaged.hip: k_attn_paged<KV16>) by value against the
float64 model tests/attn_decode_ref.py -- its operands, its input families, its per-element tolerance.

Tolerance, from the operation count.  Scores are summed as attn_partial_body sums them, so ds is the model's.  Per page walked the stream adds ONE
fused rescale of each accumulator, acc = fma(acc, e^(m_old - m_new), page_sum), and one of l: two roundings of 2^-24 relative to sum_j p_j |v_jd|,
2^-23 per page.  Per split the merge adds fma(acc, s_old, o_c * s_c) on o and on l; beyond what the model's 2^-22 term counts, another 2^-23.  So
    tol_paged = tol() + 2^-23 (pages + n_splits) sum_j p_j |v_jd|        pages = pos // 64 + 1

Every launch carries 3 sequences whose page tables are a permutation of the pool dealt round-robin (non-monotone, interleaved); entries past a
context hold 0xFFFFFFFF, unnamed pages and slots at or past a position hold hostile stale values.  Checked: the rows, the appended key / value in
slot pos % 64 of page table[pos // 64], every other pool byte, the arrival counters back at 0, a second launch on the same scratch: the same bits.
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

D, N_KV, MAX_POS, N_PAGES = 128, 2, 576, 32
C_MAX = MAX_POS // 64  # 9 table entries, the largest n_splits
POSITIONS = (0, 63, 64, 65, 127, 128, 191, 300, 513)
COMPANIONS = (200, 77)  # the other two sequences of a launch
FAMILIES = ("gauss", "needle", "sunk")
REC_FLOATS = 8 + 4 * D
NOWHERE = 0xFFFFFFFF
REFS, MASTERS = {}, {}


class Rig:
    def __init__(self, hip, oracle, torch):
        self.hip, self.t = hip, torch
        sin, cos = oracle.rope_tables(D, MAX_POS, 10000.0)
        self.sin, self.cos = sin.reshape(MAX_POS, D // 2), cos.reshape(MAX_POS, D // 2)
        self.sin_d, self.cos_d = self.dev(np.asarray(sin, np.float32)), self.dev(np.asarray(cos, np.float32))

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def ref(self, kv16, H, name, pos, slot):
        """the model's step for sequence `slot` of a launch (its own keys, computed once)"""
        key = (kv16, H, name, pos, slot)
        if key not in REFS:
            if (name, slot) not in MASTERS:
                MASTERS[(name, slot)] = dr.master(name, np.random.default_rng(dr.seed_of("paged", name, slot)), MAX_POS, N_KV)
            m, dt = MASTERS[(name, slot)], dr.cache_dtype(kv16)
            q1, kn1, vn, t = dr.token(m, np.random.default_rng(dr.seed_of("paged", H, name, pos, slot)), pos, H)
            qkv = dr.raw_qkv(q1, kn1, vn, pos, self.sin, self.cos)
            kp, vp = m["k"].astype(dt).transpose(1, 0, 2), m["v"].astype(dt).transpose(1, 0, 2)  # [kv, T, D] as the pool holds them
            ex = dr.exact(qkv, kp, vp, pos, self.sin, self.cos, H, N_KV, kv16, recs=())
            g = np.arange(H) // (H // N_KV)
            pav = np.einsum("hj,hjd->hd", ex["p"], ex["aV"][g, :pos + 1])
            REFS[key] = dict(qkv=qkv, out=ex["out"], tol=dr.tol(ex), pav=pav, t=t, kp=kp, vp=vp, stale=dr.stale(name, q1, N_KV, kv16),
                             kn=dr.rope1(qkv[H * D:(H + N_KV) * D].reshape(N_KV, D), pos, self.sin, self.cos), vn=qkv[(H + N_KV) * D:].reshape(N_KV, D),
                             vt=None if t is None else np.stack([ex["V"][h // (H // N_KV), t[h]] for h in range(H)]))
        return REFS[key]


@pytest.fixture(scope="module")
def rig(hip, oracle):
    import torch

    return Rig(hip, oracle, torch)


def tables_for(seed):
    """3 tables of C_MAX entries: a permutation of the pool dealt round-robin, so every sequence's ids are non-monotone and interleaved"""
    perm = np.random.default_rng(seed).permutation(N_PAGES).astype(np.uint32)
    return [perm[s::3][:C_MAX].copy() for s in range(3)]


def build_pools(refs, tables, seq_pos, kv16):
    """logical pools K / V [page, kv, 64, D] in the cache's dtype: hostile everywhere, then each sequence's past below its position"""
    ks0, vs0 = refs[0]["stale"]
    K = np.broadcast_to(ks0[None, :, None, :], (N_PAGES, N_KV, 64, D)).copy()
    V = np.broadcast_to(vs0[None, :, None, :], (N_PAGES, N_KV, 64, D)).copy()
    for ref, tbl, pos in zip(refs, tables, seq_pos):
        ks, vs = ref["stale"]
        for c in range(min(pos, MAX_POS - 1) // 64 + 1):
            pg, lo = int(tbl[c]), c * 64
            n = max(0, min(64, pos - lo))
            K[pg], V[pg] = ks[:, None, :], vs[:, None, :]
            K[pg, :, :n], V[pg, :, :n] = ref["kp"][:, lo:lo + n], ref["vp"][:, lo:lo + n]
    return K, V


def encode(K, V, kv16):
    """logical [page, kv, 64, D] -> the pool's words: K [page][kv][R][64] (f16: dim pairs), V [page][kv][64][R]"""
    if kv16:
        Kd = K.reshape(N_PAGES, N_KV, 64, D // 2, 2).transpose(0, 1, 3, 2, 4)
    else:
        Kd = K.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(Kd).reshape(-1), np.ascontiguousarray(V).reshape(-1)


def decode_k(flat, kv16):
    if kv16:
        return flat.reshape(N_PAGES, N_KV, D // 2, 64, 2).transpose(0, 1, 3, 2, 4).reshape(N_PAGES, N_KV, 64, D)
    return flat.reshape(N_PAGES, N_KV, D, 64).transpose(0, 1, 3, 2)


def launch(rig, H, kv16, out_f16, n_splits, name, seq_pos, idle=None, seed=0):
    """one launch of 3 sequences; idle = (slot, kind) makes that sequence idle.  Checks everything the module docstring lists."""
    t, hip = rig.t, rig.hip
    refs = [rig.ref(kv16, H, name, min(p, MAX_POS - 1), s) for s, p in enumerate(seq_pos)]
    tables = tables_for(seed)
    K0, V0 = build_pools(refs, tables, seq_pos, kv16)
    tab_host = []
    for s, (tbl, pos) in enumerate(zip(tables, seq_pos)):
        tb = tbl.copy()
        tb[min(pos, MAX_POS - 1) // 64 + 1:] = NOWHERE
        if idle == (s, "page"):
            tb[pos // 64 // 2] = N_PAGES  # the first id outside the pool, inside the context
        tab_host.append(tb)
    kflat, vflat = encode(K0, V0, kv16)
    kpool, vpool = rig.dev(kflat), rig.dev(vflat)
    tab_d = [rig.dev(tb) for tb in tab_host]
    pos_d = [t.tensor([p], dtype=t.int32, device="cuda") for p in seq_pos]
    live = [not (idle and idle[0] == s) for s in range(3)]
    tp = t.tensor([0 if idle == (s, "table") else tab_d[s].data_ptr() for s in range(3)], dtype=t.int64, device="cuda")
    pp = t.tensor([0 if idle == (s, "pos") else pos_d[s].data_ptr() for s in range(3)], dtype=t.int64, device="cuda")
    qkv_d = rig.dev(np.stack([r["qkv"] for r in refs]))
    asked, n_splits = n_splits, n_splits or hip.attention_paged_splits(3, N_KV, MAX_POS)  # 0: the library's rule, the scratch sized by its report
    sb = hip.attention_paged_scratch_bytes(3, N_KV, n_splits)
    assert sb == 64 * N_KV * 4 + 3 * N_KV * n_splits * REC_FLOATS * 4
    scratch = t.zeros(sb // 4, dtype=t.float32, device="cuda")
    scratch[64 * N_KV:] = 1.0e6  # hostile records behind the zeroed counters
    odt, ndt = (t.float16, np.float16) if out_f16 else (t.float32, np.float32)
    outs = []
    for _ in range(2):  # the second launch: the same scratch, the same bits
        out = t.full((3, H * D), float("nan"), dtype=odt, device="cuda")
        hip.attention_decode_paged_dev(qkv_d, rig.sin_d, rig.cos_d, kpool, vpool, N_PAGES, tp, pp, 3, H, N_KV, D, MAX_POS, MAX_POS, asked, scratch, out,
                                       kv_f16=kv16, out_f16=out_f16)
        t.cuda.synchronize()
        assert int(scratch[: 64 * N_KV].view(t.int32).abs().sum().item()) == 0, "arrival counters not back at 0"
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint16 if out_f16 else np.uint32), outs[1].view(np.uint16 if out_f16 else np.uint32)), "a replay changed the bits"
    K1, V1 = decode_k(kpool.cpu().numpy(), kv16), vpool.cpu().numpy().reshape(N_PAGES, N_KV, 64, D)
    changed_k, changed_v = bits(K1) != bits(K0), bits(V1) != bits(V0)
    worst = 0.0
    for s, (ref, pos) in enumerate(zip(refs, seq_pos)):
        tag = (name, H, kv16, out_f16, n_splits, seq_pos, s, idle)
        if not live[s]:
            assert np.isnan(outs[0][s].astype(np.float32)).all(), (tag, "output row of an idle sequence")
            continue
        got = outs[0][s].reshape(H, D).astype(np.float64)
        tol = ref["tol"] + 2.0 ** -23 * (pos // 64 + 1 + n_splits) * ref["pav"] + (dr.half_ulp_f16(ref["out"]) if out_f16 else 0.0)
        r = dr.ratio(got, ref["out"], tol)
        print(f"PAGED {tag}: err/tol {r:.4f}")
        assert r <= 1.0, (tag, "rows", r)
        worst = max(worst, r)
        if name == "needle" and not out_f16:
            assert np.array_equal(got, ref["vt"]), (tag, "needle rows are v[t(h)] to the last bit")
        # the appended key and value, in slot pos % 64 of page table[pos // 64]
        pg, sl = int(tables[s][pos // 64]), pos % 64
        gk, gv, kn = K1[pg, :, sl].astype(np.float64), V1[pg, :, sl], ref["kn"]
        if kv16:  # the nearest f16 of the float64 rotation or its neighbour; the value's exact rounding
            near = dr.f16(kn)
            ulp = np.maximum(np.spacing(np.abs(near).astype(np.float16)), np.spacing(np.abs(gk).astype(np.float16))).astype(np.float64)
            assert np.all(np.abs(gk - near) <= ulp), (tag, "appended key")
            assert np.array_equal(bits(gv), bits(ref["vn"].astype(np.float16))), (tag, "appended value")
        else:  # three f32 roundings of x0 c -+ x1 s
            pair = np.hypot(kn[:, : D // 2], kn[:, D // 2:])
            assert np.all(np.abs(gk - kn) <= 2.0 ** -22 * np.concatenate([pair, pair], axis=1)), (tag, "appended key")
            assert np.array_equal(bits(gv), bits(ref["vn"])), (tag, "appended value")
        changed_k[pg, :, sl], changed_v[pg, :, sl] = False, False
    assert not changed_k.any() and not changed_v.any(), "a pool byte outside the appended slots changed"
    return worst


@pytest.mark.parametrize("out_f16", (False, True), ids=("o32", "o16"))
@pytest.mark.parametrize("n_splits", (1, 2, 3, C_MAX), ids=lambda p: "max" if p == C_MAX else str(p))
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("H", (8, 4, 2), ids=("g4", "g2", "g1"))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_paged_attention_by_value(rig, kv16, H, pos, n_splits, out_f16):
    for name in FAMILIES:
        launch(rig, H, kv16, out_f16, n_splits, name, (pos,) + COMPANIONS, seed=pos + 7 * n_splits)


@pytest.mark.parametrize("kind", ("table", "pos", "bound", "page"))
@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_idle_sequences_are_left_alone(rig, kv16, kind):
    """the middle sequence is idle: NULL table, NULL position, pos >= key_bound, a page id >= n_pages inside its context.  No row and no page
    of it changes (launch() checks every pool byte, the NaN-filled row and the arrival counters); the sequences on both sides are held to the model as ever"""
    seq_pos = (300, MAX_POS if kind == "bound" else 200, 77)
    for n_splits in (1, 3):
        launch(rig, 8, kv16, False, n_splits, "gauss", seq_pos, idle=(1, "none" if kind == "bound" else kind), seed=11)


def test_auto_split_count_is_honoured(rig):
    """n_splits = 0: the library's rule (9 here), through the same checks as an explicit count"""
    assert rig.hip.attention_paged_splits(3, N_KV, MAX_POS) == C_MAX
    launch(rig, 8, True, False, 0, "gauss", (300,) + COMPANIONS, seed=3)
