"""The case tables of tests/test_paged_attn_instances_gpu.py and the helpers of the older paged tests that hard-code their geometry, restated with
parameters (CPU only; tests/test_paged_attn_cases.py holds every table to the condition it exists for).

Restated from tests/test_attn_paged_gpu.py (N_KV, N_PAGES, MAX_POS are module constants there): encode, decode_k, the page dealing of tables_for
and build_pools (deal), Rig.ref (decode_ref).  From tests/test_attn_paged_shared_gpu.py: member_master (MAX_POS, N_KV; and, new, families without
a trend direction).  extra_tol takes every size from its arguments and is imported unchanged.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_decode_ref as dr  # noqa: E402
import attn_ref as ar  # noqa: E402
from test_attn_paged_shared_gpu import extra_tol  # noqa: E402

D, NOWHERE, ID_CAP = 128, 0xFFFFFFFF, 256  # ID_CAP: kPgIdCap = kPpIdCap = kShIdCap, the page ids a workgroup keeps in LDS


def pages(pos):
    """pages a sequence at position pos walks (the page of pos included)"""
    return pos // 64 + 1


# ---- the pool's word order -----------------------------------------------------------------------------------------------------------------
def encode(K, V, kv16):
    """logical [page, kv, 64, D] -> the pool's words: K [page][kv][R][64] (f16: dim pairs), V [page][kv][64][R]"""
    P, n_kv = K.shape[:2]
    Kd = K.reshape(P, n_kv, 64, D // 2, 2).transpose(0, 1, 3, 2, 4) if kv16 else K.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(Kd).reshape(-1), np.ascontiguousarray(V).reshape(-1)


def decode_k(flat, kv16, n_pages, n_kv):
    if kv16:
        return flat.reshape(n_pages, n_kv, D // 2, 64, 2).transpose(0, 1, 3, 2, 4).reshape(n_pages, n_kv, 64, D)
    return flat.reshape(n_pages, n_kv, D, 64).transpose(0, 1, 3, 2)


def deal(seed, n_pages):
    """page ids in a seeded random order: whoever draws from it gets scattered, non-monotone, interleaved ids"""
    return iter(np.random.default_rng(seed).permutation(n_pages).astype(np.uint32))


# ---- decode: the model's step of one sequence ------------------------------------------------------------------------------------------------
MASTERS, DREFS = {}, {}


def member_master(name, gm, S, seed, max_pos, n_kv):
    """a member's keys and values: the group's below 64 S, its own behind (a trend family keeps the group's direction w)"""
    m = dr.master(name, np.random.default_rng(seed), max_pos, n_kv)
    if m["w"] is not None:
        b = dr.trend_of(name, max_pos) / (dr.A_W * dr.SCALE)
        m["k"] = m["k"] + b[:, None, None] * (gm["w"] - m["w"])[None]
        m["w"] = gm["w"]
    for key in ("k", "v") + (("u",) if m["u"] is not None else ()):
        m[key][:64 * S] = gm[key][:64 * S]
    return m


def decode_ref(rope, tag, kv16, H, n_kv, name, pos, slot, max_pos, group=None, S=0, targets=None):
    """The model's step at `pos` of sequence `slot` of the launch `tag`, computed once.  group / S: the fork group whose first 64 S keys it shares.
    targets [H]: needle only, the key each head looks for (dr.token's own choice otherwise).  Keeps what the checks read and drops the model's big
    arrays: out, tol = dr.tol, pav = sum_j p_j |v_jd|, extra = extra_tol over the 64 S shared keys, the appended key / value, the stale fill."""
    key = (tag, kv16, H, n_kv, name, pos, slot, max_pos, group, S, targets)
    if key in DREFS:
        return DREFS[key]
    sin, cos = rope
    mk = (tag, name, slot, n_kv, max_pos, group, S)
    if mk not in MASTERS:
        if group is None:
            MASTERS[mk] = dr.master(name, np.random.default_rng(dr.seed_of("inst", tag, name, slot)), max_pos, n_kv)
        else:
            gk = (tag, name, "group", group, n_kv, max_pos)
            if gk not in MASTERS:
                MASTERS[gk] = dr.master(name, np.random.default_rng(dr.seed_of("inst-group", tag, name, group)), max_pos, n_kv)
            MASTERS[mk] = member_master(name, MASTERS[gk], S, dr.seed_of("inst", tag, name, slot), max_pos, n_kv)
    m, dt = MASTERS[mk], dr.cache_dtype(kv16)
    q1, kn1, vn, t = dr.token(m, np.random.default_rng(dr.seed_of("inst", tag, H, name, pos, slot)), pos, H)
    if targets is not None:
        t = np.asarray(targets)
        q1 = np.stack([4.0 * m["u"][t[h], h // (H // n_kv)] for h in range(H)])
    qkv = dr.raw_qkv(q1, kn1, vn, pos, sin, cos)
    kp, vp = m["k"][:pos + 1].astype(dt).transpose(1, 0, 2), m["v"][:pos + 1].astype(dt).transpose(1, 0, 2)  # [kv, T, D] as the pool holds them
    ex = dr.exact(qkv, kp, vp, pos, sin, cos, H, n_kv, kv16, recs=())
    g = np.arange(H) // (H // n_kv)
    DREFS[key] = dict(pos=pos, qkv=qkv, out=ex["out"], tol=dr.tol(ex), pav=np.einsum("hj,hjd->hd", ex["p"], ex["aV"][g, :pos + 1]), t=t, kp=kp, vp=vp,
                      extra=extra_tol(ex, 64 * min(S, pos >> 6), kv16), stale=dr.stale(name, q1, n_kv, kv16),
                      kn=dr.rope1(qkv[H * D:(H + n_kv) * D].reshape(n_kv, D), pos, sin, cos), vn=qkv[(H + n_kv) * D:].reshape(n_kv, D),
                      vt=None if t is None else np.stack([ex["V"][h // (H // n_kv), t[h]] for h in range(H)]))
    return DREFS[key]


def decode_tol(ref, n_records, out_f16):
    """dr.tol + 2^-23 (pages + records merged) sum_j p_j |v_jd| + the shared keys' f16 operands (+ half an f16 ulp of an f16 row)"""
    return ref["tol"] + 2.0 ** -23 * (pages(ref["pos"]) + n_records) * ref["pav"] + ref["extra"] + (dr.half_ulp_f16(ref["out"]) if out_f16 else 0.0)


# ---- decode entry: the conditions ----------------------------------------------------------------------------------------------------------------
G3 = dict(H=6, n_kv=2, max_pos=576, positions=(0, 63, 64, 130, 300), companions=(200, 77), n_splits=(1, 3, 9), families=("gauss", "needle", "sunk"))
# 64 rows: a fixed spread over 0 .. 320 with both sides of the first page end; rows 5 and 40 idle
FULL = dict(H=8, n_kv=2, max_pos=384, n_splits=2, positions=tuple({0: 0, 1: 63, 2: 64, 63: 320}.get(i, (i * 131 + 17) % 320) for i in range(64)),
            idle={5: "table", 40: "page"}, families=("gauss", "sunk"))
# rows at or beyond the caller's bound are idle; n_splits 0 is the library's rule for THIS bound: ceil(200 / 64) = 4, the largest count it takes
BOUND = dict(H=8, n_kv=2, max_pos=576, key_bound=200, positions=(199, 200, 575, 130), n_splits=(0, 2), families=("gauss", "sunk"))
# one split owns 258 pages: page_of()'s table arm serves pages 256 and 257; with two splits each owns 129 and the arm stays cold
IDCAP = dict(H=2, n_kv=1, max_pos=258 * 64, positions=(16384 + 64 + 5, 70), n_splits=(1, 2), families=("gauss", "ramp12"))


# ---- prefill entry: segment sets (past, len) ---------------------------------------------------------------------------------------------------------
SETS = {"mixed": [(0, 200), (63, 65), (130, 1)], "edges": [(65, 129), (1, 63), (64, 64)], "forked": [(64, 63), (64, 1), (130, 200)]}  # the older test's
# T = 1 | a first page filled exactly | one slot into a second page | two rows across a page end (twice) | a short tail in a third page;
# then T % 64 >= 4 with T % 4 = 0, 1, 2, 3: the 16-byte unit of commit_k that straddles the key count
SETS["tiny"] = [(0, 1), (0, 64), (0, 65), (127, 2), (63, 2), (190, 5), (3, 5), (70, 3), (20, 2), (100, 3)]
STRADDLE = [(63, 2), (127, 3), (191, 2), (63, 3)]  # two page tiles each, one 64-row block each at H = 8: more new tiles than blocks
PASTS64 = (0, 1, 62, 63, 64, 65, 127, 130)
WIDE = dict(segs=[(PASTS64[s % 8], 1 + s % 5) for s in range(64)], order=tuple((37 * s + 11) % 64 for s in range(64)),
            forks=((4, 12), (5, 13), (6, 14), (7, 15), (20, 28)), idle=(22, 41))  # forks (a, b): b reads a's first page, read-only for both
PREFILL_IDCAP = [(16420, 50), (70, 3)]  # key tiles 256 and 257 of the first segment are walked through the table


def forks_of(name):
    return ((0, 1),) if name == "forked" else WIDE["forks"] if name == "wide" else ()


def prefill_segs(name):
    return WIDE["segs"] if name == "wide" else STRADDLE if name == "straddle" else PREFILL_IDCAP if name == "idcap" else SETS[name]


def prefill_order(name):
    n = len(prefill_segs(name))
    return WIDE["order"] if name == "wide" else tuple((s + n - 1) % n for s in range(n)) if n > 1 else (0,)  # never the table's order


def new_tiles(segs):
    """page tiles that take new positions: k_paged_prefill_prep's grid needs one block column per tile"""
    return sum((past + n - 1) // 64 - past // 64 + 1 for past, n in segs)


def packed_rows(segs, order, align):
    """-> (row0 per segment, n_rows): segments packed in `order`, each start aligned; the last one's padding is not part of the call"""
    row0, cursor = [0] * len(segs), 0
    for s in order:
        row0[s], cursor = cursor, cursor + -(-segs[s][1] // align) * align
    return row0, row0[order[-1]] + segs[order[-1]][1]


PCASES = {}


def prefill_case(rope, H, n_kv, name, set_name, kv16):
    """inputs and the model's rows of one (heads, family, segment set, pool type), computed once.  The tolerance is attn_ref.tol plus, stated,
    the per-tile rescale the older test leaves to tol()'s factor 2: n_tiles 2^-23 sum_j p_j |v_jd| (one rounding of each output accumulator
    and of l per key tile; n_tiles = the key tiles of the segment, an upper count for every one of its rows)."""
    key = (H, n_kv, name, set_name, kv16)
    if key in PCASES:
        return PCASES[key]
    sin, cos = rope
    dt, segs, forks = np.float16 if kv16 else np.float32, [], dict((b, a) for a, b in forks_of(set_name))
    for s, (past, n) in enumerate(prefill_segs(set_name)):
        T, pos = past + n, np.arange(past, past + n)
        q1, k1, v, _ = ar.family(name, np.random.default_rng(ar.seed_of("inst-prefill", H, name, set_name, s)), pos, T, H, n_kv)
        k_c, v_c = k1[:past].astype(dt), v[:past].astype(dt)  # the past as the pool holds it
        if s in forks:  # the first page is the other segment's
            k_c[:64], v_c[:64] = segs[forks[s]]["k_c"][:64], segs[forks[s]]["v_c"][:64]
        q_in, k_in, v_in = ar.unrope(q1, pos, sin, cos), ar.unrope(k1[past:], pos, sin, cos), v[past:].astype(np.float32)
        kh = np.concatenate([ar.f16(k_c), ar.operands_k(k_in, pos, sin, cos)])
        vh = np.concatenate([ar.f16(v_c), ar.operands_v(v_in)])
        qh = ar.operands_q(q_in, pos, sin, cos)
        model = {}
        for o16 in (False, True):
            want, tol, p = ar.model(qh, kh, vh, pos, out_f16=o16)
            pav = np.stack([p[h] @ np.abs(vh[:, h // (H // n_kv)]) for h in range(H)], axis=1)  # [n, H, D]
            model[o16] = (want, tol + pages(T - 1) * 2.0 ** -23 * pav)
        segs.append(dict(past=past, n=n, k_c=k_c, v_c=v_c, model=model,
                         qkv=np.concatenate([q_in.reshape(n, -1), k_in.reshape(n, -1), v_in.reshape(n, -1)], axis=1)))
    PCASES[key] = segs
    return segs


# ---- shared entry: rows (group index | None, position, idle kind | None) in launch order; a group's first row is its leader -------------------------
def _members(S, positions, g=0):
    return [(g, p, None) for p in positions]


def _spread(n, lo, hi):
    return tuple(lo + (i * 29) % (hi - lo + 1) for i in range(n))


SUFFIX_ROWS = _members(6, (384, 400, 447, 448, 450))
HEALTHY = [(1, 130, None), (1, 140, None), (None, 77, None)]
# name: dict(H, n_kv, max_pos, key_bound, runs {group: S}, rows, n_splits, nss, families, unchecked groups)
SHARED = {}


def _shared(name, rows, runs, nss, H=8, n_kv=2, max_pos=512, key_bound=None, n_splits=2, families=("fall12", "newtok", "ramp12"), unchecked=()):
    SHARED[name] = dict(H=H, n_kv=n_kv, max_pos=max_pos, key_bound=key_bound or max_pos, runs=runs, rows=rows, n_splits=n_splits, nss=nss, families=families,
                        unchecked=unchecked)


for _n, _nss in ((6, 1), (6, 2), (22, 1), (22, 2)):  # group 3: 18 rows (a member across tiles 0 | 1), 66 rows (several)
    _shared(f"g3-{_n}m-{_nss}", _members(2, _spread(_n, 128, 200)), {0: 2}, _nss, H=6)
for _n, _nss in ((4, 1), (8, 2), (12, 1), (24, 2), (28, 1)):  # group 4: 16, 32, 48 rows without a padding row; 96 and 112 rows, nt = 6, 7
    _shared(f"g4-{_n}m", _members(2, _spread(_n, 128, 200)), {0: 2}, _nss)
for _ns, _nss in ((1, 5), (1, 6), (3, 5), (2, 1)):  # the suffix behind 5 | 6 | 1 lead records, with and without arrival counters
    _shared(f"suffix-{_ns}-{_nss}", SUFFIX_ROWS, {0: 6}, _nss, n_splits=_ns)
_shared("leader-null", [(0, 150, "table"), (0, 128, None), (0, 191, None), (0, 260, None)], {0: 2}, 2)
_shared("leader-page", [(0, 150, "page"), (0, 128, None), (0, 191, None), (0, 260, None)], {0: 2}, 2)
_shared("dead-group", [(0, 150, "table"), (0, 160, "page"), (0, 170, "pos")] + HEALTHY, {0: 2, 1: 2}, 2)
# THE BROKEN PROMISE of include/bitnet_hip_pagedshared.h: a live member at 100 under a run of 2 pages.  Its group's values are not asserted.
_shared("broken", [(0, 130, None), (0, 100, None), (0, 140, None)] + HEALTHY, {0: 2, 1: 2}, 2, unchecked=(0,))
_shared("bound", [(0, 192, None), (0, 255, None), (0, 256, None), (0, 230, None)], {0: 3}, 2, key_bound=256)
# 258 shared pages in ONE shared split: page_of()'s table arm serves pages 256 and 257.  The needle heads look into exactly those pages.
_shared("idcap", _members(258, (258 * 64 + 3, 258 * 64 + 40)), {0: 258}, 1, H=2, n_kv=1, max_pos=259 * 64, n_splits=1, families=("gauss", "needle"))
IDCAP_TARGETS = (256 * 64 + 5, 257 * 64 + 63)


def shared_live(case):
    """per row: live by the entry's rules (pointers, position below the bound, page ids inside the pool)"""
    return [idle is None and pos < case["key_bound"] for _, pos, idle in case["rows"]]


def shared_rows(case, group):
    """query rows and 16-row tiles of a group's shared pass"""
    n = sum(live and g == group for (g, _, _), live in zip(case["rows"], shared_live(case)))
    rows = n * (case["H"] // case["n_kv"])
    return rows, -(-rows // 16)


def straddlers(case, group):
    """live members of a group whose heads lie in two 16-row tiles"""
    grp = case["H"] // case["n_kv"]
    n = shared_rows(case, group)[0] // grp
    return [i for i in range(n) if (i * grp) // 16 != (i * grp + grp - 1) // 16]
