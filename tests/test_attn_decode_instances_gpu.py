"""Every instance of the one-token decode attention (kernels_attn.hip), by value, against the float64 model tests/attn_decode_ref.py.

Instances and the test that runs each (`wide` = 128-position records, NH = 2; kv16 = f16 caches):
  k_attn_partial<1, false>   test_batch1_records_and_rows[*-narrow-kv32]     k_attn_partial<2, false>   test_batch1_records_and_rows[*-wide-kv32]
  k_attn_partial<1, true>    test_batch1_records_and_rows[*-narrow-kv16]     k_attn_partial<2, true>    test_batch1_records_and_rows[*-wide-kv16]
      each twice per case: with BITNET_HIP_ATTN_PARTIAL (the records stay in `scratch` and are read back: the producer of records by value)
      and combined (the output row, the appended key / value, every other cache byte, the guards);
  k_attn_combine<NR>         the combined launch of the same test; NR follows the layout's record count (attn_combine_nr: <= 8 -> 1, <= 16 -> 2,
                             <= 40 -> 5, else 8), the layouts sit on both sides of every threshold:
        max_pos   records of 64 -> NR              records of 128 -> NR
        300       5 -> 1 (last tile padding)       3 -> 1 (the last record's second half lies past the allocation)
        512       8 -> 1                           4 -> 1
        576       9 -> 2                           5 -> 1
        1024      16 -> 2                          8 -> 1
        1088      17 -> 5                          9 -> 2
        2560      40 -> 5                          20 -> 5
        2624      41 -> 8                          21 -> 5
        4096      64 -> 8                          32 -> 5
        4160      65 -> 8 + one trip of the loop behind 8 * NR, one record (pos 4159)       33 -> 5
        6208      97 -> 8 + two trips, the second with one record (pos >= 6144)             49 -> 8
        8256      (wide only)                      65 -> 8 + one trip (pos >= 8192)
  k_attn_partial_batch<false | true>, k_attn_combine_batch<2 | 5 | 8>   test_batched_form_by_value at max_pos 576 / 1088 / 2624, 4160 (NR 8 and the loop: pos 4159)
  k_attn_partial_rows<false | true>,  k_attn_combine_rows<1 | 2 | 5 | 8> test_rows_form_by_value: NR comes from key_bound (130 -> 1 at every layout, max_pos -> 2 / 5 / 8 / 8 + loop),
                             n_chunks_max from the layout: the two clamps of attn_combine_body; f32 and f16 output rows
  k_attn_combine_batch<1> has no layout of its own here: at <= 8 records it is the NR = 1 body that k_attn_combine<1> and k_attn_combine_rows<1> run, and
  tests/test_batch_ops_gpu.py holds the batched form bit-equal to batch-1 at max_pos 300.
No decode-attention entry refuses a max_pos that is not a multiple of 64 (300 runs in all of them: the caches are padded to whole tiles).

Head shapes (n_heads, n_kv) = (2, 2), (4, 2), (6, 2), (8, 2): query groups 1 to 4 (3 leaves the fourth RoPE wave without a head); all four at max_pos 512 and
300, (6, 2) and (8, 2) elsewhere.  Positions: 0, 1, 62, 63, 64, 65, 127, 128, 129, the last position of record 8 / 16 / 40 / 64 / 96 and the first of the
next, max_pos - 1 -- `gauss` and `needle` at all of them, the other families at 37, just past the last 128-boundary, and max_pos - 1.  Thinned for the
file's wall time at the three largest layouts (4160, 6208, 8256) only: there `gauss` skips the LAST position of records 8 / 16 / 40 / 64 / 96 (it runs
at the first of the next, where the record count steps); `needle` keeps both sides, with targets on both sides of every boundary.

Every case: a device master of the family's caches is cloned, the slots at and past pos are overwritten with hostile stale values
(attn_decode_ref.stale), every record in `scratch` is pre-filled with (m, l, o) = (1e4, 1e3, 1e6) -- a combine that merges one record too many is
wrong by orders of magnitude -- and the buffers sit between guard words.  Rows are held to attn_decode_ref.tol() per element, records to rec_tol();
needle rows equal v[t(h)] to the last bit.  The worst err / tol per instance and family is printed when the module ends (lines starting ATTND).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_decode_ref as dr  # noqa: E402
import extend_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

D = 128
N_KV = 2
REC_FLOATS = 2 * 4 + 4 * D  # (m, l)[4], o[4][128]
TABLE_POS = 8256
LAYOUTS = (300, 512, 576, 1024, 1088, 2560, 2624, 4096, 4160, 6208, 8256)
WIDE_ONLY = (8256,)
THIN = (4160, 6208, 8256)
ALL_HEADS = ((2, 2), (4, 2), (6, 2), (8, 2))
OTHERS = ("ramp12", "fall12", "newtok", "oldonly", "sunk")
BATCH_LAYOUTS = (576, 1088, 2624, 4160)
BATCH_FAMILIES = ("gauss", "ramp12", "sunk", "needle")
SENT = 0x5A
GUARD = 0xA5
WORST = {}  # (instance, family) -> (err / tol, case)


def heads_of(L):
    return ALL_HEADS if L in (300, 512) else ((6, 2), (8, 2))


def boundary(L):
    """the first slot of the last record (of either size) that starts below max_pos - 1"""
    return (L - 2) // 128 * 128


def positions(L, wide):
    rec = 128 if wide else 64
    ps = {0, 1, 62, 63, 64, 65, 127, 128, 129, L - 1}
    for r in (8, 16, 40, 64, 96):
        ps |= {r * rec - 1, r * rec}
    return sorted(p for p in ps if p < L)


def cases_of(L, wide):
    """[(family, pos)]"""
    rec = 128 if wide else 64
    thinned = {r * rec - 1 for r in (8, 16, 40, 64, 96)} if L in THIN else set()
    out = [(name, p) for p in positions(L, wide) for name in ("gauss", "needle") if not (name == "gauss" and p in thinned)]
    return out + [(name, p) for name in OTHERS for p in (37, boundary(L), L - 1)]


def note(inst, name, r, case):
    if r > WORST.get((inst, name), (-1.0, None))[0]:
        WORST[(inst, name)] = (r, case)


class Guarded:
    """nbytes of device memory between two 64-byte guards that must survive every launch"""

    def __init__(self, t, nbytes):
        self.t = t
        self.buf = t.full((nbytes + 128,), GUARD, dtype=t.uint8, device="cuda")
        self.raw = self.buf[64: 64 + nbytes]

    def view(self, dtype):
        return self.raw.view(dtype)

    def check(self, tag):
        g = self.t.cat([self.buf[:64], self.buf[-64:]])
        assert bool((g == GUARD).all().item()), (tag, "guard overwritten")


class Rig:
    """the library, the RoPE tables on both sides, and per layout: the families' masters (host and device), the guarded buffers, the model's results"""

    def __init__(self, hip, oracle, torch):
        self.hip, self.t = hip, torch
        sin, cos = oracle.rope_tables(D, TABLE_POS, 10000.0)  # row p depends on p alone: one table serves every layout
        self.sin, self.cos = sin.reshape(TABLE_POS, D // 2), cos.reshape(TABLE_POS, D // 2)
        self.sin_d, self.cos_d = self.dev(np.asarray(sin, np.float32)), self.dev(np.asarray(cos, np.float32))
        self.L = None
        tmpl = np.empty(REC_FLOATS, np.float32)
        tmpl[0:8:2], tmpl[1:8:2], tmpl[8:] = dr.DEAD_RECORD
        self.tmpl = tmpl
        self.tmpl_d = self.dev(tmpl)

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def layout(self, L):
        if self.L != L:  # one layout's masters and results at a time
            self.L, self.masters, self.casts, self.dmasters, self.bufs, self.refs, self.ref_block = L, {}, {}, {}, {}, {}, None
        return self

    # ---- inputs ----
    def master(self, name):
        if name not in self.masters:
            self.masters[name] = dr.master(name, np.random.default_rng(dr.seed_of("decode", self.L, name)), self.L, N_KV)
        return self.masters[name]

    def cast(self, name, kv16):
        """the master's keys / values in the cache's dtype, [kv, T, D] (host) and in the cache's layout (device)"""
        key = (name, kv16)
        if key not in self.casts:
            m, dt = self.master(name), dr.cache_dtype(kv16)
            k, v = m["k"].astype(dt), m["v"].astype(dt)
            self.casts[key] = (np.ascontiguousarray(k.transpose(1, 0, 2)), np.ascontiguousarray(v.transpose(1, 0, 2)))
            self.dmasters[key] = (self.dev(er.encode_k(k, self.L, kv16)), self.dev(er.encode_v(v, self.L, kv16)))
        return self.casts[key]

    def ref(self, heads, kv16, name, pos, recs):
        """the model's results for one step (computed once per layout, head shape and cache type; the operands are dropped)"""
        block = (heads, kv16)
        if self.ref_block != block:
            self.ref_block, self.refs = block, {}
        key = (name, pos)
        if key not in self.refs or not set(recs) <= set(self.refs[key]["rec"]):
            H, n_kv = heads
            m = self.master(name)
            q1, kn1, vn, t = dr.token(m, np.random.default_rng(dr.seed_of("decode", self.L, H, name, pos)), pos, H)
            qkv = dr.raw_qkv(q1, kn1, vn, pos, self.sin, self.cos)
            kp, vp = self.cast(name, kv16)
            ex = dr.exact(qkv, kp, vp, pos, self.sin, self.cos, H, n_kv, kv16, recs)
            if name == "needle":  # the family's condition, from the model
                assert all(ex["p"][h, t[h]] >= 1.0 - 2.0 ** -60 for h in range(H)), (self.L, heads, pos)
            tl = dr.tol(ex)
            self.refs[key] = dict(qkv=qkv, out=ex["out"], tol=tl, tol16=tl + dr.half_ulp_f16(ex["out"]), t=t, stale=dr.stale(name, q1, n_kv, kv16),
                                  kn=dr.rope1(qkv[H * D:(H + n_kv) * D].reshape(n_kv, D), pos, self.sin, self.cos), vn=qkv[(H + n_kv) * D:].reshape(n_kv, D),
                                  rec={r: (ex["rec"][r], dr.rec_tol(ex, r)) for r in recs},
                                  vt=None if t is None else np.stack([ex["V"][h // (H // n_kv), t[h]] for h in range(H)]))
        return self.refs[key]

    # ---- device buffers of one (layout, cache type): caches for up to four sequences, one scratch area per sequence ----
    def buffers(self, kv16):
        if kv16 not in self.bufs:
            C = er.chunks(self.L)
            nbytes = N_KV * C * 64 * D * (2 if kv16 else 4)
            sb = int(self.hip.c.bitnet_hip_attention_scratch_bytes(N_KV, self.L))
            assert sb == N_KV * C * REC_FLOATS * 4
            self.bufs[kv16] = dict(k=[Guarded(self.t, nbytes) for _ in range(4)], v=[Guarded(self.t, nbytes) for _ in range(4)],
                                   scratch=Guarded(self.t, 4 * sb), sb=sb, C=C)
        return self.bufs[kv16]

    def cdt(self, kv16):
        return self.t.float16 if kv16 else self.t.float32

    def kslot(self, x, pos, kv16):
        """the elements of slot `pos` in a flat per-element tensor laid out as the K cache -> an indexed view"""
        C = er.chunks(self.L)
        if kv16:
            return x.view(N_KV, C, D // 2, 64, 2)[:, pos // 64, :, pos % 64, :]
        return x.view(N_KV, C, D, 64)[:, pos // 64, :, pos % 64]

    def vslot(self, x, pos):
        return x.view(N_KV, er.chunks(self.L) * 64, D)[:, pos]

    def fill_caches(self, b, kv16, name, stale, pos):
        """sequence slot b: the family's master, hostile values in every slot at and past pos -> (k, v, clones of both)"""
        t, C = self.t, er.chunks(self.L)
        bufs = self.buffers(kv16)
        self.cast(name, kv16)
        mk, mv = self.dmasters[(name, kv16)]
        k, v = bufs["k"][b].view(self.cdt(kv16)), bufs["v"][b].view(self.cdt(kv16))
        k.copy_(mk), v.copy_(mv)
        ks, vs = self.dev(stale[0]), self.dev(stale[1])
        c, p = divmod(pos, 64)
        if kv16:
            k5, ks5 = k.view(N_KV, C, D // 2, 64, 2), ks.view(N_KV, D // 2, 2)
            k5[:, c, :, p:, :] = ks5[:, :, None, :]
            k5[:, c + 1:] = ks5[:, None, :, None, :]
        else:
            k4 = k.view(N_KV, C, D, 64)
            k4[:, c, :, p:] = ks[:, :, None]
            k4[:, c + 1:] = ks[:, None, :, None]
        v.view(N_KV, C * 64, D)[:, pos:] = vs[:, None, :]
        return k, v, k.clone(), v.clone()

    def fill_records(self, area, sb):
        """one sequence's record area: every record hostile"""
        area.view(self.t.float32).view(-1, REC_FLOATS)[:] = self.tmpl_d

    def check_append(self, k, v, k0, v0, ref, pos, kv16, tag):
        """the key / value appended at pos; every other element of both caches keeps its bits"""
        t = self.t
        it = t.int16 if kv16 else t.int32
        nk, nv = k.view(it) != k0.view(it), v.view(it) != v0.view(it)
        self.kslot(nk, pos, kv16)[...] = False
        self.vslot(nv, pos)[...] = False
        assert int(nk.sum().item()) == 0 and int(nv.sum().item()) == 0, (tag, "a cache element outside the appended slot changed")
        gk = self.kslot(k, pos, kv16).reshape(N_KV, D).cpu().numpy().astype(np.float64)
        gv = self.vslot(v, pos).cpu().numpy()
        kn = ref["kn"]
        if kv16:  # the key on the nearest f16 of the float64 rotation or on its neighbour; the value the exact f16 rounding
            near = dr.f16(kn)
            ulp = np.maximum(np.spacing(np.abs(near).astype(np.float16)), np.spacing(np.abs(gk).astype(np.float16))).astype(np.float64)
            assert np.all(np.abs(gk - near) <= ulp), (tag, "appended key")
            assert np.array_equal(gv.view(np.uint16), ref["vn"].astype(np.float16).view(np.uint16)), (tag, "appended value")
        else:  # three f32 roundings of x0 c -+ x1 s: 2^-22 of the rotation pair's length (one element of a pair can cancel)
            pair = np.hypot(kn[:, : D // 2], kn[:, D // 2:])
            assert np.all(np.abs(gk - kn) <= 2.0 ** -22 * np.concatenate([pair, pair], axis=1)), (tag, "appended key")
            assert np.array_equal(gv.view(np.uint32), ref["vn"].view(np.uint32)), (tag, "appended value")

    def check_records(self, area_np, ref, heads, pos, rec, n_rec, tag):
        """area_np: one sequence's record area as float32 [rows, 520] (read back).  Live records of the group's live heads against the model; every
        other row keeps the hostile bits.  -> max(err / tol)"""
        H, n_kv = heads
        group = H // n_kv
        R = pos // rec + 1
        rows = area_np.shape[0]
        live = np.zeros(rows, bool)
        for g in range(n_kv):
            live[g * n_rec: g * n_rec + R] = True
        assert np.array_equal(area_np[~live].view(np.uint32), np.broadcast_to(self.tmpl.view(np.uint32), ((~live).sum(), REC_FLOATS))), (tag, "a dead record changed")
        a = area_np[: n_kv * n_rec].reshape(n_kv, n_rec, REC_FLOATS)[:, :R]
        m = a[:, :, 0:8:2][:, :, :group].transpose(0, 2, 1).reshape(H, R)
        l = a[:, :, 1:8:2][:, :, :group].transpose(0, 2, 1).reshape(H, R)
        o = a[:, :, 8:].reshape(n_kv, R, 4, D)[:, :, :group].transpose(0, 2, 1, 3).reshape(H, R, D)
        (m_ref, l_ref, o_ref), (tm, tl, to) = ref["rec"][rec]
        m, l, o = m.astype(np.float64), l.astype(np.float64), o.astype(np.float64)
        assert np.isfinite(m).all() and np.isfinite(l).all() and np.isfinite(o).all(), (tag, "a live record is not finite")
        f = np.exp(m - m_ref)
        r = max(dr.ratio(m, m_ref, tm), dr.ratio(l * f, l_ref, tl), dr.ratio(o * f[..., None], o_ref, to))
        assert r <= 1.0, (tag, "records", r)
        return r

    def check_rows(self, got, ref, name, tag, out_f16=False):
        H = ref["out"].shape[0]
        got = got.reshape(H, D).astype(np.float64)
        assert np.isfinite(got).all(), (tag, "an element the call did not write, or a NaN / inf it computed")
        r = dr.ratio(got, ref["out"], ref["tol16"] if out_f16 else ref["tol"])
        assert r <= 1.0, (tag, "rows", r)
        if name == "needle":
            assert np.array_equal(got, ref["vt"]), (tag, "needle rows are v[t(h)] to the last bit", ref["t"])
        return r


@pytest.fixture(scope="module")
def rig(hip, oracle):
    import torch

    yield Rig(hip, oracle, torch)
    for (inst, name), (r, case) in sorted(WORST.items()):
        print(f"ATTND instance={inst} family={name}: worst err/tol {r:.4f} at {case}")


# ---- batch-1: the four k_attn_partial<NH, KV16> instances, records and rows -----------------------------------------------------------------
B1 = [(L, h, w, k) for L in LAYOUTS for h in heads_of(L) for k in (False, True) for w in ((True,) if L in WIDE_ONLY else (False, True))]
b1_id = lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{'wide' if c[2] else 'narrow'}-{'kv16' if c[3] else 'kv32'}"  # noqa: E731


@pytest.mark.parametrize("case", B1, ids=b1_id)
def test_batch1_records_and_rows(rig, case):
    """attention_decode_q_dev.  Per (family, position): the partial launch -- every live record's (m, l, o) against the model, every record at or past
    the live count untouched; then the combined launch on the same pre-filled scratch -- the row within tol(), the appended key and value, every other
    byte of both caches, the guard words round out, scratch and both caches."""
    L, heads, wide, kv16 = case
    H, n_kv = heads
    t, hip = rig.t, rig.hip
    rig.layout(L)
    bufs = rig.buffers(kv16)
    rec = 128 if wide else 64
    n_rec = (L + rec - 1) // rec
    inst = f"k_attn_partial<{2 if wide else 1},{'true' if kv16 else 'false'}>"
    area = bufs["scratch"].raw[: bufs["sb"]]
    for name, pos in cases_of(L, wide):
        tag = (b1_id(case), name, pos)
        ref = rig.ref(heads, kv16, name, pos, (128,) if L in WIDE_ONLY else (64, 128))  # (shared by the narrow and the wide instance)
        qkv_d, pos_d = rig.dev(ref["qkv"]), t.tensor([pos], dtype=t.int32, device="cuda")
        # -- the records
        k, v, k0, v0 = rig.fill_caches(0, kv16, name, ref["stale"], pos)
        rig.fill_records(area, bufs["sb"])
        hip.attention_decode_q_dev(qkv_d, rig.sin_d, rig.cos_d, k, v, H, n_kv, D, L, pos_d, area, None, None, wide=wide, kv_f16=kv16, partial=True)
        t.cuda.synchronize()
        rr = rig.check_records(area.view(t.float32).cpu().numpy().reshape(-1, REC_FLOATS), ref, heads, pos, rec, n_rec, tag)
        note(inst + " records", name, rr, tag)
        # -- the row, on fresh caches and the same hostile scratch
        k, v, k0, v0 = rig.fill_caches(0, kv16, name, ref["stale"], pos)
        rig.fill_records(area, bufs["sb"])
        out = Guarded(t, H * D * 4)
        out.view(t.float32).fill_(float("nan"))
        hip.attention_decode_q_dev(qkv_d, rig.sin_d, rig.cos_d, k, v, H, n_kv, D, L, pos_d, area, out.view(t.float32), None, wide=wide, kv_f16=kv16)
        t.cuda.synchronize()
        assert int(pos_d.item()) == pos
        r = rig.check_rows(out.view(t.float32).cpu().numpy(), ref, name, tag)
        note(inst + " + k_attn_combine", name, r, tag)
        rig.check_append(k, v, k0, v0, ref, pos, kv16, tag)
        for g in (out, bufs["scratch"], bufs["k"][0], bufs["v"][0]):
            g.check(tag)


# ---- the batched and the rows form ---------------------------------------------------------------------------------------------------------
BR = [(L, h, k) for L in BATCH_LAYOUTS for h in ((6, 2), (8, 2)) for k in (False, True)]
br_id = lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{'kv16' if c[2] else 'kv32'}"  # noqa: E731


def ptr_table(t, tensors):
    return t.tensor([0 if x is None else x.data_ptr() for x in tensors], dtype=t.int64, device="cuda")


def run_multi(rig, case, name, seq_pos, key_bound=None, out_f16=False):
    """One launch of the batched (key_bound None) or the rows form.  seq_pos: per sequence a position, or None for a NULL slot.  Sequences at
    pos >= key_bound are beyond the bound.  Live rows within tol(); the appended slots; idle and beyond-bound sequences untouched bit for bit."""
    L, heads, kv16 = case
    H, n_kv = heads
    t, hip = rig.t, rig.hip
    rig.layout(L)
    bufs = rig.buffers(kv16)
    sb, n = bufs["sb"], len(seq_pos)
    rows = key_bound is not None
    alive = [p is not None and (not rows or p < key_bound) for p in seq_pos]
    tag0 = (br_id(case), name, tuple(seq_pos), key_bound, out_f16)
    refs, caches, pos_d = [None] * n, [None] * n, [None] * n
    qkv = np.full((n, (H + 2 * n_kv) * D), np.nan, np.float32)
    for b, p in enumerate(seq_pos):
        area = bufs["scratch"].raw[b * sb:(b + 1) * sb]
        if p is None:
            area.fill_(SENT)
            continue
        pos_d[b] = t.tensor([p], dtype=t.int32, device="cuda")
        if alive[b]:
            refs[b] = rig.ref(heads, kv16, name, p, (64,))
            qkv[b] = refs[b]["qkv"]
            caches[b] = rig.fill_caches(b, kv16, name, refs[b]["stale"], p)
            rig.fill_records(area, sb)
        else:  # beyond the bound: a well-formed sequence (its slot below max_pos) that the launch must leave alone
            inner = min(p, L - 1)
            ref = rig.ref(heads, kv16, name, inner, (64,))
            qkv[b] = ref["qkv"]
            caches[b] = rig.fill_caches(b, kv16, name, ref["stale"], inner)
            area.fill_(SENT)
    esz = 2 if out_f16 else 4
    out = Guarded(t, n * H * D * esz)
    out.raw.fill_(SENT)
    kt = ptr_table(t, [None if c is None else c[0] for c in caches])
    vt = ptr_table(t, [None if c is None else c[1] for c in caches])
    pt = ptr_table(t, pos_d)
    qkv_d = rig.dev(qkv)
    odt = t.float16 if out_f16 else t.float32
    if rows:
        hip.attention_decode_rows_dev(qkv_d, rig.sin_d, rig.cos_d, kt, vt, pt, n, H, n_kv, D, L, key_bound, bufs["scratch"].raw, out.view(odt), kv_f16=kv16,
                                      out_f16=out_f16)
        inst = f"k_attn_partial_rows<{'true' if kv16 else 'false'}> + k_attn_combine_rows" + (" f16 rows" if out_f16 else "")
    else:
        hip.attention_decode_batch_dev(qkv_d, rig.sin_d, rig.cos_d, kt, vt, pt, n, H, n_kv, D, L, bufs["scratch"].raw, out.view(odt), None, kv_f16=kv16)
        inst = f"k_attn_partial_batch<{'true' if kv16 else 'false'}> + k_attn_combine_batch"
    t.cuda.synchronize()
    got = out.raw.cpu().numpy().reshape(n, H * D * esz)
    scr = bufs["scratch"].raw[: n * sb].cpu().numpy().reshape(n, sb)
    for b, p in enumerate(seq_pos):
        tag = tag0 + (b,)
        if alive[b]:
            assert int(pos_d[b].item()) == p
            r = rig.check_rows(got[b].view(np.float16 if out_f16 else np.float32), refs[b], name, tag, out_f16)
            note(inst, name, r, tag)
            k, v, k0, v0 = caches[b]
            rig.check_append(k, v, k0, v0, refs[b], p, kv16, tag)
            rr = rig.check_records(scr[b].view(np.float32).reshape(-1, REC_FLOATS), refs[b], heads, p, 64, er.chunks(L), tag)
            note(inst.split(" + ")[0] + " records", name, rr, tag)
        else:
            assert np.all(got[b] == SENT), (tag, "output row of an idle sequence")
            assert np.all(scr[b] == SENT), (tag, "record area of an idle sequence")
            if caches[b] is not None:
                k, v, k0, v0 = caches[b]
                it = t.int16 if kv16 else t.int32
                assert t.equal(k.view(it), k0.view(it)) and t.equal(v.view(it), v0.view(it)), (tag, "caches of a sequence beyond the bound")
    for g in [out, bufs["scratch"]] + bufs["k"][:n] + bufs["v"][:n]:
        g.check(tag0)


@pytest.mark.parametrize("case", BR, ids=br_id)
def test_batched_form_by_value(rig, case):
    """attention_decode_batch_dev, n_seq = 3: a live sequence, a NULL slot, a live sequence at another position.  max_pos - 1 runs the whole layout
    (at 4160: 65 records, the loop behind 8 * NR); (129, 37) leaves most of the NR records up front dead."""
    L = case[0]
    for name in BATCH_FAMILIES:
        run_multi(rig, case, name, [L - 1, None, 129])
        run_multi(rig, case, name, [129, None, 37])


@pytest.mark.parametrize("case", BR, ids=br_id)
def test_rows_form_by_value(rig, case):
    """attention_decode_rows_dev, n_seq = 4: live, NULL, live, and a sequence at pos >= key_bound.  key_bound = max(pos) + 1 and = max_pos: with
    short positions NR comes from the bound (130 -> 3 records -> 1) and n_chunks_max from the layout; f32 and f16 output rows."""
    L = case[0]
    for name in BATCH_FAMILIES:
        for out_f16 in (False, True):
            run_multi(rig, case, name, [L - 1, None, 129, L], key_bound=L, out_f16=out_f16)
            run_multi(rig, case, name, [129, None, 37, 130], key_bound=130, out_f16=out_f16)
            run_multi(rig, case, name, [129, None, 37, L], key_bound=L, out_f16=out_f16)
