"""GPU checks of bitnet_hip_attention_packed_dev: several sequences' new tokens in ONE prep launch and ONE attention launch
(k_packed_prep + k_prefill_attn_packed), each segment at its own past length over its own caches.

Per segment the contract is bitnet_hip_attention_extend_dev's, so the gates are that operator's (tests/test_extend_gpu.py,
tests/test_prefill_parity.py): max|diff| <= 6e-3 and cosine >= 0.9999 against float64 (tests/extend_ref.py) for the f16 operand
rounding; 2e-4 of max|base| against the existing operator on the same operands; appended cache rows bit for bit.  What is new is
that segments share a launch, and that is checked WITHOUT a tolerance: replacing one segment's rows and past changes no bit of any
other segment's output or cache, stale slots and padding rows hold NaNs that must never surface, and bystanders' caches and the
guard bytes around the workspace keep their bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402
from test_extend_gpu import Op, bits, cosine  # noqa: E402

pytestmark = pytest.mark.gpu

D = 128
CACHE_F16, OUT_F16 = 1, 2
MAX_POS = 300  # 5 chunks of 64: the last tile of every cache is partly padding
GUARD = 256

SETS = {
    "one": [(0, 65)],
    "three_fresh": [(0, 21), (0, 130), (0, 64)],
    "four_live": [(33, 1), (0, 64), (70, 37), (64, 65)],
    # more segments than BITNET_HIP_BATCH_MAX; lengths from {1, 2, 5, 21, 63, 64, 65}, pasts from {0, 1, 63, 64, 100}
    "twelve": [(0, 1), (1, 2), (63, 5), (64, 21), (100, 63), (0, 64), (1, 65), (63, 1), (64, 2), (100, 5), (0, 21), (1, 63)],
}
HEADS = [(4, 2), (6, 3), (3, 3)]  # row alignment 64, 64, 128
# GQA group 4: k_prefill_attn_packed<4,4,2>, whose workgroups hold 32 queries, so TWO workgroups share every 64-row record -- the instantiation
# the 2B-4T model (20/5) runs.  The last set is a full table: BITNET_HIP_PACK_MAX segments.
HEADS_G4 = [(8, 2), (20, 5)]
SETS_G4 = dict(SETS, sixty_four=[((0, 1, 63, 64, 100)[i % 5], (1, 2, 5, 21, 63, 64, 65)[i % 7]) for i in range(64)])


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


class Pack:
    """the segments of one case: per segment a sequence of past + len tokens, an Op (its caches), the packed row layout"""

    def __init__(self, hip, oracle, t, n_heads, n_kv, f16, segs, seed):
        self.hip, self.t, self.n_heads, self.n_kv, self.f16, self.segs = hip, t, n_heads, n_kv, f16, segs
        self.ld = (n_heads + 2 * n_kv) * D
        self.align = hip.attention_packed_row_align(n_heads, n_kv)
        rng = self.rng = np.random.default_rng(seed)
        self.seq = [rng.normal(0, rng.uniform(1.2, 1.5), (p + n, self.ld)).astype(np.float32) for p, n in segs]
        self.ops = [Op(hip, oracle, t, n_heads, n_kv, MAX_POS, f16) for _ in segs]
        # row starts in a shuffled order, so the order in the row space is not the table order
        self.row0 = [0] * len(segs)
        at = 0
        for s in rng.permutation(len(segs)):
            self.row0[s] = at
            at = (at + segs[s][1] + self.align - 1) // self.align * self.align
        self.n_rows = max(r + n for r, (_, n) in zip(self.row0, segs)) + 3  # three trailing padding rows
        for i, (p, n) in enumerate(segs):
            self.fill_past(self.ops[i], self.seq[i], p, chain=i % 2 == 1)

    def fill_past(self, op, seq, past, chain):
        """positions 0 .. past - 1 by the whole-prompt operator, or by two continuations from an empty cache; NaNs everywhere beyond"""
        if past > 0:
            if chain and past > 1:
                op.extend(seq[:past // 2], 0)
                op.extend(seq[past // 2:past], past // 2)
            else:
                op.prefill(seq[:past])
        k, v = op.caches()
        k[past:], v[past:] = np.nan, np.nan
        dt = self.t.float16 if self.f16 else self.t.float32
        op.kc = self.t.from_numpy(er.encode_k(k, er.chunks(MAX_POS) * 64, self.f16)).to(dt).cuda()
        op.vc = self.t.from_numpy(er.encode_v(v, er.chunks(MAX_POS) * 64, self.f16)).to(dt).cuda()

    def rows(self, seq=None):
        """the packed [n_rows, ld] matrix: every segment's new rows at its row0, NaNs in every padding row"""
        seq = self.seq if seq is None else seq
        qkv = np.full((self.n_rows, self.ld), np.nan, np.float32)
        for r, (p, n), x in zip(self.row0, self.segs, seq):
            qkv[r:r + n] = x[p:]
        return qkv

    def snapshot(self):
        return [(op.kc.clone(), op.vc.clone()) for op in self.ops]

    def call(self, qkv, caches, out_f16=False, misalign=False):
        """-> out [n_rows, heads * D] float32 (numpy); `caches`: [(kc, vc)] device tensors, written in place"""
        t = self.t
        past, ln = [p for p, _ in self.segs], [n for _, n in self.segs]
        wsb = self.hip.attention_packed_workspace_bytes(self.n_heads, self.n_kv, self.n_rows, past, ln)
        assert wsb > 0
        ws = t.full((wsb + 2 * GUARD,), 0xA5, dtype=t.uint8, device="cuda")
        ws[GUARD:GUARD + wsb] = 0xFF  # NaN patterns: nothing the call did not write may be read
        out = t.full((self.n_rows, self.n_heads * D), float("nan"), dtype=t.float16 if out_f16 else t.float32, device="cuda")
        if misalign:  # rows 4 bytes off a 16-byte boundary: the query image comes from the query-prep launch
            buf = t.zeros(qkv.size + 1, dtype=t.float32, device="cuda")
            buf[1:] = t.from_numpy(qkv.ravel()).cuda()
            q_ptr = buf.data_ptr() + 4
        else:
            buf = t.from_numpy(qkv).cuda()
            q_ptr = buf.data_ptr()
        op = self.ops[0]
        self.hip.attention_packed_dev(q_ptr, self.n_rows, op.sin_d, op.cos_d, self.row0, ln, past, [c[0] for c in caches], [c[1] for c in caches], self.n_heads,
                                      self.n_kv, D, MAX_POS, ws.data_ptr() + GUARD, wsb, out, (CACHE_F16 if self.f16 else 0) | (OUT_F16 if out_f16 else 0))
        t.cuda.synchronize()
        g = ws.cpu().numpy()
        assert (g[:GUARD] == 0xA5).all() and (g[GUARD + wsb:] == 0xA5).all(), "guard bytes around the workspace changed"
        return out.float().cpu().numpy()

    def decode(self, c):
        return er.decode_k(c[0].cpu().numpy(), self.n_kv, MAX_POS, self.f16), er.decode_v(c[1].cpu().numpy(), self.n_kv, MAX_POS, self.f16)

    def padding_rows(self):
        pad = np.ones(self.n_rows, bool)
        for r, (_, n) in zip(self.row0, self.segs):
            pad[r:r + n] = False
        return pad


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def dev_bits(t, x):
    return x.view(t.int16 if x.dtype == t.float16 else t.int32)


G4_CASES = [(n, h, k) for n in SETS_G4 for h in HEADS_G4 for k in (False, True) if n in ("four_live", "twelve") or (n == "sixty_four") == (h == (20, 5))]


@pytest.mark.parametrize("name,heads,f16", G4_CASES, ids=lambda x: x if isinstance(x, str) else f"{x[0]}x{x[1]}" if isinstance(x, tuple) else "kv16" if x else "kv32")
def test_group_4_heads_and_a_full_table(hip, oracle, torch_, name, heads, f16):
    """the same checks on the 32-query workgroups of GQA group 4 (8/2: every set but the full table; 20/5: the live sets and the full table)"""
    check_pack(hip, oracle, torch_, SETS_G4[name], heads, f16, name)


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"{h[0]}x{h[1]}")
@pytest.mark.parametrize("name", list(SETS))
def test_packed_segments_against_f64_the_solo_operator_and_each_other(hip, oracle, torch_, name, heads, f16):
    check_pack(hip, oracle, torch_, SETS[name], heads, f16, name)


def check_pack(hip, oracle, torch_, segs, heads, f16, name):
    t = torch_
    n_heads, n_kv = heads
    P = Pack(hip, oracle, t, n_heads, n_kv, f16, segs, seed=11 * len(segs) + n_heads + (100 if f16 else 0))
    # a bystander: a cache of random bits that is in no table
    by = t.from_numpy(P.rng.integers(0, 2 ** 31 - 1, P.ops[0].elems // (2 if f16 else 1), dtype=np.int32)).cuda()
    by0 = by.clone()
    before = P.snapshot()
    qkv = P.rows()
    c1 = P.snapshot()
    out1 = P.call(qkv, c1)
    assert t.equal(by, by0)
    assert np.isfinite(out1).all(), "a NaN from a stale slot or a padding row surfaced (padding rows must be finite too)"
    for i, ((past, n), r0, op) in enumerate(zip(segs, P.row0, P.ops)):
        T = past + n
        got = out1[r0:r0 + n].reshape(n, n_heads, D)
        # ---- float64 ----
        pos = np.arange(T)
        _, k_all, v_all = er.split_qkv(P.seq[i], n_heads, n_kv)
        k_all = er.rope_np(k_all, op.sin[pos, None, :], op.cos[pos, None, :])
        want, _, _ = er.extend_f64(P.seq[i][past:], k_all[:past], v_all[:past], n_heads, n_kv, op.sin, op.cos)
        err, c = float(np.max(np.abs(got - want))), cosine(got, want)
        print(f"{name} {n_heads}/{n_kv} f16={f16} segment {i} past={past} len={n} row0={r0}: max|diff| {err:.3e} cosine {c:.8f}")
        assert err <= 6e-3, (i, err)
        assert c >= 0.9999, (i, c)
        # ---- the existing operator on this segment alone, on a copy of the same caches ----
        op.kc, op.vc = before[i][0].clone(), before[i][1].clone()
        base = op.extend(P.seq[i][past:], past).reshape(n, n_heads, D)
        d = float(np.max(np.abs(got - base)))
        print(f"    vs attention_extend_dev alone: max|diff| {d:.3e} of max|base| {np.max(np.abs(base)):.3f}")
        assert d <= 2e-4 * np.max(np.abs(base)), (i, d)
        assert t.equal(dev_bits(t, op.kc), dev_bits(t, c1[i][0])) and t.equal(dev_bits(t, op.vc), dev_bits(t, c1[i][1])), f"segment {i}: cache differs from the solo operator's"
        # ---- slots outside [past, past + n) keep their bits (NaNs beyond, the past below) ----
        k0, v0 = P.decode(before[i])
        k1, v1 = P.decode(c1[i])
        assert same_bits(k1[:past], k0[:past]) and same_bits(v1[:past], v0[:past])
        assert same_bits(k1[T:], k0[T:]) and same_bits(v1[T:], v0[T:])
        assert np.isfinite(k1[past:T].astype(np.float32)).all() and np.isfinite(v1[past:T].astype(np.float32)).all()
    # ---- repeatability: the same call on the same caches gives the same bytes ----
    c2 = P.snapshot()
    out2 = P.call(qkv, c2)
    assert same_bits(out2, out1)
    for a, b in zip(c1, c2):
        assert t.equal(dev_bits(t, a[0]), dev_bits(t, b[0])) and t.equal(dev_bits(t, a[1]), dev_bits(t, b[1]))
    # ---- isolation: one segment's rows AND its past replaced by other data; nobody else may notice ----
    if len(segs) > 1:
        j = 1
        past_j, n_j = segs[j]
        other = list(P.seq)
        other[j] = P.rng.normal(0, 3.0, P.seq[j].shape).astype(np.float32)
        P.fill_past(P.ops[j], other[j], past_j, chain=False)
        c3 = P.snapshot()
        c3[j] = (P.ops[j].kc.clone(), P.ops[j].vc.clone())
        for i in range(len(segs)):
            if i != j:
                c3[i] = (before[i][0].clone(), before[i][1].clone())
        out3 = P.call(P.rows(other), c3)
        changed = False
        for i, ((past, n), r0) in enumerate(zip(segs, P.row0)):
            if i == j:
                changed = not same_bits(out3[r0:r0 + n], out1[r0:r0 + n])
                continue
            assert same_bits(out3[r0:r0 + n], out1[r0:r0 + n]), f"segment {i}'s output changed with segment {j}'s data"
            assert t.equal(dev_bits(t, c3[i][0]), dev_bits(t, c1[i][0])) and t.equal(dev_bits(t, c3[i][1]), dev_bits(t, c1[i][1])), f"segment {i}'s cache changed"
        assert changed, "the replaced segment itself must change (the check would be vacuous otherwise)"


@pytest.mark.parametrize("heads", [(4, 2), (3, 3)], ids=lambda h: f"{h[0]}x{h[1]}")
def test_f16_output_rows_and_unaligned_rows(hip, oracle, torch_, heads):
    """BITNET_HIP_ATTN_OUT_F16: the f32 rows rounded once (as test_f16_output_rows_and_a_reused_workspace checks for extend); and rows that
    are not 16-byte aligned take the query-prep launch: the same arithmetic, so the segments' rows agree within the operator's own 2e-4"""
    n_heads, n_kv = heads
    for f16 in (False, True):
        P = Pack(hip, oracle, torch_, n_heads, n_kv, f16, SETS["four_live"], seed=77)
        qkv = P.rows()
        a = P.call(qkv, P.snapshot())
        b = P.call(qkv, P.snapshot(), out_f16=True)
        m = P.call(qkv, P.snapshot(), misalign=True)
        assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(m).all()
        live = ~P.padding_rows()
        half_ulp = 0.5 * np.spacing(np.abs(a[live]).astype(np.float16)).astype(np.float64)
        assert np.all(np.abs(b[live].astype(np.float64) - a[live]) <= half_ulp + 2.0 ** -23 * np.abs(a[live]))
        d = float(np.max(np.abs(m[live] - a[live])))
        print(f"{n_heads}/{n_kv} f16={f16}: unaligned rows vs aligned max|diff| {d:.3e} of {np.max(np.abs(a[live])):.3f}")
        assert d <= 2e-4 * np.max(np.abs(a[live]))
