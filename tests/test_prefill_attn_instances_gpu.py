"""Every path through prefill_attn_body (kernels_prefill_attn.hip), by value, against the float64 model tests/attn_ref.py.

One flash-attention body serves the whole-prompt forward, the continuation (extend), the packed forward, the token-parallel (sharded)
prefill and the host drop-in; it is instantiated for HW = 4 / 2 / 1 query heads per workgroup, plain and packed.  Every case here compares
ALL output rows with attn_ref.exact() on the f16 operands the kernel makes, element by element under attn_ref.tol()
(2^-10 sum_j p_j |v_jd| + 2^-20 max|v|, + half an f16 ulp for f16 rows), on the input families of attn_ref.family(): inputs that move the
running reference point in every key tile, let it go stale, put the mass on the last visible keys, sink every real score below a padded
key's, or make the answer one exact row of v.  Output buffers are NaN-prefilled and must come back finite; every case prints max(err/tol)
on a line that starts with ATTN.

Head shapes: (4, 1), (8, 2) -> HW 4; (4, 2) -> HW 2; (6, 1) -> HW 2 with three head groups per KV head; (3, 3) -> HW 1; (5, 1) -> HW 1,
group of 5.  The key split (ksplit > 1, the surplus-part marks, k_prefill_merge, extend's bound on the partials) is reached at these
sizes in a child process with BITNET_HIP_ATTN_SPLIT_TILES=1; a second child with BITNET_HIP_ATTN_HEAD_FAST=0 must reproduce the parent's
bits.  Past keys of a continuation are read back from the cache (the layouts tests/kv_read.py decodes, through tests/extend_ref.py)."""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_ref as ar  # noqa: E402
import extend_ref as er  # noqa: E402
from kv_read import bits  # noqa: E402

pytestmark = pytest.mark.gpu

D = 128
CACHE_F16, OUT_F16 = 1, 2
MAX_POS = 512
HEADS = [(4, 1), (8, 2), (4, 2), (6, 1), (3, 3), (5, 1)]
EXTENDS = [(1, 129), (63, 2), (64, 66), (37, 93), (100, 100)]
SPLIT_FAMILIES = ("gauss", "ramp12", "steep", "needle", "sunk")
hid = lambda h: f"{h[0]}x{h[1]}"  # noqa: E731


class Rig:
    """the library, the RoPE tables on both sides, and one call per entry point (pytest fixture and child processes alike)"""

    def __init__(self, hip, oracle, torch):
        self.hip, self.oracle, self.t = hip, oracle, torch
        sin, cos = oracle.rope_tables(D, MAX_POS, 10000.0)
        self.sin, self.cos = sin.reshape(MAX_POS, D // 2), cos.reshape(MAX_POS, D // 2)
        self.sin_d, self.cos_d = self.dev(sin), self.dev(cos)

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

    def rows(self, a, misalign=False):
        """-> (the tensor that owns the rows, their device pointer); misalign: 4 bytes off a 16-byte boundary (the f16 query image path)"""
        if not misalign:
            buf = self.dev(a)
            return buf, buf.data_ptr()
        buf = self.t.zeros(a.size + 1, dtype=self.t.float32, device="cuda")
        buf[1:] = self.dev(a).ravel()
        return buf, buf.data_ptr() + 4

    def caches(self, n_kv, f16):
        dt = self.t.float16 if f16 else self.t.float32
        n = n_kv * er.chunks(MAX_POS) * 64 * D
        return self.t.zeros(n, dtype=dt, device="cuda"), self.t.zeros(n, dtype=dt, device="cuda")

    def read(self, kc, vc, n_kv, f16):
        """-> (k [slots, kv, D], v [slots, kv, D]) in the cache's own dtype"""
        return er.decode_k(kc.cpu().numpy(), n_kv, MAX_POS, f16), er.decode_v(vc.cpu().numpy(), n_kv, MAX_POS, f16)

    def out(self, n, n_heads, flags):
        return self.t.full((n, n_heads * D), float("nan"), dtype=self.t.float16 if flags & OUT_F16 else self.t.float32, device="cuda")

    def ws(self, nbytes):
        assert nbytes > 0
        return self.t.full((nbytes,), 0xFF, dtype=self.t.uint8, device="cuda")  # NaN patterns: nothing the call did not write may be read

    def fresh(self, qkv, n_heads, n_kv, flags, kc, vc, misalign=False, reps=1):
        T = qkv.shape[0]
        keep, ptr = self.rows(qkv, misalign)
        wsb = self.hip.attention_prefill_workspace_bytes(n_heads, n_kv, T)
        ws = self.ws(wsb)
        for _ in range(reps):  # a repeat runs on the workspace the call before left
            out = self.out(T, n_heads, flags)
            self.hip.attention_prefill_flags_dev(ptr, self.sin_d, self.cos_d, kc, vc, n_heads, n_kv, D, MAX_POS, T, ws, wsb, out, flags)
            self.t.cuda.synchronize()
        return out.cpu().numpy().reshape(T, n_heads, D)

    def extend(self, qkv_new, past, n_heads, n_kv, flags, kc, vc, misalign=False, reps=1):
        n = qkv_new.shape[0]
        keep, ptr = self.rows(qkv_new, misalign)
        wsb = self.hip.attention_extend_workspace_bytes(n_heads, n_kv, past, n)
        ws = self.ws(wsb)
        for _ in range(reps):  # (a repeat rewrites the new slots with the same values)
            out = self.out(n, n_heads, flags)
            self.hip.attention_extend_dev(ptr, self.sin_d, self.cos_d, kc, vc, n_heads, n_kv, D, MAX_POS, past, n, ws, wsb, out, flags)
            self.t.cuda.synchronize()
        return out.cpu().numpy().reshape(n, n_heads, D)

    def sharded(self, q_local, block_pos, kv_all, n_heads, n_kv, reps=1):
        nq, T = q_local.shape[0], kv_all.shape[0]
        kc, vc = self.caches(n_kv, False)
        wsb = self.hip.attention_prefill_sharded_workspace_bytes(n_heads, n_kv, nq, T)
        ws = self.ws(wsb)
        q_d, kv_d = self.dev(q_local), self.dev(kv_all)
        bp = self.t.from_numpy(np.asarray(block_pos, np.int32)).cuda()
        for _ in range(reps):
            out = self.out(nq, n_heads, 0)
            self.hip.attention_prefill_sharded_dev(q_d, n_heads * D, bp, nq, kv_d, 2 * n_kv * D, T, self.sin_d, self.cos_d, kc, vc, n_heads, n_kv, D,
                                                   MAX_POS, ws, wsb, out)
            self.t.cuda.synchronize()
        return out.cpu().numpy().reshape(nq, n_heads, D)


@pytest.fixture(scope="module")
def rig(hip, oracle):
    import torch

    return Rig(hip, oracle, torch)


# ---- inputs, the model, the comparison -----------------------------------------------------------------------------------------
def inputs(sin, cos, name, tag, pos_q, T, n_heads, n_kv, causal=True, rope=True):
    """one family -> f32 inputs q [n, heads, D], k [T, kv, D], v [T, kv, D] and the needle's targets (seeded by the case's name alone)"""
    rng = np.random.default_rng(ar.seed_of(name, tag, n_heads, n_kv, T))
    q1, k1, v, t = ar.family(name, rng, pos_q, T, n_heads, n_kv, causal)
    if not rope:
        return q1.astype(np.float32), k1.astype(np.float32), v.astype(np.float32), t
    return ar.unrope(q1, pos_q, sin, cos), ar.unrope(k1, np.arange(T), sin, cos), v.astype(np.float32), t


def qkv_rows(q_in, k_in, v_in, past, seed):
    """[T, (heads + 2 kv) * D] rows of a sequence whose queries exist for the positions past .. T - 1 only (earlier query rows: noise)"""
    T, n = k_in.shape[0], q_in.shape[0]
    q = np.random.default_rng(seed).normal(0, 1.5, (T, q_in.shape[1] * D)).astype(np.float32)
    q[past:] = q_in.reshape(n, -1)
    return np.concatenate([q, k_in.reshape(T, -1), v_in.reshape(T, -1)], axis=1)


STRICT = True  # a child process prints every case's line and leaves the verdict on the figures to its parent


def check(got, qh, kh, vh, pos_q, name, t, label, causal=True, out_f16=False):
    """all rows of all heads under the tolerance; the family's own condition from the model; -> max(err/tol)"""
    want, tl, p = ar.model(qh, kh, vh, pos_q, causal, out_f16)
    n, n_heads = qh.shape[:2]
    if name != "needle":
        s = ar.scores(qh, kh, pos_q, causal)
        assert np.max(np.abs(s)) <= 128.0, (label, np.max(np.abs(s)))
    else:
        for h in range(n_heads):
            assert np.min(p[h][np.arange(n), t[:, h]]) >= 1.0 - 2.0 ** -20, label
    assert got.shape == want.shape
    g = got.astype(np.float64)
    assert np.isfinite(g).all(), f"{label}: a row the call did not write, or a NaN / inf it computed"
    ratio = float(np.max(np.abs(g - want) / tl))
    print(f"ATTN {label} family={name}: max(err/tol) {ratio:.3f}")
    assert ratio <= 1.0 or not STRICT, (label, name, ratio)
    if name == "needle":  # the answer is one row of v (on a 1/64 grid: exact in f16), to the floor term alone
        group = n_heads // kh.shape[1]
        for h in range(n_heads):
            d = np.abs(g[:, h] - vh[t[:, h], h // group])
            assert np.all(d <= 2.0 ** -20 * np.max(np.abs(vh[:, h // group]))), (label, h, float(d.max()))
    return ratio


def run_fresh(rig, heads, T, name, flags, misalign=False, reps=1, tag="fresh"):
    n_heads, n_kv = heads
    pos = np.arange(T)
    q_in, k_in, v_in, t = inputs(rig.sin, rig.cos, name, "fresh", pos, T, n_heads, n_kv)
    kc, vc = rig.caches(n_kv, flags & CACHE_F16)
    got = rig.fresh(qkv_rows(q_in, k_in, v_in, 0, 0), n_heads, n_kv, flags, kc, vc, misalign, reps)
    qh, kh, vh = ar.operands_q(q_in, pos, rig.sin, rig.cos), ar.operands_k(k_in, pos, rig.sin, rig.cos), ar.operands_v(v_in)
    r = check(got, qh, kh, vh, pos, name, t, f"path={tag} heads={hid(heads)} T={T} flags={flags}", out_f16=bool(flags & OUT_F16))
    return r, got, (kc, vc)


def run_extend(rig, heads, past, n, name, flags, fill="prefill", misalign=False, reps=1, tag="extend"):
    n_heads, n_kv = heads
    T, f16c = past + n, flags & CACHE_F16
    pos = np.arange(T)
    q_in, k_in, v_in, t = inputs(rig.sin, rig.cos, name, "extend", pos[past:], T, n_heads, n_kv)
    qkv = qkv_rows(q_in, k_in, v_in, past, seed=past)
    kc, vc = rig.caches(n_kv, f16c)
    # ---- the past: one whole-prompt call, or two continuations from an empty cache ----
    if fill == "prefill":
        rig.fresh(qkv[:past], n_heads, n_kv, f16c, kc, vc)
    else:
        cut = past // 2
        if cut:
            rig.extend(qkv[:cut], 0, n_heads, n_kv, f16c, kc, vc)
        rig.extend(qkv[cut:past], cut, n_heads, n_kv, f16c, kc, vc)
    k_c, v_c = rig.read(kc, vc, n_kv, f16c)
    got = rig.extend(qkv[past:], past, n_heads, n_kv, flags, kc, vc, misalign, reps)
    # past operands from the cache's values (exact f32 -> one f16 rounding; f16 as they are), new ones from the model
    kh = np.concatenate([ar.f16(k_c[:past]), ar.operands_k(k_in[past:], pos[past:], rig.sin, rig.cos)])
    vh = np.concatenate([ar.f16(v_c[:past]), ar.operands_v(v_in[past:])])
    qh = ar.operands_q(q_in, pos[past:], rig.sin, rig.cos)
    r = check(got, qh, kh, vh, pos[past:], name, t, f"path={tag} heads={hid(heads)} past={past} new={n} flags={flags} fill={fill}", out_f16=bool(flags & OUT_F16))
    return r, got, (kc, vc)


SHARD_T, SHARD_BLOCKS = 256, (3, 0)  # query blocks at non-adjacent, non-increasing positions of a 256-key context


def run_sharded(rig, heads, name, reps=1, tag="sharded"):
    n_heads, n_kv = heads
    T = SHARD_T
    pos_q = np.concatenate([np.arange(64 * b, 64 * b + 64) for b in SHARD_BLOCKS])
    q_in, k_in, v_in, t = inputs(rig.sin, rig.cos, name, "sharded", pos_q, T, n_heads, n_kv)
    kv_all = np.concatenate([k_in.reshape(T, -1), v_in.reshape(T, -1)], axis=1)
    got = rig.sharded(q_in.reshape(len(pos_q), -1), [64 * b for b in SHARD_BLOCKS], kv_all, n_heads, n_kv, reps)
    pos = np.arange(T)
    qh, kh, vh = ar.operands_q(q_in, pos_q, rig.sin, rig.cos), ar.operands_k(k_in, pos, rig.sin, rig.cos), ar.operands_v(v_in)
    return check(got, qh, kh, vh, pos_q, name, t, f"path={tag} heads={hid(heads)} T={T} blocks={SHARD_BLOCKS}")


# ---- the fresh prompt ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 200])
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_fresh_prompt_every_instance(rig, heads, T):
    """attention_prefill_flags_dev, f32 and f16 caches: one row, one row short of a tile, a tile, one row more; 130 / 200 rows (3 / 4 key
    tiles, the last partly padding, two query blocks at HW 1) on every family"""
    for name in (ar.FAMILIES if T >= 130 else ("gauss", "needle")):
        for flags in (0, CACHE_F16):
            run_fresh(rig, heads, T, name, flags)


# ---- the continuation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past,n", EXTENDS)
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_extend_every_instance(rig, heads, past, n):
    """attention_extend_dev over a past left by a whole-prompt call or by two continuations; flag words 0, f16 caches, f16 output rows"""
    for i, name in enumerate(("ramp12", "steep", "needle", "sunk")):
        for flags in (0, CACHE_F16, OUT_F16):
            run_extend(rig, heads, past, n, name, flags, fill="prefill" if (i + past) % 2 == 0 else "chain")


# ---- the packed forward --------------------------------------------------------------------------------------------------------
PACK_SEGS = [(0, 70), (37, 30), (64, 1)]
PACK_FAMILIES = [("ramp12", "needle", "sunk"), ("steep", "ramp6", "needle")]


def run_packed(rig, heads, f16c, fams, misalign=False):
    """-> (caches after the call, ratios).  The helper of tests/test_attention_packed_gpu.py (row layout in a shuffled order, NaN padding rows,
    NaNs in every cache slot beyond a segment's past, guard bytes around the workspace) on this module's inputs."""
    from test_attention_packed_gpu import Pack

    n_heads, n_kv = heads
    P = Pack(rig.hip, rig.oracle, rig.t, n_heads, n_kv, bool(f16c), PACK_SEGS, seed=5)
    info = []
    for i, ((past, n), name) in enumerate(zip(PACK_SEGS, fams)):
        T = past + n
        pos = np.arange(T)
        op = P.ops[i]
        q_in, k_in, v_in, t = inputs(op.sin, op.cos, name, f"packed{i}", pos[past:], T, n_heads, n_kv)
        P.seq[i] = qkv_rows(q_in, k_in, v_in, past, seed=i)
        P.fill_past(op, P.seq[i], past, chain=i % 2 == 1)
        info.append((q_in, k_in, v_in, t))
    caches = P.snapshot()
    before = [P.decode(c) for c in caches]
    out = P.call(P.rows(), caches, misalign=misalign)
    assert np.isfinite(out).all(), "padding rows must be finite too"
    ratios = []
    for i, ((past, n), name, r0) in enumerate(zip(PACK_SEGS, fams, P.row0)):
        q_in, k_in, v_in, t = info[i]
        op, pos = P.ops[i], np.arange(past + n)
        k_c, v_c = before[i]
        kh = np.concatenate([ar.f16(k_c[:past]), ar.operands_k(k_in[past:], pos[past:], op.sin, op.cos)])
        vh = np.concatenate([ar.f16(v_c[:past]), ar.operands_v(v_in[past:])])
        qh = ar.operands_q(q_in, pos[past:], op.sin, op.cos)
        got = out[r0:r0 + n].reshape(n, n_heads, D)
        ratios.append(check(got, qh, kh, vh, pos[past:], name, t,
                            f"path=packed{'-misaligned' if misalign else ''} heads={hid(heads)} seg={i} past={past} len={n} row0={r0} cache_f16={int(bool(f16c))}"))
    return caches, ratios


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_packed_every_instance(rig, heads):
    """attention_packed_dev: three segments (fresh, mid-tile past, whole-tile past with ONE new row), each on a different family, on even
    head groups (row alignment 64) and odd ones (128)"""
    assert rig.hip.attention_packed_row_align(*heads) == (128 if (heads[0] // heads[1]) % 2 else 64)
    for fams in PACK_FAMILIES:
        for f16c in (0, 1):
            run_packed(rig, heads, f16c, fams)


# ---- the token-parallel prefill ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_sharded_blocks_out_of_order(rig, heads):
    """attention_prefill_sharded_dev: the query blocks at positions 192 and 0 of a 256-key context (at HW 1 both in ONE workgroup)"""
    for name in ("ramp12", "needle"):
        run_sharded(rig, heads, name)


# ---- the host drop-in ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_host_dropin(rig, causal):
    """bitnet_hip_attention on [batch, heads, seq, 128] tensors: no RoPE, one KV head per head (HW 1), with and without the mask"""
    heads, seq, batch = 3, 130, 2
    scale = float(ar.SCALE_F32)
    pos = np.arange(seq)
    for name in ("sunk", "gauss", "needle"):
        ins = [inputs(None, None, name, f"host{b}{causal}", pos, seq, heads, heads, causal, rope=False) for b in range(batch)]
        q, k, v = (np.stack([x[i].transpose(1, 0, 2) for x in ins]) for i in range(3))
        got = rig.hip.attention(q, k, v, seq, heads, D, causal=causal, scale=scale).reshape(batch, heads, seq, D)
        for b, (q_in, k_in, v_in, t) in enumerate(ins):
            qh, kh, vh = ar.operands_q(q_in, pos, None, None, ar.qmul_of(scale)), ar.operands_k(k_in, pos, None, None), ar.operands_v(v_in)
            check(got[b].transpose(1, 0, 2), qh, kh, vh, pos, name, t, f"path=host heads={heads} seq={seq} causal={int(causal)} batch={b}", causal=causal)


# ---- rows that are not 16-byte aligned: the f16 query image ------------------------------------------------------------------------
def same_bits(a, b):
    return all(np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())) for x, y in zip(a, b))


@pytest.mark.parametrize("heads", [(8, 2), (4, 2), (3, 3)], ids=hid)
def test_misaligned_rows(rig, heads):
    """buffers 4 bytes off a 16-byte boundary: the query image comes from the prep launches instead of the attention kernel's own f32 reads,
    the k | v rows are read element by element; the same tolerance, and the caches of the aligned call bit for bit"""
    for flags in (0, CACHE_F16):
        _, _, c0 = run_fresh(rig, heads, 130, "ramp12", flags)
        _, _, c1 = run_fresh(rig, heads, 130, "ramp12", flags, misalign=True, tag="fresh-misaligned")
        assert same_bits(c0, c1)
        _, _, c0 = run_extend(rig, heads, 37, 93, "ramp12", flags)
        _, _, c1 = run_extend(rig, heads, 37, 93, "ramp12", flags, misalign=True, tag="extend-misaligned")
        assert same_bits(c0, c1)
        p0, _ = run_packed(rig, heads, flags, ("ramp12", "ramp12", "ramp12"))
        p1, _ = run_packed(rig, heads, flags, ("ramp12", "ramp12", "ramp12"), misalign=True)
        for a, b in zip(p0, p1):
            assert same_bits(a, b)


# ---- child processes: switches the library reads once ------------------------------------------------------------------------------
def split_cases(rig):
    """child A: with BITNET_HIP_ATTN_SPLIT_TILES=1 every launch below is key-split (one tile per part, up to 8 parts); each call runs twice
    on a workspace that started as 0xFF bytes.  T <= 512: 8 tiles, no part is left with an empty tile range."""
    print(f"WS {rig.hip.attention_prefill_workspace_bytes(4, 1, 130)}")
    for heads in HEADS:
        for name in SPLIT_FAMILIES:
            for T in (130, 200, 512):
                run_fresh(rig, heads, T, name, 0, reps=2, tag="split-fresh")
            for i, (past, n) in enumerate(((37, 163), (100, 300))):
                run_extend(rig, heads, past, n, name, (0, CACHE_F16)[i], reps=2, tag="split-extend")
            run_sharded(rig, heads, name, reps=2, tag="split-sharded")


def fresh_digests(rig):
    """sha256 of the output bits of the fresh T = 200 cases"""
    dig = {}
    for heads in HEADS:
        for name in ar.FAMILIES:
            _, got, _ = run_fresh(rig, heads, 200, name, 0, tag="head-order")
            dig[f"{hid(heads)}/{name}"] = hashlib.sha256(np.ascontiguousarray(got, np.float32).tobytes()).hexdigest()
    return dig


def child(mode, **env):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout.splitlines()


def test_key_split_at_small_sizes(rig):
    """ksplit > 1, parts / per, the surplus-part marks, k_prefill_merge and extend's AttnPartials::kBound layout at 3- to 8-tile prompts"""
    lines = child("split", BITNET_HIP_ATTN_SPLIT_TILES="1")
    ws = [int(l.split()[1]) for l in lines if l.startswith("WS ")]
    assert ws and ws[0] > rig.hip.attention_prefill_workspace_bytes(4, 1, 130), "the child did not reserve partials: the switch was not read"
    ratios = [(l, float(l.rsplit(" ", 1)[1])) for l in lines if l.startswith("ATTN ")]
    for l, _ in ratios:
        print(l)
    assert len(ratios) == len(HEADS) * len(SPLIT_FAMILIES) * 6
    assert all(r <= 1.0 for _, r in ratios)


def test_head_order_switch_changes_no_bit(rig):
    """BITNET_HIP_ATTN_HEAD_FAST=0 only changes which workgroup runs where (EXPERIMENTS.md): the fresh T = 200 outputs keep their bits"""
    mine = fresh_digests(rig)
    lines = child("head_order", BITNET_HIP_ATTN_HEAD_FAST="0")
    theirs = dict(l.split()[1:3] for l in lines if l.startswith("HASH "))
    assert theirs.keys() == mine.keys()
    assert theirs == mine


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    lib = importlib.import_module("bitnet-rs_amd").load()
    lib.init(0)
    from oracle import oracle as orc

    orc.build()
    r = Rig(lib, orc, torch)
    if sys.argv[1] == "split":
        STRICT = False
        split_cases(r)
    else:
        for key, h in fresh_digests(r).items():
            print(f"HASH {key} {h}")
