#!/usr/bin/env python3
"""Does a libbitnet_hip.so size and launch the prompt attention the way another one does?  The check for a change of the launch layer in
csrc/kernels_prefill_attn.hip that leaves the kernels alone (tools/isa_equal.py proves that half):
    python tools/attn_launch_compare.py sizes [LIB]   the five size / alignment functions over a grid (CPU only)
    python tools/attn_launch_compare.py calls [LIB]   one small call through every prompt attention entry (GPU): a SHA-256 per output and cache
LIB defaults to this tree's library; build the other revision's in a worktree, run both, and diff the two outputs: they must be equal line
for line (the kernels are deterministic).  `calls` under `rocprofv3 --kernel-trace` gives the dispatch list to compare as well."""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
D = 128
HEADS = [(4, 2), (3, 3), (6, 3), (8, 2), (20, 5)]
LENGTHS = [1, 63, 64, 65, 128, 1023, 1024, 1025, 4096, 8192]


def sizes(hip):
    for h, k in HEADS + [(5, 2), (0, 1), (4, 0)]:  # the last three: refused, 0
        print(f"row_align {h}/{k}: {hip.attention_packed_row_align(h, k)}")
    for h, k in HEADS:
        for n in LENGTHS:
            print(f"prefill {h}/{k} T={n}: {hip.attention_prefill_workspace_bytes(h, k, n)}")
            for m in LENGTHS:  # n queries over m keys | past m, n new tokens
                print(f"sharded {h}/{k} nq={n} ctx={m}: {hip.attention_prefill_sharded_workspace_bytes(h, k, n, m)}"
                      f"  extend past={m} n={n}: {hip.attention_extend_workspace_bytes(h, k, m, n)}")
            print(f"extend {h}/{k} past=0 n={n}: {hip.attention_extend_workspace_bytes(h, k, 0, n)}")
        for n_seq in (1, 2, 64):
            for past in LENGTHS:
                for ln in LENGTHS:
                    pa, la = [(past * (s + 1)) % 8193 for s in range(n_seq)], [1 + (ln + 7 * s) % 8192 for s in range(n_seq)]
                    rows = sum((x + 127) // 128 * 128 for x in la) + 3
                    print(f"packed {h}/{k} x{n_seq} past0={past} len0={ln}: {hip.attention_packed_workspace_bytes(h, k, rows, pa, la)}")
    for args in ((5, 2, 0, 8), (4, 2, 8, 0), (4, 2, 1 << 30, 8), (0, 2, 0, 8), (4, 0, 0, 8)):
        print(f"extend refused {args}: {hip.attention_extend_workspace_bytes(*args)}")
    for args in ((5, 2, 64, [0], [8]), (4, 2, 64, [0], [0]), (4, 2, 0, [0], [8]), (4, 2, 64, [-1], [8]), (4, 2, 64, [1 << 24], [8]), (4, 2, 1 << 24, [0], [8]),
                 (4, 2, 64, [0] * 65, [1] * 65), (4, 2, 1 << 23, [(1 << 24) - 70] * 2, [64] * 2)):
        print(f"packed refused {args[:3]} x{len(args[3])}: {hip.attention_packed_workspace_bytes(*args)}")


def calls(hip):
    import torch as t
    from oracle import oracle as orc
    from test_attention_packed_gpu import SETS, Pack
    from test_extend_gpu import Op

    hip.init(0)
    vp, sz = C.c_void_p, C.c_size_t
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a)).cuda()
    sha = lambda x: hashlib.sha256((x.cpu().numpy() if hasattr(x, "cpu") else np.ascontiguousarray(x)).tobytes()).hexdigest()[:32]

    def report(name, out, *caches):
        t.cuda.synchronize()
        print(f"{name}: out {sha(out)}" + "".join(f" cache{i} {sha(c)}" for i, c in enumerate(caches)), flush=True)

    def setup(T, h, k, max_pos, f16, seed, nq=None):
        rng = np.random.default_rng(seed)
        qkv = rng.normal(0, 1.3, (T, (h + 2 * k) * D)).astype(np.float32)
        sin, cos = orc.rope_tables(D, max_pos, 10000.0)
        dt = t.float16 if f16 else t.float32
        kc, vc = t.zeros(k * max_pos * D, dtype=dt, device="cuda"), t.zeros(k * max_pos * D, dtype=dt, device="cuda")
        wsb = hip.attention_prefill_sharded_workspace_bytes(h, k, nq or T, T)
        ws = t.full((wsb,), 0xFF, dtype=t.uint8, device="cuda")
        return qkv, dev(sin), dev(cos), kc, vc, ws, wsb

    # ---- the whole-prompt entries; T = 2200 x 8/8 is key-split ----
    for T, h, k, max_pos in ((70, 4, 2, 512), (130, 3, 3, 512), (2200, 8, 8, 4096)):
        qkv, sin, cos, kc, vc, ws, wsb = setup(T, h, k, max_pos, False, T)
        out = t.full((T, h * D), float("nan"), device="cuda")
        hip.attention_prefill_dev(dev(qkv), sin, cos, kc, vc, h, k, D, max_pos, T, ws, wsb, out)
        report(f"prefill_dev T={T} {h}/{k}", out, kc, vc)
        qkv, sin, cos, kc, vc, ws, wsb = setup(T, h, k, max_pos, True, T)
        f = hip.c.bitnet_hip_attention_prefill_kv16_dev
        f.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, sz, vp, sz, vp, vp]
        hip._check(f(dev(qkv).data_ptr(), sin.data_ptr(), cos.data_ptr(), kc.data_ptr(), vc.data_ptr(), h, k, D, max_pos, T, ws.data_ptr(), wsb, out.data_ptr(), None))
        report(f"prefill_kv16_dev T={T} {h}/{k}", out, kc, vc)
        for mis in (0, 1):
            buf = t.zeros(qkv.size + 1, device="cuda")
            buf[mis:][:qkv.size] = dev(qkv).ravel()
            o16 = t.full((T, h * D), float("nan"), dtype=t.float16, device="cuda")
            hip.attention_prefill_flags_dev(buf.data_ptr() + 4 * mis, sin, cos, kc, vc, h, k, D, max_pos, T, ws, wsb, o16, 1 | 2)
            report(f"prefill_flags_dev OUT_F16 T={T} {h}/{k} misalign={mis}", o16, kc, vc)
    # ---- query rows of one rank over the whole context: sharded (absolute order), gathered (zigzag) in one phase and in two ----
    h, k, T, world, max_pos = 4, 2, 512, 2, 512
    chunk, nq = T // (2 * world), T // world
    rows_of = lambda r: np.concatenate([np.arange(r * chunk, (r + 1) * chunk), np.arange((2 * world - 1 - r) * chunk, (2 * world - r) * chunk)])
    qkv, sin, cos, kc, vc, ws, wsb = setup(T, h, k, max_pos, False, 5, nq)
    rows = rows_of(1)
    q_local, bp = dev(qkv[rows][:, :h * D]), dev(rows[::64].astype(np.int32))
    out = t.full((nq, h * D), float("nan"), device="cuda")
    hip.attention_prefill_sharded_dev(q_local, h * D, bp, nq, dev(qkv[:, h * D:]), 2 * k * D, T, sin, cos, kc, vc, h, k, D, max_pos, ws, wsb, out)
    report("prefill_sharded_dev", out, kc, vc)
    kv = qkv[:, h * D:][np.concatenate([rows_of(r) for r in range(world)])]
    f = hip.c.bitnet_hip_attention_prefill_gathered_phase_dev
    f.argtypes = [vp, sz, vp, sz, vp, sz, sz, C.c_int, vp, vp, vp, vp, C.c_int, sz, sz, sz, sz, vp, sz, vp, C.c_int, vp]
    for wire_f16, phases in ((0, (0,)), (1, (1, 2))):
        kv_d = dev(kv.astype(np.float16) if wire_f16 else kv)
        kc.zero_(), vc.zero_(), out.fill_(float("nan")), ws.fill_(0xFF)
        for ph in phases:
            hip._check(f(q_local.data_ptr(), h * D, bp.data_ptr(), nq, kv_d.data_ptr(), T, world, wire_f16, sin.data_ptr(), cos.data_ptr(), kc.data_ptr(),
                         vc.data_ptr(), 0, h, k, D, max_pos, ws.data_ptr(), wsb, out.data_ptr(), ph, None))
        report(f"prefill_gathered_phase_dev world 2 wire_f16={wire_f16} phases {phases}", out, kc, vc)
    # ---- a live sequence, and four of them packed ----
    for past, n, h, k in ((37, 70, 4, 2), (64, 65, 3, 3), (1100, 70, 4, 2)):  # the last: key-split
        for f16 in (False, True):
            qkv = np.random.default_rng(past).normal(0, 1.3, (past + n, (h + 2 * k) * D)).astype(np.float32)
            for mis in (False, True):
                op = Op(hip, orc, t, h, k, 512 if past + n <= 512 else 2048, f16)
                op.prefill(qkv[:past])
                report(f"extend_dev past={past} n={n} {h}/{k} f16={f16} misalign={mis}", op.extend(qkv[past:], past, misalign=mis), op.kc, op.vc)
    for h, k in ((4, 2), (3, 3), (8, 2)):
        for f16 in (False, True):
            P = Pack(hip, orc, t, h, k, f16, SETS["four_live"], seed=77)
            for mis in (False, True):
                snap = P.snapshot()
                out = P.call(P.rows(), snap, misalign=mis)
                report(f"packed_dev four_live {h}/{k} f16={f16} misalign={mis}", out, *[c for pair in snap for c in pair])
    # ---- the host entry ----
    rng = np.random.default_rng(3)
    q, kk, v = (rng.normal(0, 1.2, (2, 3, 70, D)).astype(np.float32) for _ in range(3))
    for causal in (True, False):
        print(f"attention host causal={causal}: out {sha(hip.attention(q, kk, v, 70, 3, D, causal=causal, scale=0.11))}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("sizes", "calls"):
        sys.exit(__doc__)
    import torch  # noqa: F401  (ahead of the library: bitnet-rs_amd.load())

    pkg = importlib.import_module("bitnet-rs_amd")
    {"sizes": sizes, "calls": calls}[sys.argv[1]](pkg.HipLib(sys.argv[2]) if len(sys.argv) > 2 else pkg.HipLib())
