#!/usr/bin/env python3
"""Does a libbitnet_hip.so refuse and launch the decode step's operators the way another one does?  The check for a change of the decode launch
layer (gemv_geometry / fill_gemv_q_prefix / the pickers in csrc/kernels_{mfma,gemvq,batch,attn,decode}.hip, the entry fronts in csrc/abi.hip)
that leaves the kernels alone (tools/isa_equal.py proves that half):
    python tools/decode_launch_compare.py refusals [LIB]   every refusal of the QAct GEMV, merge, decode attention and logits entries: one fault
                                                            at a time, then the multi-fault cases that pin each entry's precedence; prints
                                                            entry | case | rc | message.  The cases that need a weights handle run only with a GPU.
    python tools/decode_launch_compare.py calls [LIB]      one small call per kernel instance reachable through those entries (GPU), fixed seeds:
                                                            a SHA-256 per output buffer
LIB defaults to this tree's library; build the other revision's in a worktree and diff the two outputs: they must be equal line for line (the
kernels are deterministic).  Each library runs in a process of its own under a time limit of its own, chained so that the first non-zero status
ends the sitting -- a refusal is a line, anything else (a GPU error, a fault, a timeout) ends the process non-zero and nothing more may start:
    timeout -k 10 420 python tools/decode_launch_compare.py calls OTHER.so > a.txt && timeout -k 10 420 python tools/decode_launch_compare.py calls > b.txt && diff a.txt b.txt
`calls` once more per library under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python ...` (nothing else collected in that run) gives
the dispatch lists to compare in kernel name, grid, workgroup size and LDS_Block_Size."""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
D = 128
SILU = 1  # BITNET_HIP_FUSE_SILU_MUL
KINDS = ("qk256", "f32", "f16")  # no scales | 32-block scales that are no f16 values | that are
# (rows, cols, paired): the smallest shapes at which each (ring, copy passes) instance of k_gemv_q is still selected; 8448 columns are past
# mfma_supported's 8192 (the line records the refusal), 13824 x 2560 is the model's gate|up
GEMV_SHAPES = [(32, 256, False), (32, 2304, True), (32, 3328, True), (32, 3840, False), (32, 4352, False), (32, 4352, True), (32, 6400, False),
               (32, 7424, False), (32, 8448, False), (13824, 2560, True)]


def report(hip, name, fn):
    """run one refusal case: `fn` returns the rc"""
    rc = fn()
    print(f"{name} | {rc} | {hip.last_error() if rc else ''}", flush=True)


def upload(hip, rng, rows, cols, kind, block=32):
    if kind == "qk256":
        return hip.weights_upload_qk256(rng.integers(0, 256, rows * cols // 4, dtype=np.uint8), rows, cols, cols // 4)
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(rows, cols), p=[0.5, 0.25, 0.25])
    packed = (codes[:, 0::4] | codes[:, 1::4] << 2 | codes[:, 2::4] << 4 | codes[:, 3::4] << 6).astype(np.uint8).reshape(-1)
    scales = rng.uniform(0.01, 2.0, rows * cols // block).astype(np.float32)
    return hip.weights_upload_i2s(packed, scales.astype(np.float16).astype(np.float32) if kind == "f16" else scales, rows, cols, block)


def upload_shape(hip, rng, rows, cols, paired, kind):
    if not paired:
        return upload(hip, rng, rows, cols, kind), ()
    parts = (upload(hip, rng, rows // 2, cols, kind), upload(hip, rng, rows // 2, cols, kind))
    return hip.weights_concat(list(parts), interleave16=True), parts


# ---------------------------------------------------------------- refusals
def refusals(hip):
    c = hip.c
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    vp = C.c_void_p
    NOH = 12345  # no such handle

    def nulls(n, *skip):  # every argument tuple with exactly one of n pointers NULL
        return [(i, tuple(None if j == i else p for j in range(n))) for i in range(n) if i not in skip]

    # ---- the QAct GEMV entries: their own first lines (no handle behind them) ----
    gq = lambda h, qin, y, qo, flags=0, ln=None, st=None, res=None: c.bitnet_hip_gemv_q_dev(h, qin, st, ln, 0.0, res, flags, y, qo, None, None, None)
    gb = lambda h, n, qin, y, qo, flags=0, ln=None, st=None, res=None: c.bitnet_hip_gemv_q_batch_dev(h, n, qin, st, ln, 0.0, res, flags, y, qo, None, None, None)
    report(hip, "gemv_q_dev | unknown handle", lambda: gq(NOH, p, p, None))
    report(hip, "gemv_q_dev | unknown handle + null qact_in (the handle first)", lambda: gq(NOH, None, p, None))
    for n in (0, 9):
        report(hip, f"gemv_q_batch_dev | n_seq {n}", lambda: gb(NOH, n, p, p, None))
    report(hip, "gemv_q_batch_dev | n_seq 0 + null qact_in + unknown handle (n_seq first)", lambda: gb(NOH, 0, None, p, None))
    report(hip, "gemv_q_batch_dev | null qact_in", lambda: gb(NOH, 2, None, p, None))
    report(hip, "gemv_q_batch_dev | null y and qact_out", lambda: gb(NOH, 2, p, None, None))
    report(hip, "gemv_q_batch_dev | null qact_in + unknown handle (the pointers first)", lambda: gb(NOH, 2, None, None, None))
    report(hip, "gemv_q_batch_dev | unknown handle", lambda: gb(NOH, 2, p, None, p))
    # ---- the merging o-projection ----
    report(hip, "gemv_attn_merge_dev | unknown handle", lambda: c.bitnet_hip_gemv_attn_merge_dev(NOH, p, 4, 2, 256, p, p, None, None))
    report(hip, "gemv_attn_merge_q_dev | null qact_out", lambda: c.bitnet_hip_gemv_attn_merge_q_dev(NOH, p, 4, 2, 256, p, p, None, None, None, None, None))
    report(hip, "gemv_attn_merge_q_dev | unknown handle", lambda: c.bitnet_hip_gemv_attn_merge_q_dev(NOH, p, 4, 2, 256, p, p, None, p, None, None, None))
    mr = lambda qo, rec: c.bitnet_hip_gemv_attn_merge_rec_q_dev(NOH, p, 4, 2, 256, p, p, None, qo, None, None, rec, None)
    report(hip, "gemv_attn_merge_rec_q_dev | null qact_out", lambda: mr(None, 4))
    report(hip, "gemv_attn_merge_rec_q_dev | max_records 5", lambda: mr(p, 5))
    report(hip, "gemv_attn_merge_rec_q_dev | null qact_out + max_records 5 (the pointer first)", lambda: mr(None, 5))
    report(hip, "gemv_attn_merge_rec_q_dev | unknown handle", lambda: mr(p, 8))
    # ---- decode attention, batch-1: (entry, pointers ahead of the sizes, pointers behind them, the call) ----
    at = {
        "attention_decode_dev": (8, lambda a, h, k, d: c.bitnet_hip_attention_decode_dev(*a[:5], h, k, d, 512, *a[5:], None)),
        "attention_decode_wide_dev": (8, lambda a, h, k, d: c.bitnet_hip_attention_decode_wide_dev(*a[:5], h, k, d, 512, *a[5:], None)),
        "attention_decode_partial_dev": (7, lambda a, h, k, d: c.bitnet_hip_attention_decode_partial_dev(*a[:5], h, k, d, 512, *a[5:], None)),
    }
    for flags in (0, 1, 2, 4, 7):  # a[7], a[8] = out, qact_out
        at[f"attention_decode_q_dev flags {flags}"] = (9, lambda a, h, k, d, f=flags: c.bitnet_hip_attention_decode_q_dev(*a[:5], h, k, d, 512, a[5], a[6], f, a[7], a[8], None))
    for entry, (n, call) in at.items():
        ok = (p,) * n
        for i, a in nulls(n):
            report(hip, f"{entry} | null pointer {i}", lambda: call(a, 4, 2, 64))  # with a bad head_dim behind it: refused (the pointer) or refused (the shape)
        if n == 9:
            report(hip, f"{entry} | null out and qact_out", lambda: call((p,) * 7 + (None, None), 4, 2, 64))
        for h, k, d in ((4, 0, 128), (5, 2, 128), (4, 2, 64), (8, 1, 128), (4, 0, 64), (5, 2, 64), (8, 1, 64)):  # the last three: two faults
            report(hip, f"{entry} | heads {h}/{k} head_dim {d}", lambda: call(ok, h, k, d))
        report(hip, f"{entry} | null pointer 0 + heads 4/0", lambda: call((None,) + ok[1:], 4, 0, 128))
    # ---- decode attention, batched ----
    ab = lambda a, n=2, h=4, k=2, d=128, mp=320, f=0: c.bitnet_hip_attention_decode_batch_dev(*a[:6], n, h, k, d, mp, a[6], f, a[7], a[8], None)
    ok = (p,) * 9
    for n in (0, 9):
        report(hip, f"attention_decode_batch_dev | n_seq {n}", lambda: ab(ok, n=n))
    for i, a in nulls(9):
        report(hip, f"attention_decode_batch_dev | null pointer {i}", lambda: ab(a, f=1))  # with bad flags behind it
    report(hip, "attention_decode_batch_dev | null out and qact_out", lambda: ab((p,) * 7 + (None, None)))
    for f in (1, 4, 3, 8):
        report(hip, f"attention_decode_batch_dev | flags {f}", lambda: ab(ok, f=f))
    for h, k, d, mp in ((4, 0, 128, 320), (5, 2, 128, 320), (4, 2, 128, 0), (4, 2, 64, 320), (8, 1, 128, 320), (4, 0, 128, 0), (4, 2, 64, 0), (5, 2, 64, 0)):
        report(hip, f"attention_decode_batch_dev | heads {h}/{k} head_dim {d} max_pos {mp}", lambda: ab(ok, h=h, k=k, d=d, mp=mp))
    report(hip, "attention_decode_batch_dev | n_seq 0 + null pointer 0 (n_seq first)", lambda: ab((None,) + ok[1:], n=0))
    report(hip, "attention_decode_batch_dev | flags 1 + heads 4/0 (the flags first)", lambda: ab(ok, k=0, f=1))
    # ---- the logits head and the plain argmax ----
    lg = lambda a, hidden=512, n_wg=8: c.bitnet_hip_logits_f16_dev(a[0], a[1], None, 1e-5, hidden, 100, a[2], a[3], n_wg, None, None, None, None, None)
    lb = lambda a, hidden=512, n_seq=2, n_wg=8: c.bitnet_hip_logits_f16_batch_dev(a[0], a[1], None, 1e-5, hidden, 100, n_seq, a[2], a[3], n_wg, None, None, None, None, None)
    ok = (p,) * 4
    for name, call in (("logits_f16_dev", lg), ("logits_f16_batch_dev", lb)):
        for i, a in nulls(4):
            report(hip, f"{name} | null pointer {i}", lambda: call(a, hidden=768))
        for hidden in (0, 256, 768, 8704, 1 << 40):
            report(hip, f"{name} | hidden {hidden}", lambda: call(ok, hidden=hidden))
        for n_wg in (0, 65536):
            report(hip, f"{name} | n_wg {n_wg}", lambda: call(ok, n_wg=n_wg))
        report(hip, f"{name} | hidden 768 + n_wg 0 (hidden first)", lambda: call(ok, hidden=768, n_wg=0))
    for n in (0, 9):
        report(hip, f"logits_f16_batch_dev | n_seq {n}", lambda: lb(ok, n_seq=n))
    report(hip, "logits_f16_batch_dev | n_seq 0 + null pointer 0 (n_seq first)", lambda: lb((None,) + ok[1:], n_seq=0))
    for n, hidden in ((8, 5120), (5, 8192), (8, 8192)):
        report(hip, f"logits_f16_batch_dev | {n} x {hidden}: LDS", lambda: lb(ok, hidden=hidden, n_seq=n))
    report(hip, "logits_f16_batch_dev | 8 x 5120 + n_wg 0 (the LDS first)", lambda: lb(ok, hidden=5120, n_seq=8, n_wg=0))
    am = lambda a, n=10, n_wg=4: c.bitnet_hip_argmax_dev(a[0], n, a[1], n_wg, a[2], None)
    for i, a in nulls(3):
        report(hip, f"argmax_dev | null pointer {i}", lambda: am(a, n=0))
    report(hip, "argmax_dev | n 0", lambda: am((p,) * 3, n=0))
    report(hip, "argmax_dev | n_wg 0", lambda: am((p,) * 3, n_wg=0))
    if not hip.is_available():
        return
    # ---- behind a weights handle (GPU): the shared front of the two QAct GEMV entries, then the merging o-projection ----
    import torch as t

    hip.init(0)
    rng = np.random.default_rng(11)
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a)).cuda()
    z = lambda n, dt=t.uint8: t.zeros(n, dtype=dt, device="cuda")
    ptr = lambda x: None if x is None else vp(x.data_ptr())
    plain, (paired, parts) = upload(hip, rng, 32, 512, "qk256"), upload_shape(hip, rng, 32, 512, True, "qk256")
    b256, ragged, wide = upload(hip, rng, 32, 512, "f32", 256), upload(hip, rng, 24, 512, "qk256"), upload(hip, rng, 32, 4352, "qk256")
    gam, gam2, gamw = dev(rng.uniform(0.5, 1.5, 512).astype(np.float32)), dev(np.ones(512, np.float32)), dev(rng.uniform(0.5, 1.5, 4352).astype(np.float32))
    hip.weights_bind_ln(plain, gam), hip.weights_bind_ln(wide, gamw)
    q, y, st, res = z(8 * hip.qact_bytes(4352)), z(8 * 32, t.float32), z(8 * 2 * 4352 // 16, t.float64), z(8 * 32, t.float32)
    for name, call in (("gemv_q_dev", lambda h, **kw: gq(h, ptr(q), ptr(y), None, **kw)), ("gemv_q_batch_dev", lambda h, **kw: gb(h, 3, ptr(q), ptr(y), None, **kw))):
        report(hip, f"{name} | 256-element scale blocks", lambda: call(b256))
        report(hip, f"{name} | rows 24", lambda: call(ragged))
        report(hip, f"{name} | silu on an unpaired handle", lambda: call(plain, flags=SILU))
        report(hip, f"{name} | silu with a residual", lambda: call(paired, flags=SILU, res=ptr(res)))
        report(hip, f"{name} | LayerNorm without stats_in", lambda: call(plain, ln=ptr(gam)))
        report(hip, f"{name} | LayerNorm, gamma not the bound one", lambda: call(plain, ln=ptr(gam2), st=ptr(st)))
        report(hip, f"{name} | LayerNorm on a handle with nothing bound", lambda: call(paired, ln=ptr(gam), st=ptr(st)))
        report(hip, f"{name} | LayerNorm over 4352 columns", lambda: call(wide, ln=ptr(gamw), st=ptr(st)))
        report(hip, f"{name} | rows 24 + silu (the matrix first)", lambda: call(ragged, flags=SILU))
        report(hip, f"{name} | silu unpaired + LayerNorm unbound (silu first)", lambda: call(plain, flags=SILU, ln=ptr(gam2), st=ptr(st)))
        report(hip, f"{name} | LayerNorm unbound + 4352 columns (the binding first)", lambda: call(wide, ln=ptr(gam), st=ptr(st)))
        report(hip, f"{name} | accepted: LayerNorm, bound", lambda: call(plain, ln=ptr(gam), st=ptr(st)))
        report(hip, f"{name} | accepted: silu, paired", lambda: call(paired, flags=SILU))
    o1024, o2816, r24 = upload(hip, rng, 32, 1024, "qk256"), upload(hip, rng, 32, 2816, "qk256"), upload(hip, rng, 24, 1024, "qk256")
    rec, pos = z(hip.c.bitnet_hip_attention_scratch_bytes(22, 512) // 4, t.float32), z(1, t.int32)
    # (residual and gamma_out are given on purpose: k_gemv_q reads its absent epilogue operands at qin instead, and the merging form has no qin)
    mq = lambda h, heads, kv, qo=q, records=4, yy=y, pp=pos: c.bitnet_hip_gemv_attn_merge_rec_q_dev(h, ptr(rec), heads, kv, 512, ptr(pp), ptr(yy), ptr(res), ptr(qo), ptr(res), None, records, None)
    report(hip, "gemv_attn_merge_rec_q_dev | null y", lambda: mq(o1024, 8, 2, yy=None))
    report(hip, "gemv_attn_merge_rec_q_dev | null pos", lambda: mq(o1024, 8, 2, pp=None))
    report(hip, "gemv_attn_merge_rec_q_dev | cols != heads * 128", lambda: mq(o1024, 4, 2))
    report(hip, "gemv_attn_merge_rec_q_dev | group 8", lambda: mq(o1024, 8, 1))
    report(hip, "gemv_attn_merge_rec_q_dev | heads 8/0", lambda: mq(o1024, 8, 0))
    report(hip, "gemv_attn_merge_rec_q_dev | rows 24 with a QAct output", lambda: mq(r24, 8, 2))
    report(hip, "gemv_attn_merge_rec_q_dev | 8 records over 2816 columns", lambda: mq(o2816, 22, 11, records=8))
    report(hip, "gemv_attn_merge_rec_q_dev | accepted: 4 records over 2816 columns", lambda: mq(o2816, 22, 11))
    report(hip, "gemv_attn_merge_dev | 4352 columns (ring > 2)", lambda: c.bitnet_hip_gemv_attn_merge_dev(wide, ptr(rec), 34, 17, 512, ptr(pos), ptr(y), None, None))
    t.cuda.synchronize()
    for h in (plain, paired, *parts, b256, ragged, wide, o1024, o2816, r24):
        hip.weights_free(h)


# ---------------------------------------------------------------- calls
def calls(hip):
    import torch as t
    from oracle import oracle as orc

    pkg = importlib.import_module("bitnet-rs_amd")
    hip.init(0)
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a)).cuda()
    sha = lambda x: hashlib.sha256(x.contiguous().view(-1).cpu().numpy().tobytes()).hexdigest()[:32]
    nan = float("nan")
    fill = lambda n, dt=t.uint8, v=0xA5: t.full((n,), v, dtype=dt, device="cuda")

    def emit(name, fn, **outs):
        """one call -> one line: the digests of its outputs, or the refusal.  Only what the library refuses on the host before any launch counts
        as one (invalid argument, unsupported, the launcher's own hipErrorInvalidValue); anything else -- a GPU error, a fault that shows at the
        synchronize or the copy back -- ends the process with a non-zero status at once, so that nothing more starts on a faulted device"""
        try:
            fn()
        except pkg.BitNetHipError as e:
            if e.code not in (pkg.ERR_INVALID_ARGUMENT, pkg.ERR_UNSUPPORTED) and str(e) != "kernel launch failed: invalid argument":
                raise
            print(f"{name}: refused {e}", flush=True)
            return
        t.cuda.synchronize()
        print(f"{name}:" + "".join(f" {k} {sha(v)}" for k, v in outs.items()), flush=True)

    # ---- k_gemv_q / k_gemv_q_batch: every (ring, passes) instance x scale kind, with and without LayerNorm after the product ----
    for rows, cols, paired in GEMV_SHAPES + [(32, 6912, False)]:
        for kind in KINDS:
            rng = np.random.default_rng(rows * 7 + cols + KINDS.index(kind))
            h, parts = upload_shape(hip, rng, rows, cols, paired, kind)
            out_rows, flags = (rows // 2, SILU) if paired else (rows, 0)
            gamma_in = dev((rng.uniform(0.5, 1.5, cols) / (1.58 * np.sqrt(cols))).astype(np.float32))
            gamma_out = dev(rng.uniform(0.5, 1.5, out_rows).astype(np.float32))
            lns = (False, True) if cols <= 4096 else (False,)
            if True in lns and hip.gemv_q_supported(h):
                hip.weights_bind_ln(h, gamma_in)
            qb, sb, qob, sob = hip.qact_bytes(cols), hip.qact_stats_bytes(cols) // 8, hip.qact_bytes(out_rows), hip.qact_stats_bytes(out_rows) // 8
            xs = (rng.normal(0.05, 1, (8, cols)) * rng.choice([0.01, 1.0, 30.0], (8, cols))).astype(np.float32)
            res = dev(rng.normal(0, 1, (8, out_rows)).astype(np.float32))
            for ln in lns:
                qin, stin = fill(8 * qb, v=0), t.zeros(8 * sb, dtype=t.float64, device="cuda")
                for b in range(8):
                    hip.quantize_act_dev(dev(xs[b]), gamma_in if ln else None, cols, qin[b * qb:(b + 1) * qb], stin[b * sb:(b + 1) * sb])
                kw = dict(flags=flags, gamma_out=gamma_out, residual=None if paired else res)
                if ln:
                    kw.update(ln_gamma=gamma_in, ln_eps=1e-5, stats_in=stin)
                tag = f"{rows}x{cols} {kind} paired={int(paired)} ln={int(ln)}"
                if (rows, cols) != (32, 6912):  # (the batched list's extra shape)
                    y, qo, so = fill(out_rows, t.float32, nan), fill(qob), fill(sob, t.float64, nan)
                    emit(f"gemv_q_dev {tag}", lambda: hip.gemv_q_dev(h, qin, y=y, qact_out=qo, stats_out=so, **kw), y=y, qact=qo, stats=so)
                for n_seq in (1, 2, 3, 5, 8):
                    if (rows, cols) == (32, 6912) and n_seq != 8:
                        continue
                    y, qo, so = fill(n_seq * out_rows, t.float32, nan), fill(n_seq * qob), fill(n_seq * sob, t.float64, nan)
                    emit(f"gemv_q_batch_dev {tag} n_seq={n_seq}", lambda: hip.gemv_q_batch_dev(h, n_seq, qin, y=y, qact_out=qo, stats_out=so, **kw), y=y, qact=qo, stats=so)
            for w in (h, *parts):
                hip.weights_free(w)

    # ---- decode attention: record counts either side of each combine instance; the records then feed the merging GEMVs ----
    def attn_case(h, k, max_pos, f16, seed):
        rng = np.random.default_rng(seed)
        sin, cos = orc.rope_tables(D, max_pos, 10000.0)
        dt = np.float16 if f16 else np.float32
        mk = lambda: dev(rng.normal(0, 1, k * max_pos * D).astype(dt))
        return dev(rng.normal(0, 1.5, (3, (h + 2 * k) * D)).astype(np.float32)), dev(sin), dev(cos), mk, hip.c.bitnet_hip_attention_scratch_bytes(k, max_pos)

    for h, k in ((4, 2), (3, 3)):
        for max_pos in (512, 576, 1024, 1088, 2560, 2624):
            pos = t.tensor([max_pos - 3], dtype=t.int32, device="cuda")
            for f16 in (False, True):
                qkv, sin, cos, mk, sbytes = attn_case(h, k, max_pos, f16, 1000 * h + max_pos + f16)
                for wide in (False, True):
                    for partial in (False, True):
                        kc, vc, s, out, qo = mk(), mk(), fill(sbytes // 4, t.float32, 3.0), fill(h * D, t.float32, nan), fill(hip.qact_bytes(h * D))
                        emit(f"attention_decode_q_dev {h}/{k} max_pos={max_pos} f16={int(f16)} wide={int(wide)} partial={int(partial)}",
                             lambda: hip.attention_decode_q_dev(qkv[0], sin, cos, kc, vc, h, k, D, max_pos, pos, s, None if partial else out, None if partial else qo,
                                                                wide=wide, kv_f16=f16, partial=partial), out=out, qact=qo, scratch=s, kcache=kc, vcache=vc)
                poss = [t.tensor([p], dtype=t.int32, device="cuda") for p in (max_pos - 1, 0, max_pos // 2)]
                kcs, vcs = [mk() for _ in range(3)], [mk() for _ in range(3)]
                table = lambda ts: t.tensor([x.data_ptr() for x in ts], dtype=t.int64, device="cuda")
                s, out, qo = fill(3 * sbytes // 4, t.float32, 3.0), fill(3 * h * D, t.float32, nan), fill(3 * hip.qact_bytes(h * D))
                emit(f"attention_decode_batch_dev {h}/{k} max_pos={max_pos} f16={int(f16)} n_seq=3",
                     lambda: hip.attention_decode_batch_dev(qkv, sin, cos, table(kcs), table(vcs), table(poss), 3, h, k, D, max_pos, s, out, qo, kv_f16=f16),
                     out=out, qact=qo, scratch=s, **{f"kcache{i}": x for i, x in enumerate(kcs)}, **{f"vcache{i}": x for i, x in enumerate(vcs)})
            qkv, sin, cos, mk, sbytes = attn_case(h, k, max_pos, False, 1000 * h + max_pos)
            for name in ("attention_decode_dev", "attention_decode_wide_dev", "attention_decode_partial_dev"):
                kc, vc, s, out = mk(), mk(), fill(sbytes // 4, t.float32, 3.0), fill(h * D, t.float32, nan)
                args = (qkv[0], sin, cos, kc, vc, h, k, D, max_pos, pos, s) + (() if "partial" in name else (out,))
                emit(f"{name} {h}/{k} max_pos={max_pos}", lambda: getattr(hip, name)(*args), out=out, scratch=s, kcache=kc, vcache=vc)

    # ---- the merging GEMVs: k_gemv_q<.., NE, NE1, NR> over 4 and 8 records, k_gemv_mfma<.., MERGE> over 4 ----
    # (4096 columns are two copy passes, which the merging form does not take: its lines record the refusal; 2816 is the smallest (2, 0, 4) shape)
    for cols, n_kv in ((1024, 2), (2304, 9), (2560, 5), (2816, 11), (4096, 8)):
        n_heads, max_pos, rows = cols // D, 512, 32
        for kind in KINDS + ("b256",):
            rng = np.random.default_rng(cols + len(kind))
            w = upload(hip, rng, rows, cols, "f32", 256) if kind == "b256" else upload(hip, rng, rows, cols, kind)
            qkv, sin, cos, mk, sbytes = attn_case(n_heads, n_kv, max_pos, False, cols)
            res, gam = dev(rng.normal(0, 1, rows).astype(np.float32)), dev(rng.uniform(0.5, 1.5, rows).astype(np.float32))
            for records, p in ((4, 200), (8, 450)):
                if records == 8 and cols > 2560:
                    continue
                pos = t.tensor([p], dtype=t.int32, device="cuda")
                s = fill(sbytes // 4 + 16, t.float32, 3.0)
                hip.attention_decode_partial_dev(qkv[0], sin, cos, mk(), mk(), n_heads, n_kv, D, max_pos, pos, s)
                y, qo, so = fill(rows, t.float32, nan), fill(hip.qact_bytes(rows)), fill(rows // 16 * 2, t.float64, nan)
                emit(f"gemv_attn_merge_rec_q_dev {cols} {kind} records={records}",
                     lambda: hip.gemv_attn_merge_rec_q_dev(w, s, n_heads, n_kv, max_pos, pos, y, qo, records, residual=res, gamma_out=gam, stats_out=so), y=y, qact=qo, stats=so)
                if records == 4:
                    y = fill(rows, t.float32, nan)
                    emit(f"gemv_attn_merge_dev {cols} {kind}", lambda: hip.gemv_attn_merge_dev(w, s, n_heads, n_kv, max_pos, pos, y, residual=res), y=y)
            hip.weights_free(w)

    # ---- k_gemv_mfma on f32 activations: statistics vectors <= 2 and <= 4, the three LayerNorm forms, every scale kind, m = 1 and 3 ----
    for cols in (2560, 6912):
        for kind in KINDS + ("b256",):
            rng = np.random.default_rng(cols + 17 * len(kind))
            rows = 48
            w = upload(hip, rng, rows, cols, "f32", 256) if kind == "b256" else upload(hip, rng, rows, cols, kind)
            x, gam, res = dev(rng.normal(0.05, 1, (3, cols)).astype(np.float32)), dev(rng.uniform(0.5, 1.5, cols).astype(np.float32)), dev(rng.normal(0, 1, (3, rows)).astype(np.float32))
            for form in ("none", "prologue", "bound"):
                if form == "bound":
                    hip.weights_bind_ln(w, gam)
                for m in (1, 3):
                    y = fill(m * rows, t.float32, nan)
                    emit(f"gemv_fused_dev {rows}x{cols} {kind} ln={form} m={m}",
                         lambda: hip.gemv_fused_dev(w, x, y, m, ln_gamma=None if form == "none" else gam, ln_eps=1e-5, residual=res), y=y)
            hip.weights_free(w)
        rng = np.random.default_rng(cols)
        (w, parts), x, y = upload_shape(hip, rng, 64, cols, True, "qk256"), dev(rng.normal(0, 1, cols).astype(np.float32)), fill(32, t.float32, nan)
        emit(f"gemv_fused_dev 64x{cols} qk256 silu", lambda: hip.gemv_fused_dev(w, x, y, 1, flags=SILU), y=y)
        for hh in (w, *parts):
            hip.weights_free(hh)

    # ---- the logits head: one hidden size per instance of k_logits_f16 / k_logits_f16_batch ----
    vocab, n_wg, n_seq = 1031, 40, 3
    i32 = lambda v: t.tensor(v, dtype=t.int32, device="cuda")
    for hidden in (512, 1024, 1536, 2048, 2560, 3584, 4096, 4608, 8192):
        rng = np.random.default_rng(hidden)
        table, gam = dev(rng.normal(0, 1, (vocab, hidden)).astype(np.float16)), dev(rng.uniform(0.5, 1.5, hidden).astype(np.float32))
        x = dev(rng.normal(0.1, 1.0, (n_seq, hidden)).astype(np.float32))
        logits, s, tok, pos, hist = fill(vocab, t.float32, nan), fill(2 * n_wg, t.float32, 3e38), i32([-1]), i32([3]), t.full((16,), -7, dtype=t.int32, device="cuda")
        emit(f"logits_f16_dev hidden={hidden}", lambda: hip.logits_f16_dev(table, x[0], gam, 1e-5, hidden, vocab, logits, s, n_wg, token=tok, pos=pos, history=hist),
             logits=logits, scratch=s, token=tok, pos=pos, history=hist)
        lgs, toks, poss, hists = ([fill(vocab, t.float32, nan) for _ in range(n_seq)], [i32([-1]) for _ in range(n_seq)], [i32([3 + b]) for b in range(n_seq)],
                                  [t.full((16,), -7, dtype=t.int32, device="cuda") for _ in range(n_seq)])
        table_of = lambda ts: t.tensor([v.data_ptr() for v in ts], dtype=t.int64, device="cuda")
        s = fill(2 * n_wg * n_seq, t.float32, 3e38)
        emit(f"logits_f16_batch_dev hidden={hidden} n_seq={n_seq}",
             lambda: hip.logits_f16_batch_dev(table, x, gam, 1e-5, hidden, vocab, n_seq, table_of(lgs), s, n_wg, token_ptrs=table_of(toks), pos_ptrs=table_of(poss),
                                              history_ptrs=table_of(hists)),
             scratch=s, **{f"logits{b}": v for b, v in enumerate(lgs)}, **{f"token{b}": v for b, v in enumerate(toks)}, **{f"history{b}": v for b, v in enumerate(hists)})
    v, s, tok = dev(np.random.default_rng(5).normal(0, 1, 1031).astype(np.float32)), fill(2 * n_wg, t.float32, 3e38), i32([-1])
    emit("argmax_dev", lambda: hip.argmax_dev(v, 1031, s, n_wg, tok), scratch=s, token=tok)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("refusals", "calls"):
        sys.exit(__doc__)
    import torch  # noqa: F401  (ahead of the library: bitnet-rs_amd.load())

    pkg = importlib.import_module("bitnet-rs_amd")
    {"refusals": refusals, "calls": calls}[sys.argv[1]](pkg.HipLib(sys.argv[2]) if len(sys.argv) > 2 else pkg.HipLib())
