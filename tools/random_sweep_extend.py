"""Developer tool (GPU box): the continuation attention (bitnet_hip_attention_extend_dev: seq new tokens over a cache that holds `past`
positions) at random (past, seq, heads, kv heads, cache type) against the float64 restatement tests/extend_ref.py.  The past is laid down by
one whole-prompt call or by a chain of continuations; the slots beyond it hold large finite garbage.
python tools/random_sweep_extend.py [n] [seed]"""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extend_ref as er
from oracle import oracle
oracle.build()
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
D, bad = 128, 0
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
for case in range(n_cases):
    n_kv = int(rng.choice([1, 2, 4, 5, 8])); n_heads = n_kv * int(rng.choice([1, 2, 4]))
    past = int(rng.choice([0, 1, 2, 31, 63, 64, 65, 100, 127, 128, 129, 333, 512, 700, 1023, 1100, 2049]))
    seq = int(rng.choice([1, 2, 15, 16, 17, 63, 64, 65, 100, 128, 129, 200, 333]))
    f16, chain = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    T = past + seq
    max_pos = T + int(rng.integers(0, 130))
    qkv = rng.normal(0, rng.uniform(1.2, 1.5), (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    sin_d, cos_d = dev(sin), dev(cos)
    sin, cos = sin.reshape(max_pos, D // 2).astype(np.float64), cos.reshape(max_pos, D // 2).astype(np.float64)
    dt = torch.float16 if f16 else torch.float32
    elems = n_kv * er.chunks(max_pos) * 64 * D
    big = 3.0e4 if f16 else 1.0e30
    kc = (big * (2 * torch.randint(0, 2, (elems,), device="cuda") - 1)).to(dt)  # every slot starts as garbage: only written slots may be read
    vc = (big * (2 * torch.randint(0, 2, (elems,), device="cuda") - 1)).to(dt)
    flags = 1 if f16 else 0

    def extend(rows, p):
        wsb = hip.attention_extend_workspace_bytes(n_heads, n_kv, p, rows.shape[0])
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
        out = torch.full((rows.shape[0], n_heads * D), float("nan"), device="cuda")
        hip.attention_extend_dev(dev(rows), sin_d, cos_d, kc, vc, n_heads, n_kv, D, max_pos, p, rows.shape[0], ws, wsb, out, flags)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    try:
        if past and not chain:
            wsb = hip.attention_prefill_workspace_bytes(n_heads, n_kv, past)
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            out = torch.empty(past, n_heads * D, device="cuda")
            hip.attention_prefill_flags_dev(dev(qkv[:past]), sin_d, cos_d, kc, vc, n_heads, n_kv, D, max_pos, past, ws, wsb, out, flags)
        elif past:
            cuts = np.unique(np.concatenate([[0, past], rng.integers(1, max(past, 2), 2)]))
            for a, b in zip(cuts[:-1], cuts[1:]):
                extend(qkv[a:b], int(a))
        got = extend(qkv[past:], past).reshape(seq, n_heads, D)
        pos = np.arange(T)
        _, k_all, v_all = er.split_qkv(qkv, n_heads, n_kv)
        k_all = er.rope_np(k_all, sin[pos, None, :], cos[pos, None, :])
        want, _, _ = er.extend_f64(qkv[past:], k_all[:past], v_all[:past], n_heads, n_kv, sin, cos)
        err = float(np.max(np.abs(got - want)))
        v_got = er.decode_v(vc.cpu().numpy(), n_kv, max_pos, f16)[:T]
        v_want = v_all.astype(np.float16 if f16 else np.float32)
        ok = np.isfinite(got).all() and err <= 6e-3 and np.array_equal(v_got, v_want)
    except pkg.BitNetHipError as e:
        ok, err = False, repr(e)
    if not ok:
        bad += 1
        print("FAIL", past, seq, n_heads, n_kv, "f16" if f16 else "f32", "chain" if chain else "prefill", err, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
