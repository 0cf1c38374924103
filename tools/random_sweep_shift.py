"""Developer tool (GPU box): the context shift (bitnet_hip_kv_shift_dev: in place, slot j of every layer's K and V takes slot j + discard for j in
[keep, n - discard), K re-rotated) at random (layers, kv heads, max_pos, keep, discard, n, cache type, rope_theta) against the numpy restatement
(tests/shift_ref.py: shift_f32 over tests/extend_ref.py's decoded layouts).  Every slot of every cache holds normal-range random data with zeros
and -0.0 planted; the WHOLE of every cache is compared, bit for bit.
python tools/random_sweep_shift.py [n] [seed]"""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extend_ref as er
import shift_ref as sr
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 26)
D, bad = 128, 0
dev = lambda a: torch.from_numpy(a.view(np.int32).copy()).cuda()
back = lambda t: t.cpu().numpy().view(np.uint32)
table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
for case in range(n_cases):
    n_layers, n_kv = int(rng.integers(1, 4)), int(rng.choice([1, 2, 3, 5]))
    max_pos = int(rng.choice([2, 63, 64, 65, 100, 128, 129, 333, 640, 1023, 1100, 2049]))
    n = int(rng.choice([max_pos, max_pos - 1, max(1, max_pos // 2), int(rng.integers(1, max_pos + 1))]))
    keep = int(rng.choice([0, 4, min(64, n - 1), int(rng.integers(0, n))]))
    keep = max(0, min(keep, n - 1))
    room = n - keep
    discard = int(rng.choice([1, room, max(1, room // 2), max(1, room // 2 - 1), max(1, room // 2 + 1), min(room, 64), min(room, 63), int(rng.integers(1, room + 1))]))
    f16 = bool(rng.integers(0, 2))
    dt = np.float16 if f16 else np.float32
    slots = er.chunks(max_pos) * 64
    sin, cos = sr.rope_tables(max_pos, float(rng.choice([1e4, 5e5])))
    ks, vs = [], []
    for _ in range(n_layers):
        k, v = (rng.standard_normal((slots, n_kv, D)).astype(dt) for _ in range(2))
        for a in (k, v):
            at = rng.integers(0, a.size, a.size // 40 + 2)
            a.reshape(-1)[at[::2]] = 0.0
            a.reshape(-1)[at[1::2]] = -0.0
        ks.append(k), vs.append(v)
    k_d = [dev(er.encode_k(k, max_pos, f16).view(np.uint32)) for k in ks]
    v_d = [dev(er.encode_v(v, max_pos, f16).view(np.uint32)) for v in vs]
    try:
        hip.kv_shift_dev(table(k_d), table(v_d), torch.from_numpy(sin).cuda(), torch.from_numpy(cos).cuda(), n_layers, n_kv, D, max_pos, keep, discard, n,
                         kv_f16=f16)
        torch.cuda.synchronize()
        ok = True
        for l in range(n_layers):
            wk, wv = sr.shift_f32(ks[l], vs[l], sin, cos, keep, discard, n)
            ok = ok and np.array_equal(back(k_d[l]), er.encode_k(wk, max_pos, f16).view(np.uint32))
            ok = ok and np.array_equal(back(v_d[l]), er.encode_v(wv, max_pos, f16).view(np.uint32))
        err = ""
    except pkg.BitNetHipError as e:
        ok, err = False, repr(e)
    if not ok:
        bad += 1
        print("FAIL", n_layers, n_kv, max_pos, keep, discard, n, "f16" if f16 else "f32", err, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
