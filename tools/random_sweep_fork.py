"""Developer tool (GPU box): the KV fork (bitnet_hip_kv_fork_dev: cache slots [0, n) of every layer's K and V of one source into n_dst destinations)
at random (layers, kv heads, max_pos, n, n_dst, cache type) against the numpy statement of the layouts (tests/extend_ref.py: k_index for K,
[kv][C * 64][D] for V).  Source and destinations hold random 32-bit patterns; the WHOLE of every destination is compared, bit for bit, and the
source must come back unchanged.
python tools/random_sweep_fork.py [n] [seed]"""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extend_ref as er
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 17)
D, bad = 128, 0
dev = lambda a: torch.from_numpy(a.view(np.int32).copy()).cuda()
back = lambda t: t.cpu().numpy().view(np.uint32)
table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
for case in range(n_cases):
    n_layers, n_kv, n_dst = int(rng.integers(1, 5)), int(rng.choice([1, 2, 3, 5, 8])), int(rng.integers(1, 9))
    max_pos = int(rng.choice([1, 2, 63, 64, 65, 100, 128, 129, 333, 640, 1023, 1100, 2049, 4096]))
    n = int(rng.choice([0, 1, max_pos, max_pos - 1, max_pos // 2, int(rng.integers(0, max_pos + 1)), min(max_pos, 64 * int(rng.integers(0, 5)))]))
    n = max(0, min(n, max_pos))
    f16 = bool(rng.integers(0, 2))
    per = 2 if f16 else 1  # elements per 32-bit word
    head = er.chunks(max_pos) * 64 * D
    words = n_kv * head // per
    rnd = lambda: rng.integers(0, 1 << 32, size=words, dtype=np.uint32)
    src_h = [[rnd() for _ in range(n_layers)] for _ in range(2)]              # [K | V][layer]
    dst_h = [[[rnd() for _ in range(n_layers)] for _ in range(n_dst)] for _ in range(2)]  # [K | V][dst][layer]
    src_d = [[dev(a) for a in kv] for kv in src_h]
    dst_d = [[[dev(a) for a in d] for d in kv] for kv in dst_h]
    try:
        hip.kv_fork_dev(table(src_d[0]), table(src_d[1]), table([t for d in dst_d[0] for t in d]), table([t for d in dst_d[1] for t in d]), n_layers, n_dst,
                        n_kv, D, max_pos, n, kv_f16=f16)
        torch.cuda.synchronize()
        d, pos = np.meshgrid(np.arange(D), np.arange(n), indexing="ij")
        d, pos = d.reshape(-1), pos.reshape(-1)
        heads = np.arange(n_kv)[:, None] * head
        copied = [np.unique((heads + er.k_index(d, pos, f16)[None, :]).reshape(-1) // per), np.unique((heads + (pos * D + d)[None, :]).reshape(-1) // per)]
        ok = True
        for which in range(2):
            for l in range(n_layers):
                ok = ok and np.array_equal(back(src_d[which][l]), src_h[which][l])
                for j in range(n_dst):
                    want = dst_h[which][j][l].copy()
                    want[copied[which]] = src_h[which][l][copied[which]]
                    ok = ok and np.array_equal(back(dst_d[which][j][l]), want)
        err = ""
    except pkg.BitNetHipError as e:
        ok, err = False, repr(e)
    if not ok:
        bad += 1
        print("FAIL", n_layers, n_kv, max_pos, n, n_dst, "f16" if f16 else "f32", err, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
