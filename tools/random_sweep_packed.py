"""Developer tool (GPU box): the packed continuation attention (bitnet_hip_attention_packed_dev) at random (heads, kv heads, cache type, 1..64
segments of random past and length, shuffled row starts, NaNs in stale slots and padding rows) against the existing operator on each segment
alone (bitnet_hip_attention_extend_dev on a copy of the same caches) with the gates of tests/test_attention_packed_gpu.py, whose Pack it drives:
every cache bit for bit, the segment's output rows within 2e-4 of max|base|, every output row finite.
python tools/random_sweep_packed.py [n] [seed]"""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_attention_packed_gpu as tp
from oracle import oracle as orc
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
orc.build()
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 23)
D, bad = 128, 0
for case in range(n_cases):
    n_heads, n_kv = [(4, 2), (6, 3), (3, 3), (8, 2), (20, 5), (5, 5), (4, 4)][int(rng.integers(0, 7))]
    f16 = bool(rng.integers(0, 2))
    n_seq = int(rng.choice([1, 2, 3, 8, 9, 17, 64, int(rng.integers(1, 65))]))
    segs = []
    for _ in range(n_seq):
        ln = int(rng.choice([1, 2, 5, 21, 63, 64, 65, 130, int(rng.integers(1, 200))]))
        past = int(rng.choice([0, 1, 63, 64, 100, int(rng.integers(0, tp.MAX_POS))]))
        past = min(past, tp.MAX_POS - ln)
        segs.append((past, ln))
    try:
        P = tp.Pack(hip, orc, torch, n_heads, n_kv, f16, segs, seed=int(rng.integers(0, 1 << 30)))
        before, mine = P.snapshot(), P.snapshot()
        out = P.call(P.rows(), mine)
        ok, err = bool(np.isfinite(out).all()), ""
        for i, ((past, n), r0, op) in enumerate(zip(segs, P.row0, P.ops)):
            op.kc, op.vc = before[i][0].clone(), before[i][1].clone()
            base = op.extend(P.seq[i][past:], past)
            d = float(np.max(np.abs(out[r0:r0 + n] - base)))
            same = torch.equal(tp.dev_bits(torch, op.kc), tp.dev_bits(torch, mine[i][0])) and torch.equal(tp.dev_bits(torch, op.vc), tp.dev_bits(torch, mine[i][1]))
            if not (d <= 2e-4 * np.max(np.abs(base)) and same):
                ok, err = False, f"segment {i} (past {past}, len {n}): max|diff| {d:.3e} of {np.max(np.abs(base)):.3f}, caches equal {same}"
    except (pkg.BitNetHipError, AssertionError) as e:
        ok, err = False, repr(e)
    if not ok:
        bad += 1
        print("FAIL", n_heads, n_kv, "f16" if f16 else "f32", segs, err, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
