"""Developer tool (GPU box): the device sampler (sample_host / sample_dev) at random vocabularies, configs, row families, history
lengths and seeds, judged draw by draw with tests/sampler_accept.accepts against the numpy restatement of the reference's Sampler
-- the differential companion of tests/test_sampling_gpu.py.   python tools/random_sweep_sampler.py [n] [seed]"""
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("bitnet-rs_amd")
import sampler_accept as sa, sampler_cases as sc, sampler_ref as sr  # noqa: E402  (checker)

hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 120
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 9)
ROWS = [("normal", 0.05), ("normal", 1.0), ("normal", 4.0), ("normal", 12.0), ("planted", 4.0), ("equal",), ("equal_one", "slice"), ("two_interleaved",),
        ("two_blocks",), ("kth_dup",), ("zeros",), ("one_inf",), ("neginf_but_one",), ("all_neginf",), ("subnormal",), ("pen", 2.0), ("two_top",)]
bad = calls = exact = 0
worst = far = 0.0
tok = torch.zeros(1, dtype=torch.int32, device="cuda")
for case in range(n_cases):
    v = int(rng.choice([1, 2, 3, 63, 64, 65, 1000, 1024, 1025, 2049, 4097, 32000, 65536, 65537, 128256, 151936, int(rng.integers(1, 300000))]))
    t = float(rng.choice([0.0, 0.5, 0.7, 1.0, 1.3, 2.0, 1e-30, 1e30]))
    k = int(rng.choice([0, 0, 1, 2, 40, 64, 65, 1000, v - 1, v, v + 7]))
    p = float(rng.choice([1.0, 0.999999, 0.95, 0.9, 0.5, 1e-6, 0.0]))
    rp = float(rng.choice([1.0, 1.0, 1.1, 1.3, 0.5, 2.0, 1e10]))
    mode = "host" if rng.integers(0, 2) else "dev"
    steps = int(rng.choice([1, 1, 2, 5]))
    c = dict(id=f"rand-{case}-{int(rng.integers(1 << 30))}", vocab=v, cfg=(t, max(k, 0), p, rp), seed=int(rng.integers(0, 1 << 40)),
             row=(ROWS if v >= 1025 else ROWS[:9])[int(rng.integers(len(ROWS) if v >= 1025 else 9))], gen=("rand", int(rng.choice([0, 1, 37, 400])), int(rng.integers(1, 60))), steps=steps)
    if c["gen"][1] == 0:
        c["gen"] = ()
    try:
        x = sc.row(c)
        smp = hip.sampler(v, *c["cfg"], seed=c["seed"])
        ref = sr.RefSampler(*c["cfg"], seed=c["seed"])
        hist = sc.gen(c) if mode == "host" else []
        xd = torch.from_numpy(x).cuda()
        ok, why = True, ""
        for step in range(steps):
            if mode == "host":
                got = smp.sample_host(x, hist)
            else:
                smp.sample_dev(xd, tok)
                torch.cuda.synchronize()
                got = int(tok.item())
            want = ref.sample(x, hist)
            ok, why = sa.accepts(ref, got)
            calls += 1
            exact += got == want
            vd = ref.last["verdict"]
            if ok and vd["T"] > 0:
                worst, far = max(worst, vd["dist"] / vd["T"]), max(far, vd["idx"])
            if not ok:
                break
            hist = hist + [got]
        if ok and smp.draws() != ref.rng.draws:
            ok, why = False, f"draws {smp.draws()} != {ref.rng.draws}"
        smp.close()
    except pkg.BitNetHipError as e:
        ok, why = False, repr(e)
    if not ok:
        bad += 1
        print("FAIL", mode, c["vocab"], c["cfg"], c["row"], c["gen"], c["seed"], steps, why, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree ({calls} calls, {exact} equal to the restatement, worst dist/T {worst:.3f}, largest index distance {int(far)})", flush=True)
sys.exit(1 if bad else 0)
