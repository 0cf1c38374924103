"""Developer tool (GPU box): the sampler chain (min-p, typical-p, frequency / presence penalty) at random vocabularies, configs, row
families, histories and seeds, judged draw by draw with tests/sampler_chain_accept.accepts against the numpy restatement
(tests/sampler_chain_ref.py) -- the differential companion of tests/test_sampler_chain_gpu.py.  Prints how many draws the rule called
undecided (a deciding comparison inside the derived tolerance).   python tools/random_sweep_sampler_chain.py [n] [seed]"""
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("bitnet-rs_amd")
import sampler_cases as sc, sampler_chain_accept as ca, sampler_chain_ref as cr  # noqa: E402  (checker)

hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 120
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 11)
ROWS = [("normal", 4.0), ("normal", 12.0), ("planted", 4.0), ("equal",), ("equal_one", "slice"), ("two_interleaved",), ("two_blocks",), ("zeros",),
        ("one_inf",), ("neginf_but_one",), ("all_neginf",), ("pen", 2.0), ("two_top",)]
bad = calls = exact = undecided = 0
tok = torch.zeros(1, dtype=torch.int32, device="cuda")
for case in range(n_cases):
    v = int(rng.choice([2, 63, 64, 65, 1000, 1024, 1025, 2049, 4097, 32000, 65537, 128256, int(rng.integers(2, 200000))]))
    t = float(rng.choice([0.0, 0.5, 0.7, 1.0, 1.3]))
    k = int(rng.choice([0, 0, 1, 2, 40, 64, 65, 1000]))
    p = float(rng.choice([1.0, 0.95, 0.9, 0.5]))
    rp = float(rng.choice([1.0, 1.1, 1.3]))
    ex = dict(min_p=float(rng.choice([0.0, 0.02, 0.05, 0.3, 1.0, -1.0, 2.0])),
              typical_p=float(rng.choice([1.0, 0.9, 0.5, 0.2, 0.0, 3.0])),
              frequency_penalty=float(rng.choice([0.0, 0.0, 0.2, 1.0, -0.3])), presence_penalty=float(rng.choice([0.0, 0.0, 0.1, 0.8, -0.2])))
    mode = "host" if rng.integers(0, 2) else "dev"
    steps = int(rng.choice([1, 2, 5]))
    c = dict(id=f"rand-{case}-{int(rng.integers(1 << 30))}", vocab=v, cfg=(t, k, p, rp), seed=int(rng.integers(0, 1 << 40)),
             row=(ROWS if v >= 1025 else ROWS[:8])[int(rng.integers(len(ROWS) if v >= 1025 else 8))], gen=("rand", int(rng.choice([0, 1, 37])), int(rng.integers(1, 30))), steps=steps)
    if c["gen"][1] == 0:
        c["gen"] = ()
    try:
        x = sc.row(c)
        smp = hip.sampler(v, *c["cfg"], seed=c["seed"], **ex)
        ref = cr.ChainRef(*c["cfg"], seed=c["seed"], **ex)
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
            ok, why = ca.accepts(ref, got)
            calls += 1
            exact += got == want
            undecided += bool(ref.last["undecided"])
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
        print("FAIL", mode, c["vocab"], c["cfg"], ex, c["row"], c["gen"], c["seed"], steps, why, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree ({calls} calls, {exact} equal to the restatement, {undecided} undecided)", flush=True)
sys.exit(1 if bad else 0)
