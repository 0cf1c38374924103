"""Developer tool (GPU box): Mirostat v2 on the device at random (vocab, tau, eta, sigma, temperature, penalties, seed; sample_dev or sample_host),
12 chained calls per case, every call judged by the rule of tests/mirostat_accept.py from the mu the device held before it, as
tests/test_mirostat_gpu.py judges its seeded cases.  Prints the share of loose draws.  python tools/random_sweep_mirostat.py [n] [seed]"""
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mirostat_cases as mc
import test_mirostat_gpu as tm
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 31)
bad = draws = loose = fallbacks = 0
for k in range(n_cases):
    vocab = int(rng.choice([1, 2, 3, 64, 257, 1024, 1025, 2049, 4099, 32000, 50257, int(rng.integers(1, 70000))]))
    pen = mc.PEN_ON if rng.integers(0, 2) else mc.PEN_OFF
    case = dict(id=f"sweep{k}", vocab=vocab, tau=float(rng.choice([0.5, 1.0, 3.0, 5.0, 8.0])), eta=float(rng.choice([0.0, 0.1, 0.5])),
                sigma=float(rng.choice([0.5, 1.0, 2.0, 4.0])), temperature=float(rng.choice([0.5, 0.7, 1.0, 1.3])), seed=int(rng.integers(0, 1 << 30)), **pen)
    host = bool(rng.integers(0, 4) == 0)
    what = f"{case} host={host}"
    try:
        x = mc.row(case)
        smp, ref = tm.make(hip, case)
        j = tm.Judged(smp, ref, case["id"])
        xd, tok = torch.from_numpy(x).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda")
        gen = []
        for _ in range(12):
            if host:
                got, _ = j.call(x, lambda: smp.sample_host(x, gen), generated=gen)
                gen = gen + [got]
            else:
                j.call(x, tm.dev_runner(torch, smp, xd, tok))
        draws += j.draws; loose += j.loose; fallbacks += j.fallbacks
        smp.close()
    except BaseException as e:  # noqa: BLE001
        if isinstance(e, (KeyboardInterrupt, SystemExit)):
            raise
        bad += 1
        print("FAIL", what, repr(e)[:600], flush=True)
print(f"{draws} draws ({loose} loose), {fallbacks} fallbacks", flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
