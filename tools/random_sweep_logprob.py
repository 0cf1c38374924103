"""Developer tool (GPU box): the logits tap's kernel (bitnet_hip_logprob_dev / _batch_dev) at random vocabularies, rows, top_n, positions and
planted ties / NaN / inf, against tests/logprob_ref.py -- the differential companion of tests/test_logprob_gpu.py: token, n_top, top_id and the
bits of top_logit and logit exact, lse within logprob_ref.lse_bound; every third case goes through a batched table beside single launches
and compares the bytes.   python tools/random_sweep_logprob.py [n] [seed]"""
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("bitnet-rs_amd")
import logprob_ref as ref  # noqa: E402  (checker)

hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 19)
CAP = 4


def random_row(v):
    x = (rng.standard_normal(v) * float(rng.choice([0.05, 1.0, 4.0, 30.0]))).astype(np.float32)
    kind = int(rng.integers(0, 8))
    if kind == 1:
        x = np.round(x * 2) / 2  # many ties
    elif kind == 2:
        x[rng.integers(0, v, min(v, 40))] = float(x.max()) + 1.0  # planted equal maxima
    elif kind == 3:
        x[rng.integers(0, v, max(1, v // 7))] = np.nan
    elif kind == 4:
        x[rng.integers(0, v, 3)] = np.inf
        x[rng.integers(0, v, 3)] = -np.inf
    elif kind == 5:
        x[:] = rng.choice([-np.inf, np.nan, 0.0, -0.0, 3.25])
    elif kind == 6:
        x[rng.integers(0, v, max(1, v // 3))] = -0.0
        x[rng.integers(0, v, max(1, v // 3))] = 0.0
    return x.astype(np.float32)


def entry(v, x, token, q):
    t = dict(logits=torch.from_numpy(x).cuda(), pos=torch.full((1,), q, dtype=torch.int32, device="cuda"),
             history=torch.zeros(CAP, dtype=torch.int32, device="cuda"), records=torch.full((CAP * 176,), 0xA5, dtype=torch.uint8, device="cuda"),
             scratch=torch.zeros(hip.logprob_scratch_bytes(v), dtype=torch.uint8, device="cuda"))
    t["history"][q] = token
    return t


def args(t, top_n):
    return pkg.LogprobArgs.make(t["logits"], t["pos"], t["history"], t["records"], t["scratch"], CAP, top_n)


def judge(rec, want, v):
    if int(rec["token"]) != want.token or int(rec["n_top"]) != want.n_top:
        return "token / n_top"
    if not np.array_equal(rec["top_id"][:want.n_top], want.top_id):
        return f"top_id {rec['top_id'][:want.n_top].tolist()} != {want.top_id.tolist()}"
    if not ref.same_bits(rec["top_logit"][:want.n_top], want.top_logit):
        return "top_logit bits"
    if not (ref.same_bits(rec["logit"], want.logit) or (np.isnan(want.logit) and np.isnan(rec["logit"]))):
        return "logit bits"
    got = float(rec["lse"])
    if np.isinf(want.lse):
        return "" if got == want.lse else f"lse {got} != {want.lse}"
    return "" if abs(got - want.lse) <= ref.lse_bound(v, want.lse) else f"lse {got} vs {want.lse}: {abs(got - want.lse):.3e} > {ref.lse_bound(v, want.lse):.3e}"


bad = 0
worst = 0.0
for case in range(n_cases):
    v = int(rng.choice([1, 2, 3, 19, 20, 21, 63, 64, 65, 1000, 1023, 1024, 1025, 2049, 4097, 32000, 65536, 65537, 128256, 151936, int(rng.integers(1, 300000))]))
    n_entries = int(rng.integers(2, 9)) if case % 3 == 2 else 1
    es, why = [], ""
    for _ in range(n_entries):
        x, token, q, top_n = random_row(v), int(rng.integers(-1, v + 1)), int(rng.integers(0, CAP)), int(rng.choice([0, 1, 5, 20, int(rng.integers(0, 21))]))
        es.append((x, token, q, top_n, entry(v, x, token, q)))
    for x, token, q, top_n, t in es:
        hip.logprob_dev(args(t, top_n), v)
    torch.cuda.synchronize()
    for x, token, q, top_n, t in es:
        rec = t["records"].cpu().numpy().view(pkg.LOGPROB_DTYPE)[q]
        want = ref.record(x, token, top_n)
        why = why or judge(rec, want, v)
        if np.isfinite(want.lse):
            worst = max(worst, abs(float(rec["lse"]) - want.lse) / ref.lse_bound(v, want.lse))
    if n_entries > 1 and not why:
        twins = [entry(v, x, token, q) for x, token, q, top_n, t in es]
        table = torch.from_numpy(np.frombuffer(b"".join(bytes(args(t, e[3])) for t, e in zip(twins, es)), np.uint8).copy()).cuda()
        hip.logprob_batch_dev(table, n_entries, v)
        torch.cuda.synchronize()
        for t, e in zip(twins, es):
            if not (torch.equal(t["records"], e[4]["records"]) and torch.equal(t["scratch"], e[4]["scratch"])):
                why = "batched launch differs from the single launches"
    if why:
        bad += 1
        print(f"case {case}: vocab {v}, {n_entries} entries: {why}", flush=True)
print(f"{n_cases} cases, worst lse error / bound {worst:.3f}")
print("random_sweep_logprob:", "OK" if not bad else f"{bad} FAILED")
sys.exit(1 if bad else 0)
