"""Developer tool (GPU box): the sampler's CONSTRAINTS stage at random -- vocabulary, path (greedy, one-lane top-k, full vocabulary, Mirostat),
penalties, bias / allowed / hold lists, min_tokens, no_repeat_ngram, prompt, seed; sample_dev or sample_host -- through the equivalence of
tests/test_constraint_gpu.py: a constrained sampler on the raw rows against an unconstrained one on the rows edited by tests/constraint_ref.py,
12 steps, every word equal.  python tools/random_sweep_constraints.py [n] [seed]"""
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import constraint_ref as cr
import test_constraint_gpu as tc
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 34)
bad = edited = 0
paths = list(tc.PATHS)
for k in range(n_cases):
    vocab = int(rng.choice([1, 2, 3, 63, 64, 65, 257, 1024, 1025, 2049, 4097, 32000, 50257, int(rng.integers(1, 70000))]))
    path = paths[int(rng.integers(0, len(paths)))]
    kw, miro = tc.PATHS[path]
    ids = lambda n: [int(t) for t in rng.integers(0, vocab, n)]
    edge = tc.edge_ids(vocab)
    cfg = {}
    if rng.integers(0, 3):
        pool = ids(int(rng.integers(1, 40))) + edge
        cfg["bias"] = [(t, float(rng.choice([-np.inf, -3.0, -0.5, 0.0, 1.0, 6.0]))) for t in rng.permutation(pool)[:int(rng.integers(1, len(pool) + 1))]]
    if rng.integers(0, 3) == 0:
        cfg["allowed"] = sorted(set(ids(int(rng.integers(1, 30))) + edge[:int(rng.integers(0, len(edge) + 1))]))
    if rng.integers(0, 2):
        cfg["hold"] = (ids(int(rng.integers(1, 32))) + edge)[:32]
        cfg["min_tokens"] = int(rng.integers(0, 10))
    if rng.integers(0, 3):
        cfg["no_repeat_ngram"] = int(rng.integers(1, 9))
    if not cr.is_on(cfg):
        cfg["no_repeat_ngram"] = 2
    small = ids(3)  # a prompt over three tokens repeats n-grams
    prompt = [small[int(i)] for i in rng.integers(0, 3, int(rng.integers(0, 24)))]
    host = bool(rng.integers(0, 4) == 0)
    what = f"vocab {vocab} {path} host={host} cfg={ {a: (b if a != 'bias' else len(b)) for a, b in cfg.items()} } prompt {len(prompt)}"
    try:
        xs = [(float(rng.choice([1.0, 3.0])) * rng.standard_normal(vocab)).astype(np.float32) for _ in range(3)]
        for x in xs:
            x[edge] += np.float32(4.0)
            x[small] += np.float32(5.0)
        if host:
            A, B = hip.sampler(vocab, seed=k, **kw), hip.sampler(vocab, seed=k, **kw)
            for s in (A, B):
                if miro:
                    s.set_mirostat(*miro)
            A.set_constraints(**cfg)
            gen = list(prompt)
            for i in range(12):
                y = cr.apply(xs[i % 3], cfg, len(gen), gen)
                edited += y.tobytes() != xs[i % 3].tobytes()
                a, b = A.sample_host(xs[i % 3], gen), B.sample_host(y, gen)
                assert a == b and A.draws() == B.draws() and A.mirostat_state() == B.mirostat_state(), ("step", i, a, b)
                gen.append(a)
            A.close(); B.close()
        else:
            A, B = tc.Lane(torch, hip, vocab, kw, miro, prompt, seed=k), tc.Lane(torch, hip, vocab, kw, miro, prompt, seed=k)
            A.smp.set_constraints(**cfg)
            for i in range(12):
                y = cr.apply(xs[i % 3], cfg, A.smp.chosen(), A.seq())
                edited += y.tobytes() != xs[i % 3].tobytes()
                A.step(xs[i % 3]); B.step(y)
                tc.assert_same(A, B, ("step", i))
            assert A.smp.chosen() == 12
            A.close(); B.close()
    except BaseException as e:  # noqa: BLE001
        if isinstance(e, (KeyboardInterrupt, SystemExit)):
            raise
        bad += 1
        print("FAIL", what, repr(e)[:600], flush=True)
print(f"{edited} of {12 * n_cases} rows were changed by their constraints", flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
