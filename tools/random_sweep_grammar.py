"""Developer tool (GPU box): the sampler's GRAMMAR stage at random -- vocabulary, path (greedy, one-lane top-k, full vocabulary, Mirostat), the
automaton (states, classes, ban density), start state, prompt, seed; sample_dev or sample_host -- through the equivalence of
tests/test_grammar_gpu.py: a sampler with the grammar on the raw rows against one without it on the rows edited by tests/grammar_ref.py, 12
steps, every word equal, and the device's (state, steps, violations) equal to the restatement's.  python tools/random_sweep_grammar.py [n] [seed]"""
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grammar_cases as gc
import grammar_ref as gr
import test_constraint_gpu as tc
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 37)
bad = edited = 0
paths = list(tc.PATHS)
for k in range(n_cases):
    vocab = int(rng.choice([1, 2, 3, 63, 64, 65, 257, 1024, 1025, 2049, 4097, 32000, 50257, int(rng.integers(1, 70000))]))
    path = paths[int(rng.integers(0, len(paths)))]
    kw, miro = tc.PATHS[path]
    S = int(rng.integers(3, 40))
    C_ = int(rng.choice([1, 2, 31, 32, 33, 64, 65, 1000, int(rng.integers(1, 4000))]))
    p_ban = float(rng.choice([0.0, 0.1, 0.5, 0.9, 0.99]))
    edge = gc.edge_ids(vocab)
    desc, single = gr.random_automaton(rng, S, C_, vocab, p_ban, pinned=edge)
    start = int(rng.choice([0, S - 1, S - 2, int(rng.integers(0, S))]))
    prompt = [int(t) for t in rng.integers(0, vocab, int(rng.integers(0, 24)))]
    host = bool(rng.integers(0, 4) == 0)
    what = f"vocab {vocab} {path} host={host} states {S} classes {C_} p_ban {p_ban} start {start} prompt {len(prompt)}"
    g = None
    try:
        xs = [(float(rng.choice([1.0, 3.0])) * rng.standard_normal(vocab)).astype(np.float32) for _ in range(3)]
        for x in xs:
            x[edge] += np.float32(4.0)
        g = hip.grammar(*desc)
        if host:
            A, B = hip.sampler(vocab, seed=k, **kw), hip.sampler(vocab, seed=k, **kw)
            for s in (A, B):
                if miro:
                    s.set_mirostat(*miro)
            A.set_grammar(g, start)
            gen = list(prompt)
            for i in range(12):
                st = gr.walk(desc, start, gen)
                assert g.walk(start, gen) == st
                y = gr.apply(xs[i % 3], desc, st[0])
                edited += y.tobytes() != xs[i % 3].tobytes()
                a, b = A.sample_host(xs[i % 3], gen), B.sample_host(y, gen)
                assert a == b and A.draws() == B.draws() and A.mirostat_state() == B.mirostat_state(), ("step", i, a, b)
                gen.append(a)
            assert A.grammar_state() == (start, 0, 0)
            A.close(); B.close()
        else:
            A, B = tc.Lane(torch, hip, vocab, kw, miro, prompt, seed=k), tc.Lane(torch, hip, vocab, kw, miro, prompt, seed=k)
            A.smp.set_grammar(g, start)
            s, steps, viol = start, 0, 0
            for i in range(12):
                assert A.smp.grammar_state() == (s, steps, viol), ("words before step", i)
                y = gr.apply(xs[i % 3], desc, s)
                edited += y.tobytes() != xs[i % 3].tobytes()
                A.step(xs[i % 3]); B.step(y)
                tc.assert_same(A, B, ("step", i))
                n = gr.step(desc, s, int(A.tok.item()))
                if n >= 0:
                    s, steps = n, steps + 1
                else:
                    viol += 1
            assert A.smp.grammar_state() == (s, steps, viol)
            A.close(); B.close()
    except BaseException as e:  # noqa: BLE001
        if isinstance(e, (KeyboardInterrupt, SystemExit)):
            raise
        bad += 1
        print("FAIL", what, repr(e)[:600], flush=True)
    if g is not None:
        g.close()
print(f"{edited} of {12 * n_cases} rows were changed by their grammar's mask", flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
