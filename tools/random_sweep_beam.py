"""Developer tool (GPU box): beam search on the device (HostBeamSearch: the batched step, bitnet_hip_beam_select_dev, bitnet_hip_kv_permute_dev) at a
random (model, format, cache type, n_beams, prompt length, budget, alpha, EOS, chunk) against the HOST-DRIVEN route of tests/test_beam_decoder_gpu.py
(two decoder sets, records read back, tests/beam_ref.py, fork, feed).  Equality: the ending, the hypotheses (tokens, score bits, key bits, order)
and every live beam's position, history and cache slots below the position.  The EOS of a case is a token the pilot run walked (or none).
python tools/random_sweep_beam.py [n] [seed]"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beam_ref as br
import test_batch_decoder_gpu as tb
import test_beam_decoder_gpu as td
pkg = importlib.import_module("bitnet-rs_amd")
synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 23)
MODELS = [dict(), dict(n_layers=1, n_kv_heads=1), dict(n_layers=3, n_heads=8, n_kv_heads=4, vocab=1000), dict(hidden=1024, ffn=1536, max_pos=300)]


class World(tb.World):
    def __init__(self, fmt, over):
        self.fmt = fmt
        self.cfg = cfg = synth.ModelConfig(**dict(tb.MODEL_A, **over))
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
        self.prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)


crews, bad = {}, 0
for case in range(n_cases):
    m, fmt, kv16 = int(rng.integers(0, len(MODELS))), str(rng.choice(["i2s", "qk256"])), bool(rng.integers(0, 2))
    B, budget, chunk = int(rng.integers(1, 9)), int(rng.integers(1, 13)), int(rng.integers(1, 7))
    alpha = float(rng.choice([0.0, 0.6, 1.0, 2.0]))
    if (m, fmt, kv16) not in crews:
        crews[(m, fmt, kv16)] = td.Crew(pkg, World(fmt, MODELS[m]), kv16)
    crew = crews[(m, fmt, kv16)]
    n_prompt = int(rng.choice([1, 2, 62, 63, 64, 65, 127, 128, 129, int(rng.integers(1, crew.W.cfg.max_pos - budget - 4))]))
    what = (MODELS[m], fmt, "f16" if kv16 else "f32", B, n_prompt, budget, alpha, chunk)
    try:
        members = crew.beams(B)
        crew.empty(crew.batch)
        for b, d in enumerate(members):
            d.reset()
            crew.batch.set_slot(b, d)
        bound = pkg.HostBeamSearch(crew.batch, B, -1, budget, alpha)
        lw = bound.len_weights()
        bound.close()
        eos = -1
        if rng.random() < 0.75:  # a token the search without an EOS walked: early ones end searches by the pool, late ones by the budget
            _, _, seen, _ = td.host_route(crew, B, n_prompt, -1, budget, lw)
            eos = seen[int(rng.integers(0, len(seen)))][2]
        ref, live, _, _ = td.host_route(crew, B, n_prompt, eos, budget, lw)
        search, members, _ = td.device_route(crew, B, n_prompt, eos, budget, alpha, chunk)
        st = search.state()
        assert st.done == ref.done and st.gen_len == ref.gen_len, ("ending", st.done, ref.done)
        assert td.hyps(search) == ref.hypotheses(), "hypotheses"
        td.assert_routes_equal(crew, members, live, "state")
        search.close()
        what += (eos, "pool" if ref.done & br.DONE_POOL else "budget")
        ok, err = True, ""
    except (AssertionError, pkg.BitNetHipError) as e:
        ok, err = False, repr(e)[:300]
    if not ok:
        bad += 1
        print("FAIL", what, err, flush=True)
for c in crews.values():
    c.close()
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
