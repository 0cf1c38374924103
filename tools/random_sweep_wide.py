"""Developer tool (GPU box): Decoder::step_wide at random (model A / B, storage format, cache type, digits 2..4, 1..64 members at random positions,
1..3 steps, some members sampling) with the gates of tests/test_step_wide_gpu.py, whose helpers it drives: every member's position, the slots the
call did not own bit for bit, the cache against the float64 forward at rel <= 4 u_l (+ 2^-11 with an f16 cache), the first step's logits at cosine
>= 0.9999 (greedy members: the reference's own continuation is fed, so every step's), and n steps in one call against n calls on twins bit for bit.
python tools/random_sweep_wide.py [n] [seed]"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_decoder_state_gpu as ds
import test_step_wide_gpu as tw
from oracle import oracle as orc
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
orc.build()
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 29)
worlds, bad = {}, 0
for case in range(n_cases):
    model, fmt = ("A", "B")[int(rng.integers(0, 2))], ("i2s", "qk256")[int(rng.integers(0, 2))]
    kv16, digits, n_steps = bool(rng.integers(0, 2)), int(rng.integers(2, 5)), int(rng.integers(1, 4))
    M = int(rng.choice([1, 2, 8, 9, 17, 33, 64, int(rng.integers(1, 65))])) if model == "A" else int(rng.choice([1, 3, 9, int(rng.integers(1, 18))]))
    W = worlds.setdefault((model, fmt), ds.World(synth, orc, model, fmt))
    top = W.cfg.max_pos - 1 - ds.STEPS  # the reference sequence is the forced tokens + STEPS greedy ones (n_steps <= STEPS)
    pos = [int(rng.choice([0, 1, 63, 64, 65, 127, 128, int(rng.integers(0, top))])) for _ in range(M)]
    if M == 1 and pos[0] == 0:
        pos[0] = 33
    what = f"{model} {fmt} kv16={kv16} digits={digits} steps={n_steps} M={M} pos={pos}"
    try:
        forced = [tw.tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
        refs = [W.seq(f) for f in forced]
        ms, twins = tw.group(pkg, W, kv16, M), tw.group(pkg, W, kv16, M)
        sampling = [i for i in range(M) if rng.integers(0, 8) == 0]
        for g in (ms, twins):
            for i in sampling:
                g[i].set_sampling(0.9, top_k=40, seed=100 + i)
            for m, (toks, _, _), p in zip(g, refs, pos):  # the whole reference sequence is fed: a greedy member's picks are forced tokens
                m.reset(); m.feed(toks)
            live = [(m, p) for m, p in zip(g, pos) if p > 0]
            if live:
                live[0][0].prefill_packed([m for m, _ in live], [p for _, p in live], with_logits=False, digits=2)
        before = [ds.snapshot(m, W, kv16) for m in ms]
        ms[0].step_wide(ms, n_steps, digits=digits)
        for _ in range(n_steps):
            twins[0].step_wide(twins, 1, digits=digits)
        for i, (m, t, p) in enumerate(zip(ms, twins, pos)):
            toks, ref, u = refs[i]
            assert m.position() == p + n_steps, (i, m.position())
            snap = ds.snapshot(m, W, kv16)
            ds.check_untouched(snap, before[i], p, p + n_steps, f"member {i}")
            ds.check_values(W, snap, ref, u, kv16, slice(0, p + n_steps), "wide sweep", f"member {i}")
            c = ds.cosine(m.last_logits(), ref.logits[p + n_steps - 1])
            assert c >= 0.9999, (i, "logits cosine", c)
            assert list(m.history(p + n_steps)) == [int(x) for x in toks[:p + n_steps]], (i, "history")
            tw.assert_same(tw.state(m, W.cfg, kv16), tw.state(t, W.cfg, kv16), f"member {i}: {n_steps} steps in one call against {n_steps} calls")
        tw.close(ms); tw.close(twins)
        ok, err = True, ""
    except BaseException as e:  # noqa: BLE001 (pytest.fail raises outside Exception)
        if isinstance(e, (KeyboardInterrupt, SystemExit)):
            raise
        ok, err = False, repr(e)[:600]
    if not ok:
        bad += 1
        print("FAIL", what, err, flush=True)
print(f"{n_cases - bad}/{n_cases} cases agree", flush=True)
sys.exit(1 if bad else 0)
