"""What sampling costs inside a batched decode step (host/batch_decoder.hpp): B members forked from one 128-token prompt, 64 timed steps on the
captured chain, with every member greedy (the head's fused pick) and with every member sampling under one of three configs -- G penalised argmax
(1, 0, 1, 1.1), S top-k 40 (0.7, 40, 0.95, 1.1), F full-vocabulary top-p (0.7, 0, 0.95, 1.1), each member its own seed.  One process, HIP events,
every route warmed, the routes alternated 5 times, medians.  Synthetic 2B-4T model as bench.py builds it (30 layers), f32 KV cache.  Reported per
B and config: ms per step, and the sampling overhead = sampled step - all-greedy step of the same sitting.

The file uses nothing but HostDecoder / HostBatch calls that exist since the fork work, so the SAME file measures an older tree:

    python3 tools/perf_batch_sampling.py [all|trace] [qk256,i2s] [layers = 30] [json path = profiles/batch_sampling_summary.json]
    python3 tools/perf_batch_sampling.py merge this_tree.json parent_tree.json out.json

  all:   B in {1, 2, 4, 8}, the four configs; one HostBatch per (B, config), so no route re-captures another's chain.
  trace: 8 members under F, one warm-up and 64 steps, nothing else -- for `rocprofv3 --kernel-trace --stats -- python3 tools/perf_batch_sampling.py trace`.
  merge: the two trees' files of one sitting side by side, with the ratios EXPERIMENTS.md 18 quotes."""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
CONFIGS = {"greedy": None, "G": (1.0, 0, 1.0, 1.1), "S": (0.7, 40, 0.95, 1.1), "F": (0.7, 0, 0.95, 1.1)}
PROMPT, STEPS, REPS, BS = 128, 64, 5, (1, 2, 4, 8)

if mode == "merge":
    this, parent = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
    out = {k: this[k] for k in ("layers", "prompt", "steps", "kv_cache", "reps")}
    out["formats"] = {}
    for fmt in this["formats"]:
        t, p = this["formats"][fmt], parent["formats"][fmt]
        rows = {}
        for B in t:
            rows[B] = {"this_tree": t[B], "parent": p[B], "all_greedy_ratio_to_parent": round(t[B]["greedy"]["ms_per_step"] / p[B]["greedy"]["ms_per_step"], 4)}
            for c in ("G", "S", "F"):
                rows[B][f"overhead_{c}_parent_over_this"] = round(p[B][c]["overhead_us"] / max(t[B][c]["overhead_us"], 1e-3), 2)
        out["formats"][fmt] = rows
    with open(sys.argv[4], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    sys.exit(0)

sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256,i2s").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "batch_sampling_summary.json")
med = statistics.median
result = {"layers": layers, "prompt": PROMPT, "steps": STEPS, "kv_cache": "f32", "reps": REPS, "formats": {}}
for fmt in fmts:
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512; cfg.n_layers = layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        owner.set_layer_qk256(l, w) if fmt == "qk256" else owner.set_layer_i2s(l, w, 32)
    owner.set_globals(synth.make_globals(cfg))
    owner.feed(synth.prompt(PROMPT, cfg.vocab))
    owner.prefill(PROMPT, with_logits=True, digits=2)  # the one prompt forward every member starts from
    members = [owner.shared() for _ in range(max(BS))]

    def route(batch, B, name):
        """the members take the prompt's first 127 positions (one copy launch, samplers reset), join, step, leave: the same context for every route"""
        for b in range(B):
            members[b].set_sampling(None) if CONFIGS[name] is None else members[b].set_sampling(*CONFIGS[name], seed=1000 + b)
        owner.fork_into(members[:B], PROMPT - 1)
        for b in range(B):
            batch.set_slot(b, members[b])
        ms = batch.step(STEPS, use_graph=True)
        for b in range(B):
            batch.set_slot(b, None)
        return ms

    if mode == "trace":
        batch = pkg.HostBatch(8)
        route(batch, 8, "F")
        ms = route(batch, 8, "F")
        print(fmt, "trace: 8 members under F,", STEPS, "steps:", round(ms / STEPS, 4), "ms per step", flush=True)
        batch.close()
        for d in members + [owner]:
            d.close()
        continue

    routes = [(B, name) for B in BS for name in CONFIGS]
    batches = {r: pkg.HostBatch(r[0]) for r in routes}
    for r in routes:
        route(batches[r], *r)  # every route warmed (its chain captured)
    times = {r: [] for r in routes}
    for _ in range(REPS):
        for r in routes:
            times[r].append(route(batches[r], *r))
    res = {}
    for B in BS:
        g = med(times[(B, "greedy")]) / STEPS
        res[str(B)] = {}
        for name in CONFIGS:
            m = med(times[(B, name)]) / STEPS
            res[str(B)][name] = {"ms_per_step": round(m, 4), "overhead_us": round((m - g) * 1e3, 1), "ms_all": [round(x, 2) for x in times[(B, name)]]}
        print(fmt, "B =", B, {k: (v["ms_per_step"], v["overhead_us"]) for k, v in res[str(B)].items()}, flush=True)
    result["formats"][fmt] = res
    for b in batches.values():
        b.close()
    for d in members + [owner]:
        d.close()
if mode != "trace":
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
