"""What a batched decode step buys (host/batch_decoder.hpp): aggregate tokens per second of B sequences stepped through ONE launch chain against
batch-1 Decoder.run on its step graphs, one process, HIP events, every route warmed, the routes alternated 5 times, medians.
Synthetic 2B-4T model as bench.py builds it (30 layers), both formats, f32 KV cache.

    python3 tools/perf_batch.py [all|trace] [qk256,i2s] [layers = 30] [json path = profiles/batch_summary.json]

  all:   B in {1, 2, 4, 8} sequences (one owner of the weights + borrowers), each started from its own 128-token prompt through its own prefill;
         64 timed steps per route from position 128 (rewind(128) between routes: the same context for all).  Baseline = the owner's
         run(64, with_logits) on its captured step graphs, unchanged by the batch work.  Reported per B: ms per step, aggregate tok/s, the
         ratio to batch-1 run().
  trace: 8 sequences, one warm-up and 64 steps, nothing else -- for `rocprofv3 --kernel-trace --stats -- python3 tools/perf_batch.py trace`
         (the per-kernel table of EXPERIMENTS.md 16; profiles/batch_kernel_stats.csv is that run's kernel_stats file)."""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256,i2s").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "batch_summary.json")
PROMPT, STEPS, REPS, BS = 128, 64, 5, (1, 2, 4, 8)
med = statistics.median
result = {"layers": layers, "prompt": PROMPT, "steps": STEPS, "kv_cache": "f32", "reps": REPS, "formats": {}}
for fmt in fmts:
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512; cfg.n_layers = layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        owner.set_layer_qk256(l, w) if fmt == "qk256" else owner.set_layer_i2s(l, w, 32)
    owner.set_globals(synth.make_globals(cfg))
    n_seq = max(BS) if mode != "trace" else 8
    decs = [owner] + [owner.shared() for _ in range(n_seq - 1)]
    prompt = synth.prompt(PROMPT + 64, cfg.vocab)
    for i, d in enumerate(decs):
        d.feed(prompt[i:i + PROMPT])
        d.prefill(PROMPT, with_logits=True, digits=2)

    def back(ds):
        for d in ds:
            d.rewind(PROMPT)

    def route_batch(batch, B):
        for b in range(B):
            batch.set_slot(b, decs[b])
        ms = batch.step(STEPS, use_graph=True)
        for b in range(B):
            batch.set_slot(b, None)
        back(decs[:B])
        return ms

    if mode == "trace":
        batch = pkg.HostBatch(8)
        route_batch(batch, 8)
        ms = route_batch(batch, 8)
        print(fmt, "trace: 8 sequences,", STEPS, "steps:", round(ms / STEPS, 4), "ms per step", flush=True)
        batch.close()
        for d in reversed(decs):
            d.close()
        continue

    def route_run():
        ms = owner.run(STEPS, with_logits=True, use_graph=True)
        back([owner])
        return ms

    batches = {B: pkg.HostBatch(B) for B in BS}
    route_run()
    for B in BS:
        route_batch(batches[B], B)  # every route warmed (graphs captured)
    t_run, t_b = [], {B: [] for B in BS}
    for _ in range(REPS):
        t_run.append(route_run())
        for B in BS:
            t_b[B].append(route_batch(batches[B], B))
    base = STEPS / med(t_run) * 1e3
    r = {"run_ms_per_step": round(med(t_run) / STEPS, 4), "run_tok_s": round(base, 1), "run_ms_all": [round(x, 2) for x in t_run], "batch": {}}
    for B in BS:
        m = med(t_b[B])
        r["batch"][str(B)] = {"ms_per_step": round(m / STEPS, 4), "aggregate_tok_s": round(B * STEPS / m * 1e3, 1), "ratio_to_run": round(B * STEPS / m * 1e3 / base, 2),
                              "ms_all": [round(x, 2) for x in t_b[B]]}
    print(fmt, r, flush=True)
    result["formats"][fmt] = r
    for b in batches.values():
        b.close()
    for d in reversed(decs):
        d.close()
if mode != "trace":
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
