"""What the wide decode step buys (Decoder::step_wide): aggregate tokens per second of M live sequences stepped through ONE matrix forward per
step against the same members stepped through BatchDecoder in ceil(M / 8) groups of 8 (unchanged code: the number the parent commit gives in
the same sitting).  One process, HIP events, every route warmed, the routes alternated 5 times, medians.  Synthetic 2B-4T model as bench.py
builds it (30 layers), both formats, f16 KV cache, digits 2.

    python3 tools/perf_wide.py [all|trace] [qk256,i2s] [layers = 30] [json path = profiles/wide_summary.json]

  all:   64 members (one owner of the weights + borrowers), each from its own 128-token prompt, all filled by ONE prefill_packed; 32 timed steps
         per route from position 128 (rewind(128) between routes: the same context for all).  Route A = step_wide(members[:M], 32) for M in
         {8, 16, 32, 64}; route B = the same members in ceil(M / 8) batches of 8, batch.step(32) on its captured graph one group after the other
         (the sum of the groups' event times).  Reported per M: ms per step, aggregate tok/s of both routes, their ratio, and the crossover M
         (the smallest M at which the wide step is ahead).  Then M = 64 with every member sampling (top-k 40) and its logits tap on: what the
         per-member sampler and logprob launches add to a step.
         Floor (profiles/wide_summary.json): at M = 64 the wide step's aggregate tok/s is at least 2 x the grouped batch route's.
  trace: 64 members, one warm-up call and 32 steps, nothing else -- for `rocprofv3 --kernel-trace --stats -- python3 tools/perf_wide.py trace
         qk256` (the per-kernel table of EXPERIMENTS.md 21: where an M = 64 step goes, and how much of it is the many-row matmuls at 64 rows)."""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256,i2s").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "wide_summary.json")
PROMPT, STEPS, REPS, MS, WIDE, GROUP = 128, 32, 5, (8, 16, 32, 64), 64, 8
med = statistics.median
result = {"layers": layers, "prompt": PROMPT, "steps": STEPS, "kv_cache": "f16", "digits": 2, "reps": REPS, "timing": "HIP events, ms", "formats": {}}
for fmt in fmts:
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512; cfg.n_layers = layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        owner.set_layer_qk256(l, w) if fmt == "qk256" else owner.set_layer_i2s(l, w, 32)
    owner.set_globals(synth.make_globals(cfg))
    owner.set_kv_f16(True)
    decs = [owner] + [owner.shared() for _ in range(WIDE - 1)]
    for d in decs[1:]:
        d.set_kv_f16(True)
    prompt = synth.prompt(PROMPT + WIDE, cfg.vocab)
    for i, d in enumerate(decs):
        d.feed(prompt[i:i + PROMPT])
    fill_ms = owner.prefill_packed(decs, [PROMPT] * WIDE, with_logits=True, digits=2)  # position 128, the picked token at history[128]
    print(fmt, "fill: prefill_packed of", WIDE, "x", PROMPT, "tokens:", round(fill_ms, 2), "ms", flush=True)

    def back(ds):
        for d in ds:
            d.rewind(PROMPT)

    def route_wide(M):
        ms = owner.step_wide(decs[:M], STEPS, digits=2)
        back(decs[:M])
        return ms

    if mode == "trace":
        route_wide(WIDE)
        ms = route_wide(WIDE)
        print(fmt, "trace:", WIDE, "members,", STEPS, "steps:", round(ms / STEPS, 4), "ms per step", flush=True)
        for d in reversed(decs):
            d.close()
        continue

    batches = [pkg.HostBatch(GROUP) for _ in range(WIDE // GROUP)]
    for g, batch in enumerate(batches):  # group g holds members 8 g .. 8 g + 7 for the whole sitting (members may sit in slots under a wide step)
        for b in range(GROUP):
            batch.set_slot(b, decs[GROUP * g + b])

    def route_batch(M):
        ms = sum(batches[g].step(STEPS, use_graph=True) for g in range(M // GROUP))
        back(decs[:M])
        return ms

    for M in MS:
        route_wide(M); route_batch(M)  # every route warmed (buffers grown, kernels loaded, graphs captured)
    t_w, t_b = {M: [] for M in MS}, {M: [] for M in MS}
    for _ in range(REPS):
        for M in MS:
            t_w[M].append(route_wide(M))
            t_b[M].append(route_batch(M))
    r = {"fill_packed_ms": round(fill_ms, 2), "path": owner.last_prefill_path(), "saturation_fallbacks": owner.saturation_fallbacks(), "members": {}}
    for M in MS:
        w, b = med(t_w[M]), med(t_b[M])
        r["members"][str(M)] = {"wide_ms_per_step": round(w / STEPS, 4), "wide_tok_s": round(M * STEPS / w * 1e3, 1), "batch_groups": M // GROUP,
                                "batch_ms_per_step": round(b / STEPS, 4), "batch_tok_s": round(M * STEPS / b * 1e3, 1), "ratio": round(b / w, 3),
                                "wide_ms_all": [round(x, 2) for x in t_w[M]], "batch_ms_all": [round(x, 2) for x in t_b[M]]}
    ahead = [M for M in MS if r["members"][str(M)]["ratio"] >= 1.0]
    r["crossover_members"] = min(ahead) if ahead else None
    # ---- what the per-member launches cost: every member of 64 sampling (top-k 40) with its logits tap on ----
    for i, d in enumerate(decs):
        d.set_sampling(0.8, top_k=40, top_p=0.95, seed=100 + i); d.set_logprobs(5)
    route_wide(WIDE)
    t_s = [route_wide(WIDE) for _ in range(REPS)]
    for d in decs:
        d.set_sampling(None); d.set_logprobs(None)
    greedy = med(t_w[WIDE]) / STEPS
    r["sampling_64"] = {"wide_ms_per_step": round(med(t_s) / STEPS, 4), "greedy_ms_per_step": round(greedy, 4),
                        "per_member_launches_ms_per_step": round(med(t_s) / STEPS - greedy, 4), "ms_all": [round(x, 2) for x in t_s]}
    print(fmt, r, flush=True)
    result["formats"][fmt] = r
    for batch in batches:
        for b in range(GROUP):
            batch.set_slot(b, None)
        batch.close()
    for d in reversed(decs):
        d.close()
if mode != "trace":
    ratios = {f: result["formats"][f]["members"][str(WIDE)]["ratio"] for f in result["formats"]}
    result["acceptance"] = {"case": "64 members, 32 steps from position 128: aggregate tok/s of step_wide over 8 BatchDecoder groups of 8, same sitting",
                            "floor_ratio": 2.0, "measured_ratio": ratios, "met": all(x >= 2.0 for x in ratios.values())}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
