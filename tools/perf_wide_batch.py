"""What WideBatch's one-launch tails buy (host/wide_batch.hpp): ms per step of M live sequences through the wide forward, by four routes in one
sitting -- Decoder::step_wide (unchanged code: the numbers the parent commit gives) and WideBatch.step, each with all-greedy members and with
every member sampling (top-k 40, top-p 0.95), its logits tap on (top_n 5) and stop criteria armed with a budget beyond the run.  The protocol
is tools/perf_wide.py's: one process, HIP events, every route warmed, the routes alternated 5 times, medians, every sample kept.  Synthetic
2B-4T model as bench.py builds it (30 layers), f16 KV cache, digits 2.

    python3 tools/perf_wide_batch.py [all|trace] [qk256,i2s] [layers = 30] [json path = profiles/wide_batch_summary.json]

  all:   two sets of 64 members on one owner's weights (set G greedy, set S sampling + tap + criteria), each member from its own 128-token
         prompt, each set filled by ONE prefill_packed; 32 timed steps per route from position 128 (rewind(128) between routes), M in
         {16, 32, 64}:  (a) step_wide, G   (b) step_wide, S   (c) WideBatch.step, S   (d) WideBatch.step, G.
         Reported per M: ms per step of each route, the tails (b) - (a) and (c) - (d), (d) against (a), and the sitting's spread (the largest
         (max - min) / median over the routes' five samples).
  trace: route (c) at 64 members, one warm-up call and 32 steps, nothing else -- for `rocprofv3 --kernel-trace --stats -- python3
         tools/perf_wide_batch.py trace qk256`."""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "wide_batch_summary.json")
PROMPT, STEPS, REPS, MS, WIDE = 128, 32, 5, (16, 32, 64), 64
med = statistics.median
result = {"layers": layers, "prompt": PROMPT, "steps": STEPS, "kv_cache": "f16", "digits": 2, "reps": REPS, "timing": "HIP events, ms",
          "routes": {"a": "step_wide, greedy", "b": "step_wide, sampling + tap + criteria", "c": "WideBatch.step, the members of b",
                     "d": "WideBatch.step, greedy"}, "formats": {}}
for fmt in fmts:
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512; cfg.n_layers = layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        owner.set_layer_qk256(l, w) if fmt == "qk256" else owner.set_layer_i2s(l, w, 32)
    owner.set_globals(synth.make_globals(cfg))
    owner.set_kv_f16(True)
    sets = {"G": [owner] + [owner.shared() for _ in range(WIDE - 1)], "S": [owner.shared() for _ in range(WIDE)]}
    prompt = synth.prompt(PROMPT + WIDE, cfg.vocab)
    for name, decs in sets.items():
        if name == "G" and mode == "trace":
            continue
        for i, d in enumerate(decs):
            d.set_kv_f16(True)
            d.feed(prompt[i:i + PROMPT])
        fill_ms = decs[0].prefill_packed(decs, [PROMPT] * WIDE, with_logits=True, digits=2)  # position 128, the picked token at history[128]
        print(fmt, name, "fill: prefill_packed of", WIDE, "x", PROMPT, "tokens:", round(fill_ms, 2), "ms", flush=True)
    for i, d in enumerate(sets["S"]):
        d.set_sampling(0.8, top_k=40, top_p=0.95, seed=100 + i); d.set_logprobs(5); d.set_stop(max_tokens=1 << 20)
    batches = {name: pkg.HostWideBatch(WIDE) for name in sets}

    def back(ds):
        for d in ds:
            d.rewind(PROMPT)  # (clears a stop and keeps the count: the budget lies beyond every run of the sitting)

    def members(name, M):  # the batch of set `name` holds its first M members
        for b in range(WIDE):
            batches[name].set_slot(b, sets[name][b] if b < M else None)

    def route(kind, M):
        name = "G" if kind in "ad" else "S"
        ds = sets[name][:M]
        ms = ds[0].step_wide(ds, STEPS, digits=2) if kind in "ab" else batches[name].step(STEPS, digits=2)
        back(ds)
        return ms

    if mode == "trace":
        members("S", WIDE)
        route("c", WIDE)
        ms = route("c", WIDE)
        print(fmt, "trace:", WIDE, "members,", STEPS, "steps:", round(ms / STEPS, 4), "ms per step; tail launches", batches["S"].tail_launches(), flush=True)
    else:
        t = {M: {k: [] for k in "abcd"} for M in MS}
        for M in MS:
            members("G", M); members("S", M)
            for k in "abcd":
                route(k, M)  # every route warmed (buffers grown, kernels loaded, tables built)
        for _ in range(REPS):
            for M in MS:
                members("G", M); members("S", M)
                route("c", M); route("d", M)  # (the tables follow the member count outside the timed part: one untimed call each)
                for k in "abcd":
                    t[M][k].append(route(k, M))
        r = {"saturation_fallbacks": owner.saturation_fallbacks(), "members": {}}
        for M in MS:
            m = {k: med(t[M][k]) / STEPS for k in "abcd"}
            spread = max((max(v) - min(v)) / med(v) for v in t[M].values())
            r["members"][str(M)] = {**{k + "_ms_per_step": round(v, 4) for k, v in m.items()}, "tail_step_wide_ms": round(m["b"] - m["a"], 4),
                                    "tail_wide_batch_ms": round(m["c"] - m["d"], 4), "d_over_a": round(m["d"] / m["a"], 4),
                                    "c_over_b": round(m["c"] / m["b"], 4), "spread": round(spread, 4),
                                    "ms_all": {k: [round(x, 2) for x in v] for k, v in t[M].items()}}
        r["tail_launches_c"] = list(batches["S"].tail_launches())
        print(fmt, r, flush=True)
        result["formats"][fmt] = r
    for name, batch in batches.items():
        for b in range(WIDE):
            batch.set_slot(b, None)
        batch.close()
    for d in reversed(sets["S"] + sets["G"]):
        d.close()
if mode != "trace":
    ok = {f: all(v["c_over_b"] < 1.0 - v["spread"] for v in result["formats"][f]["members"].values()) for f in result["formats"]}
    result["acceptance"] = {"d_equals_a_within_spread": {f: all(abs(v["d_over_a"] - 1.0) <= v["spread"] for v in result["formats"][f]["members"].values())
                                                         for f in result["formats"]}, "c_below_b_by_more_than_spread": ok}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
