"""What the logits tap (Decoder::set_logprobs, csrc/kernels_logprob.hip) costs per decode step, on the synthetic 2B-4T model as bench.py builds it
(30 layers, f32 KV cache), each configuration with logprobs off, at top_n = 0 and at top_n = 20:

  batch-1: run(256) on the captured graphs from a 128-token prompt, greedy; and the same with the sampler on (S: 0.7, 40, 0.95, 1.1) and the tap
           off -- what the existing sampling launch adds, measured in the same sitting;
  batch:   an 8-member HostBatch.step(256), the members forked from one 128-token prompt;
  kernel:  the isolated kernel at vocab 128256 under HIP events (1000 launches back to back, random-normal row), beside bitnet_hip_sample_dev (S).

One process, every route warmed, the routes alternated 5 times, medians.  The partition's workgroup count can be overridden for the nwg choice
(EXPERIMENTS.md 19): BITNET_HIP_LOGPROB_WGS=16|32|64|128 python3 tools/perf_logprobs.py kernel

    python3 tools/perf_logprobs.py [all|kernel] [qk256,i2s] [layers = 30] [json path = profiles/logprobs_summary.json]"""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256,i2s").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "logprobs_summary.json")
PROMPT, STEPS, REPS, B = 128, 256, 5, 8
S = (0.7, 40, 0.95, 1.1)
med = statistics.median
result = {"layers": layers, "prompt": PROMPT, "steps": STEPS, "kv_cache": "f32", "reps": REPS, "logprob_wgs": os.environ.get("BITNET_HIP_LOGPROB_WGS", "default")}


def kernel_times():
    V, N = 128256, 1000
    logits = torch.from_numpy(np.random.default_rng(1).standard_normal(V).astype(np.float32)).cuda()
    pos = torch.zeros(1, dtype=torch.int32, device="cuda"); hist = torch.zeros(8, dtype=torch.int32, device="cuda")
    recs = torch.zeros(4 * 176, dtype=torch.uint8, device="cuda"); scratch = torch.zeros(hip.logprob_scratch_bytes(V), dtype=torch.uint8, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    sampler = hip.sampler(V, *S, seed=3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(REPS):
            e0.record()
            for _ in range(N):
                fn()
            e1.record(); torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / N)
        return round(med(runs), 2)

    out = {}
    for top_n in (0, 1, 5, 20):
        a = pkg.LogprobArgs.make(logits, pos, hist, recs, scratch, 4, top_n)
        out[f"logprob_top{top_n}_us"] = timed(lambda: hip.logprob_dev(a, V))
    out["sample_S_us"] = timed(lambda: sampler.sample_dev(logits, tok))
    sampler.close()
    return out


result["kernel_vocab_128256"] = kernel_times()
print("kernel", result["kernel_vocab_128256"], flush=True)
if mode == "all":
    result["formats"] = {}
    for fmt in fmts:
        cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512; cfg.n_layers = layers
        owner = pkg.HostDecoder(cfg)
        for l in range(cfg.n_layers):
            w = synth.make_layer(cfg, l, fmt=fmt, block=32)
            owner.set_layer_qk256(l, w) if fmt == "qk256" else owner.set_layer_i2s(l, w, 32)
        owner.set_globals(synth.make_globals(cfg))
        prompt = synth.prompt(PROMPT, cfg.vocab)
        members = [owner.shared() for _ in range(B)]
        # batch-1: one decoder per route, so that no route drops another's graphs
        solo = {"off": (None, None), "top0": (None, 0), "top20": (None, 20), "S_off": (S, None), "S_top20": (S, 20)}
        solo_dec = {k: owner.shared() for k in solo}
        for k, (sampling, top_n) in solo.items():
            solo_dec[k].set_sampling(*sampling, seed=7) if sampling else solo_dec[k].set_sampling(None)
            solo_dec[k].set_logprobs(top_n)

        def run_solo(k):
            d = solo_dec[k]
            d.reset(); d.feed(prompt); d.prefill(PROMPT, with_logits=True, digits=2)
            return d.run(STEPS, with_logits=True, use_graph=True)

        owner.feed(prompt); owner.prefill(PROMPT, with_logits=True, digits=2)
        batches = {k: pkg.HostBatch(B) for k in ("off", "top0", "top20")}

        def run_batch(k):
            for m in members:
                m.set_logprobs({"off": None, "top0": 0, "top20": 20}[k])
            owner.fork_into(members, PROMPT - 1)
            for b, m in enumerate(members):
                batches[k].set_slot(b, m)
            ms = batches[k].step(STEPS, use_graph=True)
            for b in range(B):
                batches[k].set_slot(b, None)
            return ms

        routes = [("solo", k) for k in solo] + [("batch", k) for k in batches]
        fn = {"solo": run_solo, "batch": run_batch}
        for kind, k in routes:
            fn[kind](k)  # warmed: graphs captured
        times = {r: [] for r in routes}
        for _ in range(REPS):
            for r in routes:
                times[r].append(fn[r[0]](r[1]))
        res = {}
        for kind in ("solo", "batch"):
            base = med(times[(kind, "off")]) / STEPS
            res[kind] = {}
            for (kd, k) in routes:
                if kd != kind:
                    continue
                m = med(times[(kd, k)]) / STEPS
                res[kind][k] = {"ms_per_step": round(m, 4), "added_us": round((m - base) * 1e3, 2), "ms_all": [round(x, 2) for x in times[(kd, k)]]}
            print(fmt, kind, {k: (v["ms_per_step"], v["added_us"]) for k, v in res[kind].items()}, flush=True)
        result["formats"][fmt] = res
        for b in batches.values():
            b.close()
        for d in members + list(solo_dec.values()) + [owner]:
            d.close()
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
