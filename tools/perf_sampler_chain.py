"""What the sampler chain (min-p, typical-p, frequency / presence penalty) costs, and that its neutral values cost nothing.

    python3 tools/perf_sampler_chain.py [launch|decode|all] [json path = profiles/sampler_chain_summary.json]

  launch: the isolated k_sample launch at vocabulary 128256 on paths S (0.7, top-k 40, 0.95, 1.1) and F (0.7, top-k 0, 0.95, 1.1): a captured
          graph of 128 bitnet_hip_sample_dev launches over one sigma-4 row, replayed 9 times after a warm-up, HIP events around each replay;
          the configs are alternated replay by replay.  us per launch: median, and the spread (max - min) / median of the 9.
  decode: the batch-1 decode step (Decoder::run, 64 graph-replayed steps) and the 8-member batched step (HostBatch.step, 64 steps) of the
          synthetic 2B-4T model, sampling under F with neutral values and with every stage switched on; medians of 5, alternated.

The neutral configs go through the entry points that exist since the sampler was added, and a tree without bitnet_hip_sampler_create_ex runs
them alone, so the SAME file measures the parent commit in the same sitting (copy it into that tree's tools/)."""
import importlib, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sampler_chain_summary.json")
hip = pkg.load(); hip.init(0)
HAS_EX = hasattr(pkg, "SamplingConfigEx")
VOCAB, LAUNCHES, REPLAYS = 128256, 128, 9
BASE = {"S": (0.7, 40, 0.95, 1.1), "F": (0.7, 0, 0.95, 1.1)}
STAGES = {"neutral": {}, "min_p": dict(min_p=0.05), "typical_p": dict(typical_p=0.9), "penalties": dict(frequency_penalty=0.2, presence_penalty=0.1),
          "all": dict(min_p=0.05, typical_p=0.9, frequency_penalty=0.2, presence_penalty=0.1)}
med = statistics.median
result = {"has_ex": HAS_EX}


def launch_part():
    x = torch.from_numpy((4.0 * np.random.default_rng(1).standard_normal(VOCAB)).astype(np.float32)).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    routes = {}
    for path, base in BASE.items():
        for name, ex in STAGES.items():
            if ex and not HAS_EX:
                continue
            smp = hip.sampler(VOCAB, *base, seed=7, **ex) if ex else hip.sampler(VOCAB, *base, seed=7)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(stream):
                smp.sample_dev(x, tok, stream=stream.cuda_stream)
                stream.synchronize()
                with torch.cuda.graph(g, stream=stream):
                    for _ in range(LAUNCHES):
                        smp.sample_dev(x, tok, stream=stream.cuda_stream)
            routes[(path, name)] = (smp, g)
    times = {r: [] for r in routes}
    for rep in range(REPLAYS + 1):
        for r, (smp, g) in routes.items():
            smp.reset()  # every replay starts from empty counts: the same work each time
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record(); torch.cuda.synchronize()
            if rep:
                times[r].append(1000 * a.elapsed_time(b) / LAUNCHES)
    out = {}
    for (path, name), t in times.items():
        out[f"{path}/{name}"] = {"us_per_launch": round(med(t), 2), "spread": round((max(t) - min(t)) / med(t), 4), "all": [round(v, 2) for v in t]}
        print(path, name, out[f"{path}/{name}"], flush=True)
    for smp, _ in routes.values():
        smp.close()
    return out


def decode_part():
    PROMPT, STEPS, REPS = 128, 64, 5
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    owner.set_globals(synth.make_globals(cfg))
    owner.feed(synth.prompt(PROMPT, cfg.vocab))
    owner.prefill(PROMPT, with_logits=True, digits=2)
    members = [owner.shared() for _ in range(8)]
    configs = {"neutral": {}}
    if HAS_EX:
        configs["all"] = STAGES["all"]

    def route(batch, B, name):
        for b in range(B):
            members[b].set_sampling(*BASE["F"], seed=1000 + b, **configs[name])
        owner.fork_into(members[:B], PROMPT - 1)
        for b in range(B):
            batch.set_slot(b, members[b])
        ms = batch.step(STEPS, use_graph=True)
        for b in range(B):
            batch.set_slot(b, None)
        return ms

    routes = [(B, name) for B in (1, 8) for name in configs]
    batches = {r: pkg.HostBatch(r[0]) for r in routes}
    for r in routes:
        route(batches[r], *r)
    times = {r: [] for r in routes}
    solo = {name: [] for name in configs}
    for _ in range(REPS):
        for r in routes:
            times[r].append(route(batches[r], *r) / STEPS)
        for name in configs:  # the batch-1 decoder's own graphs (Decoder::run)
            d = members[0]
            d.set_sampling(*BASE["F"], seed=1000, **configs[name])
            owner.fork_into([d], PROMPT - 1)
            solo[name].append(d.run(STEPS, with_logits=True, use_graph=True) / STEPS)
    out = {}
    for name in configs:
        t = solo[name][1:]  # the first pass captures
        out[f"decoder_run/{name}"] = {"ms_per_step": round(med(t), 4), "spread": round((max(t) - min(t)) / med(t), 4)}
    for (B, name), t in times.items():
        out[f"batch{B}/{name}"] = {"ms_per_step": round(med(t), 4), "spread": round((max(t) - min(t)) / med(t), 4)}
    for k, v in out.items():
        print(k, v, flush=True)
    for b in batches.values():
        b.close()
    for d in members + [owner]:
        d.close()
    return out


if mode in ("launch", "all"):
    result["launch"] = launch_part()
if mode in ("decode", "all"):
    result["decode"] = decode_part()
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
