"""What the stop criteria on the device cost per step, and what queueing chunks buys against the route it replaces.

    python3 tools/perf_stop.py [launch|decode|generate|wasted|all] [json path = profiles/stop_summary.json]

  launch:   the isolated k_stop launch: a captured graph of 128 bitnet_hip_stop_dev launches per config, replayed 9 times after a warm-up, HIP
            events around each replay, the configs alternated replay by replay.  Configs: the empty config; 32 stop ids with 16 sequences of 32
            tokens (none matching: every launch does the whole comparison).  us per launch: median, and the spread (max - min) / median.
  decode:   the batch-1 decode step (Decoder::run, 64 graph-replayed greedy steps) and the 8-member batched step (HostBatch.step, 64 steps) of the
            synthetic 2B-4T model with the criteria off, the empty config, and the full config; medians of 5, alternated.
  generate: generate(256, chunk) for chunk 1, 4, 16 and 64 (criteria that never hold: all 256 steps run) against the route it replaces --
            run(1) plus a read-back of the token per step -- by wall clock over 256 tokens, median of 5, alternated.
  wasted:   the mean number of frozen steps per request at each chunk size, stop steps uniform in 1..256: a count, computed on the CPU."""
import importlib, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stop_summary.json")
LAUNCHES, REPLAYS = 128, 9
FULL = dict(stop_ids=tuple(range(200000, 200032)), sequences=tuple(tuple(range(300000 + 40 * s, 300032 + 40 * s)) for s in range(16)))  # ids no vocabulary holds
CONFIGS = {"off": None, "empty": dict(), "32_ids_16x32_sequences": FULL}
CHUNKS = (1, 4, 16, 64)
med = statistics.median
result = {}


def stat(t, key, scale=1.0, digits=4):
    return {key: round(scale * med(t), digits), "spread": round((max(t) - min(t)) / med(t), 4), "all": [round(scale * v, digits) for v in t]}


def launch_part():
    hip = pkg.load(); hip.init(0)
    stream = torch.cuda.Stream()
    routes = {}
    for name, cfg in CONFIGS.items():
        if cfg is None:
            continue
        stop = pkg.Stop(hip, **cfg)
        hist = torch.arange(4096, dtype=torch.int32, device="cuda")
        pos = torch.full((1,), 100, dtype=torch.int32, device="cuda")  # the position stays: every launch counts history[100] and compares
        nf = torch.zeros(1, dtype=torch.int32, device="cuda"); tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            stop.launch(pos, hist, 4096, nf, tok, stream=stream.cuda_stream)
            stream.synchronize()
            with torch.cuda.graph(g, stream=stream):
                for _ in range(LAUNCHES):
                    stop.launch(pos, hist, 4096, nf, tok, stream=stream.cuda_stream)
        routes[name] = (stop, g, (hist, pos, nf, tok))
    times = {r: [] for r in routes}
    for rep in range(REPLAYS + 1):
        for r, (stop, g, _) in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record(); torch.cuda.synchronize()
            if rep:
                times[r].append(1000 * a.elapsed_time(b) / LAUNCHES)
    out = {}
    for name, t in times.items():
        out[name] = stat(t, "us_per_launch", digits=2)
        out[name]["state"] = routes[name][0].state().astuple()
        print("launch", name, out[name], flush=True)
    return out


def model():
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    owner.set_globals(synth.make_globals(cfg))
    return cfg, owner


def configure(d, name):
    if CONFIGS[name] is None:
        d.set_stop(off=True)
    else:
        d.set_stop(**CONFIGS[name])


def decode_part():
    PROMPT, STEPS, REPS = 128, 64, 5
    cfg, owner = model()
    owner.feed(synth.prompt(PROMPT, cfg.vocab))
    owner.prefill(PROMPT, with_logits=True, digits=2)
    members = [owner.shared() for _ in range(8)]
    batches = {name: pkg.HostBatch(8) for name in CONFIGS}  # one batch per config: each keeps the chain it captured
    solo, batch = {n: [] for n in CONFIGS}, {n: [] for n in CONFIGS}
    for _ in range(REPS + 1):
        for name in CONFIGS:
            d = members[0]
            configure(d, name)
            owner.fork_into([d], PROMPT - 1)
            solo[name].append(d.run(STEPS, with_logits=True, use_graph=True) / STEPS)
        for name in CONFIGS:
            for m in members:
                configure(m, name)
            owner.fork_into(members, PROMPT - 1)
            for b, m in enumerate(members):
                batches[name].set_slot(b, m)
            batch[name].append(batches[name].step(STEPS, use_graph=True) / STEPS)
            for b in range(8):
                batches[name].set_slot(b, None)
    out = {}
    for name in CONFIGS:
        out[f"decoder_run/{name}"] = stat(solo[name][1:], "ms_per_step")  # the first pass captures
        out[f"batch8/{name}"] = stat(batch[name][1:], "ms_per_step")
    for k in ("decoder_run", "batch8"):
        for name in ("empty", "32_ids_16x32_sequences"):
            out[f"{k}/{name}"]["added_us"] = round(1000 * (out[f"{k}/{name}"]["ms_per_step"] - out[f"{k}/off"]["ms_per_step"]), 2)
    for k, v in out.items():
        print("decode", k, v, flush=True)
    for b in batches.values():
        b.close()
    for d in members + [owner]:
        d.close()
    return out


def generate_part():
    PROMPT, TOKENS, REPS = 32, 256, 5
    cfg, dec = model()
    prompt = synth.prompt(PROMPT, cfg.vocab)
    times = {f"generate_chunk{c}": [] for c in CHUNKS}
    times["run1_plus_token_readback"] = []

    def start(stop):
        dec.set_stop(**FULL) if stop else dec.set_stop(off=True)
        dec.reset(); dec.feed(prompt); dec.run(PROMPT - 1, with_logits=False, use_graph=True)
        dec.prepare_graphs(True)  # switching the criteria drops the graphs: capture outside the clock, for both routes

    for rep in range(REPS + 1):
        for c in CHUNKS:
            start(True)
            t0 = time.perf_counter()
            steps, _ = dec.generate(TOKENS, chunk=c)
            times[f"generate_chunk{c}"].append((time.perf_counter() - t0) / TOKENS)
            assert steps == TOKENS
        start(False)
        t0 = time.perf_counter()
        for i in range(TOKENS):
            dec.run(1, with_logits=True, use_graph=True)
            dec.history(PROMPT + i + 1)[-1]  # the host reads the token to decide
        times["run1_plus_token_readback"].append((time.perf_counter() - t0) / TOKENS)
    out = {k: stat(t[1:], "ms_per_token", scale=1000.0) for k, t in times.items()}
    base = out["run1_plus_token_readback"]["ms_per_token"]
    for c in CHUNKS:
        out[f"generate_chunk{c}"]["speedup_over_run1"] = round(base / out[f"generate_chunk{c}"]["ms_per_token"], 3)
    for k, v in out.items():
        print("generate", k, v, flush=True)
    dec.close()
    return out


def wasted_part():
    out = {}
    for c in CHUNKS:
        out[f"chunk{c}"] = round(float(np.mean([-(-k // c) * c - k for k in range(1, 257)])), 3)
    print("wasted (mean frozen steps per request, stop step uniform in 1..256)", out, flush=True)
    return out


if mode in ("launch", "all"):
    result["launch"] = launch_part()
if mode in ("decode", "all"):
    result["decode"] = decode_part()
if mode in ("generate", "all"):
    result["generate"] = generate_part()
if mode in ("wasted", "all"):
    result["wasted_steps"] = wasted_part()
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
