"""What Mirostat v2 on the device costs, against two launches of the SAME build, and against the host route it replaces.

    python3 tools/perf_mirostat.py [launch|decode|host|all] [json path = profiles/mirostat_summary.json]

  launch: the isolated k_sample launch at vocabulary 128256 over one sigma-4 row: Mirostat (tau 5, eta 0.1, temperature 0.7) against plain
          temperature sampling on path F (0.7, top-k 0, top-p 1) and top-k 0 / top-p 0.9 on path F.  A captured graph of 128
          bitnet_hip_sample_dev launches per config, replayed 9 times after a warm-up, HIP events around each replay, the configs alternated
          replay by replay.  us per launch: median, and the spread (max - min) / median of the 9.
  decode: the batch-1 decode step (Decoder::run, 64 graph-replayed steps) and the 8-member batched step (HostBatch.step, 64 steps) of the
          synthetic 2B-4T model under the same three configs; medians of 5, alternated.
  host:   the route Mirostat on the device replaces, per token: a with-logits graph step, last_logits() (513 KB to the host), the numpy
          restatement (tests/mirostat_ref.py) as a stand-in for a host sampler, feed() of its token; against the graph step with Mirostat on the
          device.  Wall clock per token over 32 tokens, median of 5; reported as a ratio, with the restatement's own share beside it."""
import importlib, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mirostat_summary.json")
hip = pkg.load(); hip.init(0)
VOCAB, LAUNCHES, REPLAYS = 128256, 128, 9
CONFIGS = {"temperature": ((0.7, 0, 1.0, 1.1), None), "top_p_0.9": ((0.7, 0, 0.9, 1.1), None), "mirostat": ((0.7, 0, 1.0, 1.1), (5.0, 0.1))}
med = statistics.median
result = {}


def launch_part():
    x = torch.from_numpy((4.0 * np.random.default_rng(1).standard_normal(VOCAB)).astype(np.float32)).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    routes = {}
    for name, (base, miro) in CONFIGS.items():
        smp = hip.sampler(VOCAB, *base, seed=7)
        if miro:
            smp.set_mirostat(*miro)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            smp.sample_dev(x, tok, stream=stream.cuda_stream)
            stream.synchronize()
            with torch.cuda.graph(g, stream=stream):
                for _ in range(LAUNCHES):
                    smp.sample_dev(x, tok, stream=stream.cuda_stream)
        routes[name] = (smp, g)
    times = {r: [] for r in routes}
    for rep in range(REPLAYS + 1):
        for r, (smp, g) in routes.items():
            smp.reset()  # every replay starts from empty counts and mu = 2 * tau: the same work each time
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record(); torch.cuda.synchronize()
            if rep:
                times[r].append(1000 * a.elapsed_time(b) / LAUNCHES)
    out = {}
    for name, t in times.items():
        out[name] = {"us_per_launch": round(med(t), 2), "spread": round((max(t) - min(t)) / med(t), 4), "all": [round(v, 2) for v in t]}
        if name == "mirostat":
            out[name]["state_after_128"] = routes[name][0].mirostat_state()
        print(name, out[name], flush=True)
    for smp, _ in routes.values():
        smp.close()
    return out


def model():
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    owner.set_globals(synth.make_globals(cfg))
    return cfg, owner


def configure(d, name, seed):
    base, miro = CONFIGS[name]
    d.set_mirostat(None)
    d.set_sampling(*base, seed=seed)
    if miro:
        d.set_mirostat(*miro)


def decode_part():
    PROMPT, STEPS, REPS = 128, 64, 5
    cfg, owner = model()
    owner.feed(synth.prompt(PROMPT, cfg.vocab))
    owner.prefill(PROMPT, with_logits=True, digits=2)
    members = [owner.shared() for _ in range(8)]

    def route(batch, B, name):
        for b in range(B):
            configure(members[b], name, 1000 + b)
        owner.fork_into(members[:B], PROMPT - 1)
        for b in range(B):
            batch.set_slot(b, members[b])
        ms = batch.step(STEPS, use_graph=True)
        for b in range(B):
            batch.set_slot(b, None)
        return ms

    routes = [(B, name) for B in (1, 8) for name in CONFIGS]
    batches = {r: pkg.HostBatch(r[0]) for r in routes}
    for r in routes:
        route(batches[r], *r)
    times = {r: [] for r in routes}
    solo = {name: [] for name in CONFIGS}
    for _ in range(REPS + 1):
        for r in routes:
            times[r].append(route(batches[r], *r) / STEPS)
        for name in CONFIGS:  # the batch-1 decoder's own graphs (Decoder::run)
            d = members[0]
            configure(d, name, 1000)
            owner.fork_into([d], PROMPT - 1)
            solo[name].append(d.run(STEPS, with_logits=True, use_graph=True) / STEPS)
    out = {}
    for name in CONFIGS:
        t = solo[name][1:]  # the first pass captures
        out[f"decoder_run/{name}"] = {"ms_per_step": round(med(t), 4), "spread": round((max(t) - min(t)) / med(t), 4)}
    for (B, name), t in times.items():
        t = t[1:]
        out[f"batch{B}/{name}"] = {"ms_per_step": round(med(t), 4), "spread": round((max(t) - min(t)) / med(t), 4)}
    for k, v in out.items():
        print(k, v, flush=True)
    for b in batches.values():
        b.close()
    for d in members + [owner]:
        d.close()
    return out


def host_part():
    import mirostat_ref as mr
    PROMPT, TOKENS, REPS = 32, 32, 5
    cfg, dec = model()
    prompt = synth.prompt(PROMPT, cfg.vocab)
    dev, host, share = [], [], []
    for rep in range(REPS + 1):
        configure(dec, "mirostat", 5)
        dec.reset(); dec.feed(prompt); dec.run(PROMPT - 1, with_logits=False, use_graph=True)
        t0 = time.perf_counter()
        dec.run(TOKENS, with_logits=True, use_graph=True)
        dec.position()
        dev.append((time.perf_counter() - t0) / TOKENS)
        # the host route: the greedy full head gives the logits, the host samples, feed() puts its token where the next step reads it
        dec.set_mirostat(None); dec.set_sampling(None)
        ref = mr.MirostatRef(5.0, 0.1, seed=5, temperature=0.7, repetition_penalty=1.1)
        dec.reset(); dec.feed(prompt); dec.run(PROMPT - 1, with_logits=False, use_graph=True)
        gen, in_ref = [], 0.0
        t0 = time.perf_counter()
        for _ in range(TOKENS):
            dec.run(1, with_logits=True, use_graph=True)
            logits = dec.last_logits()
            t1 = time.perf_counter()
            tok = ref.sample(logits, gen)
            in_ref += time.perf_counter() - t1
            gen.append(tok)
            dec.feed([tok])
        host.append((time.perf_counter() - t0) / TOKENS)
        share.append(in_ref / TOKENS)
    dev, host, share = dev[1:], host[1:], share[1:]
    out = {"device_ms_per_token": round(1000 * med(dev), 4), "host_route_ms_per_token": round(1000 * med(host), 4),
           "of_which_numpy_restatement_ms": round(1000 * med(share), 4), "ratio": round(med(host) / med(dev), 2),
           "ratio_without_the_restatement": round((med(host) - med(share)) / med(dev), 2)}
    print(out, flush=True)
    dec.close()
    return out


if mode in ("launch", "all"):
    result["launch"] = launch_part()
if mode in ("decode", "all"):
    result["decode"] = decode_part()
if mode in ("host", "all"):
    result["host_route"] = host_part()
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
