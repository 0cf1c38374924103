"""What the sampler's CONSTRAINTS stage costs, as deltas over the same build with constraints off, and whether the off path moved.

    python3 tools/perf_constraints.py [launch|decode|all] [--parent-lib path/to/a/parent/libbitnet_hip.so]
                                       [--control-lib another/libbitnet_hip.so ...] [--json profiles/constraints_summary.json]

  launch: the isolated k_sample launch at vocabulary 128256 (temperature 0.7, top-p 0.9, repetition penalty 1.1: path F) over one sigma-4 row,
          with pos / history words and 4095 history tokens in front of the position:
            (a) constraints off; (b) 300 bias entries; (c) an allowed list of 10 ids; (d) no_repeat_ngram = 3; (e) all of these and a hold list.
          A captured graph of 64 bitnet_hip_sample_dev launches per config (the position is put back in front of every replay, so every launch
          of every replay scans the same 4095..4158 tokens), replayed 9 times after a warm-up, HIP events around each replay, the configs
          alternated replay by replay.  us per launch: median and (max - min) / median; (b)..(e) also as the delta over (a).
  gate:   with --parent-lib, (a) again through the parent commit's library and through this build's, both driven by the same raw ctypes calls
          in this process: five runs, each with a fresh sampler object and fresh device words per library (where the buffers land moves the
          launch by tenths of a microsecond), the libraries alternated replay by replay, the order of creation alternated run by run, 9
          replays per run.  The gate: the median of this build's five medians lies inside the min-max spread of the parent's five.  Exit
          status 1 if it does not.  Every --control-lib is measured the same way and only reported (the parent's library once more: what
          another object of the same code differs by).
  decode: the batch-1 graph step (Decoder::run, 64 replayed steps) of the synthetic 2B-4T model with (a) and (e); medians of 5, alternated."""
import ctypes as C
import importlib, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


parent_lib = opt("--parent-lib", None)
control_libs = []
while "--control-lib" in args:
    control_libs.append(opt("--control-lib", None))
out_path = opt("--json", os.path.join(ROOT, "profiles", "constraints_summary.json"))
mode = args[0] if args else "all"
hip = pkg.load(); hip.init(0)
VOCAB, LAUNCHES, REPLAYS, HIST = 128256, 64, 9, 4095
BASE = dict(temperature=0.7, top_k=0, top_p=0.9, repetition_penalty=1.1)
med = statistics.median
rng = np.random.default_rng(1)
ROW = (4.0 * rng.standard_normal(VOCAB)).astype(np.float32)
HISTORY = rng.integers(0, VOCAB, HIST + LAUNCHES + 8).astype(np.int32)
HISTORY[:HIST] = np.resize(rng.integers(0, 64, 37), HIST)  # a repeating prefix: the 3-gram block finds matches all along it
BIAS = {int(t): float(v) for t, v in zip(rng.choice(VOCAB, 300, replace=False), rng.uniform(-5, 5, 300))}
ALLOWED = [int(t) for t in np.argsort(ROW)[-10:]]
CONFIGS = {"a_off": None, "b_bias_300": dict(bias=BIAS), "c_allowed_10": dict(allowed=ALLOWED), "d_ngram_3": dict(no_repeat_ngram=3),
           "e_all": dict(bias=BIAS, allowed=ALLOWED, no_repeat_ngram=3, hold=[ALLOWED[-1], ALLOWED[-2]], min_tokens=1 << 30)}
result = {}


def words():
    return dict(x=torch.from_numpy(ROW).cuda(), tok=torch.zeros(1, dtype=torch.int32, device="cuda"),
                pos=torch.full((1,), HIST - 1, dtype=torch.int32, device="cuda"), hist=torch.from_numpy(HISTORY).cuda(),
                nf=torch.full((1,), HIST, dtype=torch.int32, device="cuda"))


def timed_replay(graph, w, reset):
    reset()
    w["pos"].fill_(HIST - 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); graph.replay(); b.record(); torch.cuda.synchronize()
    return 1000 * a.elapsed_time(b) / LAUNCHES


def capture(launch, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        launch(stream.cuda_stream)
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(LAUNCHES):
                launch(stream.cuda_stream)
    return g


def launch_part():
    stream = torch.cuda.Stream()
    routes = {}
    for name, con in CONFIGS.items():
        smp, w = hip.sampler(VOCAB, seed=7, **BASE), words()
        if con:
            smp.set_constraints(**con)
        g = capture(lambda s, smp=smp, w=w: smp.sample_dev(w["x"], w["tok"], w["pos"], w["hist"], w["nf"], stream=s), stream)
        routes[name] = (smp, w, g)
    times = {r: [] for r in routes}
    for rep in range(REPLAYS + 1):
        for r, (smp, w, g) in routes.items():
            t = timed_replay(g, w, smp.reset)  # every replay starts from empty counts: the same work each time
            if rep:
                times[r].append(t)
    out = {}
    for name, t in times.items():
        out[name] = {"us_per_launch": round(med(t), 2), "spread": round((max(t) - min(t)) / med(t), 4), "all": [round(v, 2) for v in t]}
        if name != "a_off":
            out[name]["delta_over_a_us"] = round(med(t) - med(times["a_off"]), 2)
        print(name, out[name], flush=True)
    for smp, _, _ in routes.values():
        smp.close()
    return out


class RawSampler:
    """the five calls (a) needs, through plain ctypes: the same driver for a parent commit's library and for this build's"""

    def __init__(self, path):
        self.c = C.CDLL(path)
        cfg = pkg.SamplingConfig.make(BASE["temperature"], BASE["top_k"], BASE["top_p"], BASE["repetition_penalty"], 7)
        self.h = C.c_void_p()
        self.c.bitnet_hip_sampler_create.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
        self.c.bitnet_hip_sample_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
        self.c.bitnet_hip_sampler_reset.argtypes = [C.c_void_p]
        self.c.bitnet_hip_sampler_destroy.argtypes = [C.c_void_p]
        self.c.bitnet_hip_sampler_destroy.restype = None
        assert self.c.bitnet_hip_sampler_create(VOCAB, C.byref(cfg), C.byref(self.h)) == 0
        self.w = words()

    def launch(self, stream):
        w = self.w
        rc = self.c.bitnet_hip_sample_dev(self.h, w["x"].data_ptr(), VOCAB, w["tok"].data_ptr(), w["pos"].data_ptr(), w["hist"].data_ptr(), w["nf"].data_ptr(), stream)
        assert rc == 0

    def reset(self):
        assert self.c.bitnet_hip_sampler_reset(self.h) == 0


def gate_part():
    """five runs per library, each run a FRESH sampler object with fresh device words (where its buffers land moves the launch by some tenths
    of a microsecond: the parent's library a second time shows it), the libraries alternating within a run and the order of creation
    alternating from run to run"""
    stream = torch.cuda.Stream()
    libs = {"parent": parent_lib, "this_build": hip.path}
    for i, path in enumerate(control_libs):  # measured the same way and only reported beside
        libs[f"control_{i}"] = path
    medians, toks = {k: [] for k in libs}, {}
    for run in range(5):
        order = list(libs) if run % 2 == 0 else list(libs)[::-1]
        sides = {k: RawSampler(libs[k]) for k in order}
        graphs = {k: capture(sides[k].launch, stream) for k in order}
        times = {k: [] for k in order}
        for rep in range(REPLAYS + 1):
            for k in order:
                t = timed_replay(graphs[k], sides[k].w, sides[k].reset)
                if rep:
                    times[k].append(t)
        for k in order:
            medians[k].append(med(times[k]))
            toks[k] = int(sides[k].w["tok"].item())
            sides[k].c.bitnet_hip_sampler_destroy(sides[k].h)
        del graphs, sides
    lo, hi = min(medians["parent"]), max(medians["parent"])
    mine = med(medians["this_build"])
    out = {"parent_medians_us": [round(v, 2) for v in medians["parent"]], "this_build_medians_us": [round(v, 2) for v in medians["this_build"]],
           "parent_min_max_us": [round(lo, 2), round(hi, 2)], "this_build_median_us": round(mine, 2), "parent_median_us": round(med(medians["parent"]), 2),
           "inside_the_parents_spread": bool(lo <= mine <= hi), "same_last_token": toks["parent"] == toks["this_build"]}
    for k in libs:
        if k.startswith("control"):
            out[k + "_medians_us"] = [round(v, 2) for v in medians[k]]
    print("gate", out, flush=True)
    return out


def decode_part():
    PROMPT, STEPS, REPS = 128, 64, 5
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 512
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        dec.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    dec.set_globals(synth.make_globals(cfg))
    prompt = synth.prompt(PROMPT, cfg.vocab)
    dec.set_sampling(seed=11, **BASE)
    times = {"a_off": [], "e_all": []}
    for rep in range(REPS + 1):
        for name in times:
            dec.set_constraints(**CONFIGS[name]) if CONFIGS[name] else dec.set_constraints()
            dec.reset(); dec.feed(prompt); dec.run(PROMPT - 1, with_logits=False, use_graph=True)
            times[name].append(dec.run(STEPS, with_logits=True, use_graph=True) / STEPS)
    out = {}
    for name, t in times.items():
        t = t[1:]  # the first pass captures
        out[f"decoder_run/{name}"] = {"ms_per_step": round(med(t), 4), "spread": round((max(t) - min(t)) / med(t), 4)}
    out["delta_e_over_a_us"] = round(1000 * (out["decoder_run/e_all"]["ms_per_step"] - out["decoder_run/a_off"]["ms_per_step"]), 2)
    for k, v in out.items():
        print(k, v, flush=True)
    dec.close()
    return out


if mode in ("launch", "all"):
    result["launch"] = launch_part()
    if parent_lib:
        result["gate"] = gate_part()
if mode in ("decode", "all"):
    result["decode"] = decode_part()
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
if "gate" in result and not result["gate"]["inside_the_parents_spread"]:
    sys.exit(1)
