"""What the sampler's GRAMMAR stage costs, what path F gained on masked rows, and whether the off path moved.

    python3 tools/perf_grammar.py [launch|decode|all] [--parent-lib path/to/a/parent/libbitnet_hip.so]
                                  [--control-lib another/copy/of/the/parent/libbitnet_hip.so] [--json profiles/grammar_summary.json]

  launch: the isolated k_sample launch at vocabulary 128256 (temperature 0.7, top-p 0.9, repetition penalty 1.1: path F) over one sigma-4 row.
          A captured graph of 64 bitnet_hip_sample_dev launches per config, replayed 9 times after a warm-up, HIP events around each replay, the
          configs alternated replay by replay in ONE sitting; us per launch, median and (max - min) / median:
            (a) grammar off, the raw row;
            (c) grammar off, the row pre-edited to -inf but for 10 ids (EXPERIMENTS.md 34.3's (c), whoever wrote the -inf);
            (g) a grammar state that allows the same 10 ids, the raw row;
            (h) a grammar state that bans 300 ids, the raw row: what the stage itself adds;
          and with --parent-lib, (a) and (c) through the parent commit's library in the same sitting.  Masked rows: (c) and (g) of this build
          must both be faster than the parent's (c) by more than the sitting's spread; exit status 1 if not.
  gate:   with --parent-lib, (a) through the parent's library and through this build's, the same raw ctypes driver for both, in this process:
          five runs, each with a fresh sampler object and fresh device words per library, the libraries alternated replay by replay, the
          order of creation alternated run by run, 9 replays per run; --control-lib, a second object of the parent, the same way.  The gate:
          this build's median of five is not slower than the parent's slowest run by more than the control's median differs from the
          parent's.  Exit status 1 if it is.  On these rows, and on (c), the last token, the history and the word counter through both
          libraries must be equal: path F's histogram change is bit-identical to the parent.
  decode: the batch-1 graph step (Decoder::run, 64 replayed steps) of the synthetic 2B-4T model with the grammar off and on (the 10-id
          state); medians of 5, alternated."""
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
control_lib = opt("--control-lib", None)
out_path = opt("--json", os.path.join(ROOT, "profiles", "grammar_summary.json"))
mode = args[0] if args else "all"
hip = pkg.load(); hip.init(0)
VOCAB, LAUNCHES, REPLAYS = 128256, 64, 9
BASE = dict(temperature=0.7, top_k=0, top_p=0.9, repetition_penalty=1.1)
med = statistics.median
rng = np.random.default_rng(1)
ROW = (4.0 * rng.standard_normal(VOCAB)).astype(np.float32)
TEN = np.sort(np.argsort(ROW)[-10:])
EDITED = np.full(VOCAB, -np.inf, np.float32)
EDITED[TEN] = ROW[TEN]
BAN300 = rng.choice(np.setdiff1d(np.arange(VOCAB), TEN), 300, replace=False)
result = {}
failed = []


def one_state(allowed=None, banned=None):
    """a one-state automaton: class 1 is allowed and stays in the state, class 0 is banned"""
    tc = np.zeros(VOCAB, np.uint16) if allowed is not None else np.ones(VOCAB, np.uint16)
    if allowed is not None:
        tc[allowed] = 1
    else:
        tc[banned] = 0
    return tc, np.array([[-1, 0]], np.int32)


class RawSampler:
    """the calls a timed sampler needs, through plain ctypes: the same driver for a parent commit's library and for this build's"""

    def __init__(self, path, row, grammar=None):
        self.c = c = C.CDLL(path)
        cfg = pkg.SamplingConfig.make(BASE["temperature"], BASE["top_k"], BASE["top_p"], BASE["repetition_penalty"], 7)
        self.h = C.c_void_p()
        c.bitnet_hip_sampler_create.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
        c.bitnet_hip_sample_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
        c.bitnet_hip_sampler_reset.argtypes = [C.c_void_p]
        c.bitnet_hip_sampler_draws.argtypes = [C.c_void_p, C.c_void_p]
        c.bitnet_hip_sampler_destroy.argtypes = [C.c_void_p]
        c.bitnet_hip_sampler_destroy.restype = None
        assert c.bitnet_hip_sampler_create(VOCAB, C.byref(cfg), C.byref(self.h)) == 0
        self.g = None
        if grammar is not None:
            self.desc = pkg.GrammarDesc.make(*grammar)
            self.g = C.c_void_p()
            c.bitnet_hip_grammar_create.argtypes = [C.c_void_p, C.c_void_p]
            c.bitnet_hip_sampler_set_grammar.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
            c.bitnet_hip_grammar_destroy.argtypes = [C.c_void_p]
            c.bitnet_hip_grammar_destroy.restype = None
            assert c.bitnet_hip_grammar_create(C.byref(self.desc), C.byref(self.g)) == 0
            assert c.bitnet_hip_sampler_set_grammar(self.h, self.g, 0) == 0
        self.w = dict(x=torch.from_numpy(row).cuda(), tok=torch.zeros(1, dtype=torch.int32, device="cuda"),
                      pos=torch.full((1,), -1, dtype=torch.int32, device="cuda"), hist=torch.full((LAUNCHES + 8,), -1, dtype=torch.int32, device="cuda"),
                      nf=torch.zeros(1, dtype=torch.int32, device="cuda"))

    def launch(self, stream):
        w = self.w
        assert self.c.bitnet_hip_sample_dev(self.h, w["x"].data_ptr(), VOCAB, w["tok"].data_ptr(), w["pos"].data_ptr(), w["hist"].data_ptr(),
                                            w["nf"].data_ptr(), stream) == 0

    def reset(self):
        assert self.c.bitnet_hip_sampler_reset(self.h) == 0

    def words(self):
        """what a replay left: the history of the 64 tokens and the word counter"""
        d = C.c_uint64(0)
        assert self.c.bitnet_hip_sampler_draws(self.h, C.byref(d)) == 0
        return self.w["hist"].cpu().numpy().tolist(), int(d.value)

    def close(self):
        self.c.bitnet_hip_sampler_destroy(self.h)
        if self.g:
            self.c.bitnet_hip_grammar_destroy(self.g)


def capture(side, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        side.launch(stream.cuda_stream)
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(LAUNCHES):
                side.launch(stream.cuda_stream)
    return g


def timed_replay(graph, side):
    side.reset()  # every replay starts from empty counts and the grammar's start state: the same work each time
    side.w["pos"].fill_(-1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); graph.replay(); b.record(); torch.cuda.synchronize()
    return 1000 * a.elapsed_time(b) / LAUNCHES


def sitting(sides, stream):
    """the sides' graphs replayed alternately, REPLAYS times after a warm-up; -> {name: [us per launch]}"""
    graphs = {k: capture(s, stream) for k, s in sides.items()}
    times = {k: [] for k in sides}
    for rep in range(REPLAYS + 1):
        for k in sides:
            t = timed_replay(graphs[k], sides[k])
            if rep:
                times[k].append(t)
    return times


def launch_part():
    stream = torch.cuda.Stream()
    sides = {"a_off": RawSampler(hip.path, ROW), "c_preedited_10": RawSampler(hip.path, EDITED),
             "g_grammar_10": RawSampler(hip.path, ROW, one_state(allowed=TEN)), "h_grammar_ban_300": RawSampler(hip.path, ROW, one_state(banned=BAN300))}
    if parent_lib:
        sides["parent_a_off"] = RawSampler(parent_lib, ROW)
        sides["parent_c_preedited_10"] = RawSampler(parent_lib, EDITED)
    times = sitting(sides, stream)
    out = {}
    for name, t in times.items():
        out[name] = {"us_per_launch": round(med(t), 2), "spread": round((max(t) - min(t)) / med(t), 4), "all": [round(v, 2) for v in t]}
        print(name, out[name], flush=True)
    words = {k: s.words() for k, s in sides.items()}
    out["g_equals_c_tokens"] = words["g_grammar_10"] == words["c_preedited_10"]  # the equivalence, once more
    out["h_over_a_us"] = round(out["h_grammar_ban_300"]["us_per_launch"] - out["a_off"]["us_per_launch"], 2)
    out["c_over_a_us"] = round(out["c_preedited_10"]["us_per_launch"] - out["a_off"]["us_per_launch"], 2)
    out["g_over_a_us"] = round(out["g_grammar_10"]["us_per_launch"] - out["a_off"]["us_per_launch"], 2)
    if parent_lib:
        spread_us = max(max(t) - min(t) for t in times.values())
        pc = out["parent_c_preedited_10"]["us_per_launch"]
        out["sitting_spread_us"] = round(spread_us, 2)
        out["masked_gain_c_us"] = round(pc - out["c_preedited_10"]["us_per_launch"], 2)
        out["masked_gain_g_us"] = round(pc - out["g_grammar_10"]["us_per_launch"], 2)
        out["masked_rows_faster_than_parent"] = bool(out["masked_gain_c_us"] > spread_us and out["masked_gain_g_us"] > spread_us)
        out["bit_identical_to_parent"] = bool(words["a_off"] == words["parent_a_off"] and words["c_preedited_10"] == words["parent_c_preedited_10"])
        if not out["masked_rows_faster_than_parent"]:
            failed.append("masked rows are not faster than the parent's by more than the sitting's spread")
        if not out["bit_identical_to_parent"]:
            failed.append("tokens or word counters differ from the parent's")
    if not out["g_equals_c_tokens"]:
        failed.append("the grammar's tokens differ from the pre-edited row's")
    for k in ("h_over_a_us", "c_over_a_us", "g_over_a_us", "sitting_spread_us", "masked_gain_c_us", "masked_gain_g_us", "masked_rows_faster_than_parent",
              "bit_identical_to_parent", "g_equals_c_tokens"):
        if k in out:
            print(k, out[k], flush=True)
    for s in sides.values():
        s.close()
    return out


def gate_part():
    """five runs per library, each run a FRESH sampler object with fresh device words, the libraries alternating within a run and the order
    of creation alternating from run to run (EXPERIMENTS.md 34.3)"""
    stream = torch.cuda.Stream()
    libs = {"parent": parent_lib, "this_build": hip.path}
    if control_lib:
        libs["control"] = control_lib
    medians, same = {k: [] for k in libs}, True
    for run in range(5):
        order = list(libs) if run % 2 == 0 else list(libs)[::-1]
        sides = {k: RawSampler(libs[k], ROW) for k in order}
        times = sitting(sides, stream)
        words = {k: sides[k].words() for k in order}
        same = same and words["parent"] == words["this_build"]
        for k in order:
            medians[k].append(med(times[k]))
            sides[k].close()
        del sides
    slowest, pmed, mine = max(medians["parent"]), med(medians["parent"]), med(medians["this_build"])
    allowance = abs(med(medians["control"]) - pmed) if control_lib else 0.0
    out = {k + "_medians_us": [round(v, 2) for v in m] for k, m in medians.items()}
    out.update(parent_slowest_us=round(slowest, 2), parent_median_us=round(pmed, 2), this_build_median_us=round(mine, 2),
               control_differs_by_us=round(allowance, 2), not_slower=bool(mine <= slowest + allowance), same_tokens_and_word_counters=bool(same))
    print("gate", out, flush=True)
    if not out["not_slower"]:
        failed.append("the off path is slower than the parent's slowest run by more than the control differs")
    if not same:
        failed.append("gate rows: tokens or word counters differ from the parent's")
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
    tc = np.zeros(cfg.vocab, np.uint16)
    tc[rng.choice(cfg.vocab, 10, replace=False)] = 1
    g = hip.grammar(tc, np.array([[-1, 0]], np.int32))
    times = {"grammar_off": [], "grammar_10": []}
    for rep in range(REPS + 1):
        for name in times:
            dec._check(dec.c.bitnet_host_set_grammar(dec.h, g.h if name == "grammar_10" else None, 0))
            dec.reset(); dec.feed(prompt); dec.run(PROMPT - 1, with_logits=False, use_graph=True)
            times[name].append(dec.run(STEPS, with_logits=True, use_graph=True) / STEPS)
    out = {}
    for name, t in times.items():
        t = t[1:]  # the first pass captures
        out[f"decoder_run/{name}"] = {"ms_per_step": round(med(t), 4), "spread": round((max(t) - min(t)) / med(t), 4)}
    out["delta_on_over_off_us"] = round(1000 * (out["decoder_run/grammar_10"]["ms_per_step"] - out["decoder_run/grammar_off"]["ms_per_step"]), 2)
    for k, v in out.items():
        print(k, v, flush=True)
    dec._check(dec.c.bitnet_host_set_grammar(dec.h, None, 0))
    dec.close()
    g.close()
    return out


if mode in ("launch", "all"):
    result["launch"] = launch_part()
    if parent_lib:
        result["gate"] = gate_part()
if mode in ("decode", "all"):
    result["decode"] = decode_part()
result["failed"] = failed
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
sys.exit(1 if failed else 0)
