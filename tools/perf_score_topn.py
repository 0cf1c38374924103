"""What prompt top-N costs on the synthetic 2B-4T model as bench.py builds it (vocabulary 128256), n = 4096 prompt rows, top_n = 20, three routes
alternated in one sitting (one process, every route warmed, REPS rounds, medians):

  score_topn   HostDecoder.score_topn(n, 20): the prompt forward + the head with the top-K epilogue + k_score_topn (its own HIP events)
  score        HostDecoder.score(n) of the same build: the prompt forward + the head, no top list
  composed     the route score_topn replaces: HostDecoder.score(n, logits_rows = n) (its own HIP events; the read-back of the [n, vocab]
               logits is outside them) + bitnet_hip_logprob_rows_dev over the n / 64 groups of 64 rows of that [n, vocab] buffer (HIP events)

and, from the logits the composed route returns, how many rows take k_score_topn's escape and how many blocks they recompute: per 128-entry
block the 4 best and the 5th value, T = the top_n-th best candidate, a block is suspect when its 5th value >= T (csrc/kernels_score.hip).

    python3 tools/perf_score_topn.py [qk256|i2s] [layers = 30] [n = 4096] [json path = profiles/score_topn_summary.json]"""
import ctypes as C, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
fmt = sys.argv[1] if len(sys.argv) > 1 else "qk256"
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 30
N = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "score_topn_summary.json")
TOP_N, REPS, K, G = 20, 5, 4, 64
med = statistics.median
cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = N + 64; cfg.n_layers = layers
V = cfg.vocab
dec = pkg.HostDecoder(cfg)
for l in range(cfg.n_layers):
    w = synth.make_layer(cfg, l, fmt=fmt, block=32)
    dec.set_layer_qk256(l, w) if fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
dec.set_globals(synth.make_globals(cfg))
prompt = synth.prompt(N, V)


def fed():
    dec.reset(); dec.feed(prompt)


def run_topn():
    fed(); dec.score_topn(N, TOP_N)
    return dec.last_score_topn_ms


def run_score():
    fed()
    return dec.score(N).ms


fed()
res = dec.score(N, logits_rows=N)
logits = torch.from_numpy(res.logits).cuda()
# one entry per row: record [row] of one array, the row's own scratch slot of its group, its target as the "chosen" token
pos = torch.arange(N, dtype=torch.int32, device="cuda")
hist = torch.from_numpy(np.concatenate([prompt[1:], [0]]).astype(np.int32)).cuda()
recs = torch.zeros(N * pkg.LOGPROB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
sb = hip.logprob_scratch_bytes(V)
scratch = torch.zeros(G * sb, dtype=torch.uint8, device="cuda")
entries = (pkg.LogprobArgs * N)(*[pkg.LogprobArgs.make(logits.data_ptr() + 4 * V * r, pos.data_ptr() + 4 * r, hist.data_ptr(), recs.data_ptr(),
                                                        scratch.data_ptr() + sb * (r % G), N, TOP_N) for r in range(N)])
table = torch.from_numpy(np.frombuffer(bytes(entries), np.uint8).copy()).cuda()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def run_select():
    e0.record()
    for g in range(0, N, G):
        hip.logprob_rows_dev(table.data_ptr() + g * C.sizeof(pkg.LogprobArgs), min(G, N - g), V)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_composed():
    fed()
    return dec.score(N, logits_rows=N).ms + run_select()


routes = {"score_topn": run_topn, "score": run_score, "composed": run_composed}
for f in routes.values():
    f()
times = {k: [] for k in routes}
for _ in range(REPS):
    for k, f in routes.items():
        times[k].append(f())
select_ms = med([run_select() for _ in range(REPS)])

# the two routes agree, and the escape as the kernel decides it
fed()
rec = dec.score_topn(N, TOP_N)
old = recs.cpu().numpy().view(pkg.LOGPROB_DTYPE)
same = bool(np.array_equal(rec["top_id"][:N - 1], old["top_id"][:N - 1]))
nb = (V + 127) // 128
lp = np.full((N, nb * 128), -np.inf, np.float32); lp[:, :V] = res.logits
top5 = -np.sort(-lp.reshape(N, nb, 128), axis=2)[:, :, :K + 1]
T = -np.sort(-top5[:, :, :K].reshape(N, -1), axis=1)[:, TOP_N - 1]
suspect = (top5[:, :, K] >= T[:, None]).sum(axis=1)
result = {"device": torch.cuda.get_device_name(0), "fmt": fmt, "layers": layers, "n": N, "vocab": V, "top_n": TOP_N, "K": K, "reps": REPS,
          "ms": {k: round(med(v), 3) for k, v in times.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
          "composed_select_ms": round(select_ms, 3),
          "topn_added_over_score_ms": round(med(times["score_topn"]) - med(times["score"]), 3),
          "topn_over_composed": round(med(times["score_topn"]) / med(times["composed"]), 4),
          "rows_taking_the_escape": int((suspect > 0).sum()), "blocks_recomputed": int(suspect.sum()), "top_ids_equal_composed": same,
          "topn_workspace_bytes": hip.score_topn_workspace_bytes(N, cfg.hidden, V), "composed_logits_bytes": 4 * N * V}
dec.close()
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
