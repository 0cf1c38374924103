"""What a context shift costs (Decoder::shift, bitnet_hip_kv_shift_dev) against what it replaces, one process and sitting, every shape warmed,
medians of five alternations.  Synthetic 2B-4T model as bench.py builds it (30 layers, 5 KV heads, D = 128), max_pos 4096, f32 and f16 caches, a
sequence at position 4095.

    python3 tools/perf_shift.py [json path = profiles/shift_summary.json] [layers = 30]

  1. the kernel alone on caches of the same geometry: HIP events around one bitnet_hip_kv_shift_dev launch for (keep, discard) = (4, 2045) (disjoint
     ranges: segments split over workgroups), (4, 1) and (4, 64) (overlapping ranges: one workgroup walks a segment); bytes = moved positions x
     2 (K, V) x layers x kv heads x D x element size, read once and written once;
  2. the call: HostDecoder.shift(4, 2045) at position 4095, wall clock around the call (it returns synchronised and includes the history round trip),
     alternated with what the parent commit offers for the same outcome: reset(), feed() of the 2050 surviving tokens, prefill(2050, digits = 2) --
     wall clock likewise, and the prefill's own event time.  Floor: the shift at least 10 x faster."""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shift_ref as sr
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shift_summary.json")
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 30
cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 4096; cfg.n_layers = layers
P, KEEP, ROUNDS, REPS = 4095, 4, 5, 9
SHIFTS = (2045, 1, 64)
med = statistics.median
result = {"layers": layers, "n_kv_heads": cfg.n_kv_heads, "head_dim": cfg.head_dim, "max_pos": cfg.max_pos, "position": P, "keep": KEEP, "kernel": {}, "call": {}}

# ---- 1. the kernel alone ----
sin, cos = sr.rope_tables(cfg.max_pos, cfg.rope_theta)
sin_d, cos_d = torch.from_numpy(sin).cuda(), torch.from_numpy(cos).cuda()
table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
for f16 in (False, True):
    es = 2 if f16 else 4
    elems = cfg.n_kv_heads * cfg.max_pos * cfg.head_dim
    dt = torch.float16 if f16 else torch.float32
    kc, vc = ([torch.randn(elems, dtype=dt, device="cuda") for _ in range(layers)] for _ in range(2))
    k_t, v_t = table(kc), table(vc)
    rows = {}
    for discard in SHIFTS:
        moved = P - KEEP - discard
        nbytes = 2 * moved * 2 * layers * cfg.n_kv_heads * cfg.head_dim * es  # read + write
        fn = lambda: hip.kv_shift_dev(k_t, v_t, sin_d, cos_d, layers, cfg.n_kv_heads, cfg.head_dim, cfg.max_pos, KEEP, discard, P, kv_f16=f16)
        fn(); fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        rows[f"discard{discard}"] = {"moved_positions": moved, "bytes": nbytes, "us": round(med(ms) * 1e3, 2), "tbs": round(nbytes / med(ms) / 1e9, 3)}
        print("kernel", "f16" if f16 else "f32", discard, rows[f"discard{discard}"], flush=True)
    result["kernel"]["f16" if f16 else "f32"] = rows
    del kc, vc, k_t, v_t
    torch.cuda.empty_cache()

# ---- 2. the call against the re-prefill ----
dec = pkg.HostDecoder(cfg)
for l in range(cfg.n_layers):
    dec.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
dec.set_globals(synth.make_globals(cfg))
prompt = np.asarray(synth.prompt(P, cfg.vocab), np.int32)


def at_the_wall(f16):
    dec.reset(); dec.set_kv_f16(f16); dec.feed(prompt)
    dec.prefill(P, with_logits=True, digits=2)
    assert dec.position() == P


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


for f16 in (False, True):
    shift_ms = {d: [] for d in SHIFTS}
    re_wall, re_event = [], []
    for r in range(1 + ROUNDS):  # the first round warms every shape
        for d in SHIFTS:
            at_the_wall(f16)
            ms, _ = wall(lambda: dec.shift(KEEP, d))
            assert dec.position() == P - d
            shift_ms[d].append(ms)
        at_the_wall(f16)
        hist = np.asarray(dec.history(P))
        survivors = np.concatenate([hist[:KEEP], hist[KEEP + 2045:]])

        def re_prefill():
            dec.reset(); dec.feed(survivors)
            return dec.prefill(len(survivors), with_logits=True, digits=2)

        ms, ev = wall(re_prefill)
        re_wall.append(ms), re_event.append(ev)
    row = {f"shift_discard{d}_ms": round(med(v[1:]), 4) for d, v in shift_ms.items()}
    row["re_prefill_wall_ms"], row["re_prefill_event_ms"] = round(med(re_wall[1:]), 3), round(med(re_event[1:]), 3)
    row["ratio_disjoint"] = round(row["re_prefill_wall_ms"] / row["shift_discard2045_ms"], 1)
    row["floor_10x_met"] = bool(row["ratio_disjoint"] >= 10.0)
    result["call"]["f16" if f16 else "f32"] = row
    print("call", "f16" if f16 else "f32", row, flush=True)
dec.close()
print(json.dumps(result), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
