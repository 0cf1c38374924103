"""What beam search on the device costs, one process and one sitting: the synthetic 2B-4T model (QK256), f16 cache, 8 beams, prompts of 128 and
2048 tokens, 64 new tokens, routes alternated 5 times, medians, every sample kept.

    python3 tools/perf_beam.py [json path] [layers = 30]

  (a) the floor: the plain 8-member greedy batched step with the tap at 16 -- 64 x HostBatch.step(1), what the device route's two launches add to;
      and HostBatch.step(64), the same steps queued by one call (one synchronisation);
  (b) the device route: HostBeamSearch.run(16) -- per token step(1), bitnet_hip_beam_select_dev, bitnet_hip_kv_permute_dev; 4 bytes read per chunk;
  (c) the host-driven route of tests/test_beam_decoder_gpu.py -- records read back, the rule in numpy, fork into a second decoder set, feed, step:
      the only way without the two launches, so the comparator.
  Times are host wall clock around loops whose every call returns synchronised, in ms per token.
  Then the isolated permute launch (HIP events) at n = 128 / 1024 / 4096 slots, 7 of 8 beams moving from beam 0, from = 0 and from = n - 1, against
  bitnet_hip_kv_fork_dev of the same n slots into 7 destinations."""
import ctypes as C
import importlib, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_read
import test_beam_decoder_gpu as td
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else None
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 30
B, NEW, ROUNDS, PROMPTS = 8, 64, 5, (128, 2048)
med = statistics.median
result = {"layers": layers, "beams": B, "new_tokens": NEW, "rounds": ROUNDS, "search_ms_per_token": {}, "permute": {}}


class World:
    fmt = "qk256"

    def __init__(self):
        self.cfg = cfg = synth.ModelConfig(**synth.BITNET_2B_4T)
        cfg.max_pos, cfg.n_layers = max(PROMPTS) + NEW + 64, layers
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l, fmt="qk256", block=32) for l in range(cfg.n_layers)]
        self.prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)

    def decoder(self, pkg, kv16):
        dec = pkg.HostDecoder(self.cfg)
        for l, w in enumerate(self.layers):
            dec.set_layer_qk256(l, w)
        dec.set_globals(self.glob)
        dec.reset()
        dec.set_kv_f16(kv16)
        return dec


crew = td.Crew(pkg, World(), True)
for n_prompt in PROMPTS:
    samples = {"a_step1": [], "a_step64": [], "b_device": [], "c_host": []}
    members = crew.beams(B)
    crew.empty(crew.batch)
    for b, d in enumerate(members):
        d.reset()
        crew.batch.set_slot(b, d)
    s = pkg.HostBeamSearch(crew.batch, B, -1, NEW, 1.0)
    lw = s.len_weights()
    s.close()
    for rnd in range(ROUNDS + 1):  # round 0 warms every shape and graph
        for route in ("a_step1", "a_step64", "b_device", "c_host"):
            if route.startswith("a"):
                crew.empty(crew.batch)
                for d in members:
                    d.reset()
                    d.set_logprobs(2 * B)
                td.prime(crew, members, n_prompt)
                for b, d in enumerate(members):
                    crew.batch.set_slot(b, d)
                crew.batch.step(1)
                t0 = time.perf_counter()
                if route == "a_step64":
                    crew.batch.step(NEW)
                else:
                    for _ in range(NEW):
                        crew.batch.step(1)
                sec = time.perf_counter() - t0
            elif route == "b_device":
                search, _, steps = td.device_route(crew, B, n_prompt, -1, NEW, 1.0, 16)
                assert steps == NEW
                hyp_b = td.hyps(search)
                search.close()
                sec = crew.loop_seconds
            else:
                ref, _, _, _ = td.host_route(crew, B, n_prompt, -1, NEW, lw)
                assert ref.hypotheses() == hyp_b  # the two routes found the same hypotheses
                sec = crew.loop_seconds
            if rnd:
                samples[route].append(round(sec * 1e3 / NEW, 4))
    row = {k: {"median": med(v), "samples": v} for k, v in samples.items()}
    result["search_ms_per_token"][str(n_prompt)] = row
    print("prompt", n_prompt, {k: v["median"] for k, v in row.items()}, flush=True)
cfg = crew.W.cfg
crew.close()
torch.cuda.empty_cache()


def timed(fn, reps=9):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


max_pos = 4224
words = cfg.n_kv_heads * ((max_pos + 63) // 64) * 64 * cfg.head_dim // 2  # f16 caches
caches = [[[torch.randint(-(1 << 31), (1 << 31) - 1, (words,), dtype=torch.int32, device="cuda") for _ in range(layers)] for _ in range(2)] for _ in range(B)]
table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
k_all, v_all = table([t for d in caches for t in d[0]]), table([t for d in caches for t in d[1]])
src_k, src_v = table(caches[0][0]), table(caches[0][1])
dst_k, dst_v = table([t for d in caches[1:] for t in d[0]]), table([t for d in caches[1:] for t in d[1]])
beam = pkg.Beam(hip, B, -1, 4, np.ones(5, np.float32))
state_ptr = beam.done_ptr() - pkg.BeamState.done.offset
for n in (128, 1024, 4096):
    row = {}
    for name, frm in (("from0", 0), ("from_last", n - 1)):
        st, _ = beam.read()
        for b in range(B):
            st.parent[b], st.from_[b] = 0, frm
        st.n_slots, st.stepped = n, 1
        assert kv_read.runtime().hipMemcpy(C.c_void_p(state_ptr), C.byref(st), C.sizeof(st), 1) == 0
        ms = timed(lambda: hip.kv_permute_dev(k_all, v_all, beam, layers, B, cfg.n_kv_heads, cfg.head_dim, max_pos, n, kv_f16=True))
        row[name] = {"median_us": round(med(ms) * 1e3, 2), "samples_us": [round(m * 1e3, 2) for m in ms]}
    ms = timed(lambda: hip.kv_fork_dev(src_k, src_v, dst_k, dst_v, layers, B - 1, cfg.n_kv_heads, cfg.head_dim, max_pos, n, kv_f16=True))
    row["fork_7_dst"] = {"median_us": round(med(ms) * 1e3, 2), "samples_us": [round(m * 1e3, 2) for m in ms]}
    result["permute"][str(n)] = row
    print("permute n", n, {k: v["median_us"] for k, v in row.items()}, flush=True)
print(json.dumps(result), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
