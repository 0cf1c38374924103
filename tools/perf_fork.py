"""What forking a live sequence costs (bitnet_hip_kv_fork_dev), one process and sitting, HIP events around each launch, every shape warmed, medians.
Cache geometry of the synthetic 2B-4T model as bench.py builds it (30 layers, 5 KV heads, D = 128, max_pos 4224), f32 and f16 caches.

    python3 tools/perf_fork.py [json path] [layers = 30] [prefill = 1|0]

  1. the fork of n in {128, 1024, 4096} positions into n_dst in {1, 7} destinations; payload = the bytes ONE destination receives,
     traffic = (1 + n_dst) x payload;
  2. the yardstick: ONE contiguous hipMemcpyAsync device-to-device of the n_dst = 1 payload (what the runtime makes of the same bytes as one block
     instead of 2 x layers x kv heads strided segments);
  3. what the fork replaces: the member's own prefill(n, with_logits, digits = 2) on the QK256 model (skipped with prefill = 0)."""
import ctypes as C
import importlib, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else None
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 30
with_prefill = (sys.argv[3] if len(sys.argv) > 3 else "1") != "0"
cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 4224; cfg.n_layers = layers
NS, DSTS, REPS, MAX_DST = (128, 1024, 4096), (1, 7), 9, 7
med = statistics.median
rt = C.CDLL("libamdhip64.so")
rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
rt.hipMemcpyAsync.restype = C.c_int


def timed(fn):
    """median milliseconds of REPS single calls, each between two events on the stream the call runs on (the null stream), after two warm calls"""
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return med(ms)


result = {"layers": layers, "n_kv_heads": cfg.n_kv_heads, "head_dim": cfg.head_dim, "max_pos": cfg.max_pos, "reps": REPS, "caches": {}}
chunks = (cfg.max_pos + 63) // 64
for f16 in (False, True):
    es = 2 if f16 else 4
    words = cfg.n_kv_heads * chunks * 64 * cfg.head_dim * es // 4
    # [decoder][K | V][layer] caches, each its own allocation as in a Decoder; decoder 0 is the source
    caches = [[[torch.randint(-(1 << 31), (1 << 31) - 1, (words,), dtype=torch.int32, device="cuda") for _ in range(layers)] for _ in range(2)] for _ in range(1 + MAX_DST)]
    table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
    src_k, src_v = table(caches[0][0]), table(caches[0][1])
    dst_k, dst_v = table([t for d in caches[1:] for t in d[0]]), table([t for d in caches[1:] for t in d[1]])
    rows = []
    for n in NS:
        payload = 2 * layers * cfg.n_kv_heads * n * cfg.head_dim * es
        flat_src = torch.empty(payload, dtype=torch.uint8, device="cuda")
        flat_dst = torch.empty(payload, dtype=torch.uint8, device="cuda")

        def memcpy():
            assert rt.hipMemcpyAsync(flat_dst.data_ptr(), flat_src.data_ptr(), payload, 3, None) == 0  # hipMemcpyDeviceToDevice, null stream

        ms_copy = timed(memcpy)
        row = {"n": n, "payload_bytes": payload, "memcpy_us": round(ms_copy * 1e3, 2), "memcpy_payload_tbs": round(payload / ms_copy / 1e9, 3)}
        for n_dst in DSTS:
            ms = timed(lambda: hip.kv_fork_dev(src_k, src_v, dst_k, dst_v, layers, n_dst, cfg.n_kv_heads, cfg.head_dim, cfg.max_pos, n, kv_f16=f16))
            row[f"dst{n_dst}"] = {"us": round(ms * 1e3, 2), "payload_tbs": round(payload / ms / 1e9, 3), "traffic_tbs": round((1 + n_dst) * payload / ms / 1e9, 3)}
        row["dst1_vs_memcpy"] = round(row["dst1"]["payload_tbs"] / row["memcpy_payload_tbs"], 3)
        rows.append(row)
        print("f16" if f16 else "f32", row, flush=True)
        del flat_src, flat_dst
    # one fork checked in place: destination 0 equals the source over the first 4096 V rows of the last layer and head
    torch.cuda.synchronize()
    run = 4096 * cfg.head_dim * es // 4
    off = (cfg.n_kv_heads - 1) * chunks * 64 * cfg.head_dim * es // 4
    assert torch.equal(caches[1][1][-1][off:off + run], caches[0][1][-1][off:off + run])
    result["caches"]["f16" if f16 else "f32"] = rows
    del caches, src_k, src_v, dst_k, dst_v
    torch.cuda.empty_cache()

if with_prefill:
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        dec.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    dec.set_globals(synth.make_globals(cfg))
    prompt = synth.prompt(max(NS), cfg.vocab)
    result["prefill_ms"] = {}
    for f16 in (False, True):
        per_n = {}
        for n in NS:
            ms = []
            for _ in range(1 + 5):  # the first call warms the shape (buffers grown)
                dec.reset(); dec.set_kv_f16(f16); dec.feed(prompt[:n])
                ms.append(dec.prefill(n, with_logits=True, digits=2))
            per_n[str(n)] = round(med(ms[1:]), 3)
        result["prefill_ms"]["f16" if f16 else "f32"] = per_n
        print("prefill ms", "f16" if f16 else "f32", per_n, flush=True)
    dec.close()
print(json.dumps(result), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
