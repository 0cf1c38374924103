"""What a prefix-cache snapshot costs (bitnet_hip_kv_save_dev / bitnet_hip_kv_restore_dev), one process and sitting, HIP events around each launch,
every shape warmed, medians.  Cache geometry of the synthetic 2B-4T model as bench.py builds it (30 layers, 5 KV heads, D = 128, max_pos 4224), f32
and f16 caches, n in {128, 1024, 4096} positions.

    python3 tools/perf_prefix_cache.py [json path] [layers = 30] [prefill = 1|0]

  1. the isolated save launch and the isolated restore launch (one destination, and seven), each against bitnet_hip_kv_fork_dev of the same
     positions: fork moves the same bytes without the K transpose, so it is the yardstick.  The two are ALTERNATED call by call inside one timed
     loop (the machine is shared: a drift hits both alike); payload = the bytes one destination receives = the snapshot's size.  The K part
     (the transpose through LDS) and the V part (a plain run copy) are one launch and are not timed apart here.
  2. prefill_cached with a full hit (n - 1 positions restored, one token computed) against prefill(n) on the QK256 model (skipped with
     prefill = 0): what a cached prompt costs end to end, restore and the one-token extend included, by a host clock around the synchronising call."""
import importlib, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else None
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 30
with_prefill = (sys.argv[3] if len(sys.argv) > 3 else "1") != "0"
cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 4224; cfg.n_layers = layers
NS, REPS, MAX_DST = (128, 1024, 4096), 15, 7
med = statistics.median


def alternated(fns):
    """median milliseconds of REPS calls of each function, the functions taken in turn inside one loop; each call between two events on the
    null stream; two warm rounds first"""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [med(m) for m in ms]


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
    geo = (cfg.n_kv_heads, cfg.head_dim, cfg.max_pos)
    rows = []
    for n in NS:
        payload = hip.kv_snapshot_bytes(layers, cfg.n_kv_heads, cfg.head_dim, n, kv_f16=f16)
        assert payload == 2 * layers * cfg.n_kv_heads * n * cfg.head_dim * es
        snap = torch.empty(payload // 4, dtype=torch.int32, device="cuda")
        save = lambda: hip.kv_save_dev(src_k, src_v, layers, *geo, n, snap, kv_f16=f16)
        fork = lambda d: (lambda: hip.kv_fork_dev(src_k, src_v, dst_k, dst_v, layers, d, *geo, n, kv_f16=f16))
        restore = lambda d: (lambda: hip.kv_restore_dev(snap, n, dst_k, dst_v, layers, d, *geo, n, kv_f16=f16))
        save()
        ms_save, ms_r1, ms_f1, ms_r7, ms_f7 = alternated([save, restore(1), fork(1), restore(MAX_DST), fork(MAX_DST)])
        tbs = lambda ms, k=1: round(k * payload / ms / 1e9, 3)
        row = {"n": n, "payload_bytes": payload,
               "save": {"us": round(ms_save * 1e3, 2), "payload_tbs": tbs(ms_save), "vs_fork1": round(ms_save / ms_f1, 3)},
               "restore1": {"us": round(ms_r1 * 1e3, 2), "payload_tbs": tbs(ms_r1), "vs_fork1": round(ms_r1 / ms_f1, 3)},
               "fork1": {"us": round(ms_f1 * 1e3, 2), "payload_tbs": tbs(ms_f1)},
               "restore7": {"us": round(ms_r7 * 1e3, 2), "traffic_tbs": tbs(ms_r7, 1 + MAX_DST), "vs_fork7": round(ms_r7 / ms_f7, 3)},
               "fork7": {"us": round(ms_f7 * 1e3, 2), "traffic_tbs": tbs(ms_f7, 1 + MAX_DST)}}
        rows.append(row)
        print("f16" if f16 else "f32", row, flush=True)
        # checked in place: after restore(7) and fork(7) every destination holds the source's first n V rows of the last layer and head; and on a
        # freshly scrambled K cache of destination 0 a restore alone leaves the words a fork alone leaves (head 0's whole chunks below n)
        torch.cuda.synchronize()
        run = n * cfg.head_dim * es // 4
        off = (cfg.n_kv_heads - 1) * chunks * 64 * cfg.head_dim * es // 4
        assert torch.equal(caches[1][1][-1][off:off + run], caches[0][1][-1][off:off + run])
        whole = (n // 64) * 64 * cfg.head_dim * es // 4
        caches[1][0][-1].random_()
        fork(1)()
        forked = caches[1][0][-1][:whole].clone()
        caches[1][0][-1].random_()
        restore(1)()
        torch.cuda.synchronize()
        assert torch.equal(caches[1][0][-1][:whole], forked)
        del snap
    result["caches"]["f16" if f16 else "f32"] = rows
    del caches, src_k, src_v, dst_k, dst_v
    torch.cuda.empty_cache()

if with_prefill:
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        dec.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    dec.set_globals(synth.make_globals(cfg))
    prompt = synth.prompt(max(NS), cfg.vocab)
    result["prefill_ms"], result["prefill_cached_full_hit_ms"] = {}, {}
    for f16 in (False, True):
        cold, hot = {}, {}
        for n in NS:
            cache = pkg.PrefixCache(max_memory_bytes=1 << 33)
            ms_cold, ms_hot = [], []
            for rep in range(1 + 5):  # the first round warms the shapes (buffers grown); the two are alternated
                dec.reset(); dec.set_kv_f16(f16); dec.feed(prompt[:n])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.prefill(n, with_logits=True, digits=2)  # synchronises before it returns
                ms_cold.append((time.perf_counter() - t0) * 1e3)
                if rep == 0:
                    cache.insert(dec, n)
                dec.reset(); dec.feed(prompt[:n])
                t0 = time.perf_counter()
                hit = dec.prefill_cached(cache, n, with_logits=True, digits=2)
                ms_hot.append((time.perf_counter() - t0) * 1e3)
                assert hit == n - 1
            cold[str(n)], hot[str(n)] = round(med(ms_cold[1:]), 3), round(med(ms_hot[1:]), 3)
            cache.close()
        result["prefill_ms"]["f16" if f16 else "f32"] = cold
        result["prefill_cached_full_hit_ms"]["f16" if f16 else "f32"] = hot
        print("prefill ms", "f16" if f16 else "f32", cold, "prefill_cached (full hit) ms", hot, flush=True)
    dec.close()
print(json.dumps(result), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
