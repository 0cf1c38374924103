"""What continuing a live sequence costs (Decoder::extend), one process, HIP events, every shape warmed, the routes alternated 5 times,
medians.  Synthetic 2B-4T model as bench.py builds it (30 layers), both formats, f16 KV cache.

    python3 tools/perf_extend.py [all|trace] [qk256,i2s] [layers = 30] [json path]

  1. 512 new tokens at 3584 past keys: route A = extend(512, with_logits, digits = 2); route B = run(511, no logits) + run(1, logits) on
     the step graphs -- the only route there was before extend -- both from the same prefill(3584) state (rewind(3584) + feed between them).
     Both must end with the same greedy token.
  2. prefill(1024) + 3 x extend(1024) against the one-shot prefill(4096): the cost of chunking (re-prepared past keys, narrower tiles).
  `trace`: prefill(3584) + ONE extend(512) per format and nothing else, for rocprofv3 --kernel-trace --stats (k_extend_prep per layer;
  its algorithmic bytes = the cache read + the two f16 images written are printed for comparison)."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256,i2s").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else None
PAST, NEW, T, REPS = 3584, 512, 4096, 5
med = statistics.median
result = {"layers": layers, "past": PAST, "new": NEW, "kv_cache": "f16", "digits": 2, "reps": REPS, "formats": {}}
for fmt in fmts:
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 4224; cfg.n_layers = layers
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        dec.set_layer_qk256(l, w) if fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
    dec.set_globals(synth.make_globals(cfg))
    dec.set_kv_f16(True)
    prompt = synth.prompt(T, cfg.vocab)
    dec.feed(prompt)
    ms_past = dec.prefill(PAST, with_logits=False, digits=2)

    def back():
        dec.rewind(PAST)
        dec.feed(prompt[PAST:])

    def route_a():
        ms = dec.extend(NEW, with_logits=True, digits=2)
        tok = int(dec.history(T + 1)[T])
        back()
        return ms, tok

    def route_b():
        ms = dec.run(NEW - 1, with_logits=False, use_graph=True) + dec.run(1, with_logits=True, use_graph=True)
        tok = int(dec.history(T + 1)[T])
        back()
        return ms, tok

    if mode == "trace":
        ms, tok = route_a()
        n_kv, D = cfg.n_kv_heads, cfg.head_dim
        tpad = (T + 63) // 64 * 64
        prep_bytes = 2 * n_kv * D * (PAST * 2 + NEW * 4 + NEW * 2 + tpad * 2)  # k and v: f16 cache read, f32 new rows read, f16 append, f16 image
        print(fmt, "trace: extend ms", round(ms, 3), "k_extend_prep algorithmic bytes per layer", prep_bytes, "=", round(prep_bytes / 8e12 * 1e6, 2), "us at 8 TB/s", flush=True)
        dec.close()
        continue
    route_a(); route_b()  # every shape warmed (graphs captured, buffers grown)
    a, b, toks = [], [], set()
    for _ in range(REPS):
        ms, tok = route_a(); a.append(ms); toks.add(("a", tok))
        ms, tok = route_b(); b.append(ms); toks.add(("b", tok))
    tok_a, tok_b = {t for r, t in toks if r == "a"}, {t for r, t in toks if r == "b"}
    r1 = {"extend_ms": round(med(a), 3), "decode_route_ms": round(med(b), 3), "ratio": round(med(b) / med(a), 2), "extend_ms_all": [round(x, 3) for x in a],
          "decode_route_ms_all": [round(x, 2) for x in b], "same_greedy_token": tok_a == tok_b and len(tok_a) == 1, "tokens": sorted(tok_a | tok_b),
          "prefill_3584_ms": round(ms_past, 3), "path": dec.last_prefill_path()}
    print(fmt, "512 new tokens at 3584 keys:", r1, flush=True)
    # ---- 2. chunked against one-shot ----
    def one_shot():
        dec.rewind(0); dec.feed(prompt)
        return dec.prefill(T, with_logits=True, digits=2), int(dec.history(T + 1)[T])

    def chunked():
        dec.rewind(0); dec.feed(prompt)
        ms = dec.prefill(1024, with_logits=False, digits=2)
        parts = [ms]
        for i in range(3):
            parts.append(dec.extend(1024, with_logits=(i == 2), digits=2))
        return sum(parts), parts, int(dec.history(T + 1)[T])

    one_shot(); chunked()
    o, c, parts_all, tk = [], [], [], set()
    for _ in range(REPS):
        ms, tok = one_shot(); o.append(ms); tk.add(tok)
        ms, parts, tok = chunked(); c.append(ms); parts_all.append(parts); tk.add(tok)
    r2 = {"one_shot_4096_ms": round(med(o), 3), "chunked_4x1024_ms": round(med(c), 3), "chunk_ms": [round(med([p[i] for p in parts_all]), 3) for i in range(4)],
          "same_greedy_token": len(tk) == 1}
    print(fmt, "prefill(1024) + 3 x extend(1024) vs prefill(4096):", r2, flush=True)
    result["formats"][fmt] = {"turn_512_at_3584": r1, "chunked_vs_one_shot": r2}
    dec.close()
if mode != "trace":
    print(json.dumps(result), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
