"""What packing several sequences' prompts into one forward saves (Decoder::prefill_packed), one process, every shape warmed, the two routes
alternated 5 times, medians of wall-clock times around the synchronising calls (the sequential route spans the members' own streams, so there is
no one stream to put events on).  Synthetic 2B-4T model as bench.py builds it (30 layers), both formats, f16 KV cache, digits 2.

    python3 tools/perf_packed.py [all|trace] [qk256,i2s] [layers = 30] [json path]

  1. B in {1, 2, 4, 8, 16} fresh members x L in {16, 128, 512} tokens each: route A = prefill_packed(members, [L] * B), heads included; route B = the
     same members' prefill(L) one after another (unchanged code: the number the parent commit gives in the same sitting).
  2. chat-shaped: 8 members at past 1024, 32 new tokens each, packed against 8 extend(32) calls.
  Acceptance (profiles/packed_summary.json): at 8 x 128 the packed route takes no longer than the sequential one, in both formats.
  `trace`: ONE packed forward of 8 x 128 per format behind a warm-up of the same shape, for rocprofv3 --kernel-trace --stats (k_packed_prep,
  k_prefill_attn_packed and the members' heads)."""
import importlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("bitnet-rs_amd"); synth = importlib.import_module("bitnet-rs_amd.synth")
hip = pkg.load(); hip.init(0)
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
fmts = (sys.argv[2] if len(sys.argv) > 2 else "qk256,i2s").split(",")
layers = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else None
BS, LS, REPS, PAST, NEW, MAXB = (1, 2, 4, 8, 16), (16, 128, 512), 5, 1024, 32, 16
med = statistics.median
result = {"layers": layers, "kv_cache": "f16", "digits": 2, "reps": REPS, "timing": "wall clock around the synchronising calls, ms", "formats": {}}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


for fmt in fmts:
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T); cfg.max_pos = 1152; cfg.n_layers = layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        owner.set_layer_qk256(l, w) if fmt == "qk256" else owner.set_layer_i2s(l, w, 32)
    owner.set_globals(synth.make_globals(cfg))
    owner.set_kv_f16(True)
    members = [owner] + [owner.shared() for _ in range(MAXB - 1)]
    for m in members[1:]:
        m.set_kv_f16(True)
    prompt = synth.prompt(cfg.max_pos, cfg.vocab)
    toks = [((prompt.astype("int64") + 37 * i) % cfg.vocab).astype("int32") for i in range(MAXB)]

    def fresh(ms, n):
        for i, m in enumerate(ms):
            m.reset(); m.feed(toks[i][:n])

    def packed(ms, n):
        fresh(ms, n)
        ms_ = timed(lambda: ms[0].prefill_packed(ms, [n] * len(ms), with_logits=True, digits=2))
        return ms_, [int(m.history(n + 1)[n]) for m in ms]

    def sequential(ms, n):
        fresh(ms, n)
        ms_ = timed(lambda: [m.prefill(n, with_logits=True, digits=2) for m in ms])
        return ms_, [int(m.history(n + 1)[n]) for m in ms]

    if mode == "trace":
        packed(members[:8], 128)
        ms_, _ = packed(members[:8], 128)
        print(fmt, "trace: packed 8 x 128 ms", round(ms_, 3), flush=True)
        for m in reversed(members):
            m.close()
        continue
    grid = {}
    for B in BS:
        for L in LS:
            ms = members[:B]
            packed(ms, L); sequential(ms, L)  # every shape warmed (buffers grown, kernels loaded)
            a, b, same = [], [], True
            for _ in range(REPS):
                t, ta = packed(ms, L); a.append(t)
                t, tb = sequential(ms, L); b.append(t)
                same = same and ta == tb
            grid[f"{B}x{L}"] = {"packed_ms": round(med(a), 3), "sequential_ms": round(med(b), 3), "ratio": round(med(b) / med(a), 3),
                                "packed_ms_all": [round(x, 3) for x in a], "sequential_ms_all": [round(x, 3) for x in b], "same_greedy_tokens": same,
                                "path": ms[0].last_prefill_path()}
            print(fmt, f"{B} x {L}:", grid[f"{B}x{L}"], flush=True)
    # ---- chat-shaped: 8 members at past 1024, 32 new tokens each ----
    ms = members[:8]
    fresh(ms, PAST + NEW)
    ms[0].prefill_packed(ms, [PAST] * 8, with_logits=False, digits=2)

    def back():
        for i, m in enumerate(ms):
            m.rewind(PAST); m.feed(toks[i][PAST:PAST + NEW])

    def chat_packed():
        t = timed(lambda: ms[0].prefill_packed(ms, [NEW] * 8, with_logits=True, digits=2))
        back()
        return t

    def chat_seq():
        t = timed(lambda: [m.extend(NEW, with_logits=True, digits=2) for m in ms])
        back()
        return t

    back(); chat_packed(); chat_seq()
    a, b = [], []
    for _ in range(REPS):
        a.append(chat_packed()); b.append(chat_seq())
    chat = {"packed_ms": round(med(a), 3), "sequential_ms": round(med(b), 3), "ratio": round(med(b) / med(a), 3), "packed_ms_all": [round(x, 3) for x in a],
            "sequential_ms_all": [round(x, 3) for x in b]}
    print(fmt, "8 members, 32 new tokens at 1024 keys:", chat, flush=True)
    result["formats"][fmt] = {"fresh": grid, "chat_8x32_at_1024": chat}
    for m in reversed(members):
        m.close()
if mode != "trace":
    ratios = {f: result["formats"][f]["fresh"]["8x128"]["ratio"] for f in result["formats"]}
    result["acceptance"] = {"case": "8 x 128 fresh tokens, heads included: sequential_ms / packed_ms", "floor_ratio": 1.0, "measured_ratio": ratios,
                            "met": all(r >= 1.0 for r in ratios.values())}
    print(json.dumps(result), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
