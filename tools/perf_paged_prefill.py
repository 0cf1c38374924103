"""The prompt attention over page tables (bitnet_hip_attention_paged_prefill_dev: prep + attention launch) against bitnet_hip_attention_packed_dev on
contiguous caches for the same segments, in one sitting.  (past, len) = (0, 4096), (4032, 64), (2048, 512) and 8 x (0, 512), f16 and f32 pools, the
2B-4T attention shape (20 heads, 5 KV heads, head_dim 128), f32 output rows.  Both routes of a shape are timed in interleaved rounds (HIP events
around REPS calls each); per shape the median over the rounds, the ratio and the sitting's spread (max / min over the rounds of one route) go to
profiles/paged_prefill_summary.json with each route's workspace bytes.  Pool and cache contents are zeros and the page tables a permutation: the
launches' time does not depend on the values; the RoPE tables are real.  REPS is chosen per shape so that a timed window holds at least 40 ms of work.

Then the host layer, same sitting, on the synthetic 2B-4T model as bench.py builds it (30 layers, QK256, f16 caches, digits 2, max_pos 4160), one
4096-token prompt, host clock around calls that return synchronised, HOST_ROUNDS interleaved rounds after a warm-up round:
  (b) PagedBatch open + prefill(4096) against staging prefill(4096) + admit;
  (c) the same prompt in eight prefill(512) chunks into pages, against the staging decoder's prefill(512) + seven extend(512) + admit.
A GPU is required: there is no other path."""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch as t

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, N_KV, D, MAX_POS, ROUNDS, WINDOW_US = 20, 5, 128, 4096, 5, 40000.0
HOST_ROUNDS, PROMPT, CHUNK = 5, 4096, 512
SHAPES = {"1x(0,4096)": [(0, 4096)], "1x(4032,64)": [(4032, 64)], "1x(2048,512)": [(2048, 512)], "8x(0,512)": [(0, 512)] * 8}


def timed(fn, reps):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    t.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # microseconds per call


def rope_tables():
    inv = 1.0 / (10000.0 ** (np.arange(0, D, 2, dtype=np.float64) / D))
    ang = np.arange(MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    return (t.from_numpy(f(ang).astype(np.float32)).cuda() for f in (np.sin, np.cos))


def shape(hip, name, segs, f16):
    R, align = 64 if f16 else 128, hip.attention_packed_row_align(H, N_KV)
    pasts, lens = [p for p, _ in segs], [n for _, n in segs]
    row0 = list(np.cumsum([0] + [-(-n // align) * align for n in lens[:-1]]))
    n_rows = int(row0[-1] + lens[-1])
    pages = [-(-(p + n) // 64) for p, n in segs]
    n_pages = sum(pages)
    perm, at, tables = np.random.default_rng(len(segs)).permutation(n_pages), 0, []
    for c in pages:
        tab = np.zeros(MAX_POS // 64, np.uint32)
        tab[:c] = perm[at:at + c]
        at += c
        tables.append(t.from_numpy(tab.view(np.int32)).cuda())
    kpool, vpool = (t.zeros(n_pages * N_KV * 64 * R, dtype=t.int32, device="cuda") for _ in range(2))
    kc, vc = ([t.zeros(N_KV * MAX_POS * R, dtype=t.int32, device="cuda") for _ in segs] for _ in range(2))
    qkv = t.randn((n_rows, (H + 2 * N_KV) * D), dtype=t.float32, device="cuda")
    sin, cos = rope_tables()
    out = t.zeros((n_rows, H * D), dtype=t.float32, device="cuda")
    wp, wc = hip.attention_paged_prefill_workspace_bytes(H, N_KV, n_rows), hip.attention_packed_workspace_bytes(H, N_KV, n_rows, pasts, lens)
    wsp, wsc = t.empty(wp, dtype=t.uint8, device="cuda"), t.empty(wc, dtype=t.uint8, device="cuda")
    flags = 1 if f16 else 0
    paged = lambda: hip.attention_paged_prefill_dev(qkv, n_rows, sin, cos, row0, lens, pasts, tables, kpool, vpool, n_pages, H, N_KV, D, MAX_POS, wsp, wp, out, flags=flags)  # noqa: E731
    packed = lambda: hip.attention_packed_dev(qkv, n_rows, sin, cos, row0, lens, pasts, kc, vc, H, N_KV, D, MAX_POS, wsc, wc, out, flags=flags)  # noqa: E731
    reps = {}
    for fn in (paged, packed):  # warm-up, and the window's length from a first estimate
        timed(fn, 3)
        reps[fn] = max(10, int(WINDOW_US / timed(fn, 10)) + 1)
    tp, tc = [], []
    for _ in range(ROUNDS):
        tp.append(timed(paged, reps[paged]))
        tc.append(timed(packed, reps[packed]))
    return dict(shape=name, reps_paged=reps[paged], reps_packed=reps[packed], pool="f16" if f16 else "f32", paged_us=float(np.median(tp)), packed_us=float(np.median(tc)), paged_over_packed=float(np.median(tp) / np.median(tc)),
                spread_paged=float(max(tp) / min(tp)), spread_packed=float(max(tc) / min(tc)), workspace_paged=int(wp), workspace_packed=int(wc))


def host(pkg, layers):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T)
    cfg.max_pos, cfg.n_layers = PROMPT + 64, layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    owner.set_globals(synth.make_globals(cfg))
    owner.set_kv_f16(True)
    stage = owner.shared()
    stage.set_kv_f16(True)
    prompt = synth.prompt(PROMPT + 1, cfg.vocab)
    pb = pkg.HostPagedBatch(owner, 2 * (PROMPT // 64 + 1), 2)

    def paged(chunks):
        pb.open(0)
        m = pb.member(0)
        m.feed(prompt)
        t0 = time.perf_counter()
        for c in chunks:
            pb.prefill([0], [c], with_logits=True, digits=2)
        ms = (time.perf_counter() - t0) * 1e3
        m.close()
        pb.release(0)
        return ms

    def staged(chunks):
        stage.rewind(0)
        stage.feed(prompt)
        t0 = time.perf_counter()
        stage.prefill(chunks[0], with_logits=True, digits=2)
        for c in chunks[1:]:
            stage.extend(c, with_logits=True, digits=2)
        pb.admit(1, stage, PROMPT)
        t.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        pb.release(1)
        return ms

    whole, parts = [PROMPT], [CHUNK] * (PROMPT // CHUNK)
    routes = {"b_paged_open_prefill": lambda: paged(whole), "b_staged_prefill_admit": lambda: staged(whole), "c_paged_chunks": lambda: paged(parts),
              "c_staged_chunks_admit": lambda: staged(parts)}
    samples = {k: [] for k in routes}
    for r in range(HOST_ROUNDS + 1):  # round 0 warms every route
        for k, fn in routes.items():
            ms = fn()
            if r:
                samples[k].append(ms)
    out = {k: dict(ms=float(np.median(v)), spread=float(max(v) / min(v))) for k, v in samples.items()}
    out["b_paged_over_staged"] = out["b_paged_open_prefill"]["ms"] / out["b_staged_prefill_admit"]["ms"]
    out["c_paged_over_staged"] = out["c_paged_chunks"]["ms"] / out["c_staged_chunks_admit"]["ms"]
    out.update(prompt=PROMPT, chunk=CHUNK, layers=layers, rounds=HOST_ROUNDS, staging_cache_bytes=2 * layers * cfg.n_kv_heads * (cfg.max_pos + 63) // 64 * 64 * cfg.head_dim * 2)
    print(json.dumps(out), flush=True)
    pb.close()
    stage.close()
    owner.close()
    return out


def main():
    if not t.cuda.is_available():
        sys.exit("perf_paged_prefill: no GPU")
    pkg = importlib.import_module("bitnet-rs_amd")
    hip = pkg.load()
    hip.init(0)
    rows = [shape(hip, name, segs, f16) for name, segs in SHAPES.items() for f16 in (True, False)]
    for r in rows:
        print(json.dumps(r))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.environ.get("PERF_OUT", os.path.join(root, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "paged_prefill_summary.json"), "w") as f:
        json.dump(dict(device=t.cuda.get_device_name(0), heads=H, kv_heads=N_KV, max_pos=MAX_POS, rounds=ROUNDS, window_us=WINDOW_US, launches=rows,
                       host=host(pkg, int(os.environ.get("PERF_LAYERS", "30")))), f, indent=1)


if __name__ == "__main__":
    main()
