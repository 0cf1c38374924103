#!/usr/bin/env python3
"""Timings of teacher-forced scoring on an MI355X (EXPERIMENTS.md section 10): the bench's synthetic 2B-4T model (30 layers, vocabulary
128256), both formats, n in {512, 2048, 4096}:
  prefill_ms   prefill(n, with_logits, digits 2) alone (the benchmarked prompt forward)
  score_ms     score(n) = that prefill + the head over every row (HostDecoder.score, its own HIP events)
  head_ms      the head alone: bitnet_hip_score_f16_dev on [n, 2560] rows (prologue + GEMM + combine; HIP events, warm-up, median),
               with TFLOP/s = 2 n vocab hidden / time and its share of the 2.5 PF f16 peak
  tbt_ms       the token-by-token alternative (n in {512, 4096}): run(1) + last_logits() + a host log-softmax per position
Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats` (--quick: one score per format and n, nothing else).
  python tools/perf_score.py [--quick] [--reps 5] [--out profiles/perf_score.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_F16 = 2.5e15


def head_alone(hip, torch_, n, cfg, glob, reps):
    h, v = cfg.hidden, cfg.vocab
    table = torch_.from_numpy(np.asarray(glob["embed_f16"]).view(np.int16)).cuda()
    gamma = torch_.from_numpy(np.asarray(glob["final_norm"], np.float32)).cuda()
    g = torch_.Generator(device="cuda").manual_seed(n)
    x = torch_.randn(n, h, device="cuda", generator=g)
    tg = torch_.randint(0, v, (n,), device="cuda", dtype=torch_.int32, generator=g)
    nll = torch_.zeros(n, device="cuda")
    am = torch_.zeros(n, dtype=torch_.int32, device="cuda")
    wsb = hip.score_workspace_bytes(n, h, v)
    ws = torch_.zeros(wsb, dtype=torch_.uint8, device="cuda")
    call = lambda: hip.score_f16_dev(table, x, gamma, cfg.eps, h, v, n, tg, nll, am, None, 0, ws, wsb, torch_.cuda.current_stream().cuda_stream)  # noqa: E731
    for _ in range(3):
        call()
    ts = []
    for _ in range(reps):
        e0, e1 = torch_.cuda.Event(enable_timing=True), torch_.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch_.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def token_by_token(dec, prompt, n):
    import score_ref as sr

    dec.reset()
    dec.feed(prompt[:n])
    t0 = time.perf_counter()
    tot = 0.0
    for r in range(n - 1):
        dec.run(1, with_logits=True, use_graph=True)
        tot += sr.row_nll(dec.last_logits(), int(prompt[r + 1]))
    return (time.perf_counter() - t0) * 1000.0, tot


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one score per format and n (for the kernel-trace run)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fmts", default="qk256,i2s")
    ap.add_argument("--ns", default="512,2048,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    pkg = importlib.import_module("bitnet-rs_amd")
    synth = importlib.import_module("bitnet-rs_amd.synth")
    hip = pkg.load()
    hip.init(0)
    ns = [int(s) for s in args.ns.split(",")]
    cfg = synth.ModelConfig(**dict(synth.BITNET_2B_4T, max_pos=max(ns) + 64))
    glob = synth.make_globals(cfg)
    prompt = synth.prompt(max(ns), cfg.vocab)
    rows = []
    for fmt in args.fmts.split(","):
        dec = pkg.HostDecoder(cfg)
        for l in range(cfg.n_layers):
            w = synth.make_layer(cfg, l, fmt=fmt, block=32)
            dec.set_layer_qk256(l, w) if fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
        dec.set_globals(glob)
        for n in ns:
            rec = {"fmt": fmt, "n": n}
            if args.quick:
                dec.reset()
                dec.feed(prompt[:n])
                rec["score_ms"] = dec.score(n).ms
                rows.append(rec)
                print(json.dumps(rec), flush=True)
                continue
            pf, sc = [], []
            for i in range(args.reps + 1):
                dec.reset()
                dec.feed(prompt[:n])
                ms = dec.prefill(n, with_logits=True, digits=2)
                if i:
                    pf.append(ms)
                dec.reset()
                dec.feed(prompt[:n])
                ms = dec.score(n, digits=2).ms
                if i:
                    sc.append(ms)
            rec["path"] = dec.last_prefill_path()
            rec["prefill_ms"] = round(statistics.median(pf), 3)
            rec["score_ms"] = round(statistics.median(sc), 3)
            rec["score_minus_prefill_ms"] = round(rec["score_ms"] - rec["prefill_ms"], 3)
            hm = head_alone(hip, torch, n, cfg, glob, args.reps)
            fl = 2.0 * n * cfg.vocab * cfg.hidden
            rec["head_ms"] = round(hm, 3)
            rec["head_tflops"] = round(fl / (hm * 1e-3) / 1e12, 1)
            rec["head_share_of_peak"] = round(fl / (hm * 1e-3) / PEAK_F16, 3)
            if n in (512, 4096):
                ms, _ = token_by_token(dec, prompt, n)
                rec["tbt_ms"] = round(ms, 1)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        dec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
