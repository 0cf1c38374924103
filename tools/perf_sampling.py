#!/usr/bin/env python3
"""Cost of the device sampler per decode step, next to today's greedy step.
    python tools/perf_sampling.py [--steps 256] [--reps 5] [--hidden 2560] [--layers 2]
A synthetic decoder with the 128256-entry vocabulary; HIP events around `steps` graph-replayed steps (Decoder::run), best of
`reps`, for: greedy (no sampler: k_logits_f16 + k_argmax_final), G (1, 0, 1, 1.1: penalised argmax), S (0.7, top-k 40, 0.95,
1.1) and F (0.7, top-k 0, 0.95, 1.1: full-vocabulary top-p).  Prints one JSON line: us/step of each and the difference to greedy."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bitnet-rs_amd")
synth = importlib.import_module("bitnet-rs_amd.synth")

CONFIGS = {"greedy": None, "G": (1.0, 0, 1.0, 1.1), "S": (0.7, 40, 0.95, 1.1), "F": (0.7, 0, 0.95, 1.1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=2560)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--only", choices=list(CONFIGS), help="time one config (for a profiler run of its kernels)")
    args = ap.parse_args()
    pkg.load().init(0)
    H = args.hidden
    cfg = synth.ModelConfig(hidden=H, n_layers=args.layers, n_heads=H // 128, n_kv_heads=max(1, H // 512), head_dim=128, ffn=H * 27 // 10 // 256 * 256,
                            vocab=128256, max_pos=args.steps + 16, eps=1e-5, rope_theta=500000.0)
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        dec.set_layer_qk256(l, synth.make_layer(cfg, l))
    dec.set_globals(synth.make_globals(cfg))
    prompt = synth.prompt(4, cfg.vocab)
    out = {"steps": args.steps, "vocab": cfg.vocab, "hidden": H, "layers": cfg.n_layers}
    for name, c in CONFIGS.items():
        if args.only and name != args.only:
            continue
        if c is None:
            dec.set_sampling(None)
        else:
            dec.set_sampling(*c, seed=42)
        best = None
        for _ in range(args.reps):
            dec.reset()
            dec.feed(prompt)
            dec.run(len(prompt) - 1, with_logits=False, use_graph=True)
            ms = dec.run(args.steps, with_logits=True, use_graph=True)
            best = ms if best is None else min(best, ms)
        out[name + "_us_per_step"] = round(1000 * best / args.steps, 2)
        if c is not None:
            out[name + "_draws"] = dec.sampling_draws()
    for name in ("G", "S", "F"):
        if name + "_us_per_step" in out and "greedy_us_per_step" in out:
            out[name + "_minus_greedy_us"] = round(out[name + "_us_per_step"] - out["greedy_us_per_step"], 2)
    dec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
