#!/usr/bin/env python3
"""Teacher-forced scoring on token ids: the reference's `bitnet-cli score` (crates/bitnet-cli/src/score.rs) and `eval --teacher-force-ids`
(commands/eval.rs) on this project's decoder.  This project has no tokenizer: --ids FILE holds one sequence of integer ids per line.

Each line is one reset(); feed(ids); score(len(ids)) -- one prompt forward plus the tied head over every row (HostDecoder.score), instead of
the reference's one forward per predicted token.  --max-tokens caps the predicted tokens over the whole file (score.rs:96-119).  Output: JSON
with score.rs's keys (type, tokens, mean_nll = f64 total of the f32 per-position values / tokens, ppl = exp(mean_nll), latency.total_ms) plus
eval.rs's std_nll; --dump-logit-steps N --logits-topk K adds eval.rs's LogitStep records (step, topk [id, logit] pairs, chosen_id) of the
first N predicted positions.

  python tools/score.py --synthetic qk256 --layers 2 --vocab 4096 --max-pos 1024 --ids ids.txt
  python tools/score.py --gguf model.gguf --ids ids.txt --json-out score.json"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, pkg, synth):
    if args.gguf:
        f = pkg.GgufFile(path=args.gguf)
        c = f.config()
        nh = c["n_heads"] or 20
        cfg = synth.ModelConfig(hidden=c["hidden"], n_layers=c["n_layers"], n_heads=nh, n_kv_heads=c["n_kv_heads"] or nh, head_dim=c["hidden"] // nh,
                                ffn=c["ffn"], vocab=c["vocab"], max_pos=args.max_pos or 4096, eps=c["eps"] if c["eps"] is not None else 1e-5,
                                rope_theta=c["rope_theta"] if c["rope_theta"] is not None else 10000.0)
        dec = pkg.HostDecoder(cfg)
        dec.load_gguf(f)
        f.close()
        return cfg, dec
    over = {k: v for k, v in (("n_layers", args.layers), ("vocab", args.vocab), ("max_pos", args.max_pos)) if v}
    cfg = synth.ModelConfig(**dict(synth.BITNET_2B_4T, **over))
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=args.synthetic, block=32)
        if args.synthetic == "qk256":
            dec.set_layer_qk256(l, w)
        else:
            dec.set_layer_i2s(l, w, 32)
    dec.set_globals(synth.make_globals(cfg))
    return cfg, dec


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--gguf", help="model file")
    src.add_argument("--synthetic", choices=("i2s", "qk256"), help="the synthetic model of the bench's widths")
    ap.add_argument("--layers", type=int, default=0, help="synthetic: layer count (default 30)")
    ap.add_argument("--vocab", type=int, default=0, help="synthetic: vocabulary size (default 128256)")
    ap.add_argument("--max-pos", type=int, default=0, help="KV cache positions (default 4096); a sequence may hold max_pos - 1 ids")
    ap.add_argument("--ids", required=True, help="one sequence of integer token ids per line")
    ap.add_argument("--max-tokens", type=int, default=0, help="cap on predicted tokens over the whole file (0 = none)")
    ap.add_argument("--digits", type=int, default=2, help="fixed-point digits of the prompt forward (2 = the benchmarked forward)")
    ap.add_argument("--dump-logit-steps", type=int, default=0, help="LogitStep records of the first N predicted positions")
    ap.add_argument("--logits-topk", type=int, default=10, help="entries per LogitStep record")
    ap.add_argument("--json-out", help="write the JSON here instead of stdout")
    args = ap.parse_args(argv)

    pkg = importlib.import_module("bitnet-rs_amd")
    synth = importlib.import_module("bitnet-rs_amd.synth")
    lines = [ln for ln in open(args.ids).read().splitlines() if ln.strip()]
    seqs = [[int(t) for t in ln.replace(",", " ").split()] for ln in lines]
    cfg, dec = build(args, pkg, synth)
    start = time.perf_counter()
    nlls, steps, gpu_ms = [], [], 0.0
    total = 0
    for ids in seqs:
        if len(ids) < 2:
            continue
        steps_left = args.max_tokens - total if args.max_tokens > 0 else len(ids) - 1
        take = min(steps_left, len(ids) - 1)
        if take <= 0:
            break
        if take + 1 > cfg.max_pos - 1:
            raise SystemExit(f"a sequence of {take + 1} ids does not fit max_pos {cfg.max_pos} (at most max_pos - 1 ids)")
        dump = max(0, min(args.dump_logit_steps - total, take))
        dec.reset()
        dec.feed(np.asarray(ids[:take + 1], np.int32))
        r = dec.score(take + 1, digits=args.digits, logits_rows=dump)
        gpu_ms += r.ms
        nlls.append(r.nll[:take])
        for i in range(dump):
            row = r.logits[i]
            k = min(args.logits_topk, row.size)
            top = np.argsort(-np.where(np.isnan(row), -np.inf, row), kind="stable")[:k]
            steps.append({"step": total + i, "topk": [[int(t), float(row[t])] for t in top], "chosen_id": int(ids[i + 1])})
        total += take
        if args.max_tokens > 0 and total >= args.max_tokens:
            break
    dec.close()
    v = np.concatenate(nlls) if nlls else np.zeros(0, np.float32)
    n = int(v.size)
    mean = float(np.sum(v.astype(np.float64))) / n if n else 0.0
    std = math.sqrt(float(np.sum((v.astype(np.float64) - mean) ** 2)) / n) if n else 0.0
    out = {
        "type": "score",
        "model": args.gguf or f"synthetic:{args.synthetic}",
        "dataset": args.ids,
        "tokens": n,
        "mean_nll": mean,
        "ppl": math.exp(mean),
        "std_nll": std,
        "latency": {"total_ms": (time.perf_counter() - start) * 1000.0, "gpu_ms": gpu_ms},
        "tokenizer": {"type": "none", "origin": "token ids"},
        "gen_policy": {"bos": False, "temperature": 0.0, "seed": os.environ.get("BITNET_SEED")},
    }
    if args.dump_logit_steps > 0:
        out["logits_dump"] = steps
    text = json.dumps(out, indent=2)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.write(text)
        print(f"Wrote score results to {args.json_out}")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
