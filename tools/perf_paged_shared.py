"""The fork groups' paged decode attention (bitnet_hip_attention_decode_paged_shared_dev) against bitnet_hip_attention_decode_paged_dev on the same
sequences, in one sitting: 8 / 32 / 64 members that share 512 / 4096 positions and hold one private page each, f16 and f32 pools, split counts
chosen by the library.  --base-lib names the library whose paged entry is the baseline (a build of the parent commit; default: this build's).
Both launches of a shape are timed in interleaved rounds (HIP events around REPS launches each); per shape the median over the rounds, the ratio
and the sitting's spread (max / min over the rounds of one route) go to profiles/paged_shared_summary.json.  Pool contents are zeros: the
launches' time does not depend on the values.  The 2B-4T attention shape: 20 heads, 5 KV heads, head_dim 128.

Then the whole step: PagedBatch.step with set_share(1) against set_share(0) on the synthetic 2B-4T model (f16 pools, digits 2): 8 / 32 / 64 forks
of one 448-token prompt, and the UNGROUPED case -- 8 members admitted separately, share on -- which shows what finding no group costs.  One
process, no retries; run it under `timeout`."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch as t

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, N_KV, D, ROUNDS, REPS = 20, 5, 128, 7, 20


def ptrs(xs):
    return t.tensor([x.data_ptr() for x in xs], dtype=t.int64, device="cuda")


def timed(fn):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    t.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS  # microseconds per call


def shape(hip, base, members, shared_pos, f16):
    S, R = shared_pos // 64, 64 if f16 else 128
    max_pos = shared_pos + 64
    n_pages = S + members
    kpool, vpool = (t.zeros(n_pages * N_KV * 64 * R, dtype=t.int32, device="cuda") for _ in range(2))
    perm = np.random.default_rng(members + shared_pos).permutation(n_pages)
    tables = [t.from_numpy(np.concatenate([perm[:S], perm[S + m:S + m + 1]]).astype(np.int32)).cuda() for m in range(members)]
    pos = [t.tensor([shared_pos + (7 * m) % 63], dtype=t.int32, device="cuda") for m in range(members)]
    qkv = t.randn((members, (H + 2 * N_KV) * D), dtype=t.float32, device="cuda")
    sin, cos = (t.zeros((max_pos, D // 2), dtype=t.float32, device="cuda") for _ in range(2))
    out = t.zeros((members, H * D), dtype=t.float32, device="cuda")
    splits, nss = hip.attention_paged_splits(members, N_KV, max_pos), hip.attention_paged_shared_splits(1, N_KV, S)
    scratch = t.zeros(hip.attention_paged_shared_scratch_bytes(members, N_KV, splits, nss) // 4, dtype=t.float32, device="cuda")
    tp, pp, leader, run = ptrs(tables), ptrs(pos), [0] * members, [S] * members
    plain = lambda: base.attention_decode_paged_dev(qkv, sin, cos, kpool, vpool, n_pages, tp, pp, members, H, N_KV, D, max_pos, max_pos, 0, scratch, out, kv_f16=f16)  # noqa: E731
    shared = lambda: hip.attention_decode_paged_shared_dev(qkv, sin, cos, kpool, vpool, n_pages, tp, pp, members, H, N_KV, D, max_pos, max_pos, 0, scratch, out,  # noqa: E731
                                                           leader, run, 0, kv_f16=f16)
    for fn in (plain, shared):  # warm-up
        timed(fn)
    tb, ts = [], []
    for _ in range(ROUNDS):
        tb.append(timed(plain))
        ts.append(timed(shared))
    return dict(members=members, shared_positions=shared_pos, pool="f16" if f16 else "f32", n_splits=int(splits), n_shared_splits=int(nss),
                paged_us=float(np.median(tb)), shared_us=float(np.median(ts)), shared_over_paged=float(np.median(ts) / np.median(tb)),
                spread_paged=float(max(tb) / min(tb)), spread_shared=float(max(ts) / min(ts)))


STEP_N, STEP_ROUNDS, PROMPT = 8, 5, 448


def steps(pkg, layers):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T)
    cfg.max_pos, cfg.n_layers = 512, layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    owner.set_globals(synth.make_globals(cfg))
    owner.set_kv_f16(True)
    stage = [owner.shared() for _ in range(8)]
    prompt = synth.prompt(PROMPT + 16, cfg.vocab)
    for i, d in enumerate(stage):
        d.set_kv_f16(True)
        d.feed(prompt[i:i + PROMPT + 1])
        d.prefill(PROMPT, with_logits=False, digits=2)
    out = []
    for name, M in (("forks", 8), ("forks", 32), ("forks", 64), ("ungrouped", 8)):
        pb = pkg.HostPagedBatch(owner, 8 * M + 16, M)

        def seat():
            if name == "forks":
                pb.admit(0, stage[0], PROMPT)
                for b in range(1, M):
                    pb.fork(0, b)
            else:
                for b in range(M):
                    pb.admit(b, stage[b], PROMPT)

        samples = {0: [], 1: []}
        rows = 0
        for r in range(STEP_ROUNDS + 1):  # round 0 warms both routes
            for share in (0, 1):
                seat()
                pb.set_share(share)
                t0 = time.perf_counter()
                ev = pb.step(STEP_N, 2)
                host = (time.perf_counter() - t0) * 1e3
                rows = max(rows, pb.shared_rows())
                if r:
                    samples[share].append((ev / STEP_N, host / STEP_N))
                for b in range(M):
                    pb.release(b)
        med = {k: (float(np.median([s[0] for s in v])), float(np.median([s[1] for s in v]))) for k, v in samples.items()}
        spread = max(max(s[0] for s in v) / min(s[0] for s in v) for v in samples.values())
        out.append(dict(case=name, members=M, prompt=PROMPT, steps=STEP_N, shared_rows=int(rows), off_ms_per_step_events=med[0][0], on_ms_per_step_events=med[1][0],
                        off_ms_per_step_host=med[0][1], on_ms_per_step_host=med[1][1], on_over_off_events=med[1][0] / med[0][0],
                        on_over_off_host=med[1][1] / med[0][1], spread_events=float(spread)))
        print(json.dumps(out[-1]), flush=True)
        pb.close()
    for d in reversed(stage):
        d.close()
    owner.close()
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "paged_shared_summary.json"))
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--layers", type=int, default=30)
    args = ap.parse_args()
    pkg = importlib.import_module("bitnet-rs_amd")
    hip = pkg.load()
    base = hip
    if args.base_lib:  # an older build lacks the newer entries: bind the paged header's alone
        import ctypes as C

        base = object.__new__(pkg.HipLib)
        base.path, base.c = args.base_lib, C.CDLL(os.path.abspath(args.base_lib))
        pkg.cproto.bind(base.c, pkg.paged_prototypes(), pkg.C_STRUCTS)
        base.c.bitnet_hip_get_last_error.restype = C.c_char_p
    rows = [shape(hip, base, m, sp, f16) for f16 in (True, False) for m in (8, 32, 64) for sp in (512, 4096)]
    for r in rows:
        print(json.dumps(r), flush=True)
    t.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(dict(device=t.cuda.get_device_name(0), baseline="parent build" if args.base_lib else "this build", rounds=ROUNDS, reps=REPS, shapes=rows,
                       step_rounds=STEP_ROUNDS, steps=steps(pkg, args.layers)), f, indent=1)


if __name__ == "__main__":
    main()
