"""The paged decode attention against the rows form (records + combine) on the same sequences, in one sitting: 64 and 8 sequences at 512 and 4096
keys, f16 and f32 caches, n_splits chosen by the library.  Both launches of a shape are timed in interleaved rounds (HIP events around REPS
launches each); per shape the median over the rounds, the ratio, and the sitting's spread (max / min over the rounds of one route) are written to
profiles/paged_summary.json together with the pool's bytes against the contiguous caches' bytes for the sequences' real lengths.
Cache contents are zeros: the launches' time does not depend on the values.  The 2B-4T attention shape: 20 heads, 5 KV heads, head_dim 128.

Then the whole step: PagedBatch.step against WideBatch.step for the SAME members (the synthetic 2B-4T model as bench.py builds it, 30 layers, f16
caches, digits 2, max_pos 512; 64 and 8 greedy members whose prompts hold 40 .. 390 positions, filled by one prefill_packed).  The wide members
are the staging decoders the paged batch admits from.  A round = STEP_N steps of each route, interleaved; between rounds the wide members rewind
and the paged members are released and admitted again (untimed).  Reported per member count: ms per step by HIP events (the forward) and by the
host clock around the call (with the page reservation, the copy-on-write launch and the table uploads), the ratio, the spread, and the pool's
bytes against the members' contiguous caches'."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch as t

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, N_KV, D, MAX_POS, ROUNDS, REPS = 20, 5, 128, 4096, 7, 20


def ptrs(xs):
    return t.tensor([x.data_ptr() for x in xs], dtype=t.int64, device="cuda")


def timed(fn):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    t.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS  # microseconds per launch


def shape(hip, n_seq, keys, f16):
    rng = np.random.default_rng(n_seq + keys)
    lens = rng.integers(keys // 2, keys, n_seq)  # real lengths: the last position of every sequence
    lens[0] = keys - 1
    R = 64 if f16 else 128
    chunks, words = MAX_POS // 64, N_KV * MAX_POS * R
    n_pages = int(sum(l // 64 + 1 for l in lens))
    kpool, vpool = (t.zeros(n_pages * N_KV * 64 * R, dtype=t.int32, device="cuda") for _ in range(2))
    perm, tables, at = rng.permutation(n_pages), [], 0
    for l in lens:
        tab = np.zeros(chunks, np.int32)
        tab[:l // 64 + 1] = perm[at:at + l // 64 + 1]
        at += l // 64 + 1
        tables.append(t.from_numpy(tab).cuda())
    kc, vc = ([t.zeros(words, dtype=t.int32, device="cuda") for _ in range(n_seq)] for _ in range(2))
    pos = [t.tensor([int(l)], dtype=t.int32, device="cuda") for l in lens]
    qkv = t.randn((n_seq, (H + 2 * N_KV) * D), dtype=t.float32, device="cuda")
    sin, cos = (t.zeros((MAX_POS, D // 2), dtype=t.float32, device="cuda") for _ in range(2))
    out = t.zeros((n_seq, H * D), dtype=t.float32, device="cuda")
    splits = hip.attention_paged_splits(n_seq, N_KV, keys)
    sp = t.zeros(hip.attention_paged_scratch_bytes(n_seq, N_KV, splits) // 4, dtype=t.float32, device="cuda")
    sr = t.zeros(n_seq * int(hip.c.bitnet_hip_attention_scratch_bytes(N_KV, MAX_POS)) // 4, dtype=t.float32, device="cuda")
    tp, pp, kp, vp = ptrs(tables), ptrs(pos), ptrs(kc), ptrs(vc)
    paged = lambda: hip.attention_decode_paged_dev(qkv, sin, cos, kpool, vpool, n_pages, tp, pp, n_seq, H, N_KV, D, MAX_POS, keys, 0, sp, out, kv_f16=f16)  # noqa: E731
    rows = lambda: hip.attention_decode_rows_dev(qkv, sin, cos, kp, vp, pp, n_seq, H, N_KV, D, MAX_POS, keys, sr, out, kv_f16=f16)  # noqa: E731
    for fn in (paged, rows):  # warm-up
        timed(fn)
    tp_, tr_ = [], []
    for _ in range(ROUNDS):
        tp_.append(timed(paged))
        tr_.append(timed(rows))
    page_bytes = N_KV * 64 * R * 4 * 2  # K and V of one layer
    return dict(n_seq=n_seq, keys=keys, cache="f16" if f16 else "f32", n_splits=int(splits), paged_us=float(np.median(tp_)), rows_us=float(np.median(tr_)),
                paged_over_rows=float(np.median(tp_) / np.median(tr_)), spread_paged=float(max(tp_) / min(tp_)), spread_rows=float(max(tr_) / min(tr_)),
                pool_bytes_per_layer=n_pages * page_bytes, contiguous_bytes_per_layer=n_seq * (MAX_POS // 64) * page_bytes)


STEP_N, STEP_ROUNDS, STEP_MAX_POS = 16, 5, 512


def steps(pkg, layers):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg = synth.ModelConfig(**synth.BITNET_2B_4T)
    cfg.max_pos, cfg.n_layers = STEP_MAX_POS, layers
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    owner.set_globals(synth.make_globals(cfg))
    owner.set_kv_f16(True)
    wide = [owner] + [owner.shared() for _ in range(63)]
    lens = [40 + (350 * i) // 63 for i in range(64)]
    prompt = synth.prompt(max(lens) + 64, cfg.vocab)
    for i, d in enumerate(wide):
        d.set_kv_f16(True)
        d.feed(prompt[i:i + lens[i]])
    wide[0].prefill_packed(wide, lens, with_logits=True, digits=2)
    out = []
    for M in (64, 8):
        idx = list(range(M)) if M == 64 else list(range(0, 64, 8))  # the 8 keep the spread of lengths
        n_pages = sum((lens[i] + STEP_N + 63) // 64 for i in idx)
        wb, pb = pkg.HostWideBatch(M), pkg.HostPagedBatch(owner, n_pages, M)
        for b, i in enumerate(idx):
            wb.set_slot(b, wide[i])

        def admit():
            for b, i in enumerate(idx):
                pb.admit(b, wide[i], lens[i])

        def clocked(batch):
            t0 = time.perf_counter()
            ev = batch.step(STEP_N, 2)
            return ev / STEP_N, (time.perf_counter() - t0) * 1e3 / STEP_N

        samples = {"wide": [], "paged": []}
        for r in range(STEP_ROUNDS + 1):  # round 0 warms both routes
            admit()
            for name, batch in (("paged", pb), ("wide", wb)):
                s = clocked(batch)
                if r:
                    samples[name].append(s)
            for b, i in enumerate(idx):
                pb.release(b)
                wide[i].rewind(lens[i])
        med = {k: (float(np.median([s[0] for s in v])), float(np.median([s[1] for s in v]))) for k, v in samples.items()}
        spread = max(max(s[0] for s in v) / min(s[0] for s in v) for v in samples.values())
        slots = (cfg.max_pos + 63) // 64 * 64
        out.append(dict(members=M, steps=STEP_N, lengths=f"{lens[idx[0]]}..{lens[idx[-1]]}, evenly spaced", paged_ms_per_step_events=med["paged"][0], wide_ms_per_step_events=med["wide"][0],
                        paged_ms_per_step_host=med["paged"][1], wide_ms_per_step_host=med["wide"][1], paged_over_wide_events=med["paged"][0] / med["wide"][0],
                        paged_over_wide_host=med["paged"][1] / med["wide"][1], spread_events=float(spread), pool_pages=n_pages, pool_bytes=pb.pool_bytes(),
                        contiguous_bytes=M * 2 * cfg.n_layers * cfg.n_kv_heads * slots * cfg.head_dim * 2))
        print(json.dumps(out[-1]), flush=True)
        for b in range(M):
            wb.set_slot(b, None)
        wb.close()
        pb.close()
    for d in reversed(wide):
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "paged_summary.json"))
    ap.add_argument("--layers", type=int, default=30)
    args = ap.parse_args()
    pkg = importlib.import_module("bitnet-rs_amd")
    hip = pkg.load()
    rows = [shape(hip, n_seq, keys, f16) for f16 in (True, False) for n_seq in (64, 8) for keys in (512, 4096)]
    for r in rows:
        print(json.dumps(r), flush=True)
    t.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(dict(device=t.cuda.get_device_name(0), rounds=ROUNDS, reps=REPS, shapes=rows, step_rounds=STEP_ROUNDS, steps=steps(pkg, args.layers)), f, indent=1)


if __name__ == "__main__":
    main()
