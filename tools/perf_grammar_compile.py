#!/usr/bin/env python3
"""Developer tool (GPU box): the grammar compile on the device against the numpy route, in one sitting.

    python3 tools/perf_grammar_compile.py                      # the table -> profiles/grammar_compile_summary.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/perf_grammar_compile.py --one 4000
    python3 tools/perf_grammar_compile.py --stats DIR          # folds the trace's per-kernel shares into the summary

Vocabulary: 128256 synthetic tokens of 1..16 bytes (one in 40 cut from the grammar's own keywords, half lowercase strings, the rest digits,
punctuation and arbitrary bytes).  DFAs: a trie of random keywords grown to about 100 / 1000 / 4000 states, every keyword followed by ':', a
digit loop and ',' back to the root -- the shape a JSON-schema front end emits, literal-heavy with a few loops.  Per DFA, alternating run by run,
compile_on_device (host clock; the call is synchronous; 5 timed runs after one warm-up) and token_automaton + lib.grammar(...) (5 runs, or as
many as fit NUMPY_BUDGET seconds per DFA -- the count is recorded).  A numpy cell that cannot allocate, or whose first run is estimated from the
previous DFA to pass NUMPY_SKIP seconds, is recorded as such and not run.  The two routes' tables are compared once per DFA (class count and
the expanded function)."""
import glob
import importlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "grammar_compile_summary.json")
VOCAB, SIZES, RUNS, TS = 128256, (100, 1000, 4000), 5, 32
NUMPY_BUDGET, NUMPY_SKIP = 150.0, 300.0


def keywords(rng, n_states):
    """random lowercase keywords until their trie has about n_states states"""
    words, states = [], 3
    while states < n_states:
        w = bytes(rng.integers(97, 123, int(rng.integers(6, 25))).tolist())
        words.append(w)
        states += len(w)  # an upper bound: shared prefixes are rare at these lengths
    return words


def make_dfa(G, words):
    trie = G.ByteDFA.from_choices(words)
    n = trie.n + 1  # + the value state
    nx = np.full((n, 256), -1, np.int32)
    nx[:trie.n] = trie.next
    value = trie.n
    for leaf in trie.accepting:
        nx[leaf, ord(":")] = value
    nx[value, 48:58] = value
    nx[value, ord(",")] = 0
    return G.ByteDFA(nx, 0, [value])


def make_vocab(rng, words):
    blob = b":".join(words)
    toks = [b"<eos>"]
    for i in range(1, VOCAB):
        ln = int(min(16, 1 + rng.geometric(0.22)))
        kind = 0 if i % 40 == 0 else 1 + i % 2  # some 3200 tokens spell pieces of the keywords, as a real vocabulary would
        if kind == 0:
            at = int(rng.integers(0, len(blob) - ln))
            toks.append(blob[at:at + ln])
        elif kind == 1:
            toks.append(bytes(rng.integers(97, 123, ln).tolist()))
        else:
            toks.append(bytes(rng.choice(np.frombuffer(b"0123456789:,{}\" \n", np.uint8), ln).tolist()) if i % 2 else bytes(rng.integers(0, 256, ln).tolist()))
    return toks


def device_bytes(n, total_bytes):
    """what one compile holds at its peak, from the sizes (kernels_gramc.hip): the DFA table, vals, two class buffers, the slot table, leaders"""
    slots = 64
    while slots < 2 * VOCAB:
        slots *= 2
    return n * 1024 + n + VOCAB * TS * 4 + 2 * VOCAB * 4 + slots * 4 + 16384 * 4 + 8 + VOCAB * 2 + total_bytes + (VOCAB + 1) * 4


def spread(xs):
    return {"median_ms": round(statistics.median(xs) * 1e3, 3), "min_ms": round(min(xs) * 1e3, 3), "max_ms": round(max(xs) * 1e3, 3), "runs": len(xs)}


def fold_stats(directory):
    import csv

    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(path)) if "gramc" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    summary = json.load(open(OUT))
    summary["kernel_share_4000_states"] = {re.search(r"k_gramc_\w+", r["Name"]).group(0): {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
                                                                                         "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows}
    json.dump(summary, open(OUT, "w"), indent=1)
    print(json.dumps(summary["kernel_share_4000_states"], indent=1))


def main():
    if "--stats" in sys.argv:
        return fold_stats(sys.argv[sys.argv.index("--stats") + 1])
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    pkg = importlib.import_module("bitnet-rs_amd")
    G = importlib.import_module("bitnet-rs_amd.grammar")
    lib = pkg.load()
    lib.init(0)
    one = int(sys.argv[sys.argv.index("--one") + 1]) if "--one" in sys.argv else None
    cells, host_per_state = [], 0.0
    for n_target in ((one,) if one else SIZES):
        rng = np.random.default_rng(n_target)
        words = keywords(rng, n_target)
        dfa, toks = make_dfa(G, words), make_vocab(rng, words)
        vh = lib.vocab(toks)
        g, _ = G.compile_on_device(lib, dfa, vh, 0)  # warm-up: code objects, allocator
        if one:
            print("one compile at", dfa.n, "states:", g.info())
            return
        cell = {"dfa_states": dfa.n, "vocab": VOCAB, "classes_device": g.info()[2], "device_bytes": device_bytes(dfa.n, sum(map(len, toks)))}
        dev, host, ref = [], [], None
        est = host_per_state * dfa.n
        try:
            if est > NUMPY_SKIP:
                cell["numpy"] = f"not run: about {est:.0f} s per run, estimated from the previous DFA"
            else:
                t0 = time.perf_counter()
                ref = G.token_automaton(dfa, toks, 0)
                lib.grammar(ref[0], ref[1]).close()
                host.append(time.perf_counter() - t0)
                tc, nx = g.tables()
                cell["classes_numpy"] = int(ref[1].shape[1])
                cell["tables_equal"] = bool(cell["classes_numpy"] == cell["classes_device"] and np.array_equal(nx[:, tc], ref[1][:, ref[0]]))
        except MemoryError as e:
            ref, host, cell["numpy"] = None, [], f"could not allocate: {e}"
        for _ in range(RUNS):  # alternating, so both routes see the same minutes of the shared host
            t0 = time.perf_counter()
            G.compile_on_device(lib, dfa, vh, 0)[0].close()
            dev.append(time.perf_counter() - t0)
            if ref is not None and len(host) < RUNS and sum(host) < NUMPY_BUDGET:
                t0 = time.perf_counter()
                r = G.token_automaton(dfa, toks, 0)
                lib.grammar(r[0], r[1]).close()
                host.append(time.perf_counter() - t0)
        cell["compile_on_device"] = spread(dev)
        if host:
            cell["numpy_route"] = spread(host)
            cell["speedup_of_medians"] = round(statistics.median(host) / statistics.median(dev), 1)
            host_per_state = statistics.median(host) / dfa.n
        print(json.dumps(cell), flush=True)
        cells.append(cell)
    json.dump({"tool": "tools/perf_grammar_compile.py", "cells": cells}, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
