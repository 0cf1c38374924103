"""CPU: host/prefix_index.hpp -- the prefix cache's trie, limits, eviction policies and statistics (the reference's PrefixCache,
crates/bitnet-inference/src/prefix_cache.rs, over opaque entries) -- through tests/host/prefix_index_check.cpp, a stand-alone program built
under the address and undefined-behaviour sanitizers and run as a child process.  Nothing is loaded into Python under a sanitizer.

Without arguments the program runs the scripted cases (the reference's unit tests restated, each policy's victim, the LFU tie, the TTL
fallback, both limits, "unable to free space", evict-before-replace, clear, every statistics field by value).  With a script file it applies
one operation per line; the differential sweep below generates a few thousand random operations per configuration and compares every result
line with a dictionary-based model written here from the reference's text: entries in a dict by id, keys in a dict by token tuple, no trie."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LRU, LFU, FIFO, TTL = range(4)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("prefix_index") / "prefix_index_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", f"-I{os.path.join(ROOT, 'bitnet-rs_amd', 'host')}", os.path.join(ROOT, "tests", "host", "prefix_index_check.cpp"), "-o", path]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    return path


def clean(run):
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]


def test_prefix_index_header_needs_no_hip():
    text = open(os.path.join(ROOT, "bitnet-rs_amd", "host", "prefix_index.hpp")).read()
    includes = [line for line in text.splitlines() if line.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i or '"' in i]  # the standard library only


def test_scripted_cases_under_sanitizers(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    clean(run)
    assert "prefix_index_check: ok" in run.stdout, run.stdout[-2000:]


class Model:
    """The reference's PrefixCache restated on dictionaries.  Time: a counter that moves with every stamp; TTL on the caller's seconds."""

    def __init__(self, max_entries, max_bytes, policy, min_len, ttl):
        self.max_entries, self.max_bytes, self.policy, self.min_len, self.ttl = max_entries, max_bytes, policy, min_len, ttl
        self.next_id = self.clock = 0
        self.clear()

    def clear(self):
        self.entries, self.by_key, self.memory = {}, {}, 0
        self.lookups = self.hits = self.matched = self.evictions = 0

    def stamp(self):
        self.clock += 1
        return self.clock

    def remove(self, i):
        e = self.entries.pop(i)
        del self.by_key[e["key"]]
        self.memory -= e["size"]

    def lookup(self, toks):
        self.lookups += 1
        for m in range(len(toks), 0, -1):  # the longest key that is a prefix of the query
            i = self.by_key.get(tuple(toks[:m]))
            if i is not None:
                e = self.entries[i]
                e["hits"] += 1
                e["last"] = self.stamp()
                self.hits += 1
                self.matched += m
                return f"L 1 {m} {i}"
        return "L 0 0 0"

    def evict(self, now):
        if not self.entries:
            return None
        items = list(self.entries.items())
        if self.policy == LRU:
            i = min(items, key=lambda kv: kv[1]["last"])[0]
        elif self.policy == LFU:
            i = min(items, key=lambda kv: (kv[1]["hits"], kv[1]["last"]))[0]
        else:
            pool = [kv for kv in items if now >= kv[1]["secs"] and now - kv[1]["secs"] >= self.ttl] if self.policy == TTL else []
            i = min(pool or items, key=lambda kv: kv[1]["created"])[0]
        self.remove(i)
        self.evictions += 1
        return i

    def insert(self, size, now, toks):
        if len(toks) < self.min_len:
            return "I 0 0"
        gone = []
        while len(self.entries) >= self.max_entries or self.memory + size > self.max_bytes:
            v = self.evict(now)
            if v is None:
                return " ".join(["I 0 0"] + [str(g) for g in gone])
            gone.append(v)
        old = self.by_key.get(tuple(toks))
        if old is not None:
            self.remove(old)
            gone.append(old)
        i = self.next_id
        self.next_id += 1
        t = self.stamp()
        self.entries[i] = {"key": tuple(toks), "size": size, "hits": 0, "last": t, "created": t, "secs": now}
        self.by_key[tuple(toks)] = i
        self.memory += size
        return " ".join([f"I 1 {i}"] + [str(g) for g in gone])

    def invalidate(self, toks):
        i = self.by_key.get(tuple(toks))
        if i is None:
            return "V 0 0"
        self.remove(i)
        return f"V 1 {i}"

    def stats(self):
        hr = self.hits / self.lookups if self.lookups else 0.0
        mr = 1.0 - hr if self.lookups else 0.0
        avg = self.matched / self.hits if self.hits else 0.0
        return f"S {len(self.entries)} {self.evictions} {self.memory} {hr!r} {mr!r} {avg!r}"


def sweep(rng, cfg, n_ops):
    """-> (script lines, the model's result lines).  Tokens from a 3-letter alphabet and keys of length 0..6: prefixes of one another, repeated
    keys and shared trie paths are the common case, not the exception."""
    model = Model(*cfg)
    script, want = ["C " + " ".join(str(v) for v in cfg)], []
    now = 0
    key = lambda: [int(t) for t in rng.integers(0, 3, size=int(rng.integers(0, 7)))]
    for _ in range(n_ops):
        now += int(rng.integers(0, 4))
        r = rng.random()
        if r < 0.40:
            t = key() + ([int(rng.integers(0, 3))] if rng.random() < 0.5 else [])
            script.append("L " + " ".join(map(str, t)))
            want.append(model.lookup(t))
        elif r < 0.80:
            t, size = key(), int(rng.integers(0, 40))
            script.append(f"I {size} {now} " + " ".join(map(str, t)))
            want.append(model.insert(size, now, t))
        elif r < 0.86:
            script.append(f"E {now}")
            v = model.evict(now)
            want.append("E 0 0" if v is None else f"E 1 {v}")
        elif r < 0.94:
            t = key()
            script.append("V " + " ".join(map(str, t)))
            want.append(model.invalidate(t))
        elif r < 0.95:
            script.append("X")
            model.clear()
            want.append("X")
        else:
            script.append("S")
            want.append(model.stats())
    script.append("S")
    want.append(model.stats())
    return script, want


@pytest.mark.parametrize("policy", [LRU, LFU, FIFO, TTL], ids=["lru", "lfu", "fifo", "ttl"])
def test_random_operations_against_the_dictionary_model(exe, tmp_path, policy):
    rng = np.random.default_rng(4200 + policy)
    # (max_entries, max_bytes, policy, min_prefix_length, ttl_seconds): a roomy index, a tight entry limit, a tight byte limit (some entries never fit)
    for k, cfg in enumerate([(64, 4000, policy, 1, 40), (5, 4000, policy, 2, 25), (50, 60, policy, 0, 10), (3, 30, policy, 1, 5)]):
        script, want = sweep(rng, cfg, 1500)
        path = tmp_path / f"ops{k}.txt"
        path.write_text("\n".join(script) + "\n")
        run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        clean(run)
        got = run.stdout.splitlines()
        assert len(got) == len(want), (cfg, len(got), len(want))
        for line, (g, w) in enumerate(zip(got, want)):
            if g.startswith("S "):  # the floats by value, whatever digits either side prints
                gs, ws = g.split(), w.split()
                assert gs[:4] == ws[:4] and [float(v) for v in gs[4:]] == [float(v) for v in ws[4:]], (cfg, line, script[line + 1], g, w)
            else:
                assert g == w, (cfg, line, script[line + 1], g, w)
        assert sum(w.startswith("I 1") and len(w.split()) > 3 for w in want) > 20, cfg  # evictions and replacements did happen
