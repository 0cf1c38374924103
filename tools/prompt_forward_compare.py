#!/usr/bin/env python3
"""Does a libbitnet_host.so refuse and run the prompt forward the way another one does?  The check for a change of the host layer between
Decoder::chain_applies and Decoder::finish_prefill (host/decoder.cpp: PromptForm, the four project_* functions, forward_with_repeat, AttnOp,
the guards) that leaves the kernels alone (tools/isa_equal.py proves that half):
    python tools/prompt_forward_compare.py refusals [HOSTLIB]   every refusal of the six prompt entries (prefill, extend, prefill_packed, step_wide,
                                                                 score, prefill_sharded), one fault at a time and then the multi-fault cases that pin
                                                                 each entry's order of precedence: entry | case | rc | message | position afterwards
    python tools/prompt_forward_compare.py paths [HOSTLIB]      every driver on models A and B of tests/test_decoder_state_gpu.py and the outlier variant
                                                                 of model A (the saturation repeat runs), both weight formats, both cache types, under
                                                                 every switch setting of SWITCHES: a SHA-256 of last_logits, last_hidden, the history
                                                                 and every layer's K and V cache (tests/kv_read.py), the position, last_prefill_path(),
                                                                 saturation_fallbacks() and matmul_last_tile()
HOSTLIB defaults to this tree's library; build the other revision's in a worktree and diff the two outputs: they must be equal line for line (the
kernels are deterministic).  `paths` starts one child per switch setting (some switches are read once per decoder or process), one at a time, each
under `timeout -k 10` sized to its work (a dozen small models, a few seconds each), and stops at the first child that does not exit 0: a refusal is a
line, anything else (a GPU error, a fault, a timeout) ends the sitting and nothing more may start.
    python tools/prompt_forward_compare.py child SETTING [MODELS] [HOSTLIB]   one child by hand, e.g. `child default A` under
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/prompt_forward_compare.py child default A
    (nothing else collected in that run) for the list of kernel names to compare between the two libraries."""
import ctypes as C
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SWITCHES = {
    "default": {},
    "chain0": {"BITNET_HOST_PREFILL_CHAIN": "0"},
    "chain1": {"BITNET_HOST_PREFILL_CHAIN": "1"},
    "fp6_0": {"BITNET_HOST_PREFILL_FP6": "0"},
    "hybrid0": {"BITNET_HOST_PREFILL_HYBRID": "0"},
    "hybrid2": {"BITNET_HOST_PREFILL_HYBRID": "2"},
    "qb32": {"BITNET_HOST_PREFILL_QB32": "1", "BITNET_HOST_PREFILL_HYBRID": "2"},
    "fp6od": {"BITNET_HOST_PREFILL_FP6_OD": "1"},
}
CHILD_SECONDS = 300
WORLDS = [("A", False), ("B", False), ("A", True)]  # (model, outlier)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def setup(host_lib):
    import torch  # noqa: F401  (ahead of the library: bitnet-rs_amd.load())
    import kv_read
    import test_decoder_state_gpu as ds
    from oracle import oracle as orc

    pkg = importlib.import_module("bitnet-rs_amd")
    hip = pkg.load()
    hip.init(0)
    synth = importlib.import_module("bitnet-rs_amd.synth")
    path = host_lib or pkg.HOST_LIB_PATH
    # a host library of another tree runs on the kernel library next to it ($ORIGIN): matmul_last_tile() is asked of that instance
    beside = os.path.join(os.path.dirname(os.path.abspath(path)), "libbitnet_hip.so")
    if os.path.exists(beside) and not os.path.samefile(beside, pkg.LIB_PATH):
        hip = pkg.HipLib(beside)
        hip.init(0)

    def decoder(W, kv16, cfg=None):
        dec = pkg.HostDecoder(cfg or W.cfg, path=path)
        for l, w in enumerate(W.layers):
            dec.set_layer_qk256(l, w) if W.fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
        dec.set_globals(W.glob)
        dec.reset()
        dec.set_kv_f16(kv16)
        return dec

    return pkg, hip, synth, orc, ds, kv_read, decoder, path


# ---------------------------------------------------------------- paths
def child(setting, models, host_lib):
    pkg, hip, synth, orc, ds, kv, decoder, _ = setup(host_lib)
    for model, outlier in WORLDS:
        if model + ("o" if outlier else "") not in models:
            continue
        for fmt in ("i2s", "qk256"):
            W = ds.World(synth, orc, model, fmt, outlier)
            for kv16 in (False, True):
                tag = f"{setting} {model}{'-outlier' if outlier else ''} {fmt} {'kv16' if kv16 else 'kv32'}"
                run_cases(pkg, hip, kv, decoder, W, kv16, tag)


def run_cases(pkg, hip, kv, decoder, W, kv16, tag):
    cfg, P = W.cfg, W.prompt

    def state(dec):
        p = dec.position()
        caches = " ".join(f"L{l} {sha(k)} {sha(v)}" for l in range(cfg.n_layers) for k, v in [kv.raw(dec, cfg, l, kv16)])
        try:
            tile = ",".join(f"{k}={v}" for k, v in sorted(dict(hip.matmul_last_tile()).items()))
        except pkg.BitNetHipError:  # (the f16 chain launches no tiled matmul)
            tile = "none"
        return (f"pos {p} logits {sha(dec.last_logits())} hidden {sha(dec.last_hidden())} history {sha(dec.history(p + 1))} {caches} "
                f"path {dec.last_prefill_path()} fallbacks {dec.saturation_fallbacks()} tile {tile}")

    def emit(name, dec, extra=""):
        print(f"{tag} | {name} | {extra}{state(dec)}", flush=True)

    def case(name, fn, *decs):
        """one driver call -> one line per decoder; a call the library refuses on the host (a form a launcher does not take at this size) is a
        line too, by the library's own message; a GPU error ends the process"""
        try:
            extra = fn() or ""
        except pkg.BitNetHipError as e:
            if e.code == pkg.ERR_GPU:
                raise
            print(f"{tag} | {name} | refused: {str(e).split('): ', 1)[-1]}", flush=True)
            return
        for i, d in enumerate(decs):
            emit(name + (f", member {i}" if len(decs) > 1 else ""), d, extra)

    def at(dec, toks, past):
        """a live sequence at position `past` with `toks` fed"""
        dec.reset()
        dec.feed(toks)
        if past:
            dec.prefill(past, with_logits=False, digits=2)

    dec = decoder(W, kv16)
    for digits in (2, 3, 4):
        for n in (65, 130):
            at(dec, P[:n], 0)
            case(f"prefill({n}, digits={digits})", lambda: dec.prefill(n, with_logits=True, digits=digits) and None, dec)
    for past, n in ((70, 37), (33, 1), (0, 50)):
        case(f"extend({n}) at {past}", lambda: (at(dec, P[:past + n], past), dec.extend(n, with_logits=True, digits=2)) and None, dec)

    def score():
        res = dec.score(65, digits=2, logits_rows=2)
        return f"nll {sha(res.nll)} argmax {sha(res.argmax)} rows {sha(res.logits)} "

    at(dec, P[:65], 0)
    case("score(65, logits_rows=2)", score, dec)
    for digits, wire_f16, timing in ((2, False, False), (2, True, False), (2, False, True), (2, True, True), (3, True, False)):
        at(dec, P[:128], 0)
        dec.set_phase_timing(timing)
        case(f"prefill_sharded(128, world 1, digits={digits}, wire_f16={int(wire_f16)}, timing={int(timing)})",
             lambda: dec.prefill_sharded(128, 0, 1, None, with_logits=True, digits=digits, wire_f16=wire_f16) and None, dec)
    dec.set_phase_timing(False)
    # three members, each its own tokens: the owner and two borrowers
    ms = [dec, dec.shared(), dec.shared()]
    for m in ms[1:]:
        m.set_kv_f16(kv16)
    toks = [np.asarray((P + 17 * i) % cfg.vocab, np.int32) for i in range(3)]
    pasts, ns = (0, 21, 64), (33, 1, 64)

    def place(where, extra):
        for m, t, p, n in zip(ms, toks, where, extra):
            at(m, t[:p + n], p)

    case(f"prefill_packed pasts {pasts} lengths {ns}", lambda: (place(pasts, ns), dec.prefill_packed(ms, list(ns), with_logits=True, digits=2)) and None, *ms)
    pos = (64, 5, 130)
    case(f"step_wide at {pos}, step 1 (greedy)", lambda: (place(pos, (1, 1, 1)), dec.step_wide(ms, 1, digits=2)) and None, *ms)
    ms[1].set_sampling(0.8, top_k=40, top_p=0.95, seed=7)
    case(f"step_wide at {pos}, step 2 (member 1 samples, seed 7)", lambda: dec.step_wide(ms, 1, digits=2) and None, *ms)
    for m in reversed(ms):
        m.close()


def paths(host_lib):
    for setting, env in SWITCHES.items():
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "child", setting, "A,B,Ao"] + ([host_lib] if host_lib else [])
        rc = subprocess.run(cmd, env={**os.environ, **env}).returncode
        if rc != 0:
            sys.exit(f"child {setting} ended with status {rc}: nothing more is started")


# ---------------------------------------------------------------- refusals
def refusals(host_lib):
    pkg, hip, synth, orc, ds, kv, decoder, path = setup(host_lib)
    W = ds.World(synth, orc, "A", "qk256")
    P, MP = W.prompt, W.cfg.max_pos
    ms_out = C.c_float(0)

    def report(entry, case, fn, *watch):
        try:
            rc, msg = fn(), ""
        except pkg.BitNetHipError as e:
            rc, msg = e.code, str(e)
        if rc:
            msg = msg or watch[0].error()
        print(f"{entry} | {case} | {rc} | {msg if rc else ''} | positions {[d.position() for d in watch]}", flush=True)

    def packed(members, ns, n_members=None):
        arr = (C.c_void_p * max(len(members), n_members or 0, 1))(*[m.h if m is not None else None for m in members])  # (the library reads n_members handles)
        n = None if ns is None else np.asarray(ns, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        return members[0].c.bitnet_host_prefill_packed(arr, n, len(members) if n_members is None else n_members, 1, 2, C.byref(ms_out))

    def wide(members, n_steps, n_members=None):
        arr = (C.c_void_p * max(len(members), n_members or 0, 1))(*[m.h if m is not None else None for m in members])  # (the library reads n_members handles)
        return members[0].c.bitnet_host_step_wide(arr, len(members) if n_members is None else n_members, n_steps, 2, C.byref(ms_out))

    def fed(dec, n, past=0):
        dec.reset()
        dec.feed(P[:n])
        if past:
            dec.prefill(past, with_logits=False, digits=2)
        return dec

    bare = pkg.HostDecoder(W.cfg, path=path)  # no weights, no globals
    dec = decoder(W, False)
    other = decoder(W, False)                  # another owner: other weights as far as root() goes
    b1, b16 = dec.shared(), dec.shared()
    b16.set_kv_f16(True)
    small = decoder(W, False, synth.ModelConfig(**dict(ds.MODELS["A"], max_pos=128)))
    sharded = lambda d, n, rank=0, world=1: d.prefill_sharded(n, rank, world, None, with_logits=True, digits=2, wire_f16=True) and 0

    # ---- model globals not set: ahead of everything else an entry checks ----
    report("prefill", "no globals + n 0", lambda: bare.prefill(0) and 0, bare)
    report("extend", "no globals + n 0", lambda: bare.extend(0) and 0, bare)
    report("score", "no globals + n 0", lambda: bare.score(0) and 0, bare)
    report("prefill_sharded", "no globals + bad rank", lambda: sharded(bare, 100, 3, 1), bare)
    report("prefill_packed", "driver without globals", lambda: packed([bare], [1]), bare)
    report("step_wide", "driver without globals", lambda: wide([bare], 1), bare)
    # ---- prefill ----
    fed(dec, 10)
    for n in (0, -1, 11, 1 << 20, 2**31 - 1):
        report("prefill", f"fed 10, n {n}", lambda: dec.prefill(n, digits=2) and 0, dec)
    fed(dec, MP)
    report("prefill", f"fed {MP}, n {MP}: overflow", lambda: dec.prefill(MP, digits=2) and 0, dec)
    report("prefill", f"fed {MP}, n {MP + 1}: not fed ranks before overflow", lambda: dec.prefill(MP + 1, digits=2) and 0, dec)
    fed(dec, 10, past=5)
    report("prefill", "position 5", lambda: dec.prefill(3, digits=2) and 0, dec)
    report("prefill", "position 5 + n 0 (the position first)", lambda: dec.prefill(0, digits=2) and 0, dec)
    # ---- extend ----
    for n in (0, -1, 6, 1 << 20):
        report("extend", f"position 5, fed 10, n {n}", lambda: dec.extend(n) and 0, dec)
    fed(dec, MP, past=5)
    report("extend", f"position 5, fed {MP}, n {MP - 5}: overflow", lambda: dec.extend(MP - 5) and 0, dec)
    report("extend", f"position 5, fed {MP}, n {MP}: not fed ranks before overflow", lambda: dec.extend(MP) and 0, dec)
    fed(dec, 10)
    report("extend", "position 0, fed 10, n 11", lambda: dec.extend(11) and 0, dec)
    # ---- score ----
    for n in (11, 1, 0, -1):
        report("score", f"fed 10, n {n}", lambda: dec.score(n) and 0, dec)
    report("score", "fed 10, n 5, logits_rows 6", lambda: dec.score(5, logits_rows=6) and 0, dec)
    report("score", "fed 10, n 5, logits_rows -1", lambda: dec.score(5, logits_rows=-1) and 0, dec)
    report("score", "fed 10, n 1, logits_rows 6 (n first)", lambda: dec.score(1, logits_rows=6) and 0, dec)
    fed(dec, 0)
    report("score", "fed 0, n 1 (not fed ranks before n < 2)", lambda: dec.score(1) and 0, dec)
    fed(dec, MP)
    report("score", f"fed {MP}, n {MP}: overflow", lambda: dec.score(MP) and 0, dec)
    fed(dec, 10, past=5)
    report("score", "position 5, n 5", lambda: dec.score(5) and 0, dec)
    # ---- prefill_sharded ----
    fed(dec, 10)
    dec.set_sampling(0.8, seed=1)
    report("prefill_sharded", "sampling on + bad rank (sampling first)", lambda: sharded(dec, 128, 1, 1), dec)
    dec.set_sampling(None)
    report("prefill_sharded", "rank 1 of 1 + n 100 (the rank first)", lambda: sharded(dec, 100, 1, 1), dec)
    report("prefill_sharded", "world 0", lambda: sharded(dec, 128, 0, 0), dec)
    report("prefill_sharded", "world 2 without a gather", lambda: sharded(dec, 256, 0, 2), dec)
    for n in (100, 0, -128):
        report("prefill_sharded", f"n {n}", lambda: sharded(dec, n), dec)
    report("prefill_sharded", "fed 10, n 128", lambda: sharded(dec, 128), dec)
    report("prefill_sharded", "fed 10, n 384 (not fed ranks before overflow)", lambda: sharded(dec, 384), dec)
    fed(dec, 200, past=5)
    report("prefill_sharded", "position 5 + n 100 (the length first)", lambda: sharded(dec, 100), dec)
    report("prefill_sharded", "position 5, n 128", lambda: sharded(dec, 128), dec)
    small.feed(P[:128])
    report("prefill_sharded", "max_pos 128, fed 128, n 128: overflow", lambda: sharded(small, 128), small)
    # ---- prefill_packed ----
    fed(dec, 40, past=5), fed(b1, 40), fed(b16, 40), fed(other, 40)
    grp = (dec, b1, b16, other)
    report("prefill_packed", "n_members 0 + null lengths (the count first)", lambda: packed([dec], None, 0), *grp)
    report("prefill_packed", "n_members 65", lambda: packed([dec], [1], 65), *grp)
    report("prefill_packed", "null lengths + null member (the lengths first)", lambda: packed([dec, None], None), *grp)
    report("prefill_packed", "null member", lambda: packed([dec, None], [1, 1]), *grp)
    report("prefill_packed", "a member is repeated", lambda: packed([dec, b1, b1], [1, 1, 1]), *grp)
    report("prefill_packed", "the driver repeated + other weights behind it (member order)", lambda: packed([dec, dec, other], [1, 1, 1]), *grp)
    report("prefill_packed", "other weights", lambda: packed([dec, other], [1, 1]), *grp)
    report("prefill_packed", "mixed cache types", lambda: packed([dec, b16], [1, 1]), *grp)
    report("prefill_packed", "other weights + other cache type (the weights first)", lambda: packed([dec, b1, other, b16], [1, 1, 1, 1]), *grp)
    report("prefill_packed", "member without globals (another root first)", lambda: packed([dec, bare], [1, 1]), dec, bare)
    report("prefill_packed", "mixed cache types + n 0 (the member set first)", lambda: packed([dec, b16], [0, 1]), *grp)
    for ns in ((0, 1), (1, 0), (1, -3)):
        report("prefill_packed", f"lengths {ns}", lambda: packed([dec, b1], ns), *grp)
    report("prefill_packed", "driver: 36 of 35 fed", lambda: packed([dec, b1], [36, 1]), *grp)
    report("prefill_packed", "member 1: 41 of 40 fed", lambda: packed([dec, b1], [1, 41]), *grp)
    report("prefill_packed", "member 1: 2^31 - 1 tokens", lambda: packed([dec, b1], [1, 2**31 - 1]), *grp)
    report("prefill_packed", "driver unfed + member 1 n 0 (member order)", lambda: packed([dec, b1], [36, 0]), *grp)
    fed(b1, MP)
    report("prefill_packed", f"member 1: fed {MP}, n {MP}: overflow", lambda: packed([dec, b1], [1, MP]), *grp)
    report("prefill_packed", f"member 1: fed {MP}, n {MP + 1}: not fed ranks before overflow", lambda: packed([dec, b1], [1, MP + 1]), *grp)
    # ---- step_wide ----
    fed(b1, 40)
    report("step_wide", "n_members 0 + n_steps 0 (the count first)", lambda: wide([dec], 0, 0), *grp)
    report("step_wide", "n_members 65", lambda: wide([dec], 1, 65), *grp)
    report("step_wide", "n_steps 0 + null member (the steps first)", lambda: wide([dec, None], 0), *grp)
    report("step_wide", "n_steps -1", lambda: wide([dec, b1], -1), *grp)
    report("step_wide", "null member", lambda: wide([dec, None], 1), *grp)
    report("step_wide", "a member is repeated", lambda: wide([dec, b1, b1], 1), *grp)
    report("step_wide", "other weights", lambda: wide([dec, other], 1), *grp)
    report("step_wide", "mixed cache types", lambda: wide([dec, b16], 1), *grp)
    report("step_wide", "other weights + other cache type (member order)", lambda: wide([dec, b16, other], 1), *grp)
    report("step_wide", "member without globals (another root first)", lambda: wide([dec, bare], 1), dec, bare)
    fed(b1, MP - 1, past=MP - 2)
    report("step_wide", f"member 1 at {MP - 2}, 2 steps: overflow", lambda: wide([dec, b1], 2), *grp)
    report("step_wide", f"member 1 at {MP - 2}, 2^31 - 1 steps", lambda: wide([dec, b1], 2**31 - 1), *grp)
    report("step_wide", "mixed cache types + overflow (the member set first)", lambda: wide([dec, b1, b16], 2), *grp)
    for d in (b16, b1, small, other, dec, bare):
        d.close()


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("refusals", "paths", "child"):
        sys.exit(__doc__)
    if sys.argv[1] == "child":
        rest = sys.argv[3:]
        models = rest.pop(0).split(",") if rest and not rest[0].endswith(".so") else ["A", "B", "Ao"]
        child(sys.argv[2], models, rest[0] if rest else None)
    else:
        {"refusals": refusals, "paths": paths}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else None)
