#!/usr/bin/env python3
"""Is the device code of every csrc/*.hip the same as at a git revision?  The check for a refactor that only moves or renames inlined helpers:
    python tools/isa_equal.py REV
compiles REV's csrc (git show, into a temporary directory) and the working tree's with build.py's flags + `--cuda-device-only -S`, blanks the
`__hip_cuid_<hash>` symbol (a hash of the translation unit) and prints one line per file: `identical`, or the mangled names of the functions
whose text differs.  Exit status 1 on any difference.  CPU only (cross-compiles gfx950), at most four compiles at once."""
import importlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
build = importlib.import_module("bitnet-rs_amd.build")
REL = os.path.relpath(build.CSRC, ROOT)


def functions(csrc, src, out_dir):
    """-> {function name: text}, number of kernels; everything outside a function body (descriptors, metadata) under the name '<file scope>'"""
    out = os.path.join(out_dir, src.replace(".hip", ".s"))
    flags = [f"-I{csrc}" if f == f"-I{build.CSRC}" else f for f in build.COMMON_FLAGS] + build.EXTRA.get(src, [])
    p = subprocess.run([build.HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out], capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"hipcc failed on {os.path.join(csrc, src)}\n{p.stderr[-3000:]}")
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(out).read())
    names = set(re.findall(r"\.type\s+(\S+),@function", text))
    fns, cur = {"<file scope>": []}, "<file scope>"
    for line in text.split("\n"):
        if ":" in line and line.split(":")[0] in names:  # `name:    ; @name`
            cur = line.split(":")[0]
            fns[cur] = []
        fns[cur].append(line)
        if line.startswith(".Lfunc_end"):
            cur = "<file scope>"
    return {k: "\n".join(v) for k, v in fns.items()}, len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        old_csrc = os.path.join(tmp, "csrc")
        os.makedirs(old_csrc)
        os.makedirs(os.path.join(tmp, "new"))
        names = subprocess.check_output(["git", "ls-tree", "--name-only", rev, REL + "/"], cwd=ROOT, text=True).split()
        for n in names:
            with open(os.path.join(old_csrc, os.path.basename(n)), "wb") as f:
                f.write(subprocess.check_output(["git", "show", f"{rev}:{n}"], cwd=ROOT))
        srcs = sorted(set(build.sources()) | {os.path.basename(n) for n in names if n.endswith(".hip")})
        jobs = [(d, s, o) for s in srcs for d, o in ((old_csrc, tmp), (build.CSRC, os.path.join(tmp, "new")))]
        with ThreadPoolExecutor(4) as ex:
            res = list(ex.map(lambda j: functions(*j) if os.path.exists(os.path.join(j[0], j[1])) else ({}, 0), jobs))
    bad = False
    for i, s in enumerate(srcs):
        (old, n_old), (new, n_new) = res[2 * i], res[2 * i + 1]
        diff = sorted(k for k in set(old) | set(new) if old.get(k) != new.get(k))
        bad = bad or bool(diff)
        print(f"{s:28s} " + (f"DIFFERS ({n_old} -> {n_new} kernels): " + " ".join(diff) if diff else f"identical ({n_new} kernels)"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
