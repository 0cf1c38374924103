#!/usr/bin/env python3
"""Differential sweep of bitnet_hip_stop_dev (csrc/kernels_stop.hip) against tests/stop_ref.py: N random histories over a 4-letter alphabet (so
stop ids and sequences match often), driven launch by launch; after every launch every device word and the state must be the restatement's.
The generator is tests/test_stop_gpu.py's.  python tools/random_sweep_stop.py [N] [seed]"""
import importlib, os, sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_stop_gpu as ts

pkg = importlib.import_module("bitnet-rs_amd")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    hip = pkg.load()
    hip.init(0)
    reasons = ts.sweep(torch, pkg, hip, n, seed=seed)
    print(f"{n} histories (seed {seed}): ended running / stop id / EOS / budget / sequence = {reasons}")
    print("stop sweep OK")


if __name__ == "__main__":
    main()
