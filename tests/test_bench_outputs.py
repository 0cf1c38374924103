"""GPU: a plain bench.py run is the headline alone, and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    steps = 5
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "tokens/s"
    for key in ("roofline", "per_kernel", "exact_step_check", "oracle_step_check", "i2s_stream", "cpu_baseline", "also"):
        assert key not in d, key  # measured with --full only
    logits, tokens = np.load(tmp_path / "logits.npy"), np.load(tmp_path / "tokens.npy")
    assert logits.dtype == np.float32 and logits.shape == (128256,) and np.all(np.isfinite(logits))
    assert tokens.dtype == np.float64 and tokens.shape == (steps,)
    assert [int(t) for t in tokens[-4:]] == d["last_tokens"]
    assert int(np.argmax(logits)) == int(tokens[-1])  # greedy: the last step's token is its logits' argmax
