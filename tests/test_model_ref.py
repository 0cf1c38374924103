"""tests/model_ref.py (the float64 whole-prompt forward the decoder-state tests measure against) pinned on the CPU against the oracle's
token-by-token model: logits and every layer's residual row, relative to that row's max |value|.  The oracle accumulates in f32 in a
thread-dependent order: measured 5.9e-6 (logits) / 6.1e-6 (residual stream) for BitNet32, 2.5e-6 for QK256; gated at 2e-5 (3x the worse)."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_ref as mr  # noqa: E402

CFG = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=300, eps=1e-5, rope_theta=10000.0)
N = 256


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module("bitnet-rs_amd.synth")


@pytest.fixture(scope="module", params=["i2s", "qk256"])
def case(request, synth, oracle):
    fmt = request.param
    cfg = synth.ModelConfig(**CFG)
    glob = synth.make_globals(cfg)
    layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
    dense = [mr.dense_weights(cfg, w, fmt) for w in layers]
    sin, cos = oracle.rope_tables(cfg.head_dim, cfg.max_pos, cfg.rope_theta)
    tokens = synth.prompt(N, cfg.vocab)
    ref = mr.forward(cfg, dense, glob, tokens, sin, cos)
    return fmt, cfg, glob, layers, dense, (sin, cos), tokens, ref


def test_matches_the_oracle_token_by_token(case, oracle):
    fmt, cfg, glob, layers, _, _, tokens, ref = case
    om = oracle.OracleModel(cfg, layers if fmt == "qk256" else [dict(w, ternary=32) for w in layers], glob, n_threads=8)
    worst_l = worst_r = 0.0
    for p, t in enumerate(tokens):
        _, logits, trace = om.step(int(t), want_logits=True, want_trace=True)
        worst_l = max(worst_l, float(np.max(np.abs(logits - ref.logits[p])) / np.max(np.abs(ref.logits[p]))))
        for l in range(cfg.n_layers):
            worst_r = max(worst_r, float(np.max(np.abs(trace[l] - ref.resid[l, p])) / np.max(np.abs(ref.resid[l, p]))))
    om.close()
    print(f"model_ref vs oracle [{fmt}]: logits {worst_l:.2e}, residual stream {worst_r:.2e}")
    assert worst_l <= 2e-5 and worst_r <= 2e-5, (worst_l, worst_r)


def test_f16_activation_class_model_stays_on_the_reference(case):
    fmt, cfg, glob, _, dense, (sin, cos), tokens, ref = case
    cls = mr.forward(cfg, dense, glob, tokens, sin, cos, rnd=mr.f16)
    c = min(cosine(cls.logits[p], ref.logits[p]) for p in range(N))
    u = mr.yardstick(ref, cls)
    print(f"f16-activation class model [{fmt}]: worst row cosine {c:.8f}, u_l {['%.2e' % v for v in u]}")
    assert c >= 0.9999, c
    assert all(0.0 < v < 0.05 for v in u), u  # a rounding-sized distance: neither the reference itself nor another model


def test_rows_do_not_depend_on_the_batch_they_are_computed_in(case):
    fmt, cfg, glob, _, dense, (sin, cos), tokens, ref = case
    for m in (1, 65, 130):
        part = mr.forward(cfg, dense, glob, tokens[:m], sin, cos)
        pairs = [(part.logits, ref.logits[:m])]
        for l in range(cfg.n_layers):
            pairs += [(part.K[l], ref.K[l][:m]), (part.V[l], ref.V[l][:m]), (part.resid[l], ref.resid[l, :m])]
        for a, b in pairs:
            # float64 rounding only: a BLAS product may sum in another order for another row count (2^-53 x a few thousand terms)
            assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
