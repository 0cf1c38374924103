"""HostDecoder.score_topn at the 2-layer test model against score(n, logits_rows = n) of the same decoder followed by a numpy top-N of the
returned logits: the same forward and the same head bits, so ids are equal and values bit-equal, record for record; a second call after
reset() gives the same bytes."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDE = dict(hidden=2560, n_layers=2, n_heads=20, n_kv_heads=5, head_dim=128, ffn=6912, vocab=4096, max_pos=256, eps=1e-5, rope_theta=500000.0)
TOP_N = 20


@pytest.fixture(scope="module")
def model(pkg, hip):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg = synth.ModelConfig(**WIDE)
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        dec.set_layer_qk256(l, synth.make_layer(cfg, l, fmt="qk256", block=32))
    dec.set_globals(synth.make_globals(cfg))
    yield dec, synth.prompt(130, cfg.vocab)
    dec.close()


@pytest.mark.parametrize("n", [2, 130])
def test_records_equal_the_top_n_of_the_dumped_logits(model, n):
    dec, prompt = model
    dec.reset()
    dec.feed(prompt)
    res = dec.score(n, digits=2, logits_rows=n)
    dec.reset()
    rec = dec.score_topn(prompt[:n], TOP_N)
    assert rec.shape == (n,) and dec.position() == n and dec.last_score_topn_ms > 0
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    for r in range(n):
        l = res.logits[r] + np.float32(0.0)  # the order's reading: -0.0 as +0.0 (no NaN comes out of this model)
        order = np.argsort(-l, kind="stable")[:TOP_N]
        assert rec[r]["n_top"] == TOP_N and np.array_equal(rec[r]["top_id"], order), r
        assert np.array_equal(bits(rec[r]["top_logit"]), bits(l[order])), r
        target = int(prompt[r + 1]) if r < n - 1 else -1
        if target >= 0:
            assert rec[r]["token"] == target and bits(rec[r]["logit"]) == bits(res.logits[r, target])
            assert bits(np.float32(rec[r]["lse"]) - np.float32(rec[r]["logit"])) == bits(res.nll[r])  # the lse nll was formed from
        else:
            assert np.isnan(rec[r]["logit"]) and rec[r]["token"] == -1
    dec.reset()
    dec.feed(prompt)
    assert dec.score_topn(n, TOP_N).tobytes() == rec.tobytes()
