"""GPU: PagedBatch::set_share (host/paged_batch.hpp) on the small synthetic model A of tests/test_decoder_state_gpu.py: a 70-token prompt admitted
and forked into 5 slots, a sixth, unrelated member, samplers with distinct seeds (the forks diverge), set_share(1), step(3).  The five share page 0
(page 1 takes their appends: copy-on-write), so every layer sends 5 rows through bitnet_hip_attention_decode_paged_shared_dev.  Held to: the
route counter, the share-off twin's page count, the float64 whole-prompt forward over each member's own tokens by the gate
tests/test_paged_prefill_batch_gpu.py applies to the un-shared path (last logits cosine >= 0.9999), and the unrelated member bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_decoder_state_gpu import cosine, worlds  # noqa: E402,F401
from test_prefill_packed_gpu import tokens_of  # noqa: E402

pytestmark = pytest.mark.gpu

N, N_OTHER, STEPS = 70, 30, 3


def run(pkg, W, kv16, owner, share):
    """the scene under set_share(share) -> (shared_rows, pages_in_use, [(tokens, last logits)] per member)"""
    stages = [owner.shared() for _ in range(2)]
    for i, (s, n) in enumerate(zip(stages, (N, N_OTHER))):
        s.set_kv_f16(kv16)
        s.feed(tokens_of(W, i, n + 1))
        s.prefill(n, with_logits=False, digits=2)
    batch = pkg.HostPagedBatch(owner, 16, 8)
    batch.admit(0, stages[0], N)
    for b in range(1, 5):
        batch.fork(0, b)
    batch.admit(5, stages[1], N_OTHER)
    members = [batch.member(b) for b in range(6)]
    for b, m in enumerate(members):
        m.set_sampling(0.9, top_k=20, seed=100 + b)
    batch.set_share(share)
    batch.step(STEPS, 2)
    got = [(m.history(m.position() + 1), m.last_logits()) for m in members]
    out = batch.shared_rows(), batch.pages_in_use(), got
    for d in members + [batch] + stages:
        d.close()
    return out


@pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
def test_forks_step_through_the_shared_pass(pkg, worlds, kv16):
    W = worlds("A", "qk256")
    owner = W.decoder(pkg, kv16)
    rows_on, pages_on, on = run(pkg, W, kv16, owner, 1)
    rows_off, pages_off, off = run(pkg, W, kv16, owner, 0)
    owner.close()
    assert rows_on == 5 * W.cfg.n_layers and rows_off == 0
    assert pages_on == pages_off == 1 + 5 + 1  # the shared page 0, five private copies of page 1, the other member's one
    assert len({tuple(t) for t, _ in on[:5]}) > 1, "the forks did not diverge"
    for b, (toks, logits) in enumerate(on):
        assert len(toks) == (N if b < 5 else N_OTHER) + STEPS + 1
        c = cosine(logits, W.forward([int(t) for t in toks[:-1]]).logits[-1])
        print(f"shared batch kv16={kv16} member {b}: last logits cosine against float64 {c:.6f}")
        assert c >= 0.9999, (b, c)
    assert np.array_equal(on[5][0], off[5][0]) and np.array_equal(on[5][1].view(np.uint32), off[5][1].view(np.uint32)), "the unrelated member changed"
