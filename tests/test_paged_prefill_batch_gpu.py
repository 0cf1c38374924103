"""GPU: PagedBatch::open + prefill (host/paged_batch.hpp) -- prompt forwards that write straight into KV pages, every layer attending through
bitnet_hip_attention_paged_prefill_dev -- on the small synthetic model A of tests/test_decoder_state_gpu.py.

Two members take a 171-token prompt in chunks of 70, 1 and 100 (one packed forward per chunk for both); each is then extracted and its caches held
slot by slot, and its last logits, to the float64 whole-prompt forward with that module's gates (rel <= 4 u_l (+ 2^-11 with f16 pools), cosine >=
0.9999).  A fork continues by prefill alone: its sibling's pages keep their bits and the pool grows by the copied page plus the new one.  A
prefill the pool cannot hold changes nothing.  After prefill, step() continues the members beside twins admitted through the staging route:
identical greedy tokens and last_logits cosine >= 0.9999, the criterion of tests/test_paged_batch_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_decoder_state_gpu import check_values, cosine, same_bytes, snapshot, worlds  # noqa: E402,F401
from test_prefill_packed_gpu import tokens_of  # noqa: E402

pytestmark = pytest.mark.gpu

N, CHUNKS = 171, (70, 1, 100)


@pytest.fixture(params=[False, True], ids=["kv32", "kv16"])
def scene(request, pkg, worlds):
    W, kv16 = worlds("A", "qk256"), request.param
    owner = W.decoder(pkg, kv16)
    made = [owner]

    def shared():
        d = owner.shared()
        d.set_kv_f16(kv16)
        made.append(d)
        return d

    def batch(n_pages):
        b = pkg.HostPagedBatch(owner, n_pages, 8)
        made.append(b)
        return b

    def member(b, slot, tokens):
        m = b.member(slot)
        made.append(m)
        if len(tokens):
            m.feed(tokens)
        return m

    yield W, kv16, shared, batch, member
    for d in reversed(made):
        d.close()


def held_to_f64(W, kv16, batch, slot, m, dst, forced, what):
    toks, ref, u = W.seq(forced)
    assert m.position() == N and np.array_equal(m.history(N + 1), toks[:N + 1]), what
    c = cosine(m.last_logits(), ref.logits[N - 1])
    assert c >= 0.9999, (what, "last logits", c)
    batch.extract(slot, dst)
    check_values(W, snapshot(dst, W, kv16), ref, u, kv16, slice(0, N), "paged-prefill", what)


def test_chunked_prefill_of_two_members_then_steps_beside_staged_twins(pkg, scene):
    W, kv16, shared, make_batch, member = scene
    batch, dst = make_batch(16), shared()
    forced = [tokens_of(W, i, N + 1) for i in range(2)]
    ms = []
    for i in range(2):
        batch.open(i)
        ms.append(member(batch, i, forced[i]))
    assert batch.pages_in_use() == 0
    for c in CHUNKS:
        batch.prefill([0, 1], [c, c], with_logits=c == CHUNKS[-1])
    assert batch.pages_in_use() == 2 * 3
    for i in range(2):
        held_to_f64(W, kv16, batch, i, ms[i], dst, forced[i], f"member {i} after chunks {CHUNKS}")
    twins = []
    for i in range(2):  # the staging route: one contiguous prefill, then admit
        s = shared()
        s.feed(forced[i])
        s.prefill(N, with_logits=False, digits=2)
        batch.admit(2 + i, s, N)
        twins.append(member(batch, 2 + i, []))
    batch.step(3, 2)
    for i in range(2):
        assert ms[i].position() == twins[i].position() == N + 3
        assert np.array_equal(ms[i].history(N + 4), twins[i].history(N + 4)), ("greedy tokens", i)
        c = cosine(ms[i].last_logits(), twins[i].last_logits())
        assert c >= 0.9999, ("last logits against the staged twin", i, c)


def test_a_fork_continues_by_prefill_and_its_sibling_keeps_its_pages(pkg, scene):
    W, kv16, shared, make_batch, member = scene
    batch, dst = make_batch(8), shared()
    forced = tokens_of(W, 0, N + 1)
    batch.open(0)
    member(batch, 0, forced)
    batch.prefill([0], [70], with_logits=False)
    batch.extract(0, dst)
    before = snapshot(dst, W, kv16)
    batch.fork(0, 1)
    m1 = member(batch, 1, forced[70:])
    assert batch.pages_in_use() == 2
    batch.prefill([1], [N - 70])  # positions 70 .. 170: the shared page 1 is copied, page 2 is new
    assert batch.pages_in_use() == 2 + 1 + 1
    batch.extract(0, dst)
    assert dst.position() == 70 and same_bytes(snapshot(dst, W, kv16), before, slice(0, 70)), "the sibling's pages changed"
    held_to_f64(W, kv16, batch, 1, m1, dst, forced, "the fork, continued by prefill")


def test_a_prefill_the_pool_cannot_hold_changes_nothing(pkg, scene):
    W, kv16, shared, make_batch, member = scene
    batch = make_batch(4)
    ms = []
    for i in range(2):
        batch.open(i)
        ms.append(member(batch, i, tokens_of(W, i, N + 1)))
    with pytest.raises(pkg.BitNetHipError, match="too few free pages"):
        batch.prefill([0, 1], [130, 130])  # 3 + 3 pages of 4
    assert batch.pages_in_use() == 0 and batch.pages_free() == 4 and [m.position() for m in ms] == [0, 0]
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        batch.prefill([0], [N + 2])  # more than was fed
    batch.prefill([0], [130])
    assert batch.pages_in_use() == 3 and ms[0].position() == 130 and ms[1].position() == 0
