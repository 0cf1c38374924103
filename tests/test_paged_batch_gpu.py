"""GPU: PagedBatch (host/paged_batch.hpp) -- sequences over one pool of 64-position KV pages -- against TWIN decoders with caches of their own
driven by Decoder::step_wide over the same member list.

Prompts of 61, 30 and 130 positions are prefilled on staging decoders and admitted; the first is forked twice and each fork is fed another next
token, so the forks diverge; step(2) then step(3) take the three sequences at 61 over the page boundary at 64 (copy-on-write twice: the third
sharer keeps the page).  The twins take the same prompts by Decoder::fork from the same staging decoders and the same fed tokens.

The routes differ in the attention's summation order only, so the gate is the project's standing one: identical greedy tokens and last_logits
cosine >= 0.9999.  After extract() the admitted positions are the twin's BIT FOR BIT, and so are the appended k and v of layer 0 (the same
arithmetic on the same embedding rows); deeper layers' appended rows sit behind an attention output and are held to the same cosine.
Observed on an MI355X: EXPERIMENTS.md 45."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402
from test_decoder_state_gpu import worlds  # noqa: E402,F401
from test_prefill_packed_gpu import tokens_of  # noqa: E402

pytestmark = pytest.mark.gpu

LENS = (61, 30, 130)
FED = {3: 7, 4: 11}  # the forks' own next tokens (slot 0 keeps the prompt's)
N_PAGES = 12
pages = lambda n: (n + 63) // 64  # noqa: E731


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


@pytest.fixture(scope="module", params=[False, True], ids=["kv32", "kv16"])
def scene(request, pkg, worlds):
    W, kv16 = worlds("A", "qk256"), request.param
    owner = W.decoder(pkg, kv16)
    stages, twins = [owner.shared() for _ in LENS], [owner.shared() for _ in range(5)]
    for d in stages + twins:
        d.set_kv_f16(kv16)
    for i, (s, n) in enumerate(zip(stages, LENS)):
        s.feed(tokens_of(W, i, n + 1))
        s.prefill(n, with_logits=False, digits=2)
    batch = pkg.HostPagedBatch(owner, N_PAGES, 8)
    for i, (s, n) in enumerate(zip(stages, LENS)):
        batch.admit(i, s, n)
        s.fork_into([twins[i]], n)
    batch.fork(0, 3)
    batch.fork(0, 4)
    stages[0].fork_into(twins[3:], LENS[0])
    members = [batch.member(b) for b in range(5)]
    for b, t in FED.items():
        members[b].feed([t])
        twins[b].feed([t])
    yield W, kv16, owner, batch, members, twins, stages
    for d in members:
        d.close()
    batch.close()
    for d in reversed(stages + twins + [owner]):
        d.close()


def test_members_follow_their_twins_and_pages_are_counted_once(pkg, scene):
    W, kv16, owner, batch, members, twins, stages = scene
    lens = [LENS[0], LENS[1], LENS[2], LENS[0], LENS[0]]
    assert batch.pages_in_use() == pages(61) + pages(30) + pages(130) == 5 and batch.pages_free() == N_PAGES - 5
    for n in (2, 3):
        batch.step(n, 2)
        twins[0].step_wide(twins, n, 2)
    lens = [l + 5 for l in lens]
    worst = 1.0
    for b, (m, t) in enumerate(zip(members, twins)):
        assert m.position() == t.position() == lens[b]
        assert np.array_equal(m.history(lens[b] + 1), t.history(lens[b] + 1)), ("greedy tokens", b)
        worst = min(worst, cosine(m.last_logits(), t.last_logits()))
    print("paged batch: worst last_logits cosine against the twins", worst)
    assert worst >= 0.9999
    assert not np.array_equal(members[3].history(67), members[4].history(67))  # the forks did diverge
    # every member privately: sum of ceil(L_i / 64); the three sequences at 66 no longer share their first page (two copies were made)
    assert batch.pages_in_use() == sum(pages(l) for l in lens) == 3 * 2 + 1 + 3
    dst = owner.shared()
    dst.set_kv_f16(kv16)
    worst_kv = 1.0
    for b, t in enumerate(twins):
        batch.extract(b, dst)
        n0, n1 = lens[b] - 5, lens[b]
        assert dst.position() == n1 and np.array_equal(dst.history(n1 + 1), t.history(n1 + 1))
        for l, ((k, v), (tk, tv)) in enumerate(zip(kv.all_layers(dst, W.cfg, kv16), kv.all_layers(t, W.cfg, kv16))):
            exact = slice(0, n1) if l == 0 else slice(0, n0)
            assert np.array_equal(kv.bits(k[exact]), kv.bits(tk[exact])) and np.array_equal(kv.bits(v[exact]), kv.bits(tv[exact])), (b, l)
            for p in range(n0, n1):
                worst_kv = min(worst_kv, cosine(k[p], tk[p]), cosine(v[p], tv[p]))
    print("paged batch: worst appended k / v row cosine against the twins", worst_kv)
    assert worst_kv >= 0.9999
    dst.run(1)  # an extracted sequence goes on as any other
    dst.close()
    # a pool too small: with the three sequences at 66 gone 8 pages are free; a prompt of 130 takes 3, so the third admission is refused whole
    for b in (0, 3, 4):
        batch.release(b)
    assert batch.pages_free() == 8
    batch.admit(5, stages[2], 130)
    batch.admit(6, stages[2], 130)
    with pytest.raises(pkg.BitNetHipError, match="too few free pages"):
        batch.admit(7, stages[2], 130)
    assert batch.pages_free() == 2
    for b in (1, 2, 5, 6):
        batch.release(b)
    assert batch.pages_in_use() == 0 and batch.pages_free() == N_PAGES


def test_a_decoder_without_caches_refuses_what_needs_them(pkg, scene):
    owner = scene[2]
    d = owner.shared_no_cache()
    d.feed([1, 2, 3])
    for call in (lambda: d.run(1), lambda: d.prefill(2, digits=2), lambda: d.rewind(0), lambda: d.step_wide([d], 1, 2), lambda: owner.fork_into([d], 0)):
        with pytest.raises(pkg.BitNetHipError, match="owns no KV cache"):
            call()
    d.close()
