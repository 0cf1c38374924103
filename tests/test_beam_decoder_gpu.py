"""GPU: HostBeamSearch (host/beam_search.hpp) -- the batched step, the select launch and the in-place KV permute -- against the HOST-DRIVEN route,
built here from calls that need none of the three: two sets of B decoders used alternately; per step HostBatch.step(1) on the live set, the tap
records read back, the rule in numpy (tests/beam_ref.py), Decoder::fork from every parent into its children of the other set, feed() of each
child's token.  Both routes run the same batched kernels on the same bits, so everything is compared for EQUALITY: the hypotheses (tokens, score
bits, key bits, order), each live beam's position and history, and every cache slot below the position of every layer's K and V.

Model "A" of tests/test_batch_decoder_gpu.py (max_pos 640), both storage formats, both cache types; prompt positions 0 (one fed token), 62, 63 and
127 with 6 new tokens, so the reorder crosses slots 64 and 128; B in {1, 2, 4, 8}.  The EOS ids come FROM the host route's pilot run: a token
that is never a candidate (the search ends by its budget) and the best first token (a hypothesis is pooled at the first step; with B = 1 the pool
is full and the search ends by it) -- the test asserts which ending happened."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as br  # noqa: E402
import test_batch_decoder_gpu as tb  # noqa: E402  (World, start, state, assert_same: the batch tests' own helpers)

pytestmark = pytest.mark.gpu

NEW = 6
PROMPTS = (1, 62, 63, 127)
CASES = [(f, k, B) for f in ("i2s", "qk256") for k in (False, True) for B in (1, 2, 4, 8)]
case_id = lambda c: f"{c[0]}-{'kv16' if c[1] else 'kv32'}-B{c[2]}"


class Crew:
    """the decoders of one (format, cache type): an owner, 7 borrowers for the device route, 16 more for the host route's two sets"""

    def __init__(self, pkg, W, kv16):
        self.pkg, self.W, self.kv16 = pkg, W, kv16
        self.owner = W.decoder(pkg, kv16)
        self.rest = [self.owner.shared() for _ in range(7 + 16)]
        for d in self.rest:
            d.set_kv_f16(kv16)
        self.batch, self.host_batch = pkg.HostBatch(8), pkg.HostBatch(8)

    def beams(self, B):
        return [self.owner] + self.rest[:B - 1]

    def sets(self, B):
        return self.rest[7:7 + B], self.rest[15:15 + B]

    def empty(self, batch):
        for b in range(8):
            batch.set_slot(b, None)

    def close(self):
        self.batch.close(), self.host_batch.close()
        for d in self.rest + [self.owner]:
            d.close()


@pytest.fixture(scope="module")
def crews(pkg, hip):
    import importlib

    synth = importlib.import_module("bitnet-rs_amd.synth")
    worlds, made = {}, {}

    def get(fmt, kv16):
        if fmt not in worlds:
            worlds[fmt] = tb.World(synth, fmt)
        if (fmt, kv16) not in made:
            made[(fmt, kv16)] = Crew(pkg, worlds[fmt], kv16)
        return made[(fmt, kv16)]

    yield get
    for c in made.values():
        c.close()


def prime(crew, members, n_prompt):
    """the members at one position with one prefix: the prompt on the first, a fork into the others"""
    tb.start(members[0], crew.W, n_prompt)
    if len(members) > 1:
        members[0].fork_into(members[1:], members[0].position())


def host_route(crew, B, n_prompt, eos, max_new, lw):
    """-> (ref, the live set, walked candidates [(step, walk index, token)], the first step's events); the live set's members sit in
    crew.host_batch"""
    batch = crew.host_batch
    live, idle = crew.sets(B)
    crew.empty(batch)
    for d in live + idle:
        d.reset()
        d.set_logprobs(2 * B)
    prime(crew, live, n_prompt)
    P = live[0].position()
    ref = br.BeamRef(B, eos, max_new, lw, prompt_pos=P)
    seen, first_events = [], None
    t0 = time.perf_counter()
    for s in range(max_new):
        for b, d in enumerate(live):
            batch.set_slot(b, d)
        batch.step(1)
        q = P + s + 1
        recs = [d.logprob_records(q, 1)[0] for d in live]
        ref.step([r["lse"] for r in recs], np.array([r["top_id"][:2 * B] for r in recs]), np.array([r["top_logit"][:2 * B] for r in recs]), q - 1)
        seen += [(s, r, int(recs[b]["top_id"][j])) for r, (_, b, j) in enumerate(ref.walk)]
        first_events = list(ref.events) if first_events is None else first_events
        crew.empty(batch)  # a fork refuses a destination that sits in a slot
        for parent in sorted(set(int(x) for x in ref.parent[:B])):
            children = [b for b in range(B) if ref.parent[b] == parent]
            live[parent].fork_into([idle[b] for b in children], q)
        for b in range(B):
            idle[b].feed([int(ref.token[b])])  # onto slot q: over the parent's greedy pick
        live, idle = idle, live
        if ref.done:
            break
    crew.loop_seconds = time.perf_counter() - t0  # every call above returns synchronised (tools/perf_beam.py reads it)
    for b, d in enumerate(live):
        batch.set_slot(b, d)
    return ref, live, seen, first_events


def device_route(crew, B, n_prompt, eos, max_new, alpha, chunk):
    members = crew.beams(B)
    crew.empty(crew.batch)
    for d in members:
        d.reset()
    prime(crew, members, n_prompt)
    for b, d in enumerate(members):
        crew.batch.set_slot(b, d)
    search = crew.pkg.HostBeamSearch(crew.batch, B, eos, max_new, alpha)
    search.start()
    t0 = time.perf_counter()
    steps, _ = search.run(chunk)
    crew.loop_seconds = time.perf_counter() - t0  # run() returns synchronised
    return search, members, steps


def hyps(search):
    return [(t, br.bits(s), br.bits(k)) for t, s, k in search.hypotheses()]


def assert_routes_equal(crew, members, live, what):
    cfg = crew.W.cfg
    for b, (m, h) in enumerate(zip(members, live)):
        tb.assert_same(tb.state(m, cfg, crew.kv16, logits=False), tb.state(h, cfg, crew.kv16, logits=False), f"{what}: beam {b}")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_device_route_equals_the_host_driven_route(pkg, crews, case):
    fmt, kv16, B = case
    crew = crews(fmt, kv16)
    endings = set()
    for n_prompt in PROMPTS:
        alpha = 0.0 if n_prompt in (1, 63) else 0.6
        # the length weights are the table the search itself reports: no test recomputes a power and expects its bits
        members = crew.beams(B)
        crew.empty(crew.batch)
        for b, d in enumerate(members):
            d.reset()
            crew.batch.set_slot(b, d)
        bound = pkg.HostBeamSearch(crew.batch, B, -1, NEW, alpha)
        lw = bound.len_weights()
        bound.close()
        assert lw.shape == (NEW + 1,) and lw[1] == 1.0 and (alpha != 0.0 or np.all(lw == 1.0)) and np.all(np.diff(lw[1:]) <= 0)
        # the pilot: no EOS.  It IS the comparator of a search whose EOS is never a candidate.
        ref, live, seen, _ = host_route(crew, B, n_prompt, -1, NEW, lw)
        assert ref.done == br.DONE_BUDGET
        unused = next(t for t in range(crew.W.cfg.vocab) if t not in {tok for _, _, tok in seen})
        best_first = next(tok for s, r, tok in seen if s == 0 and r == 0)

        # 1. an EOS that is never a candidate: the search ends by its budget and equals the pilot
        search, members, steps = device_route(crew, B, n_prompt, unused, NEW, alpha, chunk=4)
        st = search.state()
        assert st.done == br.DONE_BUDGET and steps == NEW and st.gen_len == NEW and st.pool_n == B
        assert hyps(search) == ref.hypotheses()
        assert_routes_equal(crew, members, live, f"prompt {n_prompt}, budget ending")
        assert crew.batch.graph_nodes() == crew.host_batch.graph_nodes()  # the two launches are not part of the captured chain
        endings.add(st.done)
        if B == 1 and alpha == 0.0:  # the member's own greedy run under attention form 0
            twin = crew.sets(1)[1][0]
            twin.reset()
            twin.set_logprobs(None)
            tb.start(twin, crew.W, n_prompt)
            twin.set_attention_form(0)
            P = twin.position()
            twin.run(NEW, with_logits=True)
            twin.set_attention_form(-1)
            assert list(twin.history(P + NEW + 1)[P + 1:]) == hyps(search)[0][0]
        # a continuation behind the finished search: both routes' beams take two more batched steps
        crew.batch.step(2)
        crew.host_batch.step(2)
        assert_routes_equal(crew, members, live, f"prompt {n_prompt}, two steps behind the search")
        search.close()

        # 2. the best first token as EOS: a hypothesis is pooled at the first step; chunk 1 and chunk 4 give the same result
        ref, live, _, first_events = host_route(crew, B, n_prompt, best_first, NEW, lw)
        assert ("eos_pooled", 0) in first_events  # the case occurred
        results = []
        for chunk in (1, 4):
            search, members, steps = device_route(crew, B, n_prompt, best_first, NEW, alpha, chunk)
            st = search.state()
            assert st.done == ref.done and st.gen_len == ref.gen_len
            assert hyps(search) == ref.hypotheses()
            assert_routes_equal(crew, members, live, f"prompt {n_prompt}, EOS {best_first}, chunk {chunk}")
            results.append((st.words()[:11], steps))
            search.close()
        # stepped (word 6) and frozen_steps (word 10) are what differs between the chunkings, if anything: chunk 4 may end on frozen steps
        assert results[0][0][:6] + results[0][0][7:10] == results[1][0][:6] + results[1][0][7:10]
        if B == 1:
            assert ref.done == br.DONE_POOL and results[0][1] == 1 and results[1][1] == 4  # three steps were queued for nothing, and frozen
        endings.add(ref.done)
    assert br.DONE_BUDGET in endings and (B > 1 or br.DONE_POOL in endings)


def test_every_refusal_leaves_every_member(pkg, crews):
    crew = crews("i2s", False)
    B, cfg = 2, crew.W.cfg
    members = crew.beams(B)
    crew.empty(crew.batch)
    for d in members:
        d.reset()
        d.set_logprobs(None)
    prime(crew, members, 20)
    for b, d in enumerate(members):
        crew.batch.set_slot(b, d)
    snap = lambda: [tb.state(d, cfg, False, logits=False) for d in members]
    before = snap()

    def unchanged(what):
        for b, (x, y) in enumerate(zip(before, snap())):
            tb.assert_same(x, y, f"{what}: member {b}")

    for args, msg in (((0, -1, 4, 0.0), "n_beams"), ((9, -1, 4, 0.0), "n_beams"), ((3, -1, 4, 0.0), "slot 2 is empty"), ((2, -2, 4, 0.0), "eos"),
                      ((2, -1, 0, 0.0), "max_new_tokens"), ((2, -1, 4, float("nan")), "alpha")):
        with pytest.raises(pkg.BitNetHipError, match=msg):
            pkg.HostBeamSearch(crew.batch, *args)
    members[1].set_sampling(0.8, top_k=40, seed=1)
    with pytest.raises(pkg.BitNetHipError, match="member 1 samples"):
        pkg.HostBeamSearch(crew.batch, 2, -1, 4, 0.0)
    members[1].set_sampling(None)
    members[0].set_stop(eos=5)
    with pytest.raises(pkg.BitNetHipError, match="stop criteria"):
        pkg.HostBeamSearch(crew.batch, 2, -1, 4, 0.0)
    members[0].set_stop(off=True)
    for d in members:  # no refused binding switched a tap on
        with pytest.raises(pkg.BitNetHipError, match="switched off"):
            d.logprob_records(0, 1)
    unchanged("refused bindings")
    search = pkg.HostBeamSearch(crew.batch, 2, -1, 4, 0.0)
    with pytest.raises(pkg.BitNetHipError, match="start\\(\\) first"):
        search.run(2)
    crew.batch.set_slot(1, None)
    members[1].rewind(19)
    crew.batch.set_slot(1, members[1])
    before = snap()
    with pytest.raises(pkg.BitNetHipError, match="different positions"):
        search.start()
    unchanged("start at different positions")
    crew.batch.set_slot(1, None)
    members[1].feed([(int(members[0].history(20)[19]) + 1) % cfg.vocab])
    members[1].run(1, with_logits=True)  # position 20 again, behind another token 19
    crew.batch.set_slot(1, members[1])
    before = snap()
    with pytest.raises(pkg.BitNetHipError, match="prefixes differ"):
        search.start()
    unchanged("start with different prefixes")
    search.close()
    crew.empty(crew.batch)
    for d in members:
        d.reset()
    prime(crew, members, 20)
    for b, d in enumerate(members):
        crew.batch.set_slot(b, d)
    before = snap()
    big = pkg.HostBeamSearch(crew.batch, 2, -1, cfg.max_pos, 0.0)
    big.start()
    with pytest.raises(pkg.BitNetHipError, match="KV cache overflow"):
        big.run(4)
    with pytest.raises(pkg.BitNetHipError, match="chunk"):
        big.run(0)
    unchanged("refused runs")
    big.close()
