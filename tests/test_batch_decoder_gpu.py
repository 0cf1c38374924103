"""GPU: BatchDecoder (host/batch_decoder.hpp) -- several live sequences stepped through one launch chain -- against TWIN decoders that run the
same steps alone.

A batch member (an owner of the weights, or decoders borrowing them: HostDecoder.shared()) must end every phase in the state its own
run(n, with_logits=True) would have left under attention form 0 (set_attention_form(0): 64-position records + combine, the form the batched
step runs): history, position, last_logits() and every layer's cache slots [0, position), BIT FOR BIT.  The twins are plain decoders with
their own copy of the weights; their batch-1 path is pinned to the oracle and to float64 elsewhere (test_decode_parity.py,
test_full_depth_parity.py, test_decoder_state_gpu.py), and equality needs no tolerance.

Model "A" of tests/test_decoder_state_gpu.py with max_pos 640; both storage formats, f32 and f16 caches."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=640, eps=1e-5, rope_theta=10000.0)
CASES = [(f, k) for f in ("i2s", "qk256") for k in (False, True)]
case_id = lambda c: f"{c[0]}-{'kv16' if c[1] else 'kv32'}"


class World:
    def __init__(self, synth, fmt):
        self.fmt = fmt
        self.cfg = cfg = synth.ModelConfig(**MODEL_A)
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
        self.prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)

    def decoder(self, pkg, kv16):
        dec = pkg.HostDecoder(self.cfg)
        for l, w in enumerate(self.layers):
            dec.set_layer_qk256(l, w) if self.fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
        dec.set_globals(self.glob)
        dec.reset()
        dec.set_kv_f16(kv16)
        return dec


@pytest.fixture(scope="module")
def worlds(pkg):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    made = {}

    def get(fmt):
        if fmt not in made:
            made[fmt] = World(synth, fmt)
        return made[fmt]

    return get


def start(dec, W, n, offset=0):
    """a sequence of n prompt tokens: n == 1 is fed only (position 0, no prefill), longer ones go through the member's own prefill"""
    toks = W.prompt[offset:offset + n]
    dec.reset()
    dec.feed(toks)
    if n > 1:
        dec.prefill(n, with_logits=True, digits=2)


def state(dec, cfg, kv16, logits=True):
    p = dec.position()
    caches = [(kv.bits(k[:p]).copy(), kv.bits(v[:p]).copy()) for k, v in kv.all_layers(dec, cfg, kv16)]
    return dict(pos=p, hist=np.asarray(dec.history(p + 1)).copy(), logits=dec.last_logits().view(np.uint32).copy() if logits else None, caches=caches)


def assert_same(a, b, what):
    assert a["pos"] == b["pos"], (what, "position", a["pos"], b["pos"])
    assert np.array_equal(a["hist"], b["hist"]), (what, "history")
    if a["logits"] is not None and b["logits"] is not None:
        assert np.array_equal(a["logits"], b["logits"]), (what, "last_logits bits", int((a["logits"] != b["logits"]).sum()))
    for l, ((ka, va), (kb, vb)) in enumerate(zip(a["caches"], b["caches"])):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), (what, f"layer {l} cache slots [0, {a['pos']})")


def twin_of(pkg, W, kv16, form0=True):
    t = W.decoder(pkg, kv16)
    if form0:
        t.set_attention_form(0)
    return t


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_members_equal_their_twins_through_joins_leaves_and_feeds(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    owner = W.decoder(pkg, kv16)
    members = [owner] + [owner.shared() for _ in range(3)]
    for m in members[1:]:
        m.set_kv_f16(kv16)
    twins = [twin_of(pkg, W, kv16) for _ in range(4)]
    lengths = [1, 63, 64, 130]  # positions 0 (fed only), 63, 64, 130
    for i, n in enumerate(lengths):
        start(members[i], W, n, offset=3 * i)
        start(twins[i], W, n, offset=3 * i)
        if n > 1:
            assert_same(state(members[i], cfg, kv16), state(twins[i], cfg, kv16), f"member {i} after its own prefill")
    batch = pkg.HostBatch(4)
    for b, m in enumerate(members):
        batch.set_slot(b, m)

    def phase(n, use_graph, what):
        batch.step(n, use_graph=use_graph)
        for i, (m, t) in enumerate(zip(members, twins)):
            t.run(n, with_logits=True, use_graph=True)
            assert_same(state(m, cfg, kv16), state(t, cfg, kv16), f"{what}: slot {i}")

    phase(10, True, "10 steps")
    # slot 1 is cleared and a new member (a prompt of 5) takes its place
    left, left_twin = members[1], twins[1]
    left_state = state(left, cfg, kv16)
    batch.set_slot(1, None)
    members[1], twins[1] = owner.shared(), twin_of(pkg, W, kv16)
    members[1].set_kv_f16(kv16)
    start(members[1], W, 5, offset=40)
    start(twins[1], W, 5, offset=40)
    batch.set_slot(1, members[1])
    phase(20, False, "20 steps after the join (eager)")
    # a feed() between steps, under the carry-on rule: it writes at max(position, fed), i.e. ONTO the picked token, and forces the two after it
    extra = W.prompt[300:303]
    members[2].feed(extra)
    twins[2].feed(extra)
    phase(40, True, "40 steps after the feed")  # members cross the 64- and the 128-key boundaries
    p2 = members[2].position()
    assert list(members[2].history(p2)[64 + 30:64 + 33]) == [int(t) for t in extra]  # the forced tokens were honoured
    assert [m.position() for m in members] == [70, 65, 134, 200]
    # the member that left equals its twin at the moment it left, and nothing touched it since
    assert_same(left_state, state(left_twin, cfg, kv16), "the member that left, against its twin")
    assert_same(left_state, state(left, cfg, kv16), "the member that left, afterwards")
    batch.close()
    for d in members + twins + [left, left_twin]:
        d.close()


def test_graph_and_eager_steps_give_equal_bits(pkg, hip, worlds):
    W = worlds("qk256")
    cfg = W.cfg
    owner = W.decoder(pkg, False)
    sets = [[owner, owner.shared()], [owner.shared(), owner.shared()]]
    batches = [pkg.HostBatch(3), pkg.HostBatch(3)]  # three slots, the middle one idle
    for ms, bt in zip(sets, batches):
        start(ms[0], W, 1)
        start(ms[1], W, 70, offset=9)
        bt.set_slot(0, ms[0])
        bt.set_slot(2, ms[1])
    batches[0].step(6, use_graph=True)
    batches[1].step(6, use_graph=False)
    for a, b in zip(*sets):
        assert_same(state(a, cfg, False), state(b, cfg, False), "graph against eager")
    for bt in batches:
        bt.close()
    for d in sets[0] + sets[1]:
        d.close()


def test_a_sampling_member_draws_its_twins_tokens(pkg, hip, worlds):
    W = worlds("i2s")
    cfg = W.cfg
    owner = W.decoder(pkg, False)
    sampler, greedy = owner.shared(), owner
    t_sampler, t_greedy = twin_of(pkg, W, False), twin_of(pkg, W, False)
    for d in (sampler, t_sampler):
        d.set_sampling(0.9, top_k=40, seed=1234)
    for d, n, off in ((sampler, 20, 0), (t_sampler, 20, 0), (greedy, 66, 7), (t_greedy, 66, 7)):
        start(d, W, n, offset=off)
    batch = pkg.HostBatch(2)
    batch.set_slot(0, sampler)
    batch.set_slot(1, greedy)
    for use_graph in (True, False):
        batch.step(12, use_graph=use_graph)
        for t in (t_sampler, t_greedy):
            t.run(12, with_logits=True, use_graph=True)
        assert_same(state(sampler, cfg, False), state(t_sampler, cfg, False), "the sampling member")
        assert_same(state(greedy, cfg, False), state(t_greedy, cfg, False), "the greedy member beside it")
        assert sampler.sampling_draws() == t_sampler.sampling_draws() > 0  # the same number of ChaCha words consumed
    assert len(set(int(t) for t in sampler.history(sampler.position())[20:])) > 4  # it did sample
    # a member switches to sampling while it sits in its slot: the next step follows (pick tables rewritten, the chain captured anew)
    for d in (greedy, t_greedy):
        d.set_sampling(0.7, top_k=40, seed=99)
    batch.step(5)
    for t in (t_sampler, t_greedy):
        t.run(5, with_logits=True, use_graph=True)
    assert_same(state(greedy, cfg, False), state(t_greedy, cfg, False), "the member that switched to sampling")
    assert_same(state(sampler, cfg, False), state(t_sampler, cfg, False), "the sampling member, after the switch beside it")
    assert greedy.sampling_draws() == t_greedy.sampling_draws() > 0
    batch.close()
    for d in (sampler, greedy, t_sampler, t_greedy):
        d.close()


def test_a_long_prompt_joins_and_equals_a_default_twin(pkg, hip, worlds):
    """past 512 keys run() takes form 0 by itself: the twin needs no override"""
    W = worlds("qk256")
    cfg = W.cfg
    owner = W.decoder(pkg, True)
    member, twin = owner.shared(), twin_of(pkg, W, True, form0=False)
    member.set_kv_f16(True)
    start(owner, W, 30)
    start(member, W, 520, offset=11)
    start(twin, W, 520, offset=11)
    assert twin.form_at(520) == 0
    batch = pkg.HostBatch(2)
    batch.set_slot(0, owner)
    batch.set_slot(1, member)
    batch.step(8)
    twin.run(8, with_logits=True, use_graph=True)
    assert_same(state(member, cfg, True), state(twin, cfg, True), "520-token prompt + 8 steps")
    batch.close()
    for d in (owner, member, twin):
        d.close()


def test_refusals_and_lifetime(pkg, hip, worlds):
    W = worlds("qk256")
    owner, other = W.decoder(pkg, False), W.decoder(pkg, False)
    a, b = owner.shared(), owner.shared()
    for d in (owner, other, a, b):
        start(d, W, 1)
    batch, batch2 = pkg.HostBatch(4), pkg.HostBatch(2)
    batch.set_slot(0, a)
    with pytest.raises(pkg.BitNetHipError, match="another owner"):
        batch.set_slot(1, other)
    b.reset()
    b.set_kv_f16(True)  # (a cache type is chosen on a fresh sequence)
    with pytest.raises(pkg.BitNetHipError, match="mixed KV cache types"):
        batch.set_slot(1, b)
    b.set_kv_f16(False)
    start(b, W, 1)
    with pytest.raises(pkg.BitNetHipError, match="already sits in a slot"):
        batch.set_slot(2, a)
    with pytest.raises(pkg.BitNetHipError, match="already sits in a slot"):
        batch2.set_slot(0, a)
    with pytest.raises(pkg.BitNetHipError, match="KV cache overflow"):
        batch.step(W.cfg.max_pos)  # from position 0, max_pos steps would pass max_pos - 1
    assert a.position() == 0  # refused before the first launch
    with pytest.raises(pkg.BitNetHipError, match="slot index out of range"):
        batch.set_slot(4, b)
    with pytest.raises(pkg.BitNetHipError, match="borrows its weights"):
        a.set_layer_qk256(0, W.layers[0])
    with pytest.raises(pkg.BitNetHipError, match="borrows its weights"):
        a.set_globals(W.glob)
    with pytest.raises(pkg.BitNetHipError, match="borrows its weights"):
        a.set_act_mode(0)
    with pytest.raises(pkg.BitNetHipError, match="live borrowers"):
        owner.set_layer_qk256(0, W.layers[0])
    with pytest.raises(pkg.BitNetHipError, match="1..8 slots"):
        pkg.HostBatch(9)
    exact = W.decoder(pkg, False)
    exact.set_act_mode(0)
    with pytest.raises(pkg.BitNetHipError, match="qact_path") as e:
        batch2.set_slot(0, exact)
    assert e.value.code == pkg.ERR_UNSUPPORTED
    batch.set_slot(1, b)
    batch.step(2)
    # lifetime: the owner goes first, then the batch, then the borrowers -- the shared weights stay until the last reference is gone
    owner.close()
    batch.step(2)
    assert a.position() == 4 and b.position() == 4
    batch.close()
    a.run(1, with_logits=True, use_graph=False)  # a borrower still decodes on the weights its (closed) owner uploaded
    assert a.position() == 5
    for d in (a, b, other, exact):
        d.close()
    batch2.close()
