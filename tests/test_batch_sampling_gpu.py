"""GPU: sampling members of a BatchDecoder (host/batch_decoder.hpp) -- all of them served by ONE bitnet_hip_sample_batch_dev launch that
reads per-slot sampler state through a device table -- against TWIN decoders that run the same steps alone under set_attention_form(0).

After every step a member's history, position, last_logits() bits, cache slots and sampling_draws() are its twin's, bit for bit; and a change
of WHICH members sample (a switch on or off, a sampling member leaving, another joining) re-captures nothing: captures() stays 1 and
graph_nodes() is one number whether one, two or three members sample.  Only a batch that never had a sampling member runs a chain one launch
shorter, and its first sampling member costs exactly one more capture.

The small synthetic model of tests/test_batch_decoder_gpu.py (restated here), both storage formats."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=640, eps=1e-5, rope_theta=10000.0)
CFG_G, CFG_S, CFG_F = (1.0, 0, 1.0, 1.1), (0.7, 40, 0.95, 1.1), (0.7, 0, 0.95, 1.1)


class World:
    def __init__(self, synth, fmt):
        self.fmt = fmt
        self.cfg = cfg = synth.ModelConfig(**MODEL_A)
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
        self.prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)

    def decoder(self, pkg):
        dec = pkg.HostDecoder(self.cfg)
        for l, w in enumerate(self.layers):
            dec.set_layer_qk256(l, w) if self.fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
        dec.set_globals(self.glob)
        dec.reset()
        return dec

    def twin(self, pkg):
        t = self.decoder(pkg)
        t.set_attention_form(0)
        return t


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
    dec.reset()
    dec.feed(W.prompt[offset:offset + n])
    dec.prefill(n, with_logits=True, digits=2)


def state(dec, cfg):
    p = dec.position()
    caches = [(kv.bits(k[:p]).copy(), kv.bits(v[:p]).copy()) for k, v in kv.all_layers(dec, cfg, False)]
    return dict(pos=p, hist=np.asarray(dec.history(p + 1)).copy(), logits=dec.last_logits().view(np.uint32).copy(), caches=caches, draws=dec.sampling_draws())


def assert_same(a, b, what):
    assert a["pos"] == b["pos"], (what, "position", a["pos"], b["pos"])
    assert np.array_equal(a["hist"], b["hist"]), (what, "history")
    assert np.array_equal(a["logits"], b["logits"]), (what, "last_logits bits", int((a["logits"] != b["logits"]).sum()))
    for l, ((ka, va), (kb, vb)) in enumerate(zip(a["caches"], b["caches"])):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), (what, f"layer {l} cache slots [0, {a['pos']})")
    assert a["draws"] == b["draws"], (what, "sampling_draws", a["draws"], b["draws"])


class Cast:
    """members in a batch and their twins, stepped side by side and compared after EVERY step"""

    def __init__(self, pkg, W, n_slots):
        self.pkg, self.W = pkg, W
        self.owner = W.decoder(pkg)
        self.batch = pkg.HostBatch(n_slots)
        self.members, self.twins, self.all = {}, {}, [self.owner]

    def join(self, b, length, offset, sampling, seed=0, member=None):
        m = member or self.owner.shared()
        t = self.W.twin(self.pkg)
        for d in (m, t):
            if sampling:
                d.set_sampling(*sampling, seed=seed)
            start(d, self.W, length, offset)
        self.batch.set_slot(b, m)
        self.members[b], self.twins[b] = m, t
        self.all += [x for x in (m, t) if x is not self.owner]

    def leave(self, b):
        self.batch.set_slot(b, None)
        return self.members.pop(b), self.twins.pop(b)

    def set_sampling(self, b, sampling, seed=0):
        for d in (self.members[b], self.twins[b]):
            d.set_sampling(*sampling, seed=seed) if sampling else d.set_sampling(None)

    def steps(self, n, what, use_graph=True):
        for i in range(n):
            self.batch.step(1, use_graph=use_graph)
            for b in self.members:
                self.twins[b].run(1, with_logits=True, use_graph=True)
                assert_same(state(self.members[b], self.W.cfg), state(self.twins[b], self.W.cfg), (what, "step", i, "slot", b))

    def close(self):
        self.batch.close()
        for d in self.all:
            d.close()


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_sampling_members_equal_their_twins_and_no_change_of_the_set_recaptures(pkg, hip, worlds, fmt):
    W = worlds(fmt)
    c = Cast(pkg, W, 4)
    # three sampling members (G, S, F under their own seeds) and a greedy one; prompts of 58..62 cross the 64-key boundary within the first steps
    c.join(0, 60, 0, CFG_G, seed=11, member=c.owner)
    c.join(1, 58, 5, CFG_S, seed=12)
    c.join(2, 62, 9, CFG_F, seed=13)
    c.join(3, 61, 14, None)
    c.steps(8, "three sampling, one greedy")
    assert c.batch.captures() == 1
    nodes = c.batch.graph_nodes()
    assert nodes > 0
    assert c.members[1].sampling_draws() >= 8 and c.members[2].sampling_draws() >= 8 and c.members[0].sampling_draws() == 0  # one word per S / F token
    c.steps(3, "the same, eagerly", use_graph=False)
    # the greedy member switches to sampling: four sample
    c.set_sampling(3, CFG_S, seed=14)
    c.steps(4, "the greedy member switched to sampling")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    # a sampling member switches to greedy, then another: two sample
    c.set_sampling(1, None)
    c.steps(3, "a sampling member switched to greedy")
    c.set_sampling(0, None)
    c.steps(3, "two sample")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    # a sampling member leaves, and its state stays what its twin's is; one samples
    left, left_twin = c.leave(2)
    c.steps(3, "a sampling member left: one samples")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    assert_same(state(left, W.cfg), state(left_twin, W.cfg), "the member that left")
    # another joins the empty slot, sampling
    c.join(2, 30, 40, CFG_F, seed=15)
    c.steps(4, "a sampling member joined the empty slot")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    # nobody samples: the launch stays in the chain (empty entries), and nothing is captured anew
    c.set_sampling(2, None)
    c.set_sampling(3, None)
    c.steps(2, "nobody samples any more")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    c.close()


def test_an_all_greedy_batch_runs_one_launch_fewer_until_its_first_sampling_member(pkg, hip, worlds):
    W = worlds("qk256")
    s = Cast(pkg, W, 2)  # a batch with a sampling member from the start: the number to compare with
    s.join(0, 10, 0, CFG_S, seed=3, member=s.owner)
    s.steps(1, "sampling from the start")
    with_sampling = s.batch.graph_nodes()
    assert s.batch.captures() == 1
    s.close()
    c = Cast(pkg, W, 2)
    c.join(0, 10, 0, None, member=c.owner)
    c.join(1, 12, 3, None)
    assert c.batch.captures() == 0 and c.batch.graph_nodes() == 0
    c.steps(3, "all greedy")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == with_sampling - 1
    c.set_sampling(1, CFG_F, seed=5)
    c.steps(3, "the first sampling member")
    assert c.batch.captures() == 2 and c.batch.graph_nodes() == with_sampling
    c.set_sampling(0, CFG_S, seed=6)
    c.set_sampling(1, None)
    c.steps(3, "the set changes again")
    assert c.batch.captures() == 2 and c.batch.graph_nodes() == with_sampling
    c.close()


def test_best_of_four_from_one_prompt_forward(pkg, hip, worlds):
    """prefill on the source, fork_into four borrowers under four seeds, all four in one batch for 16 steps: each equals a twin that took the
    same fork and ran alone, and the seeds tell them apart"""
    W = worlds("i2s")
    cfg = W.cfg
    P = 66
    sides = []
    for _ in range(2):  # the batch's side and the twins' side: each its own source and four borrowers of it
        src = W.decoder(pkg)
        start(src, W, P)
        dsts = [src.shared() for _ in range(4)]
        for i, d in enumerate(dsts):
            d.set_sampling(0.9, 0, 0.95, 1.1, seed=500 + i)
        src.fork_into(dsts, P - 1)
        sides.append((src, dsts))
    (src, members), (tsrc, twins) = sides
    for t in twins:
        t.set_attention_form(0)
    batch = pkg.HostBatch(4)
    for b, m in enumerate(members):
        batch.set_slot(b, m)
    for i in range(16):
        batch.step(1)
        for b, (m, t) in enumerate(zip(members, twins)):
            t.run(1, with_logits=True, use_graph=True)
            assert_same(state(m, cfg), state(t, cfg), ("best of four, step", i, "slot", b))
    assert batch.captures() == 1
    hists = {tuple(int(x) for x in m.history(m.position() + 1)[P:]) for m in members}
    assert len(hists) >= 2
    assert all(m.sampling_draws() == 16 for m in members)
    batch.close()
    for d in members + twins + [src, tsrc]:
        d.close()
