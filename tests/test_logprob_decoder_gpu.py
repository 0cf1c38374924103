"""GPU: the logits tap behind the decoder (Decoder::set_logprobs / logprobs, host/decoder.hpp) and behind a batch (host/batch_decoder.hpp).

Alone: after every with-logits step the record at position() is the restatement (tests/logprob_ref.py) applied to last_logits() with
token == history[position()] -- top list exact, lse within logprob_ref.lse_bound (vocab 2048: two slices of 1024, D = 23) -- for the prompt
forward's record, free and forced positions, greedy and sampling, graph and eager; a replayed run(n) leaves the same bytes as n run(1), and a
decoder with logprobs off the same tokens, logits bits and draws.  In a batch: a member's records are its twin's bytes (the twin runs alone
under set_attention_form(0)), and the launch joins the captured chain once in a batch's life.

The small synthetic model of tests/test_batch_sampling_gpu.py (restated here), both storage formats."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402
import logprob_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=640, eps=1e-5, rope_theta=10000.0)
CFG_S, CFG_F = (0.7, 40, 0.95, 1.1), (0.7, 0, 0.95, 1.1)
V = MODEL_A["vocab"]


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


def check_record(dec, top_n, what):
    """record position() against the restatement on last_logits(), token == history[position()]"""
    p = dec.position()
    rec = dec.logprob_records(p, 1)[0]
    token = int(dec.history(p + 1)[p])
    want = ref.record(dec.last_logits(), token, top_n)
    assert int(rec["token"]) == token == want.token and int(rec["n_top"]) == want.n_top, (what, p, rec["token"], token)
    assert np.array_equal(rec["top_id"][:want.n_top], want.top_id), (what, p)
    assert ref.same_bits(rec["top_logit"][:want.n_top], want.top_logit) and ref.same_bits(rec["logit"], want.logit), (what, p)
    assert (rec["top_id"][want.n_top:] == -1).all(), (what, p, "entries >= n_top keep the 0xFF bytes")
    err, bound = abs(float(rec["lse"]) - want.lse), ref.lse_bound(V, want.lse)
    print(f"{what} position {p}: lse {float(rec['lse'])!r} float64 {want.lse!r} |diff| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, p, float(rec["lse"]), want.lse, err, bound)
    lp = dec.logprobs(p, 1)
    assert lp.top_ids.shape == (1, top_n) and ref.same_bits(lp.logprob[0], np.float32(rec["logit"]) - np.float32(rec["lse"]))


def begin(dec, W, sampling, top_n, n=5, seed=21):
    dec.set_sampling(*sampling, seed=seed) if sampling else dec.set_sampling(None)
    dec.set_logprobs(top_n)
    dec.reset()
    dec.feed(W.prompt[:n])
    dec.prefill(n, with_logits=True, digits=2)


def raw(dec, n):
    return dec.logprob_records(0, n).tobytes()


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_stepwise_records_replay_and_the_untapped_twin(pkg, hip, worlds, fmt):
    W = worlds(fmt)
    dec, twin, plain = W.decoder(pkg), W.decoder(pkg), W.decoder(pkg)
    for sampling, top_n in ((None, 5), (CFG_S, 20), (CFG_F, 1)):
        stepwise = {}
        for use_graph in (True, False):
            what = (fmt, sampling, "graph" if use_graph else "eager")
            begin(dec, W, sampling, top_n)
            assert dec.position() == 5
            check_record(dec, top_n, what + ("prefill",))  # a prompt of 5 tokens with logits leaves record 5
            assert (dec.logprob_records(0, 5)["token"] == -1).all()
            for _ in range(12):
                dec.run(1, with_logits=True, use_graph=use_graph)
                check_record(dec, top_n, what)
            stepwise[use_graph] = raw(dec, 20)
        assert stepwise[True] == stepwise[False], (fmt, sampling, "graph and eager records")
        # a twin replaying run(12) in one call: the same bytes
        begin(twin, W, sampling, top_n)
        twin.run(12, with_logits=True, use_graph=True)
        assert raw(twin, 20) == stepwise[True], (fmt, sampling, "run(12) against 12 run(1)")
        # a twin with logprobs off: the same tokens, logits bits and draws
        plain.set_sampling(*sampling, seed=21) if sampling else plain.set_sampling(None)
        plain.reset()
        plain.feed(W.prompt[:5])
        plain.prefill(5, with_logits=True, digits=2)
        plain.run(12, with_logits=True, use_graph=True)
        assert np.array_equal(plain.history(18), twin.history(18)) and plain.position() == twin.position() == 17
        assert np.array_equal(plain.last_logits().view(np.uint32), twin.last_logits().view(np.uint32))
        assert plain.sampling_draws() == twin.sampling_draws()
    for d in (dec, twin, plain):
        d.close()


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_forced_positions_and_extend(pkg, hip, worlds, fmt):
    W = worlds(fmt)
    dec, twin = W.decoder(pkg), W.decoder(pkg)
    for d in (dec, twin):
        d.set_logprobs(5)
        d.reset()
        d.feed(W.prompt[:8])
    dec.run(8, with_logits=True, use_graph=True)
    for i in range(8):  # the twin stepwise: every record against its own logits
        twin.run(1, with_logits=True, use_graph=True)
        check_record(twin, 5, (fmt, "forced" if i < 7 else "free"))
    r = dec.logprob_records(0, 10)
    assert r["token"][0] == -1 and np.array_equal(r["token"][1:8], W.prompt[1:8]) and r["token"][9] == -1  # echo: the fed tokens
    assert r["token"][8] == dec.history(9)[8]
    assert raw(dec, 10) == raw(twin, 10)
    # extend over 4 more tokens with logits: one record, at the new position
    dec.feed(W.prompt[8:12])
    dec.extend(4, with_logits=True, digits=2)
    assert dec.position() == 12
    check_record(dec, 5, (fmt, "extend"))
    assert (dec.logprob_records(9, 3)["token"] == -1).all()
    for d in (dec, twin):
        d.close()


def test_reset_rewind_fork_and_refusals(pkg, hip, worlds):
    W = worlds("qk256")
    src = W.decoder(pkg)
    with pytest.raises(pkg.BitNetHipError, match="switched off"):
        src.logprobs(0, 1)
    with pytest.raises(pkg.BitNetHipError, match="top_n"):
        src.set_logprobs(21)
    with pytest.raises(pkg.BitNetHipError, match="top_n"):
        src.set_logprobs(-2)
    begin(src, W, None, 5, n=6)
    src.run(4, with_logits=True)
    for first, n in ((-1, 1), (0, MODEL_A["max_pos"] + 1), (MODEL_A["max_pos"], 1), (3, -1)):
        with pytest.raises(pkg.BitNetHipError, match="range"):
            src.logprob_records(first, n)
    assert len(src.logprob_records(MODEL_A["max_pos"] - 1, 1)) == 1
    before = raw(src, 12)
    assert (src.logprob_records(6, 5)["token"] >= 0).all()
    src.rewind(7)  # rewind keeps the records
    assert raw(src, 12) == before
    on, off = src.shared(), src.shared()
    on.set_logprobs(20)
    on.reset()
    on.feed(W.prompt[:3])
    on.prefill(3, with_logits=True, digits=2)
    assert on.logprob_records(3, 1)["token"][0] >= 0
    src.fork_into([on, off], 7)  # clears a destination that has logprobs on, leaves the source's bytes
    assert (on.logprob_records(0, MODEL_A["max_pos"])["token"] == -1).all()
    assert raw(src, 12) == before
    on.run(2, with_logits=True)
    assert (on.logprob_records(8, 2)["token"] >= 0).all() and on.logprob_records(7, 1)["token"][0] == -1
    with pytest.raises(pkg.BitNetHipError, match="switched off"):
        off.logprobs(0, 1)
    src.reset()  # reset clears
    assert (src.logprob_records(0, MODEL_A["max_pos"])["token"] == -1).all()
    src.set_logprobs(None)
    with pytest.raises(pkg.BitNetHipError, match="switched off"):
        src.logprobs(0, 1)
    for d in (on, off, src):
        d.close()


def state(dec, cfg):
    p = dec.position()
    caches = [(kv.bits(k[:p]).copy(), kv.bits(v[:p]).copy()) for k, v in kv.all_layers(dec, cfg, False)]
    return dict(pos=p, hist=np.asarray(dec.history(p + 1)).copy(), logits=dec.last_logits().view(np.uint32).copy(), caches=caches, draws=dec.sampling_draws())


def assert_same(a, b, what):
    assert a["pos"] == b["pos"], (what, "position", a["pos"], b["pos"])
    assert np.array_equal(a["hist"], b["hist"]), (what, "history")
    assert np.array_equal(a["logits"], b["logits"]), (what, "last_logits bits")
    for l, ((ka, va), (kb, vb)) in enumerate(zip(a["caches"], b["caches"])):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), (what, f"layer {l} cache")
    assert a["draws"] == b["draws"], (what, "sampling_draws")


class Cast:
    """members in a batch and their twins (alone, attention form 0), stepped side by side and compared after EVERY step"""

    def __init__(self, pkg, W, n_slots):
        self.pkg, self.W = pkg, W
        self.owner = W.decoder(pkg)
        self.batch = pkg.HostBatch(n_slots)
        self.members, self.twins, self.tops, self.all = {}, {}, {}, [self.owner]

    def join(self, b, length, offset, sampling, top_n, seed=0, member=None):
        m = member or self.owner.shared()
        t = self.W.twin(self.pkg)
        for d in (m, t):
            d.set_sampling(*sampling, seed=seed) if sampling else d.set_sampling(None)
            d.set_logprobs(top_n)
            d.reset()
            d.feed(self.W.prompt[offset:offset + length])
            d.prefill(length, with_logits=True, digits=2)
        self.batch.set_slot(b, m)
        self.members[b], self.twins[b], self.tops[b] = m, t, top_n
        self.all += [x for x in (m, t) if x is not self.owner]

    def leave(self, b):
        self.batch.set_slot(b, None)
        self.tops.pop(b)
        return self.members.pop(b), self.twins.pop(b)

    def set_logprobs(self, b, top_n):
        for d in (self.members[b], self.twins[b]):
            d.set_logprobs(top_n)
        self.tops[b] = top_n

    def steps(self, n, what):
        for i in range(n):
            self.batch.step(1, use_graph=True)
            for b in self.members:
                m, t = self.members[b], self.twins[b]
                t.run(1, with_logits=True, use_graph=True)
                assert_same(state(m, self.W.cfg), state(t, self.W.cfg), (what, "step", i, "slot", b))
                if self.tops[b] is not None:
                    p = m.position()
                    assert raw(m, p + 1) == raw(t, p + 1), (what, "step", i, "slot", b, "records")
                    assert m.logprob_records(p, 1)["token"][0] == m.history(p + 1)[p]

    def close(self):
        self.batch.close()
        for d in self.all:
            d.close()


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_batch_members_equal_their_twins_and_nothing_recaptures(pkg, hip, worlds, fmt):
    W = worlds(fmt)
    c = Cast(pkg, W, 4)
    c.join(0, 20, 0, None, 0, member=c.owner)   # A: top_n 0, greedy
    c.join(1, 33, 5, CFG_S, 5, seed=12)         # B: top_n 5, sampling
    c.join(2, 61, 9, None, 20)                  # C: top_n 20, greedy, crossing key 64 within the steps
    c.join(3, 12, 14, None, None)               # D: logprobs off
    c.steps(6, "three with logprobs, one without")
    assert c.batch.captures() == 1
    nodes = c.batch.graph_nodes()
    assert nodes > 0
    c.set_logprobs(3, 3)     # the member without switches on, one with switches off, another changes its top_n
    c.set_logprobs(0, None)
    c.set_logprobs(1, 20)
    c.steps(2, "members switched")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    left, left_twin = c.leave(2)
    c.steps(2, "a member left")
    assert raw(left, left.position() + 1) == raw(left_twin, left_twin.position() + 1)
    c.join(2, 30, 40, CFG_F, 7, seed=15)
    c.steps(2, "a member joined")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == nodes
    c.close()


def test_a_batch_without_logprobs_runs_the_shorter_chain_until_its_first_member_with(pkg, hip, worlds):
    W = worlds("qk256")
    s = Cast(pkg, W, 2)  # a batch with such a member from the start: the number to compare with
    s.join(0, 10, 0, None, 5, member=s.owner)
    s.steps(1, "logprobs from the start")
    with_tap = s.batch.graph_nodes()
    assert s.batch.captures() == 1
    s.close()
    c = Cast(pkg, W, 2)
    c.join(0, 10, 0, None, None, member=c.owner)
    c.join(1, 12, 3, None, None)
    c.steps(3, "no member with logprobs")
    assert c.batch.captures() == 1 and c.batch.graph_nodes() == with_tap - 1  # the chain as it was before the tap existed
    c.set_logprobs(1, 5)
    c.steps(3, "the first member with logprobs")
    assert c.batch.captures() == 2 and c.batch.graph_nodes() == with_tap
    c.set_logprobs(0, 20)
    c.set_logprobs(1, None)
    c.steps(2, "the set changes again")
    assert c.batch.captures() == 2 and c.batch.graph_nodes() == with_tap
    c.close()
