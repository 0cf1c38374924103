"""GPU: the stop criteria behind the decoder (Decoder::set_stop / stop_state / resume / run_until_stop, host/decoder.hpp).

The rule: STOP + RESUME EQUALS THE UNINTERRUPTED RUN.  A baseline generates 24 tokens behind a 9-token prompt, one step at a time, and records
after every step the logits, the sampler's draws and Mirostat's state.  tests/stop_ref.py applied to the baseline's history names the step k at
which criteria chosen from that history must stop.  A second decoder with those criteria then queues all 24 steps at once and must be left
exactly where a decoder that ran k steps stands -- state words, history, cache slots below the stop position, sampler state -- with
24 - k frozen steps and the logits of the baseline's step k + 1 (a frozen step consumes the stop token as that step does); resumed, it must
end on the baseline's history, logits and log-probability records.  Every comparison is on integers or bits.

The small synthetic model of tests/test_logprob_decoder_gpu.py (restated here); members borrow one owner's weights."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402
import stop_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=640, eps=1e-5, rope_theta=10000.0)
NP, NG = 9, 24  # prompt tokens, generated tokens
CFG_S, CFG_F = (0.7, 40, 0.95, 1.1), (0.7, 0, 0.95, 1.1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world(pkg, hip):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg = synth.ModelConfig(**MODEL_A)
    owner = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        owner.set_layer_qk256(l, synth.make_layer(cfg, l))
    owner.set_globals(synth.make_globals(cfg))
    owner.reset()
    prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)[:NP]
    return cfg, owner, prompt


CONFIGS = {
    "greedy_full_head": dict(screen=False),
    "greedy_screened_head": dict(),
    "sampler_S": dict(sampling=CFG_S),
    "sampler_F": dict(sampling=CFG_F),
    "mirostat": dict(sampling=(0.8, 0, 1.0, 1.1), mirostat=3.0),
    "logprobs_top5": dict(logprobs=5),
    "f16_cache": dict(kv_f16=True),
    "eager": dict(graph=False),
    "generate_chunk5": dict(chunk=5),
}


def make(world, o):
    cfg, owner, prompt = world
    d = owner.shared()
    d.reset()
    if o.get("kv_f16"):
        d.set_kv_f16(True)
    if "screen" in o:
        d.set_head_screen(o["screen"])
    if "sampling" in o:
        d.set_sampling(*o["sampling"], seed=77)
    if "mirostat" in o:
        d.set_mirostat(o["mirostat"])
    if "logprobs" in o:
        d.set_logprobs(o["logprobs"])
    d.feed(prompt)
    d.run(NP - 1, with_logits=False)  # position NP - 1: the next with-logits step places the first generated token at slot NP
    return d


def sampler_state(d):
    return d.sampling_draws(), d.mirostat_state()


def baseline(world, o):
    """24 single steps; per step (index 1..24) the logits, the sampler state; then the history, the caches and the records"""
    cfg = world[0]
    d = make(world, o)
    logits, states = [None], [sampler_state(d)]
    for _ in range(NG):
        d.run(1, use_graph=o.get("graph", True))
        logits.append(bits(d.last_logits()).copy())
        states.append(sampler_state(d))
    hist = d.history(NP + NG)
    caches = kv.all_layers(d, cfg, bool(o.get("kv_f16")))
    recs = d.logprob_records(NP, NG).tobytes() if "logprobs" in o else None
    d.close()
    return hist, logits, states, caches, recs


def criteria(hist):
    g = [int(t) for t in hist[NP:]]
    return {
        "stop_id": R.Config(stop_ids=(g[7],)),
        "sequence": R.Config(sequences=(tuple(g[9:12]),)),
        "budget": R.Config(max_tokens=5),
    }


@pytest.mark.parametrize("name", list(CONFIGS))
def test_stop_and_resume_equal_the_uninterrupted_run(pkg, world, name):
    cfg = world[0]
    o = CONFIGS[name]
    f16 = bool(o.get("kv_f16"))
    hist, logits, states, caches, recs = baseline(world, o)
    if name == "greedy_screened_head":
        probe = make(world, o)
        assert probe.head_screen() == 1
        probe.close()
    for what, crit in criteria(hist).items():
        k, want = R.first_stop(crit, hist, NP, NG)
        assert k is not None and 1 <= k < NG, (name, what, k)
        if what == "budget":
            assert k == 5
        d = make(world, o)
        d.set_stop(**crit.kwargs())
        if "chunk" in o:
            steps, _ = d.generate(NG, chunk=o["chunk"])
            assert steps == k, (name, what, steps, k)
            queued = min(-(-k // o["chunk"]) * o["chunk"], NG)
        else:
            d.run(NG, use_graph=o.get("graph", True))
            queued = NG
        st = d.stop_state()
        P = want.position
        print(f"{name} / {what}: step {k}, {st}")
        assert st.astuple() == want.public()[:5] + (queued - k,), (name, what, st, want)
        assert P == NP + k - 1 and d.position() == P
        assert np.array_equal(d.history(P + 1), hist[:P + 1]), (name, what)
        for l, ((gk, gv), (wk, wv)) in enumerate(zip(kv.all_layers(d, cfg, f16), caches)):
            assert np.array_equal(gk[:P].view(np.uint8), wk[:P].view(np.uint8)) and np.array_equal(gv[:P].view(np.uint8), wv[:P].view(np.uint8)), (name, what, l)
        assert sampler_state(d) == states[k], (name, what, sampler_state(d), states[k])
        assert np.array_equal(bits(d.last_logits()), logits[k + 1 if queued > k else k]), (name, what)
        # resume: the criteria may stop the sequence again further on (a stop id that recurs); every resume makes at least one step
        done = k
        if what == "budget":
            d.set_stop()  # the kept count would stop it at once: the empty config, armed for a new request
            d.run(NG - done, use_graph=o.get("graph", True))
            done = NG
        while done < NG:
            d.resume()
            d.run(NG - done, use_graph=o.get("graph", True))
            st = d.stop_state()
            nxt = st.position - (NP - 1) if st.stopped else NG
            assert nxt > done, (name, what, done, st)
            done = nxt
        assert d.position() == NP - 1 + NG
        assert np.array_equal(d.history(NP + NG), hist), (name, what)
        if not d.stop_state().stopped or d.stop_state().frozen_steps == 0:
            assert np.array_equal(bits(d.last_logits()), logits[NG]), (name, what)
        assert sampler_state(d) == states[NG], (name, what)
        if recs is not None:
            assert d.logprob_records(NP, NG).tobytes() == recs, (name, what)
        d.close()


def test_eos_as_the_first_generated_token_through_prefill(pkg, world):
    cfg, owner, prompt = world
    base = owner.shared()
    base.feed(prompt)
    base.prefill(NP)
    first = int(base.history(NP + 1)[NP])
    base.run(1)
    step1 = bits(base.last_logits()).copy()
    base.run(4)
    hist = base.history(NP + 6)
    base.close()
    d = owner.shared()
    d.set_stop(eos=first)
    d.feed(prompt)
    d.prefill(NP)
    assert d.stop_state().astuple() == (R.EOS, 0, first, NP, 1, 0)
    assert d.generate(10, chunk=4) == (0, 0.0)  # stopped already: nothing is queued
    d.run(NG)
    assert d.stop_state().astuple() == (R.EOS, 0, first, NP, 1, NG) and d.position() == NP
    assert np.array_equal(d.history(NP + 1), hist[:NP + 1])
    assert np.array_equal(bits(d.last_logits()), step1)
    d.resume()
    d.set_stop()  # (an empty config: the EOS id may recur)
    d.run(5)
    assert np.array_equal(d.history(NP + 6), hist)
    d.close()


def test_rewind_feed_and_reset_re_arm(pkg, world):
    cfg, owner, prompt = world
    d = owner.shared()
    d.set_stop(max_tokens=3)
    d.feed(prompt)
    d.run(NP - 1, with_logits=False)
    d.run(6)
    assert d.stop_state().astuple()[:1] + d.stop_state().astuple()[3:] == (R.MAX_TOKENS, NP + 2, 3, 3)
    d.rewind(NP + 1)  # the stop and the window go, the count stays: the next token is over the budget at once
    assert d.stop_state().astuple() == (R.NONE, 0, 0, 0, 3, 0)
    d.run(2)
    assert d.stop_state().astuple()[3:] == (NP + 2, 4, 1)
    d.feed([5])  # a new request: the count starts again, and the fed token is a prompt token
    assert d.stop_state().astuple() == (R.NONE, 0, 0, 0, 0, 0)
    d.run(4)
    assert d.stop_state().astuple()[3:] == (NP + 5, 3, 1)
    d.reset()
    assert d.stop_state().astuple() == (R.NONE, 0, 0, 0, 0, 0) and d.position() == 0
    with pytest.raises(pkg.BitNetHipError, match="33 stop ids"):
        d.set_stop(stop_ids=range(33))
    d.set_stop(off=True)
    with pytest.raises(pkg.BitNetHipError, match="no stop criteria"):
        d.stop_state()
    with pytest.raises(pkg.BitNetHipError, match="no stop criteria"):
        d.resume()
    d.close()


@pytest.mark.parametrize("with_sampling", [False, True])
def test_graph_nodes_one_more_when_on_and_the_same_when_cleared(pkg, world, with_sampling):
    cfg, owner, prompt = world
    o = dict(sampling=CFG_S, logprobs=3) if with_sampling else dict(screen=False)
    never = make(world, o)
    n0 = never.graph_nodes()
    d = make(world, o)
    d.set_stop(eos=1)
    n1 = d.graph_nodes()
    d.set_stop(eos=2, max_tokens=9)  # a new config keeps the graph
    assert d.graph_nodes() == n1
    d.set_stop(off=True)
    n2 = d.graph_nodes()
    print(f"kernel nodes: never set {n0}, on {n1}, cleared {n2}")
    assert n0 > 0 and n1 == n0 + 1 and n2 == n0
    never.close()
    d.close()
