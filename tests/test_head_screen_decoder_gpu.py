"""GPU: the decoder's screened greedy head (Decoder::set_head_screen; host/decoder.hpp) against its full head, in one process through the setter.

Plain greedy steps pick their token from the int8 screening image and leave last_logits() to a recomputation on demand: tokens and
last_logits() must be the full head's BIT FOR BIT, graph and eager, after run() and after prefill(); a step with the sampler, the logits tap or a
tracer must take the full head (the device's launch counter of the screened head does not move); a create_shared borrower decodes with the
owner's image.  Model "A" of tests/test_batch_decoder_gpu.py (2 layers, hidden 512, vocab 2048), both storage formats."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=640, eps=1e-5, rope_theta=10000.0)
STEPS = 12


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


@pytest.fixture(scope="module")
def worlds(pkg):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    made = {}

    def get(fmt):
        if fmt not in made:
            made[fmt] = World(synth, fmt)
        return made[fmt]

    return get


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def generate(dec, W, n_prompt, use_graph, prefill=False):
    """prompt, then STEPS greedy steps -> (history, last_logits bits, last_logits bits of a second call)"""
    dec.reset()
    dec.feed(W.prompt[:n_prompt])
    if prefill:
        dec.prefill(n_prompt, with_logits=True, digits=2)
        first = bits(dec.last_logits()).copy()
    else:
        dec.run(n_prompt - 1, with_logits=False, use_graph=use_graph)
        first = None
    dec.run(STEPS, with_logits=True, use_graph=use_graph)
    a = bits(dec.last_logits()).copy()
    b = bits(dec.last_logits()).copy()
    return np.asarray(dec.history(dec.position() + 1)).copy(), a, b, first


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_tokens_and_last_logits_equal_the_full_head(pkg, hip, worlds, fmt):
    W = worlds(fmt)
    dec = W.decoder(pkg)
    assert dec.head_screen() == 1  # on by default, and hidden 512 has an instance
    for use_graph in (True, False):
        for prefill in (False, True):
            dec.set_head_screen(False)
            assert dec.head_screen() == 0
            launches0 = dec.head_screen_stats()[1]
            want = generate(dec, W, 9 if not prefill else 70, use_graph, prefill)
            assert dec.head_screen_stats()[1] == launches0  # the full head ran
            dec.set_head_screen(True)
            got = generate(dec, W, 9 if not prefill else 70, use_graph, prefill)
            last, launches, total = dec.head_screen_stats()
            tag = (fmt, use_graph, prefill)
            assert launches == launches0 + STEPS + (1 if prefill else 0), tag  # every with-logits head of the run, the prompt's included
            assert 1 <= last <= W.cfg.vocab, tag
            assert np.array_equal(got[0], want[0]), (tag, "history")
            assert np.array_equal(got[1], want[1]), (tag, "last_logits", int((got[1] != want[1]).sum()))
            assert np.array_equal(got[2], got[1]), (tag, "last_logits twice")
            if prefill:
                assert np.array_equal(got[3], want[3]), (tag, "last_logits after prefill")


def test_readers_of_the_logits_force_the_full_head(pkg, hip, worlds, tmp_path):
    W = worlds("i2s")
    dec, ref_dec = W.decoder(pkg), W.decoder(pkg)
    ref_dec.set_head_screen(False)
    for d in (dec, ref_dec):
        d.feed(W.prompt[:6])
        d.run(5, with_logits=False)
        d.run(2, with_logits=True)
    assert dec.head_screen_stats()[1] == 2 and ref_dec.head_screen_stats()[1] == 0

    def step(d, how):
        if how == "sampling":
            d.set_sampling(0.8, top_k=20, seed=3)
            d.run(2, with_logits=True)
            d.set_sampling(None)
        elif how == "tap":
            d.set_logprobs(3)
            d.run(2, with_logits=True)
            d.set_logprobs(None)
        elif how == "trace":
            d.trace_step(str(tmp_path), with_logits=True)
        else:
            d.run(2, with_logits=True)

    launches = 2
    for how in ("sampling", "plain", "tap", "plain", "trace", "plain"):
        step(dec, how)
        step(ref_dec, how)
        launches += 2 if how == "plain" else 0
        assert dec.head_screen_stats()[1] == launches, how  # untouched by every step whose logits are read
        assert dec.position() == ref_dec.position()
        assert np.array_equal(dec.history(dec.position() + 1), ref_dec.history(ref_dec.position() + 1)), how
        assert np.array_equal(bits(dec.last_logits()), bits(ref_dec.last_logits())), how
    assert ref_dec.head_screen_stats()[1] == 0


def test_borrower_decodes_with_the_owners_image(pkg, hip, worlds):
    W = worlds("qk256")
    owner = W.decoder(pkg)
    twin = W.decoder(pkg)
    twin.set_head_screen(False)
    b = owner.shared()
    assert b.head_screen() == 1
    for d in (b, twin):
        d.feed(W.prompt[20:31])
        d.run(10, with_logits=False)
        d.run(STEPS, with_logits=True)
    assert b.head_screen_stats()[1] == STEPS and owner.head_screen_stats()[1] == 0  # the counters are the decoder's own
    assert np.array_equal(b.history(b.position() + 1), twin.history(twin.position() + 1))
    assert np.array_equal(bits(b.last_logits()), bits(twin.last_logits()))


def test_environment_switch_selects_the_full_head(pkg, hip, worlds, monkeypatch):
    W = worlds("i2s")
    monkeypatch.setenv("BITNET_HOST_HEAD_SCREEN", "0")
    dec = W.decoder(pkg)
    assert dec.head_screen() == 0
    dec.feed(W.prompt[:4])
    dec.run(3, with_logits=False)
    dec.run(2, with_logits=True)
    assert dec.head_screen_stats()[1] == 0
    dec.set_head_screen(True)  # builds the image now
    assert dec.head_screen() == 1
    dec.run(2, with_logits=True)
    assert dec.head_screen_stats()[1] == 2
