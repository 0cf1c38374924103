"""GPU: grammar-constrained decoding at the decoder level (Decoder::set_grammar through the exports of host/grammar_host.hpp) -- inside the captured step graphs, the
queued chunks of generate(), a HostBatch and a wide step -- on the small synthetic model of tests/test_sampling_gpu.py.

Greedy decoding under a grammar is set_sampling with temperature 0, which is bit-exact: each step's token is the first argmax of
apply(last_logits(), desc, state) with the restatement of tests/grammar_ref.py, and no tolerance is involved.  The grammars come from
bitnet-rs_amd/grammar.py over a toy byte table for the model's vocabulary."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grammar_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu
NP = 5  # prompt tokens
CHOICES = [b"yes", b"no", b"maybe", b"yesterday", b"nothing"]


def first_argmax(y):
    """the sampler's greedy pick: NaN read as -inf, the lowest index of the maximum (0 if nothing is above -inf)"""
    y = np.where(np.isnan(y), -np.inf, y)
    return int(np.argmax(y)) if np.max(y) > -np.inf else 0


@pytest.fixture(scope="module")
def tg():
    return importlib.import_module("test_sampling_gpu")


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module("bitnet-rs_amd.synth")


@pytest.fixture(scope="module")
def G():
    return importlib.import_module("bitnet-rs_amd.grammar")


def toy_table(V):
    """a byte string for every token of a vocabulary of V >= 600: the 256 single bytes, pieces of the choices, random lower-case strings of two to
    four letters, and the EOS (no bytes) at V - 1"""
    rng = np.random.default_rng(77)
    pieces = [b"ye", b"yes", b"es", b"no", b"may", b"maybe", b"be", b"ter", b"day", b"yester", b"not", b"thing", b"hing", b"ing", b"ma", b"yb", b"th",
              b"st", b"er", b"da", b"ay", b"in", b"ng", b"yes,", b"no,", b"s,", b"o,", b","]
    table = [bytes([b]) for b in range(256)] + pieces
    while len(table) < V - 1:
        table.append(bytes(rng.integers(97, 123, size=int(rng.integers(2, 5))).astype(np.uint8)))
    return table + [b""], V - 1


def choice_grammar(G, V):
    table, eos = toy_table(V)
    dfa = G.ByteDFA.from_choices(CHOICES)
    tc, nx, start = G.token_automaton(dfa, table, eos)
    return (tc, nx), start, table, eos, dfa.n


def cyclic_grammar(G, V):
    """(yes,|no,)* for ever: the transitions into the trie's accepting states lead back to the start; no EOS"""
    table, _ = toy_table(V)
    trie = G.ByteDFA.from_choices([b"yes,", b"no,"])
    nx = trie.next.copy()
    for a in trie.accepting:
        nx[nx == a] = 0
    tc, nxt, start = G.token_automaton(G.ByteDFA(nx, 0, [0]), table, None)
    return (tc, nxt), start, table


def set_grammar(dec, g, start=0):
    """bitnet_host_set_grammar on a HostDecoder, through the library the package bound from host/grammar_host.hpp; g None: off"""
    dec._check(dec.c.bitnet_host_set_grammar(dec.h, g.h if g is not None else None, int(start)))


def set_grammar_state(dec, state):
    dec._check(dec.c.bitnet_host_set_grammar_state(dec.h, int(state)))


def grammar_state(dec):
    s, n, v = C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
    dec._check(dec.c.bitnet_host_grammar_state(dec.h, C.byref(s), C.byref(n), C.byref(v)))
    return int(s.value), int(n.value), int(v.value)


def begin(dec, prompt):
    dec.reset()
    dec.feed(prompt)
    dec.run(len(prompt) - 1, with_logits=False, use_graph=True)


def generated(dec, n):
    return [int(t) for t in dec.history(NP + n)[NP:]]


def checked_steps(dec, prompt, desc, start, n, what):
    """n steps of run(1), each held against the restatement on the decoder's own logits; returns (tokens, the state after each)"""
    begin(dec, prompt)
    s, toks, states = start, [], []
    for i in range(n):
        assert grammar_state(dec) == (s, i, 0), (what, i)
        dec.run(1, with_logits=True, use_graph=True)
        got = int(dec.history(NP + i + 1)[-1])
        want = first_argmax(gr.apply(dec.last_logits(), desc, s))
        assert got == want, (what, "step", i, got, want)
        s = gr.step(desc, s, got)
        assert s >= 0, (what, "a banned token was chosen", i, got)
        toks.append(got)
        states.append(s)
    assert grammar_state(dec) == (s, n, 0) and dec.sampling_draws() == 0
    return toks, states


@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
def test_greedy_under_a_choice_grammar(hip, pkg, tg, synth, G, fmt):
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL, fmt)
    prompt = synth.prompt(NP, cfg.vocab)
    desc, start, table, eos, end = choice_grammar(G, cfg.vocab)
    g = hip.grammar(*desc)
    begin(dec, prompt)
    dec.run(16, with_logits=True, use_graph=True)
    plain = generated(dec, 16)
    with pytest.raises(pkg.BitNetHipError, match="set_grammar: sampling is off"):
        set_grammar(dec, g, start)
    set_grammar(dec, None)  # off on a decoder that never sampled: nothing to switch off
    assert grammar_state(dec) == (-1, 0, 0)
    dec.set_sampling(0.0, seed=1)
    assert grammar_state(dec) == (-1, 0, 0)
    set_grammar(dec, g, start)
    toks, states = checked_steps(dec, prompt, desc, start, 14, (fmt, "choices"))
    assert toks != plain[:14] and eos in toks
    k = toks.index(eos)
    text = b"".join(table[t] for t in toks[:k])
    assert text in CHOICES, text
    for j in range(k + 1):  # every prefix of the tokens spells a prefix of that choice
        assert text.startswith(b"".join(table[t] for t in toks[:j]))
    assert all(t == eos for t in toks[k:]) and states[k:] == [end] * (14 - k)  # in the end state only EOS is allowed
    # stop criteria on EOS and chunks: the frozen steps leave state and counters as a run that ended on EOS leaves them
    dec.set_stop(eos=eos)
    begin(dec, prompt)
    steps, _ = dec.generate(64, chunk=16)
    st = dec.stop_state()
    assert steps == k + 1 and st.stopped and st.reason == pkg.STOP_EOS and st.token == eos and st.frozen_steps == (-steps) % 16
    assert generated(dec, steps) == toks[:k + 1] and grammar_state(dec) == (end, k + 1, 0)
    dec.set_stop(off=True)
    # another start state: the second byte of a choice on
    s1 = gr.walk(desc, start, [ord("y")])[0]
    set_grammar(dec, g, s1)
    toks1, _ = checked_steps(dec, prompt, desc, s1, 12, (fmt, "from y"))
    assert (b"y" + b"".join(table[t] for t in toks1[:toks1.index(eos)])) in CHOICES
    set_grammar(dec, None)
    begin(dec, prompt)
    dec.run(16, with_logits=True, use_graph=True)
    assert generated(dec, 16) == plain and grammar_state(dec) == (-1, 0, 0)  # off again: the graphs were kept and run what they ran
    dec.close()
    g.close()


def test_resume_and_rewind_under_a_cyclic_grammar(hip, pkg, tg, synth, G):
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL)
    prompt = synth.prompt(NP, cfg.vocab)
    desc, start, table = cyclic_grammar(G, cfg.vocab)
    g = hip.grammar(*desc)
    dec.set_sampling(0.0, seed=1)
    set_grammar(dec, g, start)
    N = 24
    whole, states = checked_steps(dec, prompt, desc, start, N, "cyclic")
    text = b"".join(table[t] for t in whole)
    assert text.replace(b"yes,", b"").replace(b"no,", b"") in (b"", b"y", b"ye", b"yes", b"n", b"no")  # (yes,|no,)* and an unfinished word
    final = grammar_state(dec)
    # stop on a token of the run, resume until the end: the uninterrupted run's tokens, state and counters
    dec.set_stop(stop_ids=[whole[5]])
    begin(dec, prompt)
    done, _ = dec.generate(N, chunk=8)
    assert done == whole.index(whole[5]) + 1 and grammar_state(dec) == (states[done - 1], done, 0)
    while done < N:
        dec.resume()
        dec.run(N - done, use_graph=True)
        st = dec.stop_state()
        nxt = st.position - (NP - 1) if st.stopped else N
        assert nxt > done
        done = nxt
    assert generated(dec, N) == whole and grammar_state(dec) == final
    dec.set_stop(off=True)
    # rewind does not move the sampler: the caller sets the state from walk over the tokens that remain
    keep = 9  # generated tokens kept; the ninth is consumed again by the next step
    dec.rewind(NP - 1 + keep)
    assert grammar_state(dec) == final
    s, taken = g.walk(start, whole[:keep])
    assert taken == keep and s == states[keep - 1]
    set_grammar_state(dec, s)
    assert grammar_state(dec) == (s, final[1], 0)  # the counters stay
    dec.run(N - keep, with_logits=True, use_graph=True)
    assert generated(dec, N) == whole and grammar_state(dec) == (final[0], final[1] + N - keep, 0)
    dec.close()
    g.close()


@pytest.fixture(scope="module")
def world(pkg):
    tb = importlib.import_module("test_batch_sampling_gpu")
    return tb.World(importlib.import_module("bitnet-rs_amd.synth"), "qk256")


def follow(desc, s, toks):
    """the states along toks from s; every token must be allowed where it was chosen"""
    out = []
    for t in toks:
        s = gr.step(desc, s, t)
        assert s >= 0, ("a token the state does not allow", t, out)
        out.append(s)
    return out


def test_a_batch_of_three_two_under_one_grammar(hip, pkg, world, G):
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = world
    desc, start, table = cyclic_grammar(G, W.cfg.vocab)
    g = hip.grammar(*desc)
    starts = [start, gr.walk(desc, start, [ord("y"), ord("e")])[0], None]
    c = tb.Cast(pkg, W, 3)

    def join(b, length, offset, sampling, s0, member=None):
        m, t = member or c.owner.shared(), W.twin(pkg)
        for d in (m, t):
            if sampling:
                d.set_sampling(**sampling)
            if s0 is not None:
                set_grammar(d, g, s0)
            tb.start(d, W, length, offset)
        c.batch.set_slot(b, m)
        c.members[b], c.twins[b] = m, t
        c.all += [x for x in (m, t) if x is not c.owner]

    join(0, 20, 0, dict(temperature=0.0, seed=1), starts[0], member=c.owner)
    join(1, 22, 5, dict(temperature=0.8, top_k=8, seed=2), starts[1])
    join(2, 21, 9, None, None)  # stays greedy, no sampler
    c.steps(8, "grammared members beside a plain one")  # compares history, position, logits bits, caches, draws after every step
    for b, n in ((0, 20), (1, 22)):
        m, t = c.members[b], c.twins[b]
        toks = [int(x) for x in m.history(m.position() + 1)[n:]]  # the prompt forward's first token and eight steps
        states = follow(desc, starts[b], toks)
        assert len(toks) == 9 and grammar_state(m) == grammar_state(t) == (states[-1], 9, 0)
    assert grammar_state(c.members[2]) == (-1, 0, 0)
    # the plain member took the tokens of a run with no grammar anywhere in the group
    plain = W.twin(pkg)
    tb.start(plain, W, 21, 9)
    plain.run(8, with_logits=True, use_graph=True)
    p = plain.position()
    assert np.array_equal(plain.history(p + 1), c.members[2].history(p + 1))
    plain.close()
    c.close()
    g.close()


def test_a_step_wide_of_five_three_under_one_grammar(hip, pkg, world, G):
    """a wide step's logits are the member's own run()'s up to rounding, not bit for bit: each grammared member's token is held to the
    restatement on the member's OWN logits (exact) and must be allowed from its state; the plain members equal a wide step of plain members alone"""
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = world
    desc, start, table = cyclic_grammar(G, W.cfg.vocab)
    g = hip.grammar(*desc)
    starts = [start, None, gr.walk(desc, start, [ord("n")])[0], None, gr.walk(desc, start, [ord("y"), ord("e"), ord("s")])[0]]
    owner = W.decoder(pkg)
    ms = [owner] + [owner.shared() for _ in range(4)]
    for i, m in enumerate(ms):
        if starts[i] is not None:
            m.set_sampling(temperature=0.0, seed=1)
            set_grammar(m, g, starts[i])
        tb.start(m, W, 20 + i, 4 * i)
    first = [int(m.history(m.position() + 1)[-1]) for m in ms]  # the prompt forward's own pick moved the state once
    states = [None if s is None else follow(desc, s, [first[i]])[-1] for i, s in enumerate(starts)]
    for step in range(6):
        owner.step_wide(ms, 1, digits=2)
        for i, m in enumerate(ms):
            got = int(m.history(m.position() + 1)[-1])
            if states[i] is None:
                assert grammar_state(m) == (-1, 0, 0)
                continue
            assert got == first_argmax(gr.apply(m.last_logits(), desc, states[i])), ("wide member", i, "step", step)
            states[i] = follow(desc, states[i], [got])[-1]
            assert grammar_state(m) == (states[i], step + 2, 0)
    # the plain members against the same group of five with no grammar anywhere in it (the same samplers, the same prompts)
    o2 = W.decoder(pkg)
    ps = [o2] + [o2.shared() for _ in range(4)]
    for i, m in enumerate(ps):
        if starts[i] is not None:
            m.set_sampling(temperature=0.0, seed=1)
        tb.start(m, W, 20 + i, 4 * i)
    for step in range(6):
        o2.step_wide(ps, 1, digits=2)
    differ = 0
    for i, m in enumerate(ps):
        p = m.position()
        same = p == ms[i].position() and np.array_equal(m.history(p + 1), ms[i].history(p + 1))
        if starts[i] is None:
            assert same, ("plain member", i)
        differ += not same
    assert differ >= 1  # the grammar did move its members' tokens
    for d in ms[1:] + [owner] + ps[1:] + [o2]:
        d.close()
    g.close()
