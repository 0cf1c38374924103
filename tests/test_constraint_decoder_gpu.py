"""GPU: logit constraints at the decoder level (Decoder::set_constraints, HostDecoder.set_constraints) -- inside the captured step graphs, the
queued chunks of generate(), a HostBatch and a wide step -- on the small synthetic model of tests/test_sampler_chain_gpu.py.

Greedy decoding with constraints is set_sampling with temperature 0, which is bit-exact: each step's token is argmax(apply(last_logits(),
cfg, g, history)) with the restatement of tests/constraint_ref.py, lowest index on ties, and no tolerance is involved."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
NP = 5  # prompt tokens


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


def begin(dec, prompt):
    dec.reset()
    dec.feed(prompt)
    dec.run(len(prompt) - 1, with_logits=False, use_graph=True)


def generated(dec, n):
    return [int(t) for t in dec.history(NP + n)[NP:]]


def greedy_run(dec, prompt, n):
    begin(dec, prompt)
    dec.run(n, with_logits=True, use_graph=True)
    return generated(dec, n)


def checked_steps(dec, prompt, cfg, n, what):
    """n steps of run(1), each held against the restatement on the decoder's own logits; returns the tokens"""
    begin(dec, prompt)
    toks = []
    for i in range(n):
        seq = [int(t) for t in dec.history(NP + i)]
        g = dec.chosen()
        assert g == i, (what, i, g)
        dec.run(1, with_logits=True, use_graph=True)
        got = int(dec.history(NP + i + 1)[-1])
        want = first_argmax(cr.apply(dec.last_logits(), cfg, g, seq))
        assert got == want, (what, "step", i, got, want)
        toks.append(got)
    return toks


@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
def test_greedy_with_constraints_is_the_argmax_of_the_edited_row(hip, pkg, tg, synth, fmt):
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL, fmt)
    prompt = synth.prompt(NP, cfg.vocab)
    plain = greedy_run(dec, prompt, 32)
    with pytest.raises(pkg.BitNetHipError, match="set_constraints: sampling is off"):
        dec.set_constraints(bias={1: 1.0})
    dec.set_constraints()  # off on a decoder that never sampled: nothing to switch off
    dec.set_sampling(0.0, seed=1)
    assert greedy_run(dec, prompt, 32) == plain and dec.chosen() == 0  # temperature 0 without constraints: the decoder's own greedy tokens
    V = cfg.vocab
    con = dict(bias=[(plain[0], -np.inf), (plain[1], -4.0), (0, 3.0), (V - 1, 3.0), (plain[2], 1.0), (plain[2], -np.inf)], hold=[plain[3], V - 1],
               min_tokens=6, no_repeat_ngram=2)
    dec.set_constraints(**con)
    toks = checked_steps(dec, prompt, con, 16, (fmt, "bias-hold-ngram"))
    assert toks != plain[:16] and plain[0] not in toks and plain[2] not in toks
    assert dec.chosen() == 16 and dec.sampling_draws() == 0
    allowed = sorted(set(plain[:6]) | {0, 1, V - 1, V // 2})
    con = dict(allowed=allowed, bias={V // 2: 0.5})
    dec.set_constraints(**con)
    toks = checked_steps(dec, prompt, con, 16, (fmt, "allowed"))
    assert set(toks) <= set(allowed)
    # the first 8 tokens of the unconstrained run, banned: none of them appears in 32 constrained steps
    dec.set_constraints(bias={t: -np.inf for t in plain[:8]})
    banned_run = greedy_run(dec, prompt, 32)
    assert not set(banned_run) & set(plain[:8]) and dec.chosen() == 32
    dec.set_constraints(off=True)
    assert greedy_run(dec, prompt, 32) == plain  # off again: the graphs were kept and run what they ran
    dec.close()


def has_repeated_bigram(seq):
    seen = set()
    for a, b in zip(seq, seq[1:]):
        if (a, b) in seen:
            return True
        seen.add((a, b))
    return False


def test_no_repeat_ngram_2_repeats_no_bigram(hip, pkg, tg, synth):
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL)
    prompt = synth.prompt(NP, cfg.vocab)
    dec.set_sampling(0.0, repetition_penalty=1.0, seed=1)
    plain = list(prompt) + greedy_run(dec, prompt, 48)
    assert has_repeated_bigram(plain), "the unconstrained greedy run repeats no bigram: this test would pass vacuously"
    dec.set_constraints(no_repeat_ngram=2)
    toks = list(prompt) + greedy_run(dec, prompt, 48)
    assert not has_repeated_bigram(toks) and dec.chosen() == 48
    dec.close()


def test_eos_hold_off_with_stop_criteria_and_chunks(hip, pkg, tg, synth):
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL)
    prompt = synth.prompt(NP, cfg.vocab)
    dec.set_sampling(0.0, seed=1)
    plain = greedy_run(dec, prompt, 8)
    E = plain[2]  # the token the unconstrained run emits third
    dec.set_stop(eos=E)
    begin(dec, prompt)
    steps, _ = dec.generate(32, chunk=4)
    st = dec.stop_state()
    first = plain.index(E) + 1
    assert first <= 3 and steps == first and st.stopped and st.generated == first and st.token == E  # without the hold-off it ends at once
    dec.set_constraints(hold=[E], min_tokens=8)
    begin(dec, prompt)
    dec.set_stop(eos=E, max_tokens=18)  # the budget ends the run inside a chunk if E does not come back: the sequence stops either way
    steps, _ = dec.generate(32, chunk=4)
    st = dec.stop_state()
    n = steps
    chunked = generated(dec, n)
    assert st.generated >= 8 and E not in chunked[:8]
    assert st.stopped and 8 < n <= 18 and st.generated == n and st.token == chunked[-1]
    assert (chunked[-1] == E) == (st.reason == pkg.STOP_EOS) and (n == 18 or st.reason == pkg.STOP_EOS)
    assert st.frozen_steps == (-n) % 4 and dec.chosen() == n  # the chunk's steps behind the stop were frozen: they chose nothing
    # the same tokens from run(1) repeated
    dec.set_stop(off=True)
    begin(dec, prompt)
    for _ in range(n):
        dec.run(1, with_logits=True, use_graph=True)
    assert generated(dec, n) == chunked and dec.chosen() == n
    dec.close()


def test_fork_resets_the_count_and_keeps_each_decoders_own_config(hip, pkg, tg, synth):
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL)
    prompt = synth.prompt(NP, cfg.vocab)
    dec.set_sampling(0.0, seed=1)
    plain = greedy_run(dec, prompt, 4)
    child = dec.shared()
    child.set_sampling(0.0, seed=1)
    child.set_constraints(bias={plain[0]: -np.inf})
    child.reset()
    child.feed(prompt)
    child.run(NP - 1, with_logits=False, use_graph=True)
    child.run(3, with_logits=True, use_graph=True)
    assert child.chosen() == 3
    begin(dec, prompt)
    dec.fork_into([child], NP - 1)
    assert child.chosen() == 0 and dec.chosen() == 0
    child.feed([prompt[-1]])
    child.run(1, with_logits=True, use_graph=True)
    dec.run(1, with_logits=True, use_graph=True)
    assert int(dec.history(NP + 1)[-1]) == plain[0] != int(child.history(NP + 1)[-1])  # the source has no constraints, the destination kept its own
    child.close()
    dec.close()


@pytest.fixture(scope="module")
def world(pkg):
    tb = importlib.import_module("test_batch_sampling_gpu")
    return tb.World(importlib.import_module("bitnet-rs_amd.synth"), "qk256")


def member_config(W, i):
    V = W.cfg.vocab
    return dict(bias=[(int(W.prompt[3 + i]), -np.inf), (V - 1 - i, 2.5), (i, 2.5)], hold=[V - 1 - i], min_tokens=3, no_repeat_ngram=1 + i % 2)


def test_a_batch_member_with_constraints_gets_the_tokens_of_its_own_run(hip, pkg, world):
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = world
    c = tb.Cast(pkg, W, 3)

    def join(b, length, offset, sampling, con, member=None):
        m, t = member or c.owner.shared(), W.twin(pkg)
        for d in (m, t):
            if sampling:
                d.set_sampling(**sampling)
            if con:
                d.set_constraints(**con)
            tb.start(d, W, length, offset)
        c.batch.set_slot(b, m)
        c.members[b], c.twins[b] = m, t
        c.all += [x for x in (m, t) if x is not c.owner]

    join(0, 20, 0, dict(temperature=0.0, seed=1), member_config(W, 0), member=c.owner)
    join(1, 22, 5, dict(temperature=0.8, top_k=8, seed=2), member_config(W, 1))
    join(2, 21, 9, None, None)  # stays greedy, no sampler
    c.steps(8, "constrained members beside a greedy one")  # compares history, position, logits bits, caches, draws after every step
    for b in (0, 1):
        assert c.members[b].chosen() == c.twins[b].chosen() == 9  # the prompt forward's first token and eight steps
    # the constrained greedy member took the restatement's tokens
    m = c.members[0]
    p = m.position()
    seq = [int(t) for t in m.history(p + 1)]
    m.set_constraints(off=True)
    c.twins[0].set_constraints(off=True)
    c.steps(4, "constraints off again")
    assert c.batch.captures() == 1 and m.chosen() == 9
    assert int(W.prompt[3]) not in seq[20:]  # its banned token
    c.close()


def test_a_step_wide_member_with_constraints(hip, pkg, world):
    """a wide step's logits are the member's own run()'s up to rounding, not bit for bit: each member's token is held to the restatement on the
    member's OWN logits (exact), and to its twin's run() under attention form 0; at every one of the 12 comparisons the twin's two best edited
    logits must lie further apart than twice what the two rows differ by, so none is left undecided"""
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = world
    owner = W.decoder(pkg)
    ms = [owner, owner.shared(), owner.shared()]
    twins = [W.twin(pkg) for _ in ms]
    cons = [member_config(W, 0), None, member_config(W, 1)]
    for i, (m, t) in enumerate(zip(ms, twins)):
        for d in (m, t):
            if cons[i]:
                d.set_sampling(temperature=0.0, seed=1)
                d.set_constraints(**cons[i])
            tb.start(d, W, 20 + i, 4 * i)
    decided = 0
    for step in range(6):
        before = [([int(x) for x in m.history(m.position() + 1)], m.chosen()) for m in ms]
        owner.step_wide(ms, 1, digits=2)
        for i, (m, t) in enumerate(zip(ms, twins)):
            t.run(1, with_logits=True, use_graph=True)
            p = m.position()
            got = int(m.history(p + 1)[-1])
            seq, g = before[i]
            if cons[i]:
                assert g == step + 1 and m.chosen() == g + 1
                assert got == first_argmax(cr.apply(m.last_logits(), cons[i], g, seq)), ("wide member", i, "step", step)
                y = np.sort(np.nan_to_num(cr.apply(t.last_logits(), cons[i], g, seq), nan=-np.inf, neginf=-1e30))
                gap, noise = float(y[-1] - y[-2]), float(np.max(np.abs(m.last_logits() - t.last_logits())))
                print(f"  wide member {i} step {step}: gap {gap:.3e} between the twin's two best edited logits, rows differ by {noise:.3e}")
                assert gap > 2 * noise, ("undecided: the twin's two best logits lie closer than the rows differ", i, step, gap, noise)
                decided += 1
                assert got == int(t.history(p + 1)[-1]), ("wide member against its own run()", i, step, gap, noise)
            else:
                assert m.chosen() == 0
    assert decided == 12  # two constrained members, six steps: nobody was undecided
    for d in ms[1:] + twins + [owner]:
        d.close()
