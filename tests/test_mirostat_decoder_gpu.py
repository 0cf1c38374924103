"""GPU: Mirostat v2 through the decoder host (Decoder::set_mirostat / mirostat_state, HostDecoder.set_mirostat) on the small synthetic models
of the sampler-chain decoder tests, both storage formats.

run(16) on the step graphs equals 16 eager single steps bit for bit (history, mu, fallback count, word counter), and every one of those steps
passes the rule of tests/mirostat_accept.py, judged from last_logits() of the eager twin and the mu it held before the step.  reset() restores
mu, rewind() and shift() leave it, fork resets each destination's.  A Mirostat member of a HostBatch ends as it does alone under form 0, bit for
bit; in prefill_packed and step_wide (the same arithmetic class as extend, not the same bits) its pick passes the rule on its own logits.
set_mirostat without sampling is refused."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirostat_accept as ma  # noqa: E402
import mirostat_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SAMPLING = dict(temperature=0.7, repetition_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.05)


def switch_on(dec, tau, eta, seed):
    dec.set_sampling(SAMPLING["temperature"], 0, 1.0, SAMPLING["repetition_penalty"], seed=seed, frequency_penalty=SAMPLING["frequency_penalty"],
                     presence_penalty=SAMPLING["presence_penalty"])
    dec.set_mirostat(tau, eta)
    return mr.MirostatRef(tau, eta, seed=seed, **SAMPLING)


def judged_step(dec, ref, gen, step, what):
    """one with-logits step of `dec` (step() makes it), judged from the decoder's own logits, its mu before the step and its word counter"""
    mu_b, fb_b = dec.mirostat_state()
    d_b = dec.sampling_draws()
    step()
    p = dec.position()
    tok = int(dec.history(p + 1)[p])
    mu_a, fb_a = dec.mirostat_state()
    d_a = dec.sampling_draws()
    ref.rng.draws = d_b
    ref.sample(dec.last_logits(), gen, mu=F(mu_b))
    v = ma.judge(ref.last, ma.u_of(ref.rng, d_b), tok, F(mu_a), d_a - d_b)
    print(f"  {what}: token {tok} (restatement {ref.last['token']}) mu {mu_b!r} -> {mu_a!r} words {d_a - d_b}: {v['reason']}")
    assert v["ok"], (what, v["reason"])
    assert fb_a - fb_b == (1 if v["mode"] == "fallback" else 0), (what, fb_b, fb_a)
    gen.append(tok)
    return v


def bits(x):
    return F(x).tobytes()


@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
@pytest.mark.parametrize("tau", [5.0, 0.5])
def test_run16_on_the_graphs_equals_16_eager_steps_and_each_passes_the_rule(hip, pkg, fmt, tau):
    tg = importlib.import_module("test_sampling_gpu")
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL, fmt)
    _, twin = tg.make_decoder(pkg, synth, tg.SMALL, fmt)
    prompt = synth.prompt(5, cfg.vocab)
    n = 16
    with pytest.raises(pkg.BitNetHipError, match="sampling is off"):
        dec.set_mirostat(tau, 0.1)  # greedy decoder: refused
    assert dec.mirostat_state() == (0.0, 0)
    dec.set_mirostat(None)  # nothing to switch off: fine
    switch_on(dec, tau, 0.1, 42)
    ref = switch_on(twin, tau, 0.1, 42)
    for d in (dec, twin):
        d.reset()
        d.feed(prompt)
        d.run(len(prompt) - 1, with_logits=False, use_graph=True)
    assert dec.mirostat_state() == (2 * tau, 0)  # forced positions moved nothing
    dec.run(n, with_logits=True, use_graph=True)
    gen, modes = [], []
    for i in range(n):
        v = judged_step(twin, ref, gen, lambda: twin.run(1, with_logits=True, use_graph=False), (fmt, tau, "eager step", i))
        modes.append(v["mode"])
    L = len(prompt) + n
    assert np.array_equal(dec.history(L), twin.history(L))
    (mg, fg), (mt, ft) = dec.mirostat_state(), twin.mirostat_state()
    assert bits(mg) == bits(mt) and fg == ft and dec.sampling_draws() == twin.sampling_draws() == modes.count("draw")
    assert mg != 2 * tau
    # rewind and shift leave mu (as they leave the counts); reset restores it
    dec.rewind(len(prompt) + 8)
    assert dec.mirostat_state() == (mg, fg)
    dec.shift(2, 4)
    assert dec.mirostat_state() == (mg, fg)
    dec.reset()
    assert dec.mirostat_state() == (2 * tau, 0) and dec.sampling_draws() == 0
    # the same graphs, another tau: set_mirostat drops none
    for d in (dec, twin):
        d.set_mirostat(3.0, 0.2)
        d.reset()
        d.feed(prompt)
        d.run(len(prompt) - 1, with_logits=False, use_graph=True)
        d.run(4, with_logits=True, use_graph=d is dec)
    assert np.array_equal(dec.history(len(prompt) + 4), twin.history(len(prompt) + 4))
    assert bits(dec.mirostat_state()[0]) == bits(twin.mirostat_state()[0]) and dec.mirostat_state()[0] != 6.0
    # switched off, the sampler is the chain sampler it was; a config with a truncation stage is refused while Mirostat is on
    with pytest.raises(pkg.BitNetHipError, match="Mirostat needs"):
        dec.set_sampling(0.7, top_k=40, seed=1)
    dec.set_mirostat(None)
    dec.set_sampling(0.7, top_k=40, seed=1)
    assert dec.mirostat_state() == (0.0, 0)
    dec.close()
    twin.close()


@pytest.fixture(scope="module")
def world(pkg):
    tb = importlib.import_module("test_batch_sampling_gpu")
    return tb.World(importlib.import_module("bitnet-rs_amd.synth"), "qk256")


def test_fork_resets_each_destination(hip, pkg, world):
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = world
    src = W.decoder(pkg)
    dsts = [src.shared(), src.shared()]
    switch_on(src, 5.0, 0.1, 1)
    switch_on(dsts[0], 3.0, 0.1, 2)
    dsts[1].set_sampling(0.8, top_k=40, seed=3)  # a chain sampler, no Mirostat
    for i, d in enumerate([src] + dsts):
        tb.start(d, W, 20, 3 * i)
        d.run(4, with_logits=True, use_graph=True)
    before = src.mirostat_state()
    assert before[0] != 10.0 and dsts[0].mirostat_state()[0] != 6.0
    src.fork_into(dsts, 12)
    assert src.mirostat_state() == before                  # the source is untouched
    assert dsts[0].mirostat_state() == (6.0, 0)            # its own 2 * tau, as its sampler was reset
    assert dsts[1].mirostat_state() == (0.0, 0) and dsts[0].sampling_draws() == 0
    for d in dsts + [src]:
        d.close()


def test_a_mirostat_member_of_a_batch_ends_as_it_does_alone(hip, pkg, world):
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = world
    owner = W.decoder(pkg)
    batch = pkg.HostBatch(4)
    members = [owner, owner.shared(), owner.shared()]
    twins = [W.twin(pkg) for _ in members]
    plans = [(5.0, 0.1, 61), (0.5, 0.1, 62), None]  # a drawing member, one in the fallback regime, a greedy one
    for b, (m, t, plan) in enumerate(zip(members, twins, plans)):
        for d in (m, t):
            if plan:
                switch_on(d, *plan)
            tb.start(d, W, 58 + 2 * b, 5 * b)  # the prompts cross the 64-key boundary within the first steps
        batch.set_slot(b, m)
    for step in range(8):
        batch.step(1, use_graph=True)
        for b, (m, t) in enumerate(zip(members, twins)):
            t.run(1, with_logits=True, use_graph=True)
            tb.assert_same(tb.state(m, W.cfg), tb.state(t, W.cfg), ("step", step, "slot", b))
            (mm, fm), (mt, ft) = m.mirostat_state(), t.mirostat_state()
            assert bits(mm) == bits(mt) and fm == ft, (step, b, mm, mt, fm, ft)
    for m in members[:2]:  # the pick behind the prompt and eight steps: each one a draw or a fallback
        assert m.mirostat_state()[1] + m.sampling_draws() == 9
    assert members[0].mirostat_state()[0] != 10.0 and members[2].mirostat_state() == (0.0, 0)
    assert batch.captures() == 1
    batch.close()
    for d in members[::-1] + twins:
        d.close()


def test_prefill_packed_and_step_wide_draw_with_the_members_own_sampler(hip, pkg, world):
    W = world
    owner = W.decoder(pkg)
    ms = [owner, owner.shared(), owner.shared(), owner.shared()]
    plans = [(5.0, 0.1, 71), None, (0.5, 0.1, 72), (8.0, 0.25, 73)]
    refs = [switch_on(m, *p) if p else None for m, p in zip(ms, plans)]
    gens = [[] for _ in ms]
    ns = [33, 20, 64, 40]
    for i, (m, n) in enumerate(zip(ms, ns)):
        m.reset()
        m.feed(W.prompt[7 * i:7 * i + n])

    def judged_all(step, what):
        """one call for every member; each Mirostat member judged on its own logits"""
        before = [(m.mirostat_state(), m.sampling_draws()) if r else None for m, r in zip(ms, refs)]
        step()
        for i, (m, ref) in enumerate(zip(ms, refs)):
            p = m.position()
            tok = int(m.history(p + 1)[p])
            if ref is None:
                assert tok == int(np.argmax(m.last_logits())) and m.mirostat_state() == (0.0, 0), (what, i)
                continue
            (mu_b, fb_b), d_b = before[i]
            (mu_a, fb_a), d_a = m.mirostat_state(), m.sampling_draws()
            ref.rng.draws = d_b
            ref.sample(m.last_logits(), gens[i], mu=F(mu_b))
            v = ma.judge(ref.last, ma.u_of(ref.rng, d_b), tok, F(mu_a), d_a - d_b)
            assert v["ok"], (what, i, v["reason"])
            assert fb_a - fb_b == (1 if v["mode"] == "fallback" else 0), (what, i)
            gens[i].append(tok)

    judged_all(lambda: owner.prefill_packed(ms, ns, with_logits=True, digits=2), "prefill_packed")
    for step in range(3):
        judged_all(lambda: owner.step_wide(ms, 1, digits=2), ("step_wide", step))
    for i in (0, 2, 3):  # four picks each: a draw (one word) or a fallback (none)
        assert ms[i].sampling_draws() + ms[i].mirostat_state()[1] == 4, i
    for m in ms[::-1]:
        m.close()
