"""GPU: the stop criteria in a batch (BatchDecoder's stop table, host/batch_decoder.hpp) and in the wide step and the packed prompt forward
(Decoder::step_wide / prefill_packed, host/decoder.hpp).

HostBatch: a member's twin runs alone under set_attention_form(0), which a batch step reproduces bit for bit; tests/stop_ref.py applied to the
twin's history names the step at which criteria chosen from it must stop the member.  Three members stop at different steps, one has no
criteria, one slot is idle.  step_wide: the baseline is a second group that takes the same wide steps without criteria (a wide step is not
bit-equal to run(); the rows of one step are independent of each other, so a frozen neighbour changes nothing).  Integers and bits only."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stop_ref as R  # noqa: E402
from test_stop_decoder_gpu import CFG_S, MODEL_A, NP, bits, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu

NG = 16


def prompt_of(cfg, i):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    return np.roll(np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32), -7 * i)[:NP + i]


def member(world, i, sampling=False, form0=False):
    cfg, owner, _ = world
    d = owner.shared()
    d.reset()
    if form0:
        d.set_attention_form(0)
    if sampling:
        d.set_sampling(*CFG_S, seed=100 + i)
    p = prompt_of(cfg, i)
    d.feed(p)
    d.run(len(p) - 1, with_logits=False)
    return d, len(p)


def test_host_batch_members_stop_at_their_own_steps(pkg, world):
    cfg = world[0]
    hists, lens = [], []
    for i in range(4):
        t, n = member(world, i, sampling=(i == 1), form0=True)
        t.run(NG)
        hists.append(t.history(n + NG))
        lens.append(n)
        t.close()
    g = [[int(x) for x in h[n:]] for h, n in zip(hists, lens)]
    crits = [R.Config(max_tokens=3), R.Config(eos=g[1][8]), R.Config(sequences=(tuple(g[2][10:13]),)), None]
    want = [R.first_stop(c, h, n, NG) if c else (None, None) for c, h, n in zip(crits, hists, lens)]
    ks = [k for k, _ in want[:3]]
    assert all(k is not None for k in ks) and ks[0] == 3 and ks[2] <= 13
    ms = [member(world, i, sampling=(i == 1), form0=True)[0] for i in range(4)]  # (form 0 for the solo prompt steps too: the batch's form)
    for m, c in zip(ms, crits):
        if c:
            m.set_stop(**c.kwargs())
    b = pkg.HostBatch(5)
    assert b.live() == 0
    for slot, m in zip((0, 1, 2, 4), ms):  # slot 3 stays idle
        b.set_slot(slot, m)
    assert b.live() == 3
    b.step(2)
    nodes = b.graph_nodes()
    assert b.live() == sum(k > 2 for k in ks)
    steps, _ = b.step_until(NG - 2, 3)
    total = 2 + steps
    print(f"stop steps {ks}, {total} steps queued, {nodes} kernel nodes")
    assert b.live() == 0 and total == min(2 + -(-(max(ks) - 2) // 3) * 3, NG) and total >= max(ks)
    for i, (m, (k, w)) in enumerate(zip(ms, want)):
        if k is None:  # the member without criteria equals its solo run
            assert m.position() == lens[i] - 1 + total and np.array_equal(m.history(lens[i] + total), hists[i][:lens[i] + total]), i
            continue
        st = m.stop_state()
        assert st.astuple() == w.public()[:5] + (total - k,), (i, st, w)
        assert m.position() == w.position and np.array_equal(m.history(w.position + 1), hists[i][:w.position + 1]), i
    # resumed, the members go on to their twins' histories (the batch recounts its live members when one is armed again)
    ms[2].resume()
    assert b.live() == 1
    ms[2].set_stop(off=True)
    ms[0].set_stop(off=True)
    ms[1].set_stop(off=True)
    assert b.live() == 0
    with pytest.raises(pkg.BitNetHipError, match="needs a member with stop criteria"):
        b.step_until(4, 2)
    b.step(NG - max(ks))
    assert np.array_equal(ms[2].history(lens[2] + ks[2] + NG - max(ks)), hists[2][:lens[2] + ks[2] + NG - max(ks)])
    assert b.graph_nodes() == nodes  # once in the chain the launch stays, as the sampling launch does: nothing is re-captured
    for slot in (0, 1, 2, 4):
        b.set_slot(slot, None)
    b.close()
    for m in ms:
        m.close()


def test_wide_step_and_packed_prefill_hold_stopped_members(pkg, world):
    cfg = world[0]

    def group():
        ms = []
        for i in range(4):
            d = world[1].shared()
            d.reset()
            if i >= 2:
                d.set_sampling(*CFG_S, seed=200 + i)
            d.feed(prompt_of(cfg, i))
            ms.append(d)
        return ms

    lens = [NP + i for i in range(4)]
    base = group()
    base[0].prefill_packed(base, lens, with_logits=True, digits=2)  # every member's first token sits at slot len
    draws = [[m.sampling_draws() for m in base]]
    for _ in range(NG):
        base[0].step_wide(base, 1, digits=2)
        draws.append([m.sampling_draws() for m in base])
    hists = [m.history(n + NG + 1) for m, n in zip(base, lens)]
    g = [[int(x) for x in h[n:]] for h, n in zip(hists, lens)]
    # member 0: EOS = its very first token (placed by the packed prompt forward); 1: a budget; 2 (samples): a stop id; 3 (samples): none
    crits = [R.Config(eos=g[0][0]), R.Config(max_tokens=6), R.Config(stop_ids=(9999, g[2][5])), None]
    ms = group()
    for m, c in zip(ms, crits):
        if c:
            m.set_stop(**c.kwargs())
    ms[0].prefill_packed(ms, lens, with_logits=True, digits=2)
    assert ms[0].stop_state().astuple() == (R.EOS, 0, g[0][0], lens[0], 1, 0)
    assert ms[1].stop_state().astuple() == (R.NONE, 0, 0, 0, 1, 0)
    ms[0].step_wide(ms, NG, digits=2)
    for i, (m, c) in enumerate(zip(ms, crits)):
        if c is None:
            assert np.array_equal(m.history(lens[i] + NG + 1), hists[i]) and m.sampling_draws() == draws[NG][i], i
            continue
        # the packed forward placed generated token 1 (step 1 of the restatement); wide step s places token s + 1
        k, w = R.first_stop(c, hists[i], lens[i], NG + 1)
        st = m.stop_state()
        assert k is not None and st.astuple() == w.public()[:5] + (NG + 1 - k,), (i, st, w)
        assert m.position() == w.position and np.array_equal(m.history(w.position + 1), hists[i][:w.position + 1]), i
        assert m.sampling_draws() == draws[k - 1][i], (i, m.sampling_draws(), draws[k - 1][i])
    for m in ms + base:
        m.close()
