"""GPU: the wide step's tail tables on raw buffers, no decoder -- bitnet_hip_sample_batch_create_wide (k_sample_batch at up to 64 slots) against
TWIN samplers that take the same logits through bitnet_hip_sample_dev one by one, and bitnet_hip_logprob_rows_dev (k_logprob_batch at up to
64 entries) against bitnet_hip_logprob_dev per entry.

The criterion is equality, as in tests/test_sample_batch_gpu.py and tests/test_logprob_gpu.py, whose lanes, entries, guard words and
comparisons are imported, not restated: one kernel body serves the single launch and the table, so per slot the token, the history entry and
the position must be the twin's call after call, and the draws, the chosen count, Mirostat's mu and the grammar state at the end; a tap
entry's record bytes and re-armed scratch must be the single launch's.  No tolerance is involved.

Shapes: 9 / 33 / 64 slots (past the 8-slot table, an odd middle, the full width) at vocabularies 1000 and 2500 (1 and 3 workgroups per slot,
the last slice ragged), and 64 slots once at 128256: the real 64 x 64 grid, which is not co-resident -- a workgroup that waited for another
would hang there."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_logprob_gpu import SENTINEL, Entry, rows, table_of  # noqa: E402
from test_sample_batch_gpu import assert_equal, feed, pair, torch_  # noqa: E402,F401

pytestmark = pytest.mark.gpu

CALLS = 8
# slot i runs configuration i mod 8; `base` is the index into test_sample_batch_gpu.CONFIGS that pair() starts the lane from
KINDS = ["greedy with penalty", "S", "F", "top_k 1", "min-p + typical-p", "mirostat", "constraints with a ban list", "grammar"]
BASE = [0, 1, 2, 3, 2, 2, 1, 1]
_grammars = {}


def grammar_of(hip, vocab):
    """one token automaton per vocabulary: the trie of three words over a synthetic byte table, EOS = the last id; shared by every lane"""
    if vocab not in _grammars:
        G = importlib.import_module("bitnet-rs_amd.grammar")
        alpha = b"yesnomab"
        table = [bytes([t]) if t < 256 else bytes([alpha[t % 8], alpha[(t // 8) % 8]]) for t in range(vocab)]
        tc, nx, start = G.token_automaton(G.ByteDFA.from_choices([b"yes", b"no", b"maybe"]), table, vocab - 1)
        _grammars[vocab] = (hip.grammar(tc, nx), start)
    return _grammars[vocab]


def lanes(torch, hip, vocab, slot):
    """the member's lane and its twin's for `slot`, both on configuration slot mod 8, the same seed"""
    kind = slot % 8
    m, t = pair(torch, hip, vocab, 5 * slot + BASE[kind], pos0=slot % 16)  # (5 * slot + base) mod 5 = base; a seed of its own per slot
    for l in (m, t):
        if kind == 4:
            l.smp.configure(0.8, 0, 1.0, 1.1, seed=900 + slot, min_p=0.05, typical_p=0.9)
        elif kind == 5:
            l.smp.configure(0.7, 0, 1.0, 1.1, seed=900 + slot)  # Mirostat replaces the truncation stages: they are off
            l.smp.set_mirostat(5.0, 0.1)
        elif kind == 6:
            banned = {int(x): -np.inf for x in np.random.default_rng(slot).choice(vocab, 17, replace=False)}
            l.smp.set_constraints(bias=banned)
        elif kind == 7:
            g, start = grammar_of(hip, vocab)
            l.smp.set_grammar(g, start)
    return m, t


def end_state(l):
    return (l.smp.draws(), l.smp.chosen(), np.float32(l.smp.mirostat_state()[0]).tobytes(), l.smp.mirostat_state()[1], l.smp.grammar_state())


def close_all(table, pairs):
    table.close()
    for m, t in pairs.values():
        for l in (m, t):
            l.smp.set_grammar(None)
            l.close()


def run_case(torch, hip, vocab, n_slots, empty):
    rng = np.random.default_rng(1000 * n_slots + vocab)
    pairs = {b: lanes(torch, hip, vocab, b) for b in range(n_slots) if b not in empty}
    table = hip.sample_batch(vocab, n_slots, wide=True)
    for b, (m, _) in pairs.items():
        m.bind(table, b)
    tokens = set()
    for call in range(CALLS):
        for p in pairs.values():
            feed(rng, p)
        table.launch()  # ONE launch, grid (workgroups per slot, n_slots)
        for _, t in pairs.values():
            t.alone()
        torch.cuda.synchronize()
        for b, (m, t) in pairs.items():
            assert_equal(m, t, (vocab, n_slots, KINDS[b % 8], "call", call, "slot", b))
            w = m.words()
            assert w["pos"] == b % 16 + call + 1 and w["hist"][w["pos"]] == w["tok"] and 0 <= w["tok"] < vocab
            tokens.add(w["tok"])
    for b, (m, t) in pairs.items():
        assert end_state(m) == end_state(t), (vocab, n_slots, KINDS[b % 8], "slot", b, end_state(m), end_state(t))
    seen = {b % 8 for b in pairs}
    assert (seen == set(range(8)) or n_slots < 16) and len(seen) >= 7 and len(tokens) > 8  # (9 slots with one empty in the middle: seven of the eight)
    for b, (m, _) in pairs.items():  # every stage was live: a draw count, a chosen count, a moved mu, a walked grammar
        kind, (draws, chosen, _, _, gr) = b % 8, end_state(m)
        assert (draws == 0) == (kind == 0), (b, draws)
        assert (kind != 6 or chosen == CALLS) and (kind in (6, 7) or chosen == 0) and (gr[1] == CALLS) == (kind == 7), (b, chosen, gr)
    close_all(table, pairs)


@pytest.mark.parametrize("n_slots", [9, 33, 64])
@pytest.mark.parametrize("vocab", [1000, 2500])
def test_every_slot_equals_its_twin_over_eight_calls(hip, torch_, vocab, n_slots):
    """empty entries in the middle (slot 4) and at the end (the last slot): their workgroups return before the first barrier"""
    run_case(torch_, hip, vocab, n_slots, empty={4, n_slots - 1})


def test_the_full_grid_at_the_real_vocabulary(hip, torch_):
    """64 slots x 64 workgroups of 128256 / 64 entries: more workgroups than the chip holds at once"""
    run_case(torch_, hip, 128256, 64, empty=set())


def test_a_slot_emptied_and_bound_again_continues(hip, torch_):
    """33 slots; slot 21 (a Mirostat lane) is emptied after three calls and bound again after five: while it is empty none of its words, logits
    or guard words changes and its sampler state stays; afterwards it continues as a twin that skipped those two calls"""
    torch, vocab, n_slots, gone = torch_, 2500, 33, 21
    rng = np.random.default_rng(33)
    pairs = {b: lanes(torch, hip, vocab, b) for b in range(n_slots)}
    table = hip.sample_batch(vocab, n_slots, wide=True)
    for b, (m, _) in pairs.items():
        m.bind(table, b)
    for call in range(CALLS):
        away = 3 <= call < 5
        if call == 3:
            table.set(gone, None)
        if call == 5:
            pairs[gone][0].bind(table, gone)
        for p in pairs.values():
            feed(rng, p)
        mg = pairs[gone][0]
        before = (mg.arena.clone(), mg.larena.view(torch.int32).clone(), end_state(mg)) if away else None
        table.launch()
        for b, (_, t) in pairs.items():
            if not (away and b == gone):
                t.alone()
        torch.cuda.synchronize()
        for b, (m, t) in pairs.items():
            assert_equal(m, t, ("call", call, "slot", b))
        if away:
            assert torch.equal(mg.arena, before[0]) and torch.equal(mg.larena.view(torch.int32), before[1]) and end_state(mg) == before[2]
    for b, (m, t) in pairs.items():
        assert end_state(m) == end_state(t), b
    assert pairs[gone][0].words()["pos"] == gone % 16 + CALLS - 2 and pairs[0][0].words()["pos"] == CALLS
    with pytest.raises(Exception, match="slot 33 out of range"):
        pairs[0][0].bind(table, 33)
    close_all(table, pairs)


@pytest.mark.parametrize("n_slots", [9, 33, 64])
def test_tap_table_equals_single_launches(pkg, hip, n_slots):
    """logprob_rows_dev at top_n 0 / 5 / 20 against logprob_dev per entry: the record bytes (guards included) and the re-armed scratch are
    equal; empty entries in the middle and at the end are untouched"""
    import torch

    V = 2500 if n_slots < 64 else 128256  # 3 workgroups per entry, and once the real vocabulary's grid at the full width
    R = rows(V)
    names = list(R)
    rng = np.random.default_rng(V + n_slots)
    tops = [0, 5, 20]
    empty = {3, n_slots - 1}
    singles, batch = [Entry(pkg, hip, V) for _ in range(n_slots)], [Entry(pkg, hip, V) for _ in range(n_slots)]
    for b in range(n_slots):
        row, token, q = R[names[b % len(names)]], int(rng.integers(0, V)), int(rng.integers(0, 4))
        singles[b].set(row, token, q)
        batch[b].set(row, token, q)
        if b not in empty:
            singles[b].launch(tops[b % 3])
    table = table_of(torch, [batch[b].args(tops[b % 3], empty=b in empty) for b in range(n_slots)])
    hip.logprob_rows_dev(table, n_slots, V)
    torch.cuda.synchronize()
    for b in range(n_slots):
        got, want = batch[b].records.cpu().numpy(), singles[b].records.cpu().numpy()
        assert np.array_equal(got, want), (V, n_slots, "slot", b, "records")
        assert np.array_equal(batch[b].scratch.cpu().numpy(), singles[b].scratch.cpu().numpy()), (V, n_slots, "slot", b, "scratch")
        if b in empty:
            assert (got == SENTINEL).all() and not batch[b].scratch.any()  # an empty entry: nothing read or written
        else:
            assert (got[176:-176] != SENTINEL).any()
    with pytest.raises(pkg.BitNetHipError, match="n_slots"):
        hip.logprob_rows_dev(table, 65, V)
