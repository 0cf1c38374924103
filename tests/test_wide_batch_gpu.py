"""GPU: WideBatch (host/wide_batch.hpp) -- up to 64 decoders held in slots and stepped through the wide forward with at most one sampling, one
tap and one stop launch per step -- against TWIN decoders driven by Decoder::step_wide over the same dense member list with the same calls.

The criterion is equality, without a tolerance and without an excluded member: after every call each member's position, history, last_logits
bits and cache slots (tests/test_batch_decoder_gpu.py: state, assert_same), the bytes of its whole caches (tests/test_decoder_state_gpu.py:
snapshot, same_bytes), its log-probability records, its stop state and its sampler state (draws, chosen, Mirostat's mu and fallbacks, the
grammar state) are the twin's.  step_wide itself is held to the float64 forward by tests/test_step_wide_gpu.py, whose POSITIONS and prepare()
fill the members here too.

POSITIONS[7] = 297 sits two slots from the cache's end (max_pos 300): the calls step(1), step(1), step(2) take four slots, so that member runs
the first two calls -- to position 299, the last that exists -- and leaves its slot before the third, which it could only refuse; the twins'
list follows.  Every other member runs all four steps."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_batch_decoder_gpu import assert_same, state  # noqa: E402
from test_decoder_state_gpu import case_id, same_bytes, snapshot, worlds  # noqa: E402,F401
from test_grammar_decoder_gpu import cyclic_grammar  # noqa: E402
from test_prefill_packed_gpu import close, group, tokens_of  # noqa: E402
from test_step_wide_gpu import POSITIONS, prepare  # noqa: E402

pytestmark = pytest.mark.gpu

TWIN_CASES = [(("A", f, k), m) for f in ("i2s", "qk256") for k in (False, True) for m in (5, 17)] + [(("A", "qk256", False), 64)]


@pytest.fixture(scope="module")
def gram(hip, worlds):
    """(yes,|no,)* for ever over the toy byte table of tests/test_grammar_decoder_gpu.py: a grammar member never runs out of allowed tokens"""
    G = importlib.import_module("bitnet-rs_amd.grammar")
    desc, start, _ = cyclic_grammar(G, worlds("A", "qk256").cfg.vocab)
    g = hip.grammar(*desc)
    yield g, start
    g.close()


def configure(m, i, gram, everything=False):
    """member i's sampler by i mod 8, its tap on every third member, stop criteria on every third (budget 2: ends inside the run; 40: does not);
    everything: a drawing sampler, the tap and criteria that never fire on every member"""
    k = i % 8
    if everything:
        m.set_sampling(0.9, 40, 0.95, 1.1, seed=50 + i)
    elif k == 1:
        m.set_sampling(0.0, seed=1)  # greedy under a grammar
        m.set_grammar(*gram)
    elif k == 2:
        m.set_sampling(0.9, 40, 0.95, 1.1, seed=50 + i)  # top-k / top-p draws
    elif k == 3:
        m.set_sampling(0.7, 0, 1.0, 1.1, seed=50 + i)
        m.set_mirostat(4.0, 0.1)
    elif k == 4:
        m.set_sampling(0.8, 0, 0.9, 1.1, seed=50 + i)
        m.set_constraints(bias={int(t): -np.inf for t in range(3 * i, 3 * i + 40)}, no_repeat_ngram=2)
    elif k == 5:
        m.set_sampling(0.0, 0, 1.0, 1.3, seed=3)  # temperature 0 with a repetition penalty: no draw
    elif k == 7:
        m.set_sampling(0.8, 1, 0.9, 1.1, seed=50 + i)
    o = dict(tap=everything or i % 3 == 0, stop=everything or i % 3 == 1)
    if o["tap"]:
        m.set_logprobs(5)
    if o["stop"]:
        m.set_stop(stop_ids=() if everything else (2047,), max_tokens=1000 if everything else 2 if i % 2 else 40)
    return o


def full(m, W, kv16, o):
    mu, fb = m.mirostat_state()
    return (state(m, W.cfg, kv16), snapshot(m, W, kv16), m.logprob_records(0, W.cfg.max_pos).tobytes() if o["tap"] else None,
            m.stop_state().astuple() if o["stop"] else None, (m.sampling_draws(), m.chosen(), np.float32(mu).tobytes(), fb, m.grammar_state()))


def assert_full(a, b, what):
    assert_same(a[0], b[0], what)
    assert same_bytes(a[1], b[1]), (what, "cache snapshot bytes")
    assert a[2] == b[2], (what, "logprob records")
    assert a[3] == b[3], (what, "stop state", a[3], b[3])
    assert a[4] == b[4], (what, "sampler state", a[4], b[4])


def two_groups(pkg, W, kv16, n, gram, pos, everything=False, extra=0):
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms, twins = group(pkg, W, kv16, n + extra), group(pkg, W, kv16, n + extra)
    opts = [configure(m, i, gram, everything) for i, m in enumerate(ms)]
    for i, t in enumerate(twins):
        configure(t, i, gram, everything)
    prepare(ms[:n], forced, pos)
    prepare(twins[:n], forced, pos)
    return ms, twins, opts


def compare(ms, twins, opts, W, kv16, idx, what):
    for i in idx:
        assert_full(full(ms[i], W, kv16, opts[i]), full(twins[i], W, kv16, opts[i]), (what, "member", i))


def slots_of(batch, ms, slots):
    for i, b in enumerate(slots):
        batch.set_slot(b, ms[i])


@pytest.mark.parametrize("case,M", TWIN_CASES, ids=lambda x: str(x) if isinstance(x, int) else case_id(x))
def test_every_member_equals_its_twin_under_step_wide(pkg, hip, worlds, gram, case, M):
    model, fmt, kv16 = case
    W, pos = worlds(model, fmt), POSITIONS[:M]
    ms, twins, opts = two_groups(pkg, W, kv16, M, gram, pos)
    # the slots: a hole in the middle and a spare at the end while there is room, the dense list in member order either way
    slots = list(range(M)) if M == 64 else [i if i < M // 2 else i + 1 for i in range(M)]
    batch = pkg.HostWideBatch(64 if M == 64 else M + 2)
    slots_of(batch, ms, slots)
    inside = list(range(M))
    for call, n in enumerate((1, 1, 2)):
        for i in list(inside):
            if pos[i] + sum((1, 1, 2)[:call]) + n > W.cfg.max_pos - 1:  # the member at the cache's end leaves before the call it could only refuse
                batch.set_slot(slots[i], None)
                inside.remove(i)
        batch.step(n, digits=2)
        lst = [twins[i] for i in inside]
        lst[0].step_wide(lst, n, digits=2)
        kinds = (lambda i: i % 8 not in (0, 6), lambda i: opts[i]["tap"], lambda i: opts[i]["stop"])
        assert batch.tail_launches() == tuple(n * int(any(f(i) for i in inside)) for f in kinds)  # one launch per kind per step, whoever is in
        compare(ms, twins, opts, W, kv16, range(M), (case, M, "call", call))
    for i in range(M):
        assert ms[i].position() == min(pos[i] + 4, W.cfg.max_pos - 1) or opts[i]["stop"], i
    stopped = [i for i in range(M) if opts[i]["stop"] and ms[i].stop_state().stopped]
    live = [i for i in inside if opts[i]["stop"] and i not in stopped]
    assert batch.live() == len(live)
    if M >= 17:
        assert stopped and live, "budgets that end inside the run and budgets that do not"
    batch.close()
    close(ms)
    close(twins)


def test_an_owner_of_the_other_cache_type_outside_the_batch(pkg, hip, worlds, gram):
    """the forward is driven on the weights' owner, member or not: here the owner keeps f32 caches and sits in no slot, its five borrowers hold
    f16 caches -- the attention must read the MEMBERS' type.  The twins' step_wide is driven by a borrower, as it always is."""
    W, pos = worlds("A", "qk256"), POSITIONS[:5]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    owners, sets = [], []
    for _ in range(2):
        owner = W.decoder(pkg, False)
        ms = [owner.shared() for _ in range(5)]
        for m in ms:
            m.set_kv_f16(True)
        owners.append(owner)
        sets.append(ms)
    ms, twins = sets
    opts = [configure(m, i + 1, gram) for i, m in enumerate(ms)]
    for i, t in enumerate(twins):
        configure(t, i + 1, gram)
    prepare(ms, forced, pos)
    prepare(twins, forced, pos)
    batch = pkg.HostWideBatch(5)
    slots_of(batch, ms, range(5))
    for n in (1, 2):
        batch.step(n, digits=2)
        twins[0].step_wide(twins, n, digits=2)
        compare(ms, twins, opts, W, True, range(5), ("f32 owner outside, f16 members", n))
    assert owners[0].position() == 0 and ms[4].position() == pos[4] + 3
    batch.close()
    close(ms + twins)
    close(owners)


def test_launch_counts_and_table_writes(pkg, hip, worlds, gram):
    W, M = worlds("A", "qk256"), 64
    pos = [(37 * i) % 200 + 2 for i in range(M)]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms = group(pkg, W, False, M + 1)
    # ---- all greedy: no tail launch at all ----
    prepare(ms[:M], forced, pos)
    batch = pkg.HostWideBatch(64)
    slots_of(batch, ms[:M], range(M))
    assert batch.table_writes() == 0
    batch.step(2)
    assert batch.tail_launches() == (0, 0, 0) and batch.table_writes() == 1  # the pointer tables, once
    # ---- every member sampling, tapped and with criteria: one launch of each kind per step ----
    for i, m in enumerate(ms):
        configure(m, i, gram, everything=True)
    batch.step(1)
    assert batch.tail_launches() == (1, 1, 1)
    w = batch.table_writes()
    assert w > 1
    batch.step(3)
    assert batch.tail_launches() == (3, 3, 3)
    for _ in range(2):
        batch.step(1)
        assert batch.tail_launches() == (1, 1, 1)
    assert batch.table_writes() == w, "three calls with nothing changed upload nothing"
    assert all(m.sampling_draws() == 6 for m in ms[:M]) and batch.live() == M
    # ---- a member switches sampling off; one leaves; one joins ----
    ms[5].set_sampling(None)
    batch.step(1)
    w1 = batch.table_writes()
    assert w1 > w and batch.tail_launches() == (1, 1, 1) and ms[5].sampling_draws() == 6
    batch.set_slot(9, None)
    batch.step(1)
    w2 = batch.table_writes()
    assert w2 > w1 and ms[9].position() == pos[9] + 9 and ms[10].position() == pos[10] + 10
    ms[M].reset()
    ms[M].feed(tokens_of(W, 3, 2))
    ms[M].prefill(1, with_logits=False, digits=2)
    batch.set_slot(9, ms[M])
    batch.step(1)
    w3 = batch.table_writes()
    assert w3 > w2 and ms[M].position() == 2 and ms[M].sampling_draws() == 1
    batch.step(1)
    assert batch.table_writes() == w3 and batch.tail_launches() == (1, 1, 1)
    batch.close()
    close(ms)


@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
def test_slots_move_between_steps(pkg, hip, worlds, gram, kv16):
    """a member leaves, another joins at another position, a hole stays in the middle, a member is swapped for a twin of another sequence: the
    twins' step_wide lists follow the occupied slots in slot order"""
    W, n = worlds("A", "i2s"), 9
    pos = POSITIONS[:7] + [200, 100]
    ms, twins, opts = two_groups(pkg, W, kv16, n, gram, pos)
    batch = pkg.HostWideBatch(12)
    where = {b: b for b in range(6)}  # slot -> member; members 6, 7, 8 wait outside
    slots_of(batch, ms[:6], range(6))

    def both(k, what):
        batch.step(k, digits=2)
        lst = [twins[where[b]] for b in sorted(where)]
        lst[0].step_wide(lst, k, digits=2)
        seen.update(where.values())  # (a member that has not run a step yet has no last_logits to compare: unwritten memory)
        compare(ms, twins, opts, W, kv16, sorted(seen), what)

    seen = set()
    both(1, "six members")
    batch.set_slot(0, None)  # the lowest slot empties: the driver is the owner all the same, and it is no member now
    del where[0]
    both(1, "the owner left")
    batch.set_slot(10, ms[6])  # another joins at another position, behind a hole
    where[10] = 6
    batch.set_slot(3, None)  # a hole in the middle
    del where[3]
    both(2, "a join behind a hole, a hole in the middle")
    batch.set_slot(4, ms[7])  # a member swapped for another sequence's decoder
    where[4] = 7
    batch.set_slot(0, ms[8])
    where[0] = 8
    both(1, "a swap and a join into the lowest slot")
    batch.set_slot(3, ms[4])  # the swapped-out member comes back into the hole
    where[3] = 4
    both(1, "a return")
    steps = [1, 6, 6, 2, 5, 6, 4, 2, 2]  # (members 1 and 7 carry a budget of 2: they stop there and stay frozen)
    assert [ms[i].position() - pos[i] for i in range(n)] == [2 if i in (1, 7) else k for i, k in enumerate(steps)]
    batch.close()
    close(ms)
    close(twins)


def test_step_until_parks_the_stopped(pkg, hip, worlds, gram):
    W, kv16, pos = worlds("A", "qk256"), False, [33, 64, 130, 65]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms, twins = group(pkg, W, kv16, 4), group(pkg, W, kv16, 4)
    opts = [dict(tap=i == 3, stop=i < 3) for i in range(4)]
    for g in (ms, twins):
        for m, budget in zip(g, (2, 5, 9)):
            m.set_stop(stop_ids=(2047,), max_tokens=budget)
        g[1].set_sampling(0.9, 40, 0.95, 1.1, seed=8)
        g[3].set_logprobs(5)  # the member without criteria runs every queued step
        prepare(g, forced, pos)
    lone = pkg.HostWideBatch(2)
    lone.set_slot(1, ms[3])
    with pytest.raises(pkg.BitNetHipError, match="criteria"):
        lone.step_until(16, chunk=4)
    lone.close()
    batch = pkg.HostWideBatch(4)
    slots_of(batch, ms, range(4))
    steps, _ = batch.step_until(16, chunk=4, digits=2)
    # the stated procedure on the twins: step_wide of the un-parked list per chunk, the stop states read between chunks
    parked, queued = set(), 0
    while queued < 16 and any(i not in parked for i in range(3)):
        lst = [t for i, t in enumerate(twins) if i not in parked]
        lst[0].step_wide(lst, 4, digits=2)
        queued += 4
        parked |= {i for i in range(3) if twins[i].stop_state().stopped}
    assert steps == queued == 12 and parked == {0, 1, 2}
    compare(ms, twins, opts, W, kv16, range(4), "step_until(16, chunk 4)")
    assert [m.stop_state().generated for m in ms[:3]] == [2, 5, 9] and ms[3].position() == pos[3] + 12
    assert [ms[i].position() for i in range(3)] == [pos[i] + b for i, b in enumerate((2, 5, 9))]  # a twin parked after chunk k was never stepped again
    assert batch.live() == 0 and batch.tail_launches()[2] == 4
    # parked members stay out of a plain step too, even re-armed ...
    for g in (ms, twins):
        g[0].set_stop(stop_ids=(2047,), max_tokens=20)
    before = full(ms[0], W, kv16, opts[0])
    batch.step(1)
    twins[3].step_wide([twins[3]], 1, digits=2)
    assert_full(full(ms[0], W, kv16, opts[0]), before, "a parked member through a later step")
    # ... until set_slot clears the mark
    batch.set_slot(0, ms[0])
    batch.step(1)
    twins[0].step_wide([twins[0], twins[3]], 1, digits=2)
    compare(ms, twins, opts, W, kv16, range(4), "un-parked by set_slot")
    assert ms[0].position() == pos[0] + 3 and batch.live() == 1
    batch.close()
    close(ms)
    close(twins)


def test_admission_recipe(pkg, hip, worlds, gram):
    """four newcomers with prompts of 1, 2, 65 and 130 tokens join a running batch of five: feed, ONE prefill_packed of n - 1 tokens without
    logits (the one-token prompt is fed only), set_slot; the next wide step consumes the last prompt token and picks the first generated one"""
    W, kv16, pos, prompts = worlds("A", "qk256"), False, POSITIONS[:5], [1, 2, 65, 130]
    ms, twins, opts = two_groups(pkg, W, kv16, 5, gram, pos, extra=4)
    batch = pkg.HostWideBatch(16)
    slots_of(batch, ms[:5], range(5))
    batch.step(1)
    twins[0].step_wide(twins[:5], 1, digits=2)
    for g in (ms, twins):
        new = g[5:]
        for j, (m, n) in enumerate(zip(new, prompts)):
            m.reset()
            m.feed(tokens_of(W, 5 + j, n))
        packed = [(m, n - 1) for m, n in zip(new, prompts) if n > 1]
        packed[0][0].prefill_packed([m for m, _ in packed], [n for _, n in packed], with_logits=False, digits=2)
    for j in range(4):
        batch.set_slot(8 + j, ms[5 + j])
    batch.step(1)
    twins[0].step_wide(twins, 1, digits=2)
    for j, n in enumerate(prompts):
        m, t = ms[5 + j], twins[5 + j]
        assert m.position() == n and int(m.history(n + 1)[n]) == int(t.history(n + 1)[n]), ("the first generated token of newcomer", j)
        assert np.array_equal(m.history(n), tokens_of(W, 5 + j, n))
    compare(ms, twins, opts, W, kv16, range(9), "the step the newcomers joined")
    batch.step(2)
    twins[0].step_wide(twins, 2, digits=2)
    compare(ms, twins, opts, W, kv16, range(9), "two more steps")
    batch.close()
    close(ms)
    close(twins)


def test_refusals_leave_every_member_and_the_batch_untouched(pkg, hip, worlds, gram):
    W = worlds("A", "qk256")
    cfg = W.cfg
    ms = group(pkg, W, False, 3)
    opts = [configure(m, i + 1, gram) for i, m in enumerate(ms)]  # a grammar member, a drawing one, Mirostat; a stop, a tap
    stranger = W.decoder(pkg, False)  # other weights (another owner)
    half = ms[0].shared()
    half.set_kv_f16(True)
    everyone = ms + [stranger, half]
    for i, m in enumerate(everyone):
        m.reset()
        m.feed(tokens_of(W, i, 40))
        m.prefill(20, with_logits=True, digits=2)
    allopts = opts + [dict(tap=False, stop=False)] * 2
    batch = pkg.HostWideBatch(8)
    slots_of(batch, ms, (0, 2, 5))
    batch.step(1)

    def snap_all():
        return [full(m, W, m is half, o) for m, o in zip(everyone, allopts)], batch.table_writes(), batch.tail_launches()

    before = snap_all()

    def refused(call, match):
        with pytest.raises(pkg.BitNetHipError, match=match) as e:
            call()
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT, match
        now = snap_all()
        for a, b in zip(before[0], now[0]):
            assert_full(a, b, match)
        assert now[1:] == before[1:], (match, "the batch's tables and counters")

    refused(lambda: batch.step(0), "n_steps")
    refused(lambda: batch.step(-3), "n_steps")
    refused(lambda: batch.step(cfg.max_pos - 21), "KV cache overflow")  # 21 + 279 > max_pos - 1
    refused(lambda: batch.step(2 ** 31 - 1), "KV cache overflow")
    refused(lambda: batch.set_slot(1, stranger), "same weights")
    refused(lambda: batch.set_slot(1, half), "mixed KV cache types")
    refused(lambda: batch.set_slot(1, ms[2]), "repeated")
    refused(lambda: batch.set_slot(8, ms[2]), "out of range")
    dead = ms[0].shared()
    dead.close()
    refused(lambda: batch.set_slot(1, dead), "null member")
    batch.set_slot(2, ms[1])  # the same member into its own slot is no refusal, and changes nothing
    assert batch.table_writes() == before[1]
    # the cache's end: a member at position max_pos - 1 has no slot left
    long = ms[0].shared()
    long.reset()
    long.feed(tokens_of(W, 1, cfg.max_pos))
    long.prefill(cfg.max_pos - 2, with_logits=False, digits=2)
    batch.set_slot(7, long)
    batch.step(1)  # ... the last step that fits
    assert long.position() == cfg.max_pos - 1
    everyone.append(long)
    allopts.append(dict(tap=False, stop=False))
    before = snap_all()
    refused(lambda: batch.step(1), "KV cache overflow")
    batch.set_slot(7, None)
    batch.step(1)  # the batch goes on
    assert ms[1].position() == 23
    empty = pkg.HostWideBatch(3)
    with pytest.raises(pkg.BitNetHipError, match="empty"):
        empty.step(1)
    bare = pkg.HostDecoder(cfg)
    empty.set_slot(0, bare)
    with pytest.raises(pkg.BitNetHipError, match="model globals not set"):
        empty.step(1)
    empty.close()
    bare.close()
    batch.close()
    close([long, half, stranger])
    close(ms)
