"""GPU: Decoder::step_wide -- one decode step for up to 64 live sequences through ONE matrix forward (host/decoder.hpp) -- held to what each
member's own extend(1) is held to in tests/test_decoder_state_gpu.py, whose worlds, gates and helpers are imported, not restated: the KV cache
every member is left with against the float64 forward at rel <= 4 u_l (+ 2^-11 with an f16 cache), the slots the step did not own bit for
bit, the step's own logits and three decode steps at cosine >= 0.9999, the picked token against a twin's own extend(1) wherever the twin's two
best logits lie more than 2^-11 apart.  What a wide step adds is checked without a tolerance: the greedy pick is the first maximum of the
member's own logits, n steps in one call are n calls, members are isolated from each other and from their order, and after the step every
member carries on in a batch or alone exactly as a twin does.

Members are filled by ONE prefill_packed (a member at position 0 is fed only).  The member at position 297 sits two slots from the cache's end
(max_pos 300): the reference sequence of W.seq (three more tokens) and the three decode steps of `steps` do not fit behind it, so it is held
to the float64 forward over its 298 tokens directly -- position, untouched slots, cache values, the step's own logits, the pick -- and to the
one decode step that still fits."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_ref  # noqa: E402
import model_ref as mr  # noqa: E402
import sampler_ref as sr  # noqa: E402
from test_batch_decoder_gpu import assert_same, state  # noqa: E402
from test_decoder_state_gpu import CASES, STEPS, case_id, check_untouched, check_values, cosine, same_bytes, snapshot, steps, worlds  # noqa: E402,F401
from test_prefill_packed_gpu import close, group, tokens_of  # noqa: E402

pytestmark = pytest.mark.gpu

POSITIONS = [0, 1, 33, 63, 64, 65, 130, 297] + [(37 * i) % 290 + 2 for i in range(8, 64)]  # member i's position
WIDE_CASES = [(c, m) for c in CASES for m in (1, 9, 17)] + [(c, 64) for c in CASES if c[0] == "A"]


def positions_of(m):
    return [65] if m == 1 else POSITIONS[:m]  # (a single member at position 0 has nothing for prefill_packed to fill)


def prepare(ms, forced, pos, extra=0):
    """every member: reset, tokens [0, p + 1 + extra) fed, positions [0, p) filled by ONE prefill_packed over the members with p > 0"""
    for m, f, p in zip(ms, forced, pos):
        m.reset()
        m.feed(f[:p + 1 + extra])
    live = [(m, p) for m, p in zip(ms, pos) if p > 0]
    if live:
        live[0][0].prefill_packed([m for m, _ in live], [p for _, p in live], with_logits=False, digits=2)
    for m, p in zip(ms, pos):
        assert m.position() == p


@pytest.mark.parametrize("case,M", WIDE_CASES, ids=lambda x: str(x) if isinstance(x, int) else case_id(x))
def test_every_member_ends_as_its_own_extend_would_leave_it(pkg, hip, worlds, case, M):
    model, fmt, kv16 = case
    W, pos = worlds(model, fmt), positions_of(M)
    tail = [p + 1 + STEPS > W.cfg.max_pos - 1 for p in pos]  # no room for the reference's continuation behind the step
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    refs = []
    for f, t in zip(forced, tail):
        if t:
            ref = W.forward([int(x) for x in f])
            refs.append((f, ref, mr.yardstick(ref, W.forward([int(x) for x in f], rnd=mr.f16))))
        else:
            refs.append(W.seq(f))
    ms, twins = group(pkg, W, kv16, M), group(pkg, W, kv16, M)
    prepare(ms, forced, pos)
    prepare(twins, forced, pos)
    before = [snapshot(m, W, kv16) for m in ms]
    ms[0].step_wide(ms, 1, digits=2)
    assert ms[0].saturation_fallbacks() == 0
    undecided = []
    for i, (m, t, p) in enumerate(zip(ms, twins, pos)):
        what = f"wide step of {M} [{model} {fmt} kv16={kv16}] member {i} (p={p})"
        toks, ref, u = refs[i]
        assert m.position() == p + 1, what
        snap = snapshot(m, W, kv16)
        check_untouched(snap, before[i], p, p + 1, what)
        check_values(W, snap, ref, u, kv16, slice(0, p + 1), "wide", what)
        # the picked token: what the member's own extend(1) picks on a twin, wherever the twin's pick is decidable
        t.extend(1, with_logits=True, digits=2)
        assert t.position() == p + 1
        top = np.sort(t.last_logits())[-2:]
        if top[1] - top[0] > 2.0 ** -11 * abs(top[1]):
            assert np.array_equal(m.history(p + 2), t.history(p + 2)), what
        else:
            undecided.append(i)
            assert np.array_equal(m.history(p + 1), t.history(p + 1)), what
        if tail[i]:
            c = cosine(m.last_logits(), ref.logits[p])
            assert c >= 0.9999, (what, "the step's own logits", c)
            m.run(1, with_logits=True, use_graph=False)  # the one decode step that fits: position max_pos - 1
            assert m.position() == p + 2 and np.isfinite(m.last_logits()).all(), what
            check_untouched(snapshot(m, W, kv16), snap, p + 1, p + 2, what + ", the last decode step")
            continue
        m.feed(toks[p + 1:])  # (the pick sits unconsumed at history[p + 1]: feed() writes the reference's token onto that slot)
        steps(W, m, toks, ref, u, kv16, p + 1, "wide", what)
    assert not undecided, f"near-ties at members {undecided}: the token comparison must exclude nobody at these seeds"
    close(ms)
    close(twins)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_greedy_pick_is_the_first_maximum_and_a_forced_token_is_kept(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W, pos = worlds(model, fmt), POSITIONS[:9]
    forced = [tokens_of(W, i, p + 2) for i, p in enumerate(pos)]
    ms = group(pkg, W, kv16, len(pos))
    fed_ahead = (2, 5)  # these members hold a fed token at p + 1: the pick must not replace it
    for i, (m, f, p) in enumerate(zip(ms, forced, pos)):
        m.reset()
        m.feed(f[:p + 1 + (1 if i in fed_ahead else 0)])
    live = [(m, p) for m, p in zip(ms, pos) if p > 0]
    live[0][0].prefill_packed([m for m, _ in live], [p for _, p in live], with_logits=False, digits=2)
    for step in range(2):
        ms[0].step_wide(ms, 1, digits=2)
        for i, (m, f, p) in enumerate(zip(ms, forced, pos)):
            q = p + step
            lg = m.last_logits()
            assert m.position() == q + 1 and not np.isnan(lg).any()
            got = int(m.history(q + 2)[q + 1])
            if i in fed_ahead and step == 0:
                assert got == int(f[p + 1]), (i, "a fed token at p + 1 was replaced")
            else:
                assert got == int(np.argmax(lg)), (i, step, got, int(np.argmax(lg)))  # np.argmax: the first maximum
            assert np.array_equal(m.history(p + 1), f[:p + 1]), i
    close(ms)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_steps_in_one_call_are_three_calls(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W = worlds(model, fmt)
    pos = [62, 126, 0, 33, 200]  # 62: crosses key 64 inside the call; 126: crosses key 128
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms, twins = group(pkg, W, kv16, len(pos)), group(pkg, W, kv16, len(pos))
    for g in (ms, twins):
        g[3].set_sampling(0.9, top_k=40, seed=5)
        g[3].set_logprobs(3)
        prepare(g, forced, pos)
    ms[0].step_wide(ms, 3, digits=2)
    for _ in range(3):
        twins[0].step_wide(twins, 1, digits=2)
    for i, (m, t, p) in enumerate(zip(ms, twins, pos)):
        assert m.position() == p + 3
        assert_same(state(m, W.cfg, kv16), state(t, W.cfg, kv16), f"member {i} (p={p}): step_wide(3) against 3 x step_wide(1)")
    assert ms[3].sampling_draws() == twins[3].sampling_draws() == 3
    assert ms[3].logprob_records(0, W.cfg.max_pos).tobytes() == twins[3].logprob_records(0, W.cfg.max_pos).tobytes()
    close(ms)
    close(twins)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_members_are_isolated_ordered_freely_and_the_step_is_deterministic(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W, pos = worlds(model, fmt), POSITIONS[:9]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms, twins = group(pkg, W, kv16, len(pos)), group(pkg, W, kv16, len(pos))
    for g in (ms, twins):
        g[4].set_sampling(0.9, top_k=40, seed=5)
        g[7].set_sampling(0.8, top_k=0, top_p=0.9, seed=6)
    prepare(ms, forced, pos)
    ms[0].step_wide(ms, 2, digits=2)
    first = [state(m, W.cfg, kv16) for m in ms]
    # ---- determinism: the same call on twin decoders, sampling members with the same seeds included ----
    prepare(twins, forced, pos)
    twins[0].step_wide(twins, 2, digits=2)
    for i, t in enumerate(twins):
        assert_same(state(t, W.cfg, kv16), first[i], f"member {i}: the same wide steps on other decoders")
    # ---- member 3's current token changed: nobody else may notice, bit for bit ----
    other = list(forced)
    other[3] = forced[3].copy()
    other[3][pos[3]] = (int(other[3][pos[3]]) + 911) % W.cfg.vocab
    prepare(twins, other, pos)
    twins[0].step_wide(twins, 2, digits=2)
    for i, t in enumerate(twins):
        if i != 3:
            assert_same(state(t, W.cfg, kv16), first[i], f"member {i} with member 3's token changed")
    assert not np.array_equal(twins[3].last_logits(), ms[3].last_logits())
    # ---- the same members in another order (the driver too): every member the same bits ----
    order = [5, 0, 8, 3, 1, 7, 2, 6, 4]
    prepare(twins, forced, pos)
    twins[5].step_wide([twins[i] for i in order], 2, digits=2)
    for i, t in enumerate(twins):
        assert_same(state(t, W.cfg, kv16), first[i], f"member {i}: the members in another order")
    close(ms)
    close(twins)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_hand_over_to_a_batch_and_to_run(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W, pos = worlds(model, fmt), POSITIONS[:7] + [200, 100]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms, twins = group(pkg, W, kv16, len(pos)), group(pkg, W, kv16, len(pos))
    prepare(ms, forced, pos)
    prepare(twins, forced, pos)
    batch = pkg.HostBatch(8)
    for b in range(4):  # members may sit in batch slots while the wide step runs
        batch.set_slot(b, ms[b])
    ms[0].step_wide(ms, 1, digits=2)
    twins[0].step_wide(twins, 1, digits=2)
    for b in range(4, 8):
        batch.set_slot(b, ms[b])
    batch.step(2)
    ms[8].set_attention_form(0)  # the member taken out of the pack carries on alone
    ms[8].run(2, with_logits=True, use_graph=True)
    for i, (m, t, p) in enumerate(zip(ms, twins, pos)):
        t.set_attention_form(0)
        t.run(2, with_logits=True, use_graph=True)
        assert m.position() == p + 3
        assert_same(state(m, W.cfg, kv16), state(t, W.cfg, kv16), f"member {i} (p={p}): two {'batch steps' if i < 8 else 'run steps'} behind the wide step")
    ms[0].step_wide(ms, 1, digits=2)  # ... and back into a wide step from the batch slots
    for m, p in zip(ms, pos):
        assert m.position() == p + 4
    for b in range(8):
        batch.set_slot(b, None)
    batch.close()
    close(ms)
    close(twins)


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_samplers_and_the_logits_tap(pkg, hip, worlds, fmt):
    from test_logprob_decoder_gpu import check_record

    W, pos = worlds("A", fmt), [33, 0, 64, 130, 65]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    ms = group(pkg, W, False, len(pos))
    ms[1].set_sampling(0.0, 0, 1.0, 1.3, seed=3)  # temperature 0 with a repetition penalty: the bit-exact greedy path, no draw
    ms[2].set_sampling(0.9, top_k=40, seed=5)     # draws
    ms[2].set_logprobs(5)
    ms[3].set_logprobs(5)
    prepare(ms, forced, pos)
    ref, gen = sr.RefSampler(0.0, 0, 1.0, 1.3, seed=3), []
    for step in range(4):
        ms[0].step_wide(ms, 1, digits=2)
        q = [p + step + 1 for p in pos]
        for m, qq in zip(ms, q):
            assert m.position() == qq
        got = int(ms[1].history(q[1] + 1)[q[1]])
        assert got == ref.sample(ms[1].last_logits(), gen), (step, "the penalised argmax of the member's own logits")
        gen.append(got)
        assert ms[1].sampling_draws() == 0 and ms[2].sampling_draws() == step + 1 and ms[0].sampling_draws() == 0
        picked = int(ms[2].history(q[2] + 1)[q[2]])
        assert picked in np.argsort(ms[2].last_logits())[-40:]
        for i in (0, 3, 4):
            assert int(ms[i].history(q[i] + 1)[q[i]]) == int(np.argmax(ms[i].last_logits())), (step, i)
        for i in (2, 3):  # record p + 1: the token in history, its logit, the top 5 of last_logits()
            check_record(ms[i], 5, (fmt, "wide step", step, i))
    for i in (2, 3):
        recs = ms[i].logprob_records(0, W.cfg.max_pos)
        written = [j for j, r in enumerate(recs) if int(r["token"]) != -1]
        assert written == list(range(pos[i] + 1, pos[i] + 5)), (i, written)
        want = logprob_ref.record(ms[i].last_logits(), int(ms[i].history(pos[i] + 5)[pos[i] + 4]), 5)
        assert np.array_equal(recs[pos[i] + 4]["top_id"][:5], want.top_id)
    for i in (0, 1, 4):  # the tap is off: no record to read
        with pytest.raises(pkg.BitNetHipError, match="switched off"):
            ms[i].logprob_records(0, 1)
    close(ms)


def test_refusals_leave_every_member_untouched(pkg, hip, worlds):
    import ctypes as C

    W = worlds("A", "qk256")
    cfg = W.cfg
    ms = group(pkg, W, False, 3)
    stranger = W.decoder(pkg, False)  # other weights (another owner)
    half = ms[0].shared()
    half.set_kv_f16(True)
    for i, m in enumerate(ms + [stranger, half]):
        m.reset()
        m.feed(tokens_of(W, i, 40))
        m.prefill(20, with_logits=True, digits=2)

    def snap_all():
        return [(state(m, cfg, m is half), m.history(cfg.max_pos).copy(), snapshot(m, W, m is half)) for m in ms + [stranger, half]]

    before = snap_all()

    def unchanged(what):
        for (a0, h0, s0), (a1, h1, s1) in zip(before, snap_all()):
            assert_same(a0, a1, what)
            assert np.array_equal(h0, h1) and same_bytes(s0, s1), what

    def refused(members, n, match):
        with pytest.raises(pkg.BitNetHipError, match=match):
            members[0].step_wide(members, n)
        assert re.search(match, members[0].error()), (match, members[0].error())  # the text is on the driver
        unchanged(match)

    crowd = [ms[0].shared() for _ in range(62)]
    refused(ms + crowd, 1, "n_members")
    close(crowd)
    refused(ms, 0, "n_steps")
    refused(ms, -2, "n_steps")
    refused([ms[0], None, ms[2]], 1, "null member")
    refused([ms[0], ms[1], ms[1]], 1, "repeated")
    refused([ms[0], stranger], 1, "same weights")
    refused([ms[0], half], 1, "mixed KV cache types")
    refused(ms, cfg.max_pos - 20, "KV cache overflow")   # 20 + 280 > max_pos - 1
    refused(ms, 2 ** 31 - 1, "KV cache overflow")        # (position + n_steps must not wrap)
    dead = ms[0].shared()
    dead.close()  # a closed decoder's handle is None: the null-member refusal
    refused([ms[0], dead], 1, "null member")
    arr = (C.c_void_p * 3)(*[m.h for m in ms])
    for n_members in (0, -1):  # below 1 cannot be reached through the method (the driver is always a member): the C shim
        assert ms[0].c.bitnet_host_step_wide(arr, n_members, 1, 2, None) == -1 and "n_members" in ms[0].error(), n_members
        unchanged(n_members)
    # a rejected configuration gives a DEAD decoder (only error() and close() may be used on it): as a member it is refused by name
    synth_cfg = type(cfg)(**dict(cfg.asdict(), hidden=100))
    hc = pkg.HostConfig(**{k: (float(v) if k in ("eps", "rope_theta") else int(v)) for k, v in synth_cfg.asdict().items()})
    dead_h = ms[0].c.bitnet_host_create(C.byref(hc))
    assert dead_h
    arr2 = (C.c_void_p * 2)(ms[0].h, dead_h)
    assert ms[0].c.bitnet_host_step_wide(arr2, 2, 1, 2, None) == -1 and "dead member" in ms[0].error()
    unchanged("dead member")
    ms[0].c.bitnet_host_destroy(dead_h)
    # the cache's end: a member at position max_pos - 1 has no slot left
    long = ms[1]
    long.reset()
    long.feed(tokens_of(W, 1, cfg.max_pos))
    long.prefill(cfg.max_pos - 2, with_logits=False, digits=2)
    ms[0].step_wide(ms, 1)  # ... the last step that fits
    assert long.position() == cfg.max_pos - 1
    before = snap_all()
    refused(ms, 1, "KV cache overflow")
    # model globals not set
    bare = pkg.HostDecoder(cfg)
    with pytest.raises(pkg.BitNetHipError, match="model globals not set"):
        bare.step_wide([bare], 1)
    bare.close()
    close([half, stranger])
    close(ms)


@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_saturation_fallback_repeats_the_whole_step(pkg, hip, worlds, fmt, kv16):
    """the outlier world (one LayerNorm weight far beyond the f16 range): the step's f16 hand-over clamps, the step is repeated at 4 digits, and
    the driver counts one -- the cache and the logits pass the float64 gates of every other step"""
    W = worlds("A", fmt, outlier=True)
    pos = [64, 0, 130]
    forced = [tokens_of(W, i, p + 1) for i, p in enumerate(pos)]
    refs = [W.seq(f) for f in forced]
    ms = group(pkg, W, kv16, len(pos))
    prepare(ms, forced, pos)
    base = ms[0].saturation_fallbacks()  # (the fill may have fallen back too: it is the driver of its own pack)
    before = [snapshot(m, W, kv16) for m in ms]
    ms[0].step_wide(ms, 1, digits=2)
    assert ms[0].saturation_fallbacks() == base + 1 and ms[1].saturation_fallbacks() == 0 and ms[0].last_prefill_path() == 0
    for i, (m, p) in enumerate(zip(ms, pos)):
        what = f"outlier wide step [{fmt} kv16={kv16}] member {i} (p={p})"
        toks, ref, u = refs[i]
        assert m.position() == p + 1
        snap = snapshot(m, W, kv16)
        check_untouched(snap, before[i], p, p + 1, what)
        check_values(W, snap, ref, u, kv16, slice(0, p + 1), "wide saturation fallback", what)
        c = cosine(m.last_logits(), ref.logits[p])
        assert c >= 0.9999, (what, "the step's own logits", c)
    close(ms)
