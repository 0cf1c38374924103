"""GPU: Decoder::prefill_packed -- ONE prompt forward for several sequences, each at its own position with its own number of new tokens
(host/decoder.hpp) -- held to what each member's own extend() is held to in tests/test_decoder_state_gpu.py, whose worlds, gates and
helpers are imported, not restated: the KV cache every member is left with against the float64 forward at rel <= 4 u_l (+ 2^-11 with an
f16 cache), the slots the pack did not own bit for bit, the fill's own logits and three decode steps at cosine >= 0.9999.  What a pack
adds is checked without a tolerance: changing one member's tokens changes no bit of any other member's caches or logits, and after the
pack every member steps inside a batch exactly as its own run() would (the hand-over is complete).

Every member's sequence is a different token stream: the prompt shifted per member, plus the reference's own greedy continuation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_batch_decoder_gpu import assert_same, state  # noqa: E402
from test_decoder_state_gpu import CASES, case_id, check_untouched, check_values, same_bytes, snapshot, steps, worlds  # noqa: E402,F401

pytestmark = pytest.mark.gpu

PACKS = {
    "one": [(0, 65)],
    "three_fresh": [(0, 21), (0, 130), (0, 64)],
    "four_live": [(33, 1), (0, 64), (70, 37), (64, 65)],
    "eight_fresh": [(0, n) for n in (5, 1, 63, 64, 65, 21, 2, 107)],
    "twelve": [(0, n) for n in (1, 5, 21, 64, 64, 21, 5, 1, 5, 64, 1, 21)],  # model A only: more members than a batch has slots
}
PACK_CASES = [(c, p) for c in CASES for p in PACKS if p != "twelve" or c[0] == "A"]


def tokens_of(W, i, n, shift=37):
    """member i's forced tokens: the prompt shifted per member (tests/test_decoder_state_gpu.py::test_rewind_then_extend_other_tokens).  The pick
    behind them is compared token for token, so the stream must not end in a near-tie: the shift moves on by 1009 until the FLOAT64 reference's two
    best logits behind the last token lie more than 2^-6 of their value apart -- 32 times the 2^-11 at which a pick stops being decidable (one f16
    rounding of the tied head's operands), decided on the reference alone.  The plain shifted prompt HAS such a near-tie: model B, BitNet32-F16,
    member 0 of the four-member pack (the unshifted prompt, 34 tokens) -- its own extend() on a twin left two best logits within 2^-11 of each
    other, in both cache types, so that pick was undecidable whatever filled the cache.  Every member's pick is compared; none is skipped."""
    memo = W.__dict__.setdefault("_packed_streams", {})
    key = (i, n, shift)
    for k in range(32):
        if key in memo:
            break
        toks = ((W.prompt[:n].astype(np.int64) + shift * i + 1009 * k) % W.cfg.vocab).astype(np.int32)
        top = np.sort(W.forward([int(t) for t in toks]).logits[-1])[-2:]
        if top[1] - top[0] > 2.0 ** -6 * abs(top[1]):
            memo[key] = toks
    return memo[key]


def group(pkg, W, kv16, n):
    owner = W.decoder(pkg, kv16)
    ms = [owner] + [owner.shared() for _ in range(n - 1)]
    for m in ms[1:]:
        m.set_kv_f16(kv16)
    return ms


def prepare(ms, W, pack, forced, fill_logits=False):
    """every member: reset, its tokens fed, its past filled -- even members by prefill, odd ones by run"""
    for i, (m, (p, n)) in enumerate(zip(ms, pack)):
        m.reset()
        m.feed(forced[i][:p + n])
        if p:
            m.prefill(p, with_logits=fill_logits, digits=2) if i % 2 == 0 else m.run(p, with_logits=fill_logits, use_graph=True)
        assert m.position() == p


def close(ms):
    for m in reversed(ms):
        m.close()


@pytest.mark.parametrize("case,name", PACK_CASES, ids=lambda x: x if isinstance(x, str) else case_id(x))
def test_every_member_ends_as_its_own_extend_would_leave_it(pkg, hip, worlds, case, name):
    model, fmt, kv16 = case
    W, pack = worlds(model, fmt), PACKS[name]
    forced = [tokens_of(W, i, p + n) for i, (p, n) in enumerate(pack)]
    refs = [W.seq(f) for f in forced]  # (tokens + the reference's greedy continuation, the f64 forward, u_l)
    ms, twins = group(pkg, W, kv16, len(pack)), group(pkg, W, kv16, len(pack))
    prepare(ms, W, pack, forced)
    prepare(twins, W, pack, forced)
    before = [snapshot(m, W, kv16) for m in ms]
    ms[0].prefill_packed(ms, [n for _, n in pack], with_logits=True, digits=2)
    assert ms[0].saturation_fallbacks() == 0
    undecided = []
    for i, (m, t, (p, n)) in enumerate(zip(ms, twins, pack)):
        what = f"pack {name} [{model} {fmt} kv16={kv16}] member {i} (p={p}, n={n})"
        toks, ref, u = refs[i]
        assert m.position() == p + n, what
        snap = snapshot(m, W, kv16)
        check_untouched(snap, before[i], p, p + n, what)
        check_values(W, snap, ref, u, kv16, slice(0, p + n), "packed", what)
        # position, history and the picked token: what the member's own extend picks on a twin, wherever the twin's pick is decidable
        t.extend(n, with_logits=True, digits=2)
        assert t.position() == p + n
        top = np.sort(t.last_logits())[-2:]
        if top[1] - top[0] > 2.0 ** -11 * abs(top[1]):
            assert np.array_equal(m.history(p + n + 1), t.history(p + n + 1)), what
        else:
            undecided.append(i)
            assert np.array_equal(m.history(p + n), t.history(p + n)), what
        m.feed(toks[p + n:])  # (the pick sits unconsumed at history[p + n]: feed() writes the reference's token onto that slot)
        steps(W, m, toks, ref, u, kv16, p + n, "packed", what)
    assert not undecided, f"near-ties at members {undecided}: the token comparison must exclude nobody at these seeds"
    close(ms)
    close(twins)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_members_are_isolated_and_step_in_a_batch_as_their_own_run(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W, pack = worlds(model, fmt), PACKS["four_live"]
    ns = [n for _, n in pack]
    forced = [tokens_of(W, i, p + n) for i, (p, n) in enumerate(pack)]
    ms, twins = group(pkg, W, kv16, len(pack)), group(pkg, W, kv16, len(pack))
    prepare(ms, W, pack, forced)
    ms[0].prefill_packed(ms, ns)
    first = [state(m, W.cfg, kv16) for m in ms]
    # ---- the same pack with member 1's tokens changed: nobody else may notice, bit for bit ----
    other = list(forced)
    other[1] = tokens_of(W, 1, sum(pack[1]), shift=911)
    assert not np.array_equal(other[1], forced[1])
    prepare(twins, W, pack, other)
    twins[0].prefill_packed(twins, ns)
    for i, t in enumerate(twins):
        if i != 1:
            assert_same(state(t, W.cfg, kv16), first[i], f"member {i} with member 1's tokens changed")
    assert not np.array_equal(twins[1].last_logits(), ms[1].last_logits())
    # ---- the same pack on the twins; then the members step in a batch, the twins run alone under attention form 0 ----
    prepare(twins, W, pack, forced)
    twins[0].prefill_packed(twins, ns)
    batch = pkg.HostBatch(len(ms))
    for b, m in enumerate(ms):
        batch.set_slot(b, m)
    batch.step(2)
    for i, (m, t) in enumerate(zip(ms, twins)):
        assert_same(state(t, W.cfg, kv16), first[i], f"member {i}: the same pack on other decoders")
        t.set_attention_form(0)
        t.run(2, with_logits=True, use_graph=True)
        assert_same(state(m, W.cfg, kv16), state(t, W.cfg, kv16), f"member {i}: two batch steps behind the pack")
    # members sitting in batch slots may be packed again: the carry-on rule feeds the pick and the next tokens
    for m in ms:
        p = m.position()
        m.feed(np.concatenate([m.history(p + 1)[p:], W.prompt[:4]]).astype(np.int32))
    ms[0].prefill_packed(ms, [5] * len(ms))
    batch.step(1)
    for b in range(len(ms)):
        batch.set_slot(b, None)
    batch.close()
    close(ms)
    close(twins)


@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_without_logits_and_with_samplers_and_a_logits_tap(pkg, hip, worlds, fmt):
    W, pack = worlds("A", fmt), PACKS["four_live"]
    ns = [n for _, n in pack]
    forced = [tokens_of(W, i, p + n) for i, (p, n) in enumerate(pack)]
    ms = group(pkg, W, False, len(pack))
    # ---- with_logits=False: the positions move, nothing is picked ----
    prepare(ms, W, pack, forced)
    hist = [m.history(W.cfg.max_pos).copy() for m in ms]
    ms[0].prefill_packed(ms, ns, with_logits=False)
    for m, (p, n), h in zip(ms, pack, hist):
        assert m.position() == p + n and np.array_equal(m.history(W.cfg.max_pos), h)
        m.run(1, with_logits=True)  # p + n tokens were forced, so this step picks
        assert m.position() == p + n + 1 and np.array_equal(m.history(p + n), h[:p + n])
    # ---- samplers under different seeds on two members, the logits tap on one of them ----
    ms[1].set_sampling(0.9, top_k=40, seed=5)
    ms[2].set_sampling(0.9, top_k=40, seed=6)
    ms[2].set_logprobs(3)
    prepare(ms, W, pack, forced)
    ms[0].prefill_packed(ms, ns, with_logits=True)
    picks = []
    for m, (p, n) in zip(ms, pack):
        assert m.position() == p + n
        picks.append(int(m.history(p + n + 1)[p + n]))
        assert 0 <= picks[-1] < W.cfg.vocab
    p, n = pack[2]
    recs = ms[2].logprob_records(0, W.cfg.max_pos)
    assert int(recs[p + n]["token"]) == picks[2] and int(recs[p + n]["n_top"]) == 3
    assert all(int(r["token"]) == -1 for j, r in enumerate(recs) if j != p + n)
    # the samplers drew: a greedy twin of member 1 would have taken the argmax; the sampled token lies in the top 40 of its own logits
    for i in (1, 2):
        assert picks[i] in np.argsort(ms[i].last_logits())[-40:]
    assert picks[0] == int(np.argmax(ms[0].last_logits())) and picks[3] == int(np.argmax(ms[3].last_logits()))
    close(ms)


def test_refusals_leave_every_member_untouched(pkg, hip, worlds):
    W = worlds("A", "qk256")
    cfg = W.cfg
    ms = group(pkg, W, False, 3)
    stranger = W.decoder(pkg, False)  # other weights (another owner)
    half = ms[0].shared()
    half.set_kv_f16(True)
    for i, m in enumerate(ms + [stranger, half]):
        m.reset()
        m.feed(tokens_of(W, i, 40))
        m.prefill(20, with_logits=False, digits=2)

    def snap_all():
        return [(m.position(), m.history(cfg.max_pos).copy(), snapshot(m, W, m is half)) for m in ms + [stranger, half]]

    before = snap_all()

    def refused(members, ns, match):
        with pytest.raises(pkg.BitNetHipError, match=match):
            members[0].prefill_packed(members, ns)
        for (p0, h0, s0), (p1, h1, s1) in zip(before, snap_all()):
            assert p0 == p1 and np.array_equal(h0, h1) and same_bytes(s0, s1), match

    crowd = [ms[0].shared() for _ in range(62)]
    refused(ms + crowd, [1] * 65, "n_members")
    close(crowd)
    refused([ms[0], None, ms[2]], [5, 5, 5], "null member")
    refused([ms[0], ms[1], ms[1]], [5, 5, 5], "repeated")
    refused([ms[0], stranger], [5, 5], "same weights")
    refused([ms[0], half], [5, 5], "mixed KV cache types")
    refused(ms, [5, 0, 5], "at least 1 token")
    refused(ms, [5, -3, 5], "at least 1 token")
    refused(ms, [5, 2 ** 31 - 1, 5], "feed\\(\\) the prompt tokens first")  # (position + n must not wrap)
    refused(ms, [5, 21, 5], "feed\\(\\) the prompt tokens first")  # 20 + 21 > 40 fed tokens
    dead = ms[0].shared()
    dead.close()  # a closed decoder's handle is None: the null-member refusal
    refused([ms[0], dead], [5, 5], "null member")
    # n_members below 1 cannot be reached through the method (the driver is always a member): the C shim
    import ctypes as C
    arr, five = (C.c_void_p * 3)(*[m.h for m in ms]), (C.c_int32 * 3)(5, 5, 5)
    for n_members in (0, -1):
        assert ms[0].c.bitnet_host_prefill_packed(arr, five, n_members, 1, 2, None) == -1 and "n_members" in ms[0].error(), n_members
        for (p0, h0, s0), (p1, h1, s1) in zip(before, snap_all()):
            assert p0 == p1 and np.array_equal(h0, h1) and same_bytes(s0, s1), n_members
    assert ms[0].c.bitnet_host_prefill_packed(arr, None, 3, 1, 2, None) == -1 and "null lengths" in ms[0].error()
    # the cache's end: position 20 + n > max_pos - 1
    long = ms[1]
    long.reset()
    long.feed(tokens_of(W, 1, cfg.max_pos))
    long.prefill(20, with_logits=False, digits=2)
    before = snap_all()
    refused(ms, [5, cfg.max_pos - 20, 5], "KV cache overflow")
    ms[0].prefill_packed(ms, [5, cfg.max_pos - 21, 5])  # ... and the longest pack that fits
    assert long.position() == cfg.max_pos - 1
    # model globals not set
    bare = pkg.HostDecoder(cfg)
    with pytest.raises(pkg.BitNetHipError, match="model globals not set"):
        bare.prefill_packed([bare], [1])
    bare.close()
    close([half, stranger])
    close(ms)


@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_saturation_fallback_repeats_the_whole_pack(pkg, hip, worlds, fmt, kv16):
    """the outlier world (one LayerNorm weight far beyond the f16 range): the pack clamps, is repeated at 4 digits, and the driver counts one"""
    W = worlds("A", fmt, outlier=True)
    pack = [(0, 130), (0, 65)]
    forced = [tokens_of(W, i, n) for i, (_, n) in enumerate(pack)]
    refs = [W.seq(f) for f in forced]
    ms = group(pkg, W, kv16, 2)
    prepare(ms, W, pack, forced)
    ms[0].prefill_packed(ms, [n for _, n in pack], with_logits=True, digits=2)
    assert ms[0].saturation_fallbacks() == 1 and ms[1].saturation_fallbacks() == 0 and ms[0].last_prefill_path() == 0
    for i, (m, (_, n)) in enumerate(zip(ms, pack)):
        toks, ref, u = refs[i]
        assert m.position() == n
        check_values(W, snapshot(m, W, kv16), ref, u, kv16, slice(0, n), "packed saturation fallback", f"outlier pack member {i}")
    close(ms)
