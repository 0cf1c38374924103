"""GPU: Decoder::shift (host/decoder.hpp; HostDecoder.shift) -- keep the first `keep` positions of a live sequence, discard the next `discard`,
slide the rest down with the keys re-rotated.

(a) state      every layer's caches after shift(4, 147) at position 299 equal tests/shift_ref.py's restatement of the read-back BEFORE the call, bit
               for bit over every slot (moved, untouched, padding); position, history and log-probability records follow shift_ref's pure
               functions; the forced count is pinned through what extend() accepts and what run() leaves in the history.
(b) semantics  layer 0's K and V depend on the token and its position alone, so after the shift they are held to a FRESH decoder's prefill of the
               surviving tokens: V bit for bit; K per cache row within ||shift_ref.bound||_2 (the derived rotation bound) + (4 u_0 [+ 2^-11 with an
               f16 cache]) ||row||_2, the prompt path's own cache gate (tests/test_decoder_state_gpu.py (a); u_0 from tests/model_ref.py's
               f16-class yardstick on the same tokens).  On a ONE-layer model that makes the whole state the re-prefill's, and the next step's
               logits are held to the fresh decoder's: cosine >= 0.9999 and the same greedy token (the project's standing gates).
(c) the wall   a decoder at max_pos - 1 refuses run(1) with "KV cache overflow"; after shift(4, 148) it runs 8 steps, the first of them held to a
               float64 step over the read-back caches (extend_ref.extend_f64 per layer): cosine >= 0.9999, same token.
(d) members    a member of a HostBatch slot, and of a step_wide pack, is shifted between steps and goes on; the other members keep their bits.
(e) refusals   leave position, history and caches untouched.

Model A of tests/test_decoder_state_gpu.py (hidden 512, 2 layers, heads 4 / 2, max_pos 300) and its one-layer form; both storage formats, both
cache types."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402
import kv_read as kv  # noqa: E402
import model_ref as mr  # noqa: E402
import shift_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=300, eps=1e-5, rope_theta=10000.0)
CASES = [(f, k) for f in ("i2s", "qk256") for k in (False, True)]
case_id = lambda c: f"{c[0]}-{'kv16' if c[1] else 'kv32'}"
WORST = {}  # what -> observed worst value, printed at the end of the module


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


class World:
    def __init__(self, synth, oracle, fmt, n_layers):
        self.fmt = fmt
        self.cfg = cfg = synth.ModelConfig(**dict(MODEL_A, n_layers=n_layers))
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
        self.dense = [mr.dense_weights(cfg, w, fmt) for w in self.layers]
        sin, cos = oracle.rope_tables(cfg.head_dim, cfg.max_pos, cfg.rope_theta)  # the f32 tables the device holds
        self.sin, self.cos = sin.reshape(cfg.max_pos, er.D // 2), cos.reshape(cfg.max_pos, er.D // 2)
        self.prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)
        self._u0 = {}

    def decoder(self, pkg, kv16, owner=None):
        if owner is not None:
            dec = owner.shared()
        else:
            dec = pkg.HostDecoder(self.cfg)
            for l, w in enumerate(self.layers):
                dec.set_layer_qk256(l, w) if self.fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
            dec.set_globals(self.glob)
        dec.reset()
        dec.set_kv_f16(kv16)
        return dec

    def u0(self, tokens):
        """layer 0's yardstick on these tokens: the f16-activation class model against the float64 model (computed once per sequence)"""
        key = tuple(int(t) for t in tokens)
        if key not in self._u0:
            with np.errstate(all="ignore"):
                ref = mr.forward(self.cfg, self.dense[:1], self.glob, tokens, self.sin, self.cos)
                cls = mr.forward(self.cfg, self.dense[:1], self.glob, tokens, self.sin, self.cos, rnd=mr.f16)
            self._u0[key] = mr.yardstick(ref, cls)[0]
        return self._u0[key]

    def step_f64(self, token, pasts):
        """one decode step in float64: `token` at position past over pasts = [(k [past, kv, D], v)] per layer -> logits [vocab]"""
        cfg = self.cfg
        emb = np.asarray(self.glob["embed_f16"], np.uint16).view(np.float16).reshape(cfg.vocab, cfg.hidden).astype(np.float64)
        x = emb[int(token)][None, :]
        sin, cos = self.sin.astype(np.float64), self.cos.astype(np.float64)
        for w, (kp, vp) in zip(self.dense, pasts):
            xn = mr.layernorm(x, w["attn_norm"], cfg.eps)
            qkv = np.concatenate([xn @ w["q"].T, xn @ w["k"].T, xn @ w["v"].T], axis=1)
            att, _, _ = er.extend_f64(qkv, np.asarray(kp, np.float64), np.asarray(vp, np.float64), cfg.n_heads, cfg.n_kv_heads, sin, cos)
            x = att.reshape(1, -1) @ w["o"].T + x
            xn = mr.layernorm(x, w["ffn_norm"], cfg.eps)
            g, u = xn @ w["gate"].T, xn @ w["up"].T
            x = (g / (1.0 + np.exp(-g)) * u) @ w["down"].T + x
        return (mr.layernorm(x, np.asarray(self.glob["final_norm"], np.float64), cfg.eps) @ emb.T)[0]


@pytest.fixture(scope="module")
def worlds(pkg, oracle):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    made = {}

    def get(fmt, n_layers=2):
        if (fmt, n_layers) not in made:
            made[(fmt, n_layers)] = World(synth, oracle, fmt, n_layers)
        return made[(fmt, n_layers)]

    yield get
    for what, v in sorted(WORST.items()):
        print(f"SHIFTTABLE | {what} | {v:.8g} |")


def note(what, value, worse=max):
    WORST[what] = worse(WORST.get(what, value), value)


def whole(dec, cfg, kv16):
    """every slot of every layer, padding included: [(K [slots, kv, D], V)] in the cache's dtype"""
    return [(k.copy(), v.copy()) for k, v in kv.all_layers(dec, cfg, kv16)]


def same_bits(a, b):
    return np.array_equal(kv.bits(a), kv.bits(b))


def restated(W, before, keep, discard, n):
    return [sr.shift_f32(k, v, W.sin, W.cos, keep, discard, n) for k, v in before]


def assert_caches(got, want, what):
    for l, ((gk, gv), (wk, wv)) in enumerate(zip(got, want)):
        assert same_bits(gk, wk), (what, f"layer {l} K", int((kv.bits(gk) != kv.bits(wk)).sum()))
        assert same_bits(gv, wv), (what, f"layer {l} V", int((kv.bits(gv) != kv.bits(wv)).sum()))


def full_state(dec, cfg, kv16):
    return dict(pos=dec.position(), hist=np.asarray(dec.history(cfg.max_pos + 2)).copy(), caches=whole(dec, cfg, kv16),
                logits=dec.last_logits().view(np.uint32).copy())


def assert_state(a, b, what):
    assert a["pos"] == b["pos"], (what, "position", a["pos"], b["pos"])
    assert np.array_equal(a["hist"], b["hist"]), (what, "history")
    assert np.array_equal(a["logits"], b["logits"]), (what, "last_logits bits")
    assert_caches(a["caches"], b["caches"], what)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shift_moves_the_whole_state(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    dec = W.decoder(pkg, kv16)
    dec.set_logprobs(2)
    dec.feed(W.prompt[:295])
    dec.prefill(290, with_logits=True, digits=2)
    dec.run(9, with_logits=True, use_graph=True)  # 4 forced steps, 5 picked: records 290 .. 299, slots written by both paths
    assert dec.position() == 299
    before = whole(dec, cfg, kv16)
    hist = np.asarray(dec.history(cfg.max_pos + 2)).copy()
    recs = dec.logprob_records(0, cfg.max_pos).copy()
    logits = dec.last_logits().view(np.uint32).copy()
    assert (recs["token"][290:300] >= 0).all() and (recs["token"][:290] == -1).all()
    dec.shift(4, 147)
    assert_caches(whole(dec, cfg, kv16), restated(W, before, 4, 147, 299), "shift(4, 147) at 299")
    pos, forced, want_hist = sr.shift_state(299, 295, hist, 4, 147, cfg.max_pos)
    assert dec.position() == pos == 152
    assert np.array_equal(np.asarray(dec.history(cfg.max_pos + 2)), want_hist)
    assert want_hist[152] == hist[299] and forced == 148
    got = dec.logprob_records(0, cfg.max_pos)
    assert np.array_equal(got.view(np.uint8), sr.shift_records(recs, 299, 4, 147).view(np.uint8))
    assert (got["token"][143:153] == recs["token"][290:300]).all() and (got["token"][153:] == -1).all()
    assert np.array_equal(dec.last_logits().view(np.uint32), logits), "last_logits() stays"
    # the sequence goes on: graphs captured before the shift read the new position from device memory
    dec.run(3, with_logits=True, use_graph=True)
    assert dec.position() == 155
    now = whole(dec, cfg, kv16)
    want = restated(W, before, 4, 147, 299)
    for l in range(cfg.n_layers):
        for g, w in zip(now[l], want[l]):
            assert same_bits(g[:152], w[:152]) and same_bits(g[155:], w[155:]), f"layer {l}: three steps own slots 152 .. 154 alone"
    dec.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_last_logits_survive_the_shift_also_when_recomputed_lazily(pkg, hip, worlds, case):
    """after a plain greedy step through the screened head the logits row is recomputed on demand: asking before or after the shift gives the
    same bits"""
    fmt, kv16 = case
    W = worlds(fmt)
    asked_before, asked_after = W.decoder(pkg, kv16), None
    asked_after = W.decoder(pkg, kv16, owner=asked_before)
    for d in (asked_before, asked_after):
        start(d, W, 40)
        d.run(3, with_logits=True, use_graph=True)
    want = asked_before.last_logits().view(np.uint32).copy()
    for d in (asked_before, asked_after):
        d.shift(4, 10)
    assert np.array_equal(asked_after.last_logits().view(np.uint32), want)
    assert np.array_equal(asked_before.last_logits().view(np.uint32), want)
    for d in (asked_after, asked_before):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_forced_count_follows(pkg, hip, worlds, case):
    """fed tokens beyond the position survive the shift as fed tokens: extend() accepts exactly the new forced count, run() keeps them"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    dec = W.decoder(pkg, kv16)
    dec.feed(W.prompt[:299])
    dec.prefill(200, with_logits=True, digits=2)
    hist = np.asarray(dec.history(cfg.max_pos + 2)).copy()
    dec.shift(4, 100)
    pos, forced, want_hist = sr.shift_state(200, 299, hist, 4, 100, cfg.max_pos)
    assert (pos, forced) == (100, 199) and dec.position() == 100
    assert np.array_equal(np.asarray(dec.history(cfg.max_pos + 2)), want_hist)
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.extend(100, with_logits=False, digits=2)  # 100 + 100 > 199
    dec.run(5, with_logits=True, use_graph=True)      # device count: the fed tokens at 101 .. 105 are not replaced by picks
    assert np.array_equal(np.asarray(dec.history(cfg.max_pos + 2))[:199], want_hist[:199])
    dec.extend(94, with_logits=True, digits=2)        # 105 + 94 == 199: the host count
    assert dec.position() == 199
    # the other two branches, on the host count: f <= keep stays, f inside the discarded range becomes keep
    dec.reset()
    dec.feed(W.prompt[:3])
    dec.run(20, with_logits=True, use_graph=False)
    dec.shift(4, 10)          # forced 3 <= keep 4: stays 3
    dec.feed(W.prompt[:1])    # writes at max(position 10, forced 3)
    assert dec.position() == 10 and np.asarray(dec.history(12))[10] == W.prompt[0]
    dec.reset()
    dec.feed(W.prompt[:10])
    dec.prefill(10, with_logits=True, digits=2)
    dec.run(4, with_logits=True, use_graph=False)
    dec.shift(4, 10)          # position 14 -> 4; forced 10 in (4, 14]: becomes 4, not 10
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.extend(1, with_logits=False, digits=2)  # nothing is fed ahead of position 4
    dec.close()


def semantic_gate(W, pkg, kv16, dec, fresh, survivors, what):
    """layer 0 of `dec` (shifted) against layer 0 of `fresh` (prefill of the surviving tokens) over slots [0, len(survivors))"""
    cfg, n = W.cfg, len(survivors)
    (k, v), (fk, fv) = kv.caches(dec, cfg, 0, kv16), kv.caches(fresh, cfg, 0, kv16)
    assert same_bits(v[:n], fv[:n]), (what, "layer 0 V", int((kv.bits(v[:n]) != kv.bits(fv[:n])).sum()))
    u0 = W.u0(survivors)
    f64 = fk[:n].astype(np.float64)
    allowed = np.linalg.norm(sr.bound(f64, kv16), axis=-1) + (4.0 * u0 + (2.0 ** -11 if kv16 else 0.0)) * np.linalg.norm(f64, axis=-1)
    err = np.linalg.norm(k[:n].astype(np.float64) - f64, axis=-1)
    rel = float((err / np.linalg.norm(f64, axis=-1)).max())
    note(f"layer-0 K deviation from the re-prefill, rel 2-norm per row ({'f16' if kv16 else 'f32'} cache)", rel)
    print(f"{what}: worst layer-0 K row deviation {rel:.3e} (u_0 {u0:.3e}), worst err / allowed {float((err / allowed).max()):.3e}")
    assert (err <= allowed).all(), (what, float((err / allowed).max()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_layer_0_is_what_a_prompt_forward_of_the_survivors_writes(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    dec, fresh = W.decoder(pkg, kv16), None
    dec.feed(W.prompt[:299])
    dec.prefill(299, with_logits=True, digits=2)
    dec.shift(4, 147)
    survivors = np.concatenate([W.prompt[:4], W.prompt[151:299]])
    assert np.array_equal(np.asarray(dec.history(152)), survivors)
    fresh = W.decoder(pkg, kv16, owner=dec)
    fresh.feed(survivors)
    fresh.prefill(152, with_logits=True, digits=2)
    semantic_gate(W, pkg, kv16, dec, fresh, survivors, f"2 layers {case_id(case)}")
    for d in (fresh, dec):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_layer_model_continues_as_the_re_prefill(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt, 1)
    dec = W.decoder(pkg, kv16)
    dec.feed(W.prompt[:299])
    dec.prefill(299, with_logits=True, digits=2)
    picked = int(dec.history(300)[299])
    dec.shift(4, 147)
    survivors = np.concatenate([W.prompt[:4], W.prompt[151:299]])
    fresh = W.decoder(pkg, kv16, owner=dec)
    fresh.feed(np.concatenate([survivors, [picked]]).astype(np.int32))
    fresh.prefill(152, with_logits=False, digits=2)
    semantic_gate(W, pkg, kv16, dec, fresh, survivors, f"1 layer {case_id(case)}")
    assert int(dec.history(153)[152]) == picked == int(fresh.history(153)[152])
    for d in (dec, fresh):
        d.run(1, with_logits=True, use_graph=False)
    a, b = dec.last_logits(), fresh.last_logits()
    c = cosine(a, b)
    note("one-layer model, next-step logits cosine against the re-prefill", c, worse=min)
    print(f"one layer {case_id(case)}: logits cosine {c:.8f}, tokens {int(np.argmax(a))} / {int(np.argmax(b))}")
    assert c >= 0.9999 and int(np.argmax(a)) == int(np.argmax(b))
    assert int(dec.history(154)[153]) == int(fresh.history(154)[153])
    for d in (fresh, dec):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_past_the_wall(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    dec = W.decoder(pkg, kv16)
    dec.feed(W.prompt[:299])
    dec.prefill(299, with_logits=True, digits=2)
    assert dec.position() == cfg.max_pos - 1
    with pytest.raises(pkg.BitNetHipError, match="KV cache overflow"):
        dec.run(1, with_logits=True, use_graph=True)
    dec.shift(4, 148)
    assert dec.position() == 151
    pasts = [(k[:151], v[:151]) for k, v in whole(dec, cfg, kv16)]
    token = int(dec.history(152)[151])
    dec.run(1, with_logits=True, use_graph=True)
    got, want = dec.last_logits(), W.step_f64(token, pasts)
    c = cosine(got, want)
    note("first step past the wall, logits cosine against the float64 step", c, worse=min)
    print(f"past the wall {case_id(case)}: cosine {c:.8f}")
    assert c >= 0.9999 and int(np.argmax(got)) == int(np.argmax(want))
    dec.run(7, with_logits=True, use_graph=True)
    assert dec.position() == 159 and np.isfinite(dec.last_logits()).all()
    dec.close()


def start(dec, W, n, offset=0):
    dec.reset()
    dec.feed(W.prompt[offset:offset + n])
    dec.prefill(n, with_logits=True, digits=2)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_batch_member_is_shifted_between_steps(pkg, hip, worlds, case):
    """after HostBatch.step every member is where its own run() under attention form 0 leaves it, bit for bit: so the shifted member is held to a
    lone twin that takes the same calls, and the other members to twins that were never near a shift"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    owner = W.decoder(pkg, kv16)
    members = [owner] + [W.decoder(pkg, kv16, owner=owner) for _ in range(2)]
    twins = [W.decoder(pkg, kv16, owner=owner) for _ in range(3)]
    for i, (m, t) in enumerate(zip(members, twins)):
        start(m, W, 100 + 60 * i, offset=3 * i)
        start(t, W, 100 + 60 * i, offset=3 * i)
        t.set_attention_form(0)
    batch = pkg.HostBatch(3)
    for b, m in enumerate(members):
        batch.set_slot(b, m)
    batch.step(2)
    members[1].shift(4, 80)  # position 162 -> 82
    batch.step(3)
    for i, t in enumerate(twins):
        t.run(2, with_logits=True, use_graph=True)
        if i == 1:
            t.shift(4, 80)
        t.run(3, with_logits=True, use_graph=True)
    assert [m.position() for m in members] == [105, 85, 225]
    for i, (m, t) in enumerate(zip(members, twins)):
        assert_state(full_state(m, cfg, kv16), full_state(t, cfg, kv16), f"batch member {i}")
    batch.close()
    for d in twins + members[1:] + [owner]:
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_wide_pack_member_is_shifted_between_steps(pkg, hip, worlds, case):
    """step_wide's rows are independent: the members that are not shifted end bit for bit as in a pack where nobody was; the shifted member keeps
    the restated slots, appends its own, and its first step after the shift is held to the float64 step over its caches"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    owner = W.decoder(pkg, kv16)
    packs = []
    for _ in range(2):
        pack = [W.decoder(pkg, kv16, owner=owner) for _ in range(3)]
        for i, m in enumerate(pack):
            start(m, W, 100 + 60 * i, offset=3 * i)
        packs.append(pack)
    a, b = packs
    for pack in packs:
        pack[0].step_wide(pack, 2)
    before = whole(a[1], cfg, kv16)
    a[1].shift(4, 80)  # position 162 -> 82
    want = restated(W, before, 4, 80, 162)
    assert_caches(whole(a[1], cfg, kv16), want, "shift of a pack member")
    token = int(a[1].history(83)[82])
    a[0].step_wide(a, 1)
    got, ref = a[1].last_logits(), W.step_f64(token, [(k[:82], v[:82]) for k, v in want])
    c = cosine(got, ref)
    note("wide pack member, first step after the shift, logits cosine against the float64 step", c, worse=min)
    assert c >= 0.9999 and int(np.argmax(got)) == int(np.argmax(ref))
    a[0].step_wide(a, 2)
    b[0].step_wide(b, 1)
    b[0].step_wide(b, 2)
    assert [m.position() for m in a] == [105, 85, 225]
    for i in (0, 2):
        assert_state(full_state(a[i], cfg, kv16), full_state(b[i], cfg, kv16), f"wide pack member {i}")
    now = whole(a[1], cfg, kv16)
    for l in range(cfg.n_layers):
        for g, w in zip(now[l], want[l]):
            assert same_bits(g[:82], w[:82]) and same_bits(g[85:], w[85:]), f"layer {l}: three wide steps own slots 82 .. 84 alone"
    for d in a + b + [owner]:
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusals_modify_nothing(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    dec = W.decoder(pkg, kv16)
    start(dec, W, 130)
    dec.run(5, with_logits=True, use_graph=True)
    before = full_state(dec, cfg, kv16)
    for keep, discard, match in ((-1, 10, "keep must be >= 0"), (4, 0, "discard must be >= 1"), (4, -3, "discard must be >= 1"),
                                 (4, 132, r"keep \+ discard must be <= position\(\)"), (136, 1, r"keep \+ discard must be <= position\(\)"),
                                 (2 ** 31 - 1, 2 ** 31 - 1, r"keep \+ discard must be <= position\(\)")):
        with pytest.raises(pkg.BitNetHipError, match=match) as e:
            dec.shift(keep, discard)
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT
        assert_state(full_state(dec, cfg, kv16), before, f"refused shift({keep}, {discard})")
    dec.shift(4, 131)  # keep + discard == position(): valid, nothing moves, the position becomes keep
    assert dec.position() == 4
    assert_caches(whole(dec, cfg, kv16), before["caches"], "shift(4, 131) at 135 moves no slot")
    dec.close()
