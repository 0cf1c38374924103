"""GPU: Decoder::fork / cached_prefix (host/decoder.hpp; HostDecoder.fork_into / fork_from / cached_prefix) -- another decoder takes over the first n
positions of a live one.

After a fork every destination must be what the source would be after rewind(n): position, forced count, history[0 .. n], cache slots < n, BIT FOR
BIT, with every other cache byte of the destination left as it was and the source untouched.  What follows a fork -- decode steps (eager and from
graphs captured BEFORE the fork), extend() over fed tokens, steps inside a HostBatch -- must then equal the same calls on a decoder that reached the
state without a fork.  Equality needs no tolerance; the batch-1 and batched paths themselves are pinned elsewhere (test_decode_parity.py,
test_decoder_state_gpu.py, test_extend_gpu.py, test_batch_decoder_gpu.py).

Model "A" of tests/test_batch_decoder_gpu.py (2 layers, max_pos 640), both storage formats, f32 and f16 caches; that file's helpers restated."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_A = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=640, eps=1e-5, rope_theta=10000.0)
CASES = [(f, k) for f in ("i2s", "qk256") for k in (False, True)]
case_id = lambda c: f"{c[0]}-{'kv16' if c[1] else 'kv32'}"


class World:
    def __init__(self, synth, fmt):
        self.fmt = fmt
        self.cfg = cfg = synth.ModelConfig(**MODEL_A)
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
        self.prompt = np.asarray(synth.prompt(cfg.max_pos, cfg.vocab), np.int32)
        self.other = self.prompt[300:370].copy()  # 70 tokens that leave the prompt at position 64
        if self.other[0] == self.prompt[64]:
            self.other[0] = (self.other[0] + 1) % cfg.vocab

    def decoder(self, pkg, kv16):
        dec = pkg.HostDecoder(self.cfg)
        for l, w in enumerate(self.layers):
            dec.set_layer_qk256(l, w) if self.fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
        dec.set_globals(self.glob)
        dec.reset()
        dec.set_kv_f16(kv16)
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


def start(dec, W, n, offset=0):
    toks = W.prompt[offset:offset + n]
    dec.reset()
    dec.feed(toks)
    if n > 1:
        dec.prefill(n, with_logits=True, digits=2)


def source_calls(dec, W):
    """the source of every test: a 130-token prompt forward, then 5 decode steps -- position 135, slots written by the prompt path and the decode path"""
    start(dec, W, 130)
    dec.run(5, with_logits=True, use_graph=True)
    assert dec.position() == 135


def borrower(owner, kv16):
    d = owner.shared()
    d.set_kv_f16(kv16)
    return d


def state(dec, cfg, kv16, logits=True):
    p = dec.position()
    caches = [(kv.bits(k[:p]).copy(), kv.bits(v[:p]).copy()) for k, v in kv.all_layers(dec, cfg, kv16)]
    return dict(pos=p, hist=np.asarray(dec.history(p + 1)).copy(), logits=dec.last_logits().view(np.uint32).copy() if logits else None, caches=caches)


def assert_same(a, b, what):
    assert a["pos"] == b["pos"], (what, "position", a["pos"], b["pos"])
    assert np.array_equal(a["hist"], b["hist"]), (what, "history")
    if a["logits"] is not None and b["logits"] is not None:
        assert np.array_equal(a["logits"], b["logits"]), (what, "last_logits bits", int((a["logits"] != b["logits"]).sum()))
    for l, ((ka, va), (kb, vb)) in enumerate(zip(a["caches"], b["caches"])):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), (what, f"layer {l} cache slots [0, {a['pos']})")


def whole_caches(dec, cfg, kv16):
    """every slot of every layer, padded chunks included: [(K bits [slots, kv, D], V bits)] -- the decode is a permutation of the whole buffer"""
    return [(kv.bits(k).copy(), kv.bits(v).copy()) for k, v in kv.all_layers(dec, cfg, kv16)]


def caches_equal(a, b):
    return all(np.array_equal(ka, kb) and np.array_equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fork_copies_the_state_of_the_first_n_positions(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    dst = borrower(src, kv16)
    dst.set_sampling(0.9, top_k=40, seed=5)
    start(dst, W, 200, offset=7)  # dirtied by a prompt of its own: 200 slots, a history, one draw of its sampler
    assert dst.sampling_draws() > 0
    src_before = whole_caches(src, cfg, kv16)
    src_hist = np.asarray(src.history(cfg.max_pos + 2)).copy()
    for n in (0, 1, 63, 64, 65, 130, 135):
        prev = whole_caches(dst, cfg, kv16)
        dst.fork_from(src, n)
        got = whole_caches(dst, cfg, kv16)
        for l, ((pk, pv), (sk, sv), (gk, gv)) in enumerate(zip(prev, src_before, got)):
            wk, wv = pk.copy(), pv.copy()
            wk[:n], wv[:n] = sk[:n], sv[:n]  # the source's slots < n, the destination's own bytes everywhere else
            assert np.array_equal(gk, wk), (n, f"layer {l} K", int((gk != wk).sum()))
            assert np.array_equal(gv, wv), (n, f"layer {l} V", int((gv != wv).sum()))
        assert caches_equal(whole_caches(src, cfg, kv16), src_before), (n, "the source's caches changed")
        assert dst.position() == n and src.position() == 135
        hist = np.asarray(dst.history(cfg.max_pos + 2))
        assert np.array_equal(hist[:n + 1], src_hist[:n + 1]), (n, "history[0 .. n]")
        assert not hist[n + 1:].any(), (n, "history beyond n is zeroed")
        assert np.array_equal(np.asarray(src.history(cfg.max_pos + 2)), src_hist), (n, "the source's history changed")
        assert dst.sampling_draws() == 0, (n, "the destination's sampler is reset")
    for d in (dst, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_fork_continues_as_its_source_did(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    dst = borrower(src, kv16)
    start(dst, W, 20, offset=3)
    dst.prepare_graphs(True)  # every form's graph is captured BEFORE the fork: they read the position from device memory
    dst.run(3, with_logits=True, use_graph=True)
    dst.fork_from(src, 133)
    assert dst.position() == 133
    dst.run(2, with_logits=True, use_graph=True)
    assert_same(state(dst, cfg, kv16), state(src, cfg, kv16), "fork at 133 + 2 steps against the source at 135")
    for d in (src, dst):
        d.run(130, with_logits=True, use_graph=True)  # across 256 keys: the attention form changes on the way
    assert src.position() == 265 and src.form_at(134) != src.form_at(264)
    assert_same(state(dst, cfg, kv16), state(src, cfg, kv16), "130 more graph steps")
    for d in (dst, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_prefix_hit_then_extend_equals_rewind_then_extend(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    new_prompt = np.concatenate([W.prompt[:64], W.other])
    assert src.cached_prefix(new_prompt) == 64
    assert src.cached_prefix(src.history(src.position())) == src.position() == 135
    assert src.cached_prefix(src.history(src.position() + 1)) == 135  # the unconsumed token at history[position] is not part of the cached prefix
    assert src.cached_prefix(new_prompt[:10]) == 10 and src.cached_prefix(np.zeros(0, np.int32)) == 0
    dst, twin = borrower(src, kv16), borrower(src, kv16)
    start(dst, W, 90, offset=11)
    dst.fork_from(src, src.cached_prefix(new_prompt))
    dst.feed(W.other)  # writes at slot 64, as after a rewind
    dst.extend(70, with_logits=True, digits=2)
    source_calls(twin, W)
    twin.rewind(64)
    twin.feed(W.other)
    twin.extend(70, with_logits=True, digits=2)
    assert dst.position() == 134
    assert_same(state(dst, cfg, kv16), state(twin, cfg, kv16), "fork at 64 + extend(70) against rewind(64) + extend(70)")
    assert list(dst.history(134)[64:]) == [int(t) for t in W.other]
    for d in (dst, twin, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_call_forks_into_three_and_they_step_in_a_batch(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    forks = [borrower(src, kv16) for _ in range(3)]
    for i, d in enumerate(forks):
        start(d, W, 10 + 60 * i, offset=5 * i)  # positions 10, 70, 130: three different dirty states
    src.fork_into(forks, 65)
    src.rewind(65)  # the source joins them at the same position (a destination that is the source is refused: rewind is that call)
    members = [src] + forks
    assert [m.position() for m in members] == [65] * 4
    batch = pkg.HostBatch(4)
    for b, m in enumerate(members):
        batch.set_slot(b, m)
    batch.step(5)
    twin = W.decoder(pkg, kv16)  # its own copy of the weights, no fork anywhere
    source_calls(twin, W)
    twin.rewind(65)
    twin.set_attention_form(0)  # the form a batch steps in
    twin.run(5, with_logits=True, use_graph=True)
    want = state(twin, cfg, kv16)
    assert want["pos"] == 70
    for i, m in enumerate(members):
        assert_same(state(m, cfg, kv16), want, f"batch member {i} against the twin that rewound to 65 and ran alone")
    batch.close()
    for d in members + [twin]:
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusals_modify_nothing(pkg, hip, worlds, case):
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    dst, spare = borrower(src, kv16), borrower(src, kv16)
    start(dst, W, 40, offset=9)
    start(spare, W, 1)
    before = (dst.position(), np.asarray(dst.history(cfg.max_pos + 2)).copy(), whole_caches(dst, cfg, kv16))

    def refused(match, call):
        with pytest.raises(pkg.BitNetHipError, match=match) as e:
            call()
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT
        assert dst.position() == before[0] and np.array_equal(np.asarray(dst.history(cfg.max_pos + 2)), before[1]), match
        assert caches_equal(whole_caches(dst, cfg, kv16), before[2]), match

    refused(r"n must be in \[0, position\(\)\]", lambda: src.fork_into([dst], -1))
    refused(r"n must be in \[0, position\(\)\]", lambda: src.fork_into([dst], 136))
    refused("n_dst must be 1..8", lambda: src.fork_into([], 10))
    refused("n_dst must be 1..8", lambda: src.fork_into([dst] * 9, 10))
    closed = borrower(src, kv16)
    closed.close()
    refused("null destination", lambda: src.fork_into([dst, closed], 10))
    refused("repeated", lambda: src.fork_into([dst, spare, dst], 10))
    refused("use rewind", lambda: src.fork_into([dst, src], 10))
    stranger = W.decoder(pkg, kv16)  # the same model, but its own upload: another root
    refused("same weights", lambda: src.fork_into([dst, stranger], 10))
    refused("same weights", lambda: stranger.fork_into([dst], 0))
    other_type = borrower(src, not kv16)
    refused("mixed KV cache types", lambda: src.fork_into([dst, other_type], 10))
    batch = pkg.HostBatch(2)
    batch.set_slot(0, spare)
    refused("leave the batch first", lambda: src.fork_into([dst, spare], 10))
    # a dead destination (a rejected configuration): only the C shim can hold one, the Python wrapper raises at construction
    L = src.c
    hc = pkg.HostConfig(hidden=100, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=128, ffn=256, vocab=64, max_pos=32, eps=1e-5, rope_theta=1e4)
    dead = L.bitnet_host_create(C.byref(hc))
    assert dead

    def fork_dead():
        arr = (C.c_void_p * 2)(dst.h, dead)
        src._check(L.bitnet_host_fork(src.h, arr, 2, 10))

    refused("dead destination", fork_dead)
    L.bitnet_host_destroy(dead)
    # the source may sit in a batch slot: it is only read
    batch.set_slot(1, src)
    src.fork_into([dst], 10)
    assert dst.position() == 10 and src.position() == 135
    batch.close()
    for d in (dst, spare, other_type, stranger, src):
        d.close()
