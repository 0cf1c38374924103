"""GPU: PrefixCache (host/prefix_cache.hpp; pkg.PrefixCache) and Decoder::prefill_cached -- prompt prefixes kept as compact device snapshots.

The contract is fork-equivalence: restore(id, dsts, n) leaves every destination as Decoder::fork(src, dsts, n) would have, had src still been in
its state at insert time -- position, history, whole caches (copied slots, untouched slots, padding), sampler reset, graphs still valid; the forced
count through what it decides (where the next feed() lands, what the next steps leave).  So every check here is an equality with the fork / rewind /
prefill calls the suite pins elsewhere (test_fork_decoder_gpu.py, test_extend_gpu.py); nothing has a tolerance.

Model "A" of tests/test_fork_decoder_gpu.py (2 layers, max_pos 640), both storage formats, f32 and f16 caches; that file's helpers restated.  The
source is a 130-token prompt forward plus 5 decode steps."""
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
    """a 130-token prompt forward, then 5 decode steps -- position 135, slots written by the prompt path and the decode path"""
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


def snapshot_bytes(hip, cfg, n, kv16):
    return hip.kv_snapshot_bytes(cfg.n_layers, cfg.n_kv_heads, cfg.head_dim, n, kv_f16=kv16)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restore_leaves_what_fork_leaves(pkg, hip, worlds, case):
    """(a) restore against fork at n in {0, 1, 64, 100, 135}: position, history, whole caches, sampler reset; the forced count by where feed() lands"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    cache = pkg.PrefixCache(min_prefix_length=1)
    eid = cache.insert(src, 135)
    assert cache.entry(eid) == (135, snapshot_bytes(hip, cfg, 135, kv16)) and len(cache) == 1
    assert cache.stats()["memory_usage"] == snapshot_bytes(hip, cfg, 135, kv16) == 2 * cfg.n_layers * cfg.n_kv_heads * 135 * 128 * (2 if kv16 else 4)
    assert cache.lookup(src.history(135)) == (135, eid) and cache.lookup(src.history(134)) is None
    restored, forked = borrower(src, kv16), borrower(src, kv16)
    for d in (restored, forked):
        d.set_sampling(0.9, top_k=40, seed=5)
        start(d, W, 200, offset=7)  # dirtied by a prompt of its own: 200 slots, a history, one draw of its sampler
        assert d.sampling_draws() > 0
    src_before = whole_caches(src, cfg, kv16)
    for n in (0, 1, 64, 100, 135):
        cache.restore(eid, [restored], n)
        src.fork_into([forked], n)
        assert restored.position() == forked.position() == n
        assert restored._fed == forked._fed == min(130, n)  # the binding's fed count comes from the entry's forced count, as fork_into's from the source
        assert np.array_equal(np.asarray(restored.history(cfg.max_pos + 2)), np.asarray(forked.history(cfg.max_pos + 2))), (n, "history")
        got, want = whole_caches(restored, cfg, kv16), whole_caches(forked, cfg, kv16)
        for l, ((gk, gv), (wk, wv)) in enumerate(zip(got, want)):
            assert np.array_equal(gk, wk), (n, f"layer {l} K", int((gk != wk).sum()))
            assert np.array_equal(gv, wv), (n, f"layer {l} V", int((gv != wv).sum()))
        assert restored.sampling_draws() == forked.sampling_draws() == 0, (n, "the destination's sampler is reset")
        assert caches_equal(whole_caches(src, cfg, kv16), src_before) and src.position() == 135, (n, "the source changed")
        if n in (1, 100):  # the forced count: the next fed token lands at slot n on both, and one step (a draw of the reset samplers) leaves the same state
            for d in (restored, forked):
                d.feed([int(W.prompt[n]) ^ 1])
                d.run(1, with_logits=True, use_graph=False)
            assert_same(state(restored, cfg, kv16), state(forked, cfg, kv16), (n, "feed + one step"))
            assert int(restored.history(n + 1)[n]) == int(W.prompt[n]) ^ 1
    # the whole entry by default, and into two at once
    twin = borrower(src, kv16)
    cache.restore(eid, [restored, twin])
    assert_same(state(restored, cfg, kv16, logits=False), state(src, cfg, kv16, logits=False), "the whole entry")
    assert_same(state(twin, cfg, kv16, logits=False), state(src, cfg, kv16, logits=False), "the whole entry, second destination")
    cache.close()
    for d in (restored, forked, twin, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_restored_decoder_continues_as_its_source_did(pkg, hip, worlds, case):
    """(b) on graphs captured BEFORE the restore"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    cache = pkg.PrefixCache()
    eid = cache.insert(src, 135)
    dst = borrower(src, kv16)
    start(dst, W, 20, offset=3)
    dst.prepare_graphs(True)  # every form's graph is captured before the restore: they read the position from device memory
    dst.run(3, with_logits=True, use_graph=True)
    cache.restore(eid, [dst], 133)
    assert dst.position() == 133
    dst.run(2, with_logits=True, use_graph=True)
    assert_same(state(dst, cfg, kv16), state(src, cfg, kv16), "restore at 133 + 2 steps against the source at 135")
    for d in (src, dst):
        d.run(130, with_logits=True, use_graph=True)  # across 256 keys: the attention form changes on the way
    assert src.position() == 265 and src.form_at(134) != src.form_at(264)
    assert_same(state(dst, cfg, kv16), state(src, cfg, kv16), "130 more graph steps")
    cache.close()
    for d in (dst, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_prefix_hit_then_extend_equals_rewind_then_extend(pkg, hip, worlds, case):
    """(c) and the snapshot stands alone: the source is reset and reused before the hit is served"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    cache = pkg.PrefixCache()
    short, long_ = cache.insert(src, 64), cache.insert(src, 135)
    longer = np.concatenate([src.history(135), [1, 2, 3]])  # the 130 prompt tokens, the 5 generated ones, and a continuation
    start(src, W, 150, offset=50)  # the source moves on: nothing of the entries lives in it
    new_prompt = np.concatenate([W.prompt[:64], W.other])
    assert cache.lookup(new_prompt) == (64, short) and cache.lookup(longer) == (135, long_) and cache.lookup(W.prompt[:63]) is None
    dst, twin = borrower(src, kv16), borrower(src, kv16)
    start(dst, W, 90, offset=11)
    cache.restore(short, [dst])
    dst.feed(W.other)  # writes at slot 64, as after a rewind
    dst.extend(70, with_logits=True, digits=2)
    source_calls(twin, W)
    twin.rewind(64)
    twin.feed(W.other)
    twin.extend(70, with_logits=True, digits=2)
    assert dst.position() == 134
    assert_same(state(dst, cfg, kv16), state(twin, cfg, kv16), "restore at 64 + extend(70) against rewind(64) + extend(70)")
    assert list(dst.history(134)[64:]) == [int(t) for t in W.other]
    s = cache.stats()
    assert s["hit_rate"] == 2 / 3 and s["avg_prefix_match_length"] == (64 + 135) / 2 and s["eviction_count"] == 0
    cache.close()
    for d in (dst, twin, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prefill_cached(pkg, hip, worlds, case):
    """(d) no hit: prefill; a hit of m: fork at m + feed + extend; a hit of exactly n restores n - 1"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    cache = pkg.PrefixCache()
    a, b = borrower(src, kv16), borrower(src, kv16)
    # nothing cached: prefill, bit for bit
    for d in (a, b):
        d.reset()
        d.feed(W.prompt[:100])
    assert a.prefill_cached(cache, 100, with_logits=True, digits=2) == 0
    b.prefill(100, with_logits=True, digits=2)
    assert_same(state(a, cfg, kv16), state(b, cfg, kv16), "no hit against prefill")
    assert cache.stats()["miss_rate"] == 1.0 and len(cache) == 0  # it looked, and it never inserts
    eid = cache.insert(src, 64)
    # a miss beside an entry (the prompt leaves the key inside it)
    miss = np.concatenate([W.prompt[:40], W.other])
    for d in (a, b):
        d.reset()
        d.feed(miss)
    assert a.prefill_cached(cache, 110, digits=2) == 0
    b.prefill(110, with_logits=True, digits=2)
    assert_same(state(a, cfg, kv16), state(b, cfg, kv16), "a miss beside an entry against prefill")
    # a hit of 64 inside a prompt of 134
    new_prompt = np.concatenate([W.prompt[:64], W.other])
    a.reset()
    a.feed(new_prompt)
    assert a.prefill_cached(cache, 134, with_logits=True, digits=2) == 64
    start(b, W, 30, offset=17)
    src.fork_into([b], 64)
    b.feed(W.other)
    b.extend(70, with_logits=True, digits=2)
    assert a.position() == 134
    assert_same(state(a, cfg, kv16), state(b, cfg, kv16), "a hit of 64 against fork at 64 + feed + extend(70)")
    assert cache.entry(eid)[0] == 64 and len(cache) == 1
    # a hit of exactly n: n - 1 positions are restored, the last token is computed (its row gives the logits)
    a.reset()
    a.feed(W.prompt[:64])
    assert a.prefill_cached(cache, 64, with_logits=True, digits=2) == 63
    src.fork_into([b], 63)
    b.feed(W.prompt[63:64])
    b.extend(1, with_logits=True, digits=2)
    assert_same(state(a, cfg, kv16), state(b, cfg, kv16), "a hit of exactly n against fork at n - 1 + feed + extend(1)")
    assert a.position() == 64
    # a decoder on other weights (its own upload of the same model): the cache holds nothing for it -- a miss without a lookup, hence prefill
    stranger, lookups = W.decoder(pkg, kv16), cache.stats()
    for d in (stranger, b):
        d.reset()
        d.feed(new_prompt)
    assert stranger.prefill_cached(cache, 134, with_logits=True, digits=2) == 0
    b.prefill(134, with_logits=True, digits=2)
    assert_same(state(stranger, cfg, kv16), state(b, cfg, kv16), "a decoder of another root against prefill")
    assert cache.stats() == lookups
    stranger.close()
    # the refusals are prefill's
    with pytest.raises(pkg.BitNetHipError, match="fresh sequence"):
        a.prefill_cached(cache, 64)
    a.reset()
    a.feed(W.prompt[:10])
    with pytest.raises(pkg.BitNetHipError):
        a.prefill_cached(cache, 11)  # beyond the fed tokens
    cache.close()
    for d in (a, b, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_eviction_under_a_byte_limit_frees_and_keeps_the_right_entries(pkg, hip, worlds, case):
    """(e) a limit sized for two entries, three inserts"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    one = snapshot_bytes(hip, cfg, 64, kv16)
    cache = pkg.PrefixCache(max_memory_bytes=2 * one + one // 2, policy="lru")
    dst = borrower(src, kv16)
    start(dst, W, 80, offset=33)
    start(src, W, 64)  # the decoders' own buffers have grown to what the calls below need before the bytes are counted
    dev0 = pkg.host_device_bytes()
    ids, saved = [], []
    for offset in (0, 100, 200):
        start(src, W, 64, offset=offset)
        ids.append(cache.insert(src, 64))
        saved.append(state(src, cfg, kv16, logits=False))
    assert len(cache) == 2 and cache.stats()["eviction_count"] == 1
    assert cache.stats()["memory_usage"] == sum(cache.entry(i)[1] for i in ids[1:]) == 2 * one
    assert pkg.host_device_bytes() - dev0 >= 2 * one and pkg.host_device_bytes() - dev0 < 3 * one  # the evicted snapshot's device memory is gone
    before = state(dst, cfg, kv16, logits=False)
    with pytest.raises(pkg.BitNetHipError, match="holds no such entry"):
        cache.restore(ids[0], [dst])
    with pytest.raises(pkg.BitNetHipError, match="no entry"):
        cache.entry(ids[0])
    assert_same(state(dst, cfg, kv16, logits=False), before, "a refused restore")
    assert cache.lookup(W.prompt[:64]) is None
    for i in (1, 2):
        assert cache.lookup(W.prompt[100 * i:100 * i + 70]) == (64, ids[i])
        cache.restore(ids[i], [dst])
        assert_same(state(dst, cfg, kv16, logits=False), saved[i], f"survivor {i}")
    assert cache.invalidate(W.prompt[100:164]) and len(cache) == 1 and cache.stats()["memory_usage"] == one
    cache.clear()
    assert len(cache) == 0 and cache.stats()["memory_usage"] == 0 and pkg.host_device_bytes() - dev0 < one
    cache.close()
    for d in (dst, src):
        d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusals_modify_nothing(pkg, hip, worlds, case):
    """(f) restore's refusals are fork's; insert's leave the cache as it was"""
    fmt, kv16 = case
    W = worlds(fmt)
    cfg = W.cfg
    src = W.decoder(pkg, kv16)
    source_calls(src, W)
    cache = pkg.PrefixCache(min_prefix_length=4)
    eid = cache.insert(src, 135)
    dst, spare = borrower(src, kv16), borrower(src, kv16)
    start(dst, W, 40, offset=9)
    start(spare, W, 1)
    before = (dst.position(), np.asarray(dst.history(cfg.max_pos + 2)).copy(), whole_caches(dst, cfg, kv16))
    cache_before = (len(cache), cache.stats())

    def refused(match, call):
        with pytest.raises(pkg.BitNetHipError, match=match) as e:
            call()
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT
        assert dst.position() == before[0] and np.array_equal(np.asarray(dst.history(cfg.max_pos + 2)), before[1]), match
        assert caches_equal(whole_caches(dst, cfg, kv16), before[2]), match
        assert (len(cache), cache.stats()) == cache_before and cache.entry(eid)[0] == 135, match

    refused(r"n_positions must be in \[0, the entry's length\]", lambda: cache.restore(eid, [dst], -2))
    refused(r"n_positions must be in \[0, the entry's length\]", lambda: cache.restore(eid, [dst], 136))
    assert "n_positions must be in" in dst.error()  # the text goes on the first destination too
    refused("holds no such entry", lambda: cache.restore(eid + 1000, [dst], 10))
    refused("n_dst must be 1..8", lambda: cache.restore(eid, [], 10))
    refused("n_dst must be 1..8", lambda: cache.restore(eid, [dst] * 9, 10))
    closed = borrower(src, kv16)
    closed.close()
    refused("null destination", lambda: cache.restore(eid, [dst, closed], 10))
    refused("repeated", lambda: cache.restore(eid, [dst, spare, dst], 10))
    stranger = W.decoder(pkg, kv16)  # the same model, but its own upload: another root
    source_calls(stranger, W)
    refused("same weights", lambda: cache.restore(eid, [dst, stranger], 10))
    refused("same weights", lambda: cache.restore(eid, [stranger], 10))
    other_type = borrower(src, not kv16)
    start(other_type, W, 10)
    refused("mixed KV cache types", lambda: cache.restore(eid, [dst, other_type], 10))
    batch = pkg.HostBatch(2)
    batch.set_slot(0, spare)
    refused("leave the batch first", lambda: cache.restore(eid, [dst, spare], 10))
    L = src.c
    hc = pkg.HostConfig(hidden=100, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=128, ffn=256, vocab=64, max_pos=32, eps=1e-5, rope_theta=1e4)
    dead = L.bitnet_host_create(C.byref(hc))
    assert dead

    def restore_dead():
        arr = (C.c_void_p * 2)(dst.h, dead)
        cache._check(L.bitnet_host_prefix_cache_restore(cache.h, eid, arr, 2, 10))

    refused("dead destination", restore_dead)
    L.bitnet_host_destroy(dead)
    # insert: another root, another cache type, n out of range, a key below min_prefix_length
    refused("other weights", lambda: cache.insert(stranger, 100))
    refused("mixed KV cache types", lambda: cache.insert(other_type, 10))
    refused(r"n must be in \[1, position\(\)\]", lambda: cache.insert(src, 0))
    refused(r"n must be in \[1, position\(\)\]", lambda: cache.insert(src, 136))
    refused("below minimum 4", lambda: cache.insert(src, 3))
    # an entry larger than max_memory_bytes: refused with the cache's entries kept (the index alone would empty itself trying)
    small = pkg.PrefixCache(max_memory_bytes=snapshot_bytes(hip, cfg, 64, kv16), min_prefix_length=1)
    keep = small.insert(src, 64)
    refused("unable to free space", lambda: small.insert(src, 65))
    assert len(small) == 1 and small.entry(keep)[0] == 64 and small.stats()["eviction_count"] == 0
    small.close()
    # the source may sit in a batch slot when it is saved, and a restore into a free decoder still works after all of the above
    batch.set_slot(1, src)
    again = cache.insert(src, 100)
    cache.restore(again, [dst])
    assert dst.position() == 100 and src.position() == 135 and len(cache) == 2
    batch.close()
    cache.close()
    for d in (dst, spare, other_type, stranger, src):
        d.close()
