"""The KV cache every prompt path of a Decoder leaves behind, read back slot by slot (tests/kv_read.py) and held against the float64
whole-prompt forward (tests/model_ref.py).  The cache is the only state one decoder call hands to the next; a logits cosine over n keys
gives one wrong slot about 1 / n of the attention weight and does not see it.

(a) values    every layer, position < n and KV head: rel = ||got - want||_2 / ||want||_2 of the cache row against the f64 K / V row.
              Gate: rel <= 4 u_l (+ 2^-11 with an f16 cache: the one rounding on append), u_l = the largest such rel of the f16-activation
              class model (model_ref.forward(rnd=f16)) against the f64 model in layer l on the same tokens -- measured against the reference
              alone.  The device rounds in the same class at a few more places than the yardstick (f16 probabilities and f16 K / V operands of
              the prompt attention, the 15-bit two-digit planes, QAct records in the step path): a handful of equal independent terms is
              about 2 x, the rest is headroom.  A wrong slot, head, RoPE position or stale row has rel ~ 0.5 and more.
(b) the slots the call did not own: finite on a fresh decoder; after run / extend / rewind + extend bit-identical to what they held.
(c) equalities without a tolerance (extend at 0 == prefill, score == prefill, repeatability, f16 vs f32 cache in layer 0, sharded ranks).
(d) three decode steps on the cache (eager, graph, eager): logits cosine >= 0.9999 against the f64 logits, the appended rows pass (a).

Every sequence is the prompt + the REFERENCE's greedy continuation, fed whole: a near-tie cannot fork the sequence.
Model A: hidden 512, 2 layers, heads 4 / 2; model B: hidden 1024, 3 layers, heads 6 / 3 (q | k | v rows 768 / 384 / 384: not the hidden width);
max_pos 300 (the last cache tile is padding).  Model B was planned at hidden 768, which the decoder refuses (its logits kernel takes multiples of
512: test_the_decoder_refuses_hidden_768 pins that); 1024 is the nearest width it takes."""
import importlib
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402
import model_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = {
    "A": dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=300, eps=1e-5, rope_theta=10000.0),
    "B": dict(hidden=1024, n_layers=3, n_heads=6, n_kv_heads=3, head_dim=128, ffn=1280, vocab=2048, max_pos=300, eps=1e-5, rope_theta=10000.0),
}
LENGTHS = (21, 63, 64, 65, 107, 130, 256)
AB = [(70, 37), (21, 64), (33, 1), (64, 64), (0, 50)]  # tests/test_extend_gpu.py
STEPS = 3
CASES = [(m, f, k) for m in ("A", "B") for f in ("i2s", "qk256") for k in (False, True)]
case_id = lambda c: f"{c[0]}-{c[1]}-{'kv16' if c[2] else 'kv32'}"
TABLE = {}  # (path, fmt, cache type, layer) -> worst rel / u_l


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


class World:
    """one (model, format): weights, the dense f64 matrices, and the references per token sequence (computed once, never changed)"""

    def __init__(self, synth, oracle, model, fmt, outlier=False):
        self.model, self.fmt = model, fmt
        self.cfg = cfg = synth.ModelConfig(**MODELS[model])
        self.glob = synth.make_globals(cfg)
        self.layers = [synth.make_layer(cfg, l) if fmt == "qk256" else synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
        if outlier:  # tests/test_f16_chain.py: one channel of the last feed-forward LayerNorm weight far beyond the f16 range
            self.layers[-1]["ffn_norm"] = self.layers[-1]["ffn_norm"].copy()
            self.layers[-1]["ffn_norm"][33] = 2e5
        self.dense = [mr.dense_weights(cfg, w, fmt) for w in self.layers]
        self.rope = oracle.rope_tables(cfg.head_dim, cfg.max_pos, cfg.rope_theta)
        self.prompt = synth.prompt(cfg.max_pos, cfg.vocab)  # synth.prompt(n) is its prefix for every n
        self._seq = {}

    def forward(self, tokens, rnd=None):
        with np.errstate(all="ignore"):  # (the outlier model's class forward leaves the f16 range behind the last layer: its K / V do not)
            return mr.forward(self.cfg, self.dense, self.glob, tokens, *self.rope, rnd=rnd)

    def seq(self, forced):
        """forced tokens + the reference's own STEPS greedy tokens -> (tokens [n + STEPS], Forward over them, u_l per layer)"""
        key = tuple(int(t) for t in forced)
        if key not in self._seq:
            toks = list(key)
            for _ in range(STEPS):
                toks.append(int(np.argmax(self.forward(toks).logits[-1])))
            ref = self.forward(toks)
            self._seq[key] = (np.asarray(toks, np.int32), ref, mr.yardstick(ref, self.forward(toks, rnd=mr.f16)))
        return self._seq[key]

    def decoder(self, pkg, kv16):
        dec = pkg.HostDecoder(self.cfg)
        for l, w in enumerate(self.layers):
            dec.set_layer_qk256(l, w) if self.fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
        dec.set_globals(self.glob)
        dec.reset()
        dec.set_kv_f16(kv16)
        return dec


@pytest.fixture(scope="module")
def worlds(pkg, oracle):
    synth = importlib.import_module("bitnet-rs_amd.synth")
    made = {}

    def get(model, fmt, outlier=False):
        key = (model, fmt, outlier)
        if key not in made:
            made[key] = World(synth, oracle, model, fmt, outlier)
        return made[key]

    yield get
    if TABLE:
        print("\nworst rel / u_l per (path, format, cache, layer):")
        for (path, fmt, cache, layer), r in sorted(TABLE.items()):
            print(f"KVTABLE | {path} | {fmt} | {cache} | {layer} | {r:.3f} |")


def snapshot(dec, W, kv16):
    return kv.all_layers(dec, W.cfg, kv16)


def same_bytes(a, b, rows=slice(None)):
    return all(np.array_equal(kv.bits(x[rows]), kv.bits(y[rows])) for la, lb in zip(a, b) for x, y in zip(la, lb))


def check_values(W, snap, ref, u, kv16, rows, path, what):
    """(a) over the positions `rows` (a slice)"""
    for l, (k, v) in enumerate(snap):
        rk, rv = mr.kv_rel(k[rows], ref.K[l][rows]), mr.kv_rel(v[rows], ref.V[l][rows])
        gate = 4.0 * u[l] + (2.0 ** -11 if kv16 else 0.0)
        worst = max(float(rk.max()), float(rv.max()))
        key = (path, W.fmt, "f16" if kv16 else "f32", l)
        TABLE[key] = max(TABLE.get(key, 0.0), worst / u[l])
        if not worst <= gate:  # the error profile a finding needs: which of K / V, which positions
            bad_k, bad_v = np.argwhere(~(rk <= gate)), np.argwhere(~(rv <= gate))
            first = rows.start or 0
            prof = [f"pos {first + p}: K {rk[p].max():.2e} V {rv[p].max():.2e}" for p in sorted({int(i[0]) for i in np.r_[bad_k, bad_v]})[:12]]
            pytest.fail(f"{what} [{W.model} {W.fmt} kv16={kv16}] layer {l}: rel {worst:.3e} > gate {gate:.3e} (u_l {u[l]:.2e}); K rows over the gate "
                        f"{len(bad_k)}, V rows {len(bad_v)} of {rk.size}; " + "; ".join(prof))


def check_untouched(snap, before, lo, hi, what):
    """(b) after a call that owned positions [lo, hi): everything below and beyond keeps its bits"""
    assert same_bytes(snap, before, slice(0, lo)), f"{what}: a slot below position {lo} changed"
    assert same_bytes(snap, before, slice(hi, None)), f"{what}: a slot at or beyond position {hi} changed"


def check_finite_tail(snap, n, what):
    for k, v in snap:
        assert np.isfinite(k[n:].astype(np.float64)).all() and np.isfinite(v[n:].astype(np.float64)).all(), f"{what}: a slot beyond position {n} is not finite"


def steps(W, dec, toks, ref, u, kv16, n, path, what):
    """(d) the fill's own logits (row n - 1), then STEPS decode steps on the cache it left"""
    c = cosine(dec.last_logits(), ref.logits[n - 1])
    assert c >= 0.9999, (what, "the fill's own logits", c)
    for i in range(STEPS):
        before = snapshot(dec, W, kv16)
        dec.run(1, with_logits=True, use_graph=bool(i % 2))
        assert dec.position() == n + i + 1, what
        c = cosine(dec.last_logits(), ref.logits[n + i])
        assert c >= 0.9999, (what, f"decode step {i}", c)
        check_untouched(snapshot(dec, W, kv16), before, n + i, n + i + 1, f"{what}, decode step {i}")
    snap = snapshot(dec, W, kv16)
    check_values(W, snap, ref, u, kv16, slice(n, n + STEPS), path + " +steps", what + ", the appended rows")
    assert list(dec.history(n + STEPS)) == [int(t) for t in toks], what
    return snap


def fill_and_check(W, dec, kv16, n, fill, path, what):
    """reset, feed the whole sequence, fill n positions, then (a), (b: finite), (d).  -> the snapshot right after the fill"""
    toks, ref, u = W.seq(W.prompt[:n])
    dec.reset()
    dec.feed(toks)
    fill(dec, n)
    assert dec.position() == n, what
    snap = snapshot(dec, W, kv16)
    check_values(W, snap, ref, u, kv16, slice(0, n), path, what)
    check_finite_tail(snap, n, what)
    steps(W, dec, toks, ref, u, kv16, n, path, what)
    return snap


def form(dec, hip):
    return f"prefill path {dec.last_prefill_path()}, last tile {hip.matmul_last_tile()}"


def expected_form(fmt, digits):
    """-> (last_prefill_path, the last matmul's (digits, wave_tokens, scale_mode) or None where the tile depends on the row count)"""
    if fmt == "i2s":  # f16-valued 32-block scales: the f16 chain at 2 digits, k_gemm_mfma<NDIG, TT32, 3, 2, 1> (the K = 32 form) at 3 / 4
        return (1, None) if digits == 2 else (0, (digits, 32 if digits == 3 else 16, 3))
    return (0, None)


def test_the_decoder_refuses_hidden_768(pkg, hip):
    """why model B is 1024 wide: once the decoder takes 768, this fails and model B goes back to the planned width"""
    synth = importlib.import_module("bitnet-rs_amd.synth")
    with pytest.raises(pkg.BitNetHipError, match="multiple of 512"):
        pkg.HostDecoder(synth.ModelConfig(**dict(MODELS["B"], hidden=768)))


# ---- prefill(n, digits) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prefill_at_every_digit_count(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W = worlds(model, fmt)
    dec = W.decoder(pkg, kv16)
    for digits in (2, 3, 4):
        for n in LENGTHS:
            seen = {}

            def fill(d, n_):
                d.prefill(n_, with_logits=True, digits=digits)
                seen["path"], seen["tile"] = d.last_prefill_path(), dict(hip.matmul_last_tile())

            what = f"prefill({n}, digits={digits})"
            try:
                first = fill_and_check(W, dec, kv16, n, fill, f"prefill d{digits}", what)
            except (Exception, pytest.fail.Exception) as e:  # name the kernel form in whatever fails
                raise AssertionError(f"{what}: {seen}: {e}") from e
            path, tile = expected_form(fmt, digits)
            assert seen["path"] == path, (what, seen)
            if tile:
                assert (seen["tile"]["digits"], seen["tile"]["wave_tokens"], seen["tile"]["scale_mode"]) == tile, (what, seen)
            if n == 107:  # (c) the same fill again after reset(): the same bytes
                toks, _, _ = W.seq(W.prompt[:n])
                dec.reset()
                dec.feed(toks)
                dec.prefill(n, with_logits=True, digits=digits)
                assert same_bytes(snapshot(dec, W, kv16), first, slice(0, n)), f"{what}: a repeated fill left other bytes"
    dec.close()


# ---- run(n) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_run_token_by_token(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W = worlds(model, fmt)
    dec = W.decoder(pkg, kv16)
    for act in (1, 0):
        dec.set_act_mode(act)
        for graph in (False, True):
            for n in LENGTHS:
                what = f"run({n}, graph={graph}, act_mode={act})"
                toks, ref, u = W.seq(W.prompt[:n])
                dec.reset()
                dec.feed(toks)
                half = n // 2
                dec.run(half, with_logits=False, use_graph=graph)
                before = snapshot(dec, W, kv16)
                dec.run(n - half, with_logits=True, use_graph=graph)
                assert dec.position() == n, what
                snap = snapshot(dec, W, kv16)
                check_untouched(snap, before, half, n, what)
                check_values(W, snap, ref, u, kv16, slice(0, n), f"run act{act} {'graph' if graph else 'eager'}", what)
                steps(W, dec, toks, ref, u, kv16, n, f"run act{act}", what)
    dec.close()


# ---- the per-decoder switches that select another layer loop -----------------------------------------------------------------
SWITCHES = [("BITNET_HOST_PREFILL_CHAIN", "0"), ("BITNET_HOST_PREFILL_CHAIN", "1"), ("BITNET_HOST_PREFILL_FP6", "0"), ("BITNET_HOST_PREFILL_QB32", "1"),
            ("BITNET_HOST_PREFILL_HYBRID", "2")]
# (the QB32 case runs with BITNET_HOST_PREFILL_HYBRID=2 beside it, so that the decoder chooses the QB32 chain at these sizes; it still skips,
# at every length of LENGTHS: the o-projection's launcher takes the QB32 hand-over only from a producer that runs 64-token tiles, and at hidden
# 512 / 1024 with at most 256 rows the tile picker gives the producer narrower ones -- "FUSE_YH_QB32: this launch does not run 64-token tiles".
# tests/test_bench_prefill_instance.py holds the form at the widths where it runs)


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: f"{s[0][12:]}={s[1]}")
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prefill_under_a_layer_loop_switch(pkg, hip, worlds, monkeypatch, case, switch):
    model, fmt, kv16 = case
    name, value = switch
    if fmt == "i2s" and (name, value) == ("BITNET_HOST_PREFILL_CHAIN", "1"):
        pytest.skip("the block-scaled format takes the f16 chain by default: =1 selects nothing else")
    if fmt == "i2s" and name in ("BITNET_HOST_PREFILL_FP6", "BITNET_HOST_PREFILL_QB32", "BITNET_HOST_PREFILL_HYBRID"):
        pytest.skip("the fp6 x fp4 forms and the hybrid forward take unscaled matrices only: the switch does not reach a block-scaled model")
    W = worlds(model, fmt)
    base = W.decoder(pkg, kv16)  # the default loop, for the comparison below
    base.reset()
    base.feed(W.prompt[:21])
    base.prefill(21, with_logits=True, digits=2)  # (its own switches are read here, at its first prompt: before the environment changes)
    monkeypatch.setenv(name, value)
    if name == "BITNET_HOST_PREFILL_QB32":
        monkeypatch.setenv("BITNET_HOST_PREFILL_HYBRID", "2")  # without it the QB32 chain waits for the hybrid forward's long shares
    dec = W.decoder(pkg, kv16)   # the switches are read by the constructor / at the decoder's first prompt
    want_path = {("BITNET_HOST_PREFILL_CHAIN", "0"): 0, ("BITNET_HOST_PREFILL_CHAIN", "1"): 1, ("BITNET_HOST_PREFILL_FP6", "0"): 0,
                 ("BITNET_HOST_PREFILL_QB32", "1"): 2, ("BITNET_HOST_PREFILL_HYBRID", "2"): 0}[switch]
    for n in LENGTHS:
        toks, _, _ = W.seq(W.prompt[:n])
        if name == "BITNET_HOST_PREFILL_QB32":
            dec.reset()
            dec.feed(toks)
            try:
                dec.prefill(n, with_logits=True, digits=2)
                refusal = None if dec.last_prefill_path() == 2 else f"the decoder stays on path {dec.last_prefill_path()}"
            except pkg.BitNetHipError as e:  # only the launcher's own refusal of the form at this shape is a skip
                if "FUSE_YH_QB32: this launch does not run 64-token tiles" not in str(e):
                    raise
                refusal = "the decoder chooses it and the o-projection's launcher refuses the hand-over (" + str(e)[str(e).rindex("FUSE_YH_QB32:"):] + ")"
            if refusal:
                base.close()
                dec.close()
                pytest.skip(f"the QB32 chain is not taken at hidden {W.cfg.hidden} with {n} rows: {refusal}")
        what = f"{name}={value} prefill({n}, digits=2)"
        snap = fill_and_check(W, dec, kv16, n, lambda d, n_: d.prefill(n_, with_logits=True, digits=2), f"prefill d2 {name[12:]}={value}", what)
        assert dec.last_prefill_path() == want_path, (what, form(dec, hip))
        base.reset()
        base.feed(toks)
        base.prefill(n, with_logits=True, digits=2)
        same = same_bytes(snap, snapshot(base, W, kv16), slice(0, n))
        if name == "BITNET_HOST_PREFILL_FP6":
            assert same, f"{what}: the int8 planes and the fp6 x fp4 form multiply the same integers, the caches differ"
        else:
            assert not same, f"{what}: the same bytes as the default loop in every layer -- did the switch select anything?"
    base.close()
    dec.close()


# ---- the saturation fallback, followed by decode steps --------------------------------------------------------------------------
@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("fmt", ["i2s", "qk256"])
def test_saturation_fallback_leaves_a_cache_the_steps_agree_with(pkg, hip, worlds, fmt, kv16):
    W = worlds("A", fmt, outlier=True)
    dec = W.decoder(pkg, kv16)
    n = 256
    what = f"outlier gamma, prefill({n}, digits=2)"
    fill_and_check(W, dec, kv16, n, lambda d, n_: d.prefill(n_, with_logits=True, digits=2), "saturation fallback", what)
    assert dec.saturation_fallbacks() == 1 and dec.last_prefill_path() == 0, (dec.saturation_fallbacks(), form(dec, hip))
    dec.close()


# ---- prefill(a) / run(a), then extend(b) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_extend_behind_prefill_and_behind_run(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W = worlds(model, fmt)
    dec = W.decoder(pkg, kv16)
    for a, b in AB:
        n = a + b
        toks, ref, u = W.seq(W.prompt[:n])
        for digits in (2, 4):
            for head in ("prefill", "run"):
                what = f"{head}({a}) + extend({b}, digits={digits})"
                dec.reset()
                dec.feed(toks)
                if a:
                    dec.prefill(a, with_logits=False, digits=digits) if head == "prefill" else dec.run(a, with_logits=False, use_graph=True)
                assert dec.position() == a
                before = snapshot(dec, W, kv16)
                dec.extend(b, with_logits=True, digits=digits)
                assert dec.position() == n, what
                snap = snapshot(dec, W, kv16)
                if a:
                    check_untouched(snap, before, a, n, what + " " + form(dec, hip))
                check_values(W, snap, ref, u, kv16, slice(0, n), f"{head} + extend d{digits}", what + " " + form(dec, hip))
                steps(W, dec, toks, ref, u, kv16, n, f"{head} + extend d{digits}", what)
    dec.close()


# ---- prefill(n), rewind(m), extend(n - m) of other tokens -------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rewind_then_extend_other_tokens(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W = worlds(model, fmt)
    dec = W.decoder(pkg, kv16)
    for n, m in [(130, 0), (130, 50), (130, 64), (130, 129), (256, 64), (256, 255)]:
        what = f"prefill({n}), rewind({m}), extend({n - m})"
        first, _, _ = W.seq(W.prompt[:n])
        other = np.concatenate([W.prompt[:m], (W.prompt[m:n] + 501) % W.cfg.vocab]).astype(np.int32)
        assert not np.array_equal(other[m:], first[m:n])
        toks, ref, u = W.seq(other)
        dec.reset()
        dec.feed(first[:n])
        dec.prefill(n, with_logits=True, digits=2)
        before = snapshot(dec, W, kv16)
        dec.rewind(m)
        assert dec.position() == m
        assert same_bytes(snapshot(dec, W, kv16), before), f"{what}: rewind changed a cache byte"
        dec.feed(toks[m:])
        dec.extend(n - m, with_logits=True, digits=2)
        assert dec.position() == n, what
        snap = snapshot(dec, W, kv16)
        check_untouched(snap, before, m, n, what)
        check_values(W, snap, ref, u, kv16, slice(0, n), "rewind + extend", what)
        steps(W, dec, toks, ref, u, kv16, n, "rewind + extend", what)
    dec.close()


# ---- score(n), extend at position 0 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_score_and_extend_at_zero_are_prefill(pkg, hip, worlds, case):
    model, fmt, kv16 = case
    W = worlds(model, fmt)
    dec = W.decoder(pkg, kv16)
    for n in LENGTHS:
        toks, ref, u = W.seq(W.prompt[:n])
        dec.reset()
        dec.feed(toks)
        dec.prefill(n, with_logits=True, digits=2)
        want, logits, hist = snapshot(dec, W, kv16), dec.last_logits().copy(), dec.history(n + 1).copy()
        # extend(n) at position 0 "IS prefill"
        dec.reset()
        dec.feed(toks)
        dec.extend(n, with_logits=True, digits=2)
        assert same_bytes(snapshot(dec, W, kv16), want, slice(0, n)), f"extend({n}) at position 0: other cache bytes than prefill({n})"
        assert np.array_equal(dec.last_logits(), logits)
        # score(n): the cache, position, history and last logits of prefill(n, with_logits=True)
        dec.reset()
        dec.feed(toks[:n])
        res = dec.score(n, digits=2)
        assert np.isfinite(res.nll).all()
        snap = snapshot(dec, W, kv16)
        assert same_bytes(snap, want, slice(0, n)), f"score({n}): other cache bytes than prefill({n})"
        assert dec.position() == n and np.array_equal(dec.last_logits(), logits)
        assert np.array_equal(dec.history(n), hist[:n])
        check_values(W, snap, ref, u, kv16, slice(0, n), "score", f"score({n})")
        dec.feed(toks[n:])  # (the pick sits unconsumed at history[n]: feed() writes the reference's token onto that slot)
        steps(W, dec, toks, ref, u, kv16, n, "score", f"score({n})")
    dec.close()


# ---- an f16 cache against the f32 cache of the same fill ----------------------------------------------------------------------
@pytest.mark.parametrize("model,fmt", [(m, f) for m in ("A", "B") for f in ("i2s", "qk256")])
def test_layer_0_of_an_f16_cache_is_the_f32_cache_rounded(pkg, hip, worlds, model, fmt):
    """layer 0's q | k | v rows do not depend on the cache type: the f16 cache holds them within one f16 ulp of the f32 cache's"""
    W = worlds(model, fmt)
    d32, d16 = W.decoder(pkg, False), W.decoder(pkg, True)
    for n in (65, 256):
        toks, _, _ = W.seq(W.prompt[:n])
        for d in (d32, d16):
            d.reset()
            d.feed(toks)
            d.prefill(n, with_logits=True, digits=2)
        (k32, v32), (k16, v16) = kv.caches(d32, W.cfg, 0, False), kv.caches(d16, W.cfg, 0, True)
        for a, b in ((k32, k16), (v32, v16)):
            a, b = a[:n].astype(np.float64), b[:n].astype(np.float64)
            ulp = np.spacing(np.abs(a).astype(np.float16)).astype(np.float64)
            assert np.all(np.abs(a - b) <= ulp), float(np.max(np.abs(a - b) / ulp))
    d32.close()
    d16.close()


# ---- prefill_sharded: rank threads on one GPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sharded_prefill_leaves_every_rank_the_same_cache(pkg, hip, worlds, case, world):
    import torch

    model, fmt, kv16 = case
    W = worlds(model, fmt)
    n = 256
    toks, ref, u = W.seq(W.prompt[:n])
    tp_mod = importlib.import_module("bitnet-rs_amd.prefill_parallel")
    decs = [W.decoder(pkg, kv16) for _ in range(world)]
    for d in decs:
        d.feed(toks)
    slots, bar, errors = [None] * world, threading.Barrier(world), []

    def gather_for(rank):  # tests/test_prefill_parity.py::test_cpp_sharded_prefill_two_ranks_one_gpu
        def gather(send, recv, nbytes, stream):
            torch.cuda.synchronize()
            slots[rank] = torch.as_tensor(tp_mod._DevBytes(send, nbytes), device="cuda").clone()
            bar.wait(timeout=60)
            torch.as_tensor(tp_mod._DevBytes(recv, nbytes * world), device="cuda").copy_(torch.cat(slots))
            torch.cuda.synchronize()
            bar.wait(timeout=60)
            return 0
        return gather

    def run(rank):
        try:
            decs[rank].prefill_sharded(n, rank, world, gather_for(rank) if world > 1 else None, with_logits=True, digits=3, wire_f16=False)
        except Exception as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    snaps = [snapshot(d, W, kv16) for d in decs]
    for r, (d, snap) in enumerate(zip(decs, snaps)):
        what = f"prefill_sharded({n}, rank {r} of {world})"
        assert d.position() == n
        check_values(W, snap, ref, u, kv16, slice(0, n), f"sharded world {world}", what)
        check_finite_tail(snap, n, what)
        assert same_bytes(snap, snaps[0], slice(0, n)), f"{what}: other cache bytes than rank 0"
    steps(W, decs[-1], toks, ref, u, kv16, n, f"sharded world {world}", f"prefill_sharded({n}, world {world}), last rank")
    for d in decs:
        d.close()
