"""GPU parity of continuing a LIVE sequence: bitnet_hip_attention_extend_dev (seq_len new tokens over a cache that holds
past_len positions; k_extend_prep + k_prefill_attn) against the float64 restatement tests/extend_ref.py and against the
one-shot prompt attention, and Decoder::extend / Decoder::rewind against the CPU oracle's token-by-token model.

Gates are the project's own for the same f16 operand rounding (tests/test_prefill_parity.py: max|diff| <= 6e-3, cosine >=
0.999995, or >= 0.99999 beyond 2000 keys; 2e-4 of max|base| between two launches that split the keys differently; logits
cosine >= 0.9999 against the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402
import sampler_accept as sa  # noqa: E402
import sampler_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

D = 128
CACHE_F16, OUT_F16 = 1, 2


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module("bitnet-rs_amd.synth")


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


# ---- the operator --------------------------------------------------------------------------------------------------------
class Op:
    """one (heads, kv, max_pos, cache type) instance of the operator with its caches on the device"""

    def __init__(self, hip, oracle, torch_, n_heads, n_kv, max_pos, f16, theta=10000.0):
        self.hip, self.t, self.n_heads, self.n_kv, self.max_pos, self.f16 = hip, torch_, n_heads, n_kv, max_pos, f16
        sin, cos = oracle.rope_tables(D, max_pos, theta)
        self.sin, self.cos = sin.reshape(max_pos, D // 2).astype(np.float64), cos.reshape(max_pos, D // 2).astype(np.float64)
        self.sin_d, self.cos_d = self.dev(sin), self.dev(cos)
        self.elems = n_kv * er.chunks(max_pos) * 64 * D
        dt = torch_.float16 if f16 else torch_.float32
        self.kc, self.vc = torch_.zeros(self.elems, dtype=dt, device="cuda"), torch_.zeros(self.elems, dtype=dt, device="cuda")

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

    def rows(self, a, misalign=False):
        """-> (the tensor that owns the rows, their device pointer); misalign: 4 bytes off a 16-byte boundary, where the query image comes
        from the prep launch instead of the attention kernel's own f32 reads (tests/test_attention_packed_gpu.py Pack.call)"""
        if not misalign:
            buf = self.dev(a)
            return buf, buf.data_ptr()
        buf = self.t.zeros(a.size + 1, dtype=self.t.float32, device="cuda")
        buf[1:] = self.dev(a).ravel()
        return buf, buf.data_ptr() + 4

    def prefill(self, qkv, kc=None, vc=None):
        """the one-shot prompt operator over all rows of qkv (fresh sequence)"""
        T = qkv.shape[0]
        wsb = self.hip.attention_prefill_workspace_bytes(self.n_heads, self.n_kv, T)
        ws = self.t.empty(wsb, dtype=self.t.uint8, device="cuda")
        out = self.t.full((T, self.n_heads * D), float("nan"), device="cuda")
        kc, vc = (self.kc, self.vc) if kc is None else (kc, vc)
        if self.f16:
            self.hip.attention_prefill_flags_dev(self.dev(qkv), self.sin_d, self.cos_d, kc, vc, self.n_heads, self.n_kv, D, self.max_pos, T, ws, wsb, out, CACHE_F16)
        else:
            self.hip.attention_prefill_dev(self.dev(qkv), self.sin_d, self.cos_d, kc, vc, self.n_heads, self.n_kv, D, self.max_pos, T, ws, wsb, out)
        self.t.cuda.synchronize()
        return out.cpu().numpy()

    def extend(self, qkv_new, past, out_f16=False, misalign=False):
        n = qkv_new.shape[0]
        buf, q_ptr = self.rows(qkv_new, misalign)
        wsb = self.hip.attention_extend_workspace_bytes(self.n_heads, self.n_kv, past, n)
        assert wsb > 0
        ws = self.t.full((wsb,), 0xFF, dtype=self.t.uint8, device="cuda")  # NaN patterns: nothing the call did not write may be read
        out = self.t.full((n, self.n_heads * D), float("nan"), dtype=self.t.float16 if out_f16 else self.t.float32, device="cuda")
        self.hip.attention_extend_dev(q_ptr, self.sin_d, self.cos_d, self.kc, self.vc, self.n_heads, self.n_kv, D, self.max_pos, past, n, ws, wsb,
                                      out, (CACHE_F16 if self.f16 else 0) | (OUT_F16 if out_f16 else 0))
        self.t.cuda.synchronize()
        return out.float().cpu().numpy()

    def caches(self):
        """-> (k [C * 64, kv, D], v [C * 64, kv, D]) as the cache's own dtype"""
        return er.decode_k(self.kc.cpu().numpy(), self.n_kv, self.max_pos, self.f16), er.decode_v(self.vc.cpu().numpy(), self.n_kv, self.max_pos, self.f16)

    def put_garbage_from(self, pos, rng):
        """large finite values into every slot at positions >= pos (what a longer, rewound sequence could have left, and worse)"""
        k, v = self.caches()
        big = 3.0e4 if self.f16 else 1.0e30  # finite in the cache's type; as f16 operands the f32 ones would be inf -> NaN
        k[pos:] = (big * rng.choice([-1.0, 1.0], k[pos:].shape)).astype(k.dtype)
        v[pos:] = (big * rng.choice([-1.0, 1.0], v[pos:].shape)).astype(v.dtype)
        dt = self.t.float16 if self.f16 else self.t.float32
        self.kc = self.t.from_numpy(er.encode_k(k, er.chunks(self.max_pos) * 64, self.f16)).to(dt).cuda()
        self.vc = self.t.from_numpy(er.encode_v(v, er.chunks(self.max_pos) * 64, self.f16)).to(dt).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def unsplit(T):
    """both the one-shot and the continuation launch walk all key tiles in ONE workgroup per query block (no key split): up to 16 tiles"""
    return T <= 1024


CASES = [(64, 64, 4, 2, 512), (37, 1, 4, 2, 512), (100, 27, 4, 4, 512), (1, 200, 20, 5, 512), (333, 300, 8, 2, 1024), (2047, 130, 20, 5, 2304),
         (4000, 64, 20, 5, 4096)]


def run_case(hip, oracle, torch_, past, n, n_heads, n_kv, max_pos, f16, fill, stale):
    T = past + n
    rng = np.random.default_rng(1000 * past + n + (7 if f16 else 0))
    qkv = rng.normal(0, rng.uniform(1.2, 1.5), (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    op = Op(hip, oracle, torch_, n_heads, n_kv, max_pos, f16)
    # ---- the past: one whole-prompt call, or a chain of continuations from an empty cache ----
    if fill == "prefill":
        op.prefill(qkv[:past])
    else:
        cuts = np.unique(np.concatenate([[0, past], rng.integers(1, max(past, 2), 3)]))
        cuts = cuts[cuts <= past]
        for a, b in zip(cuts[:-1], cuts[1:]):
            got = op.extend(qkv[a:b], int(a))
            assert np.isfinite(got).all()
    if stale:
        op.put_garbage_from(past, rng)
    k0, v0 = op.caches()
    got = op.extend(qkv[past:], past).reshape(n, n_heads, D)
    k1, v1 = op.caches()
    # ---- against float64 ----
    pos = np.arange(T)
    _, k_all, v_all = er.split_qkv(qkv, n_heads, n_kv)
    k_all = er.rope_np(k_all, op.sin[pos, None, :], op.cos[pos, None, :])
    want, _, _ = er.extend_f64(qkv[past:], k_all[:past], v_all[:past], n_heads, n_kv, op.sin, op.cos)
    assert not np.isnan(got).any()
    err, c = float(np.max(np.abs(got - want))), cosine(got, want)
    print(f"extend past={past} n={n} heads={n_heads}/{n_kv} f16={f16} fill={fill} stale={stale}: max|diff| {err:.3e} cosine {c:.8f}")
    assert err <= 6e-3, err
    assert c >= (0.99999 if T > 2000 else 0.999995), c
    # ---- the caches ----
    v_new = qkv[past:, (n_heads + n_kv) * D:].reshape(n, n_kv, D)
    assert np.array_equal(v1[past:T], v_new.astype(np.float16) if f16 else v_new)
    kn = k_all[past:T]
    if f16:
        ulp = np.spacing(np.abs(kn).astype(np.float16)).astype(np.float64)
        assert np.all(np.abs(k1[past:T].astype(np.float64) - kn) <= ulp)  # one f16 rounding of the rotated key
    else:
        assert np.all(np.abs(k1[past:T].astype(np.float64) - kn) <= 2e-6 * np.abs(kn).max())
    assert np.array_equal(bits(k1[:past]), bits(k0[:past])) and np.array_equal(bits(v1[:past]), bits(v0[:past]))  # the past is not rewritten
    assert np.array_equal(bits(k1[T:]), bits(k0[T:])) and np.array_equal(bits(v1[T:]), bits(v0[T:]))              # nor anything beyond
    return op, qkv, got


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("past,n,n_heads,n_kv,max_pos", CASES)
def test_extend_matches_f64_and_the_one_shot_prompt(hip, oracle, torch_, past, n, n_heads, n_kv, max_pos, f16):
    fill = "chain" if past in (37, 100, 333) else "prefill"  # the past: a chain of continuations from an empty cache | one whole-prompt call
    op, qkv, got = run_case(hip, oracle, torch_, past, n, n_heads, n_kv, max_pos, f16, fill, stale=False)
    # ---- against the rows [past, past + n) of the one-shot prompt over all past + n tokens ----
    T = past + n
    dt = torch_.float16 if f16 else torch_.float32
    kc2, vc2 = torch_.zeros(op.elems, dtype=dt, device="cuda"), torch_.zeros(op.elems, dtype=dt, device="cuda")
    base = op.prefill(qkv, kc2, vc2)
    rows = base[past:].reshape(n, n_heads, D)
    d = float(np.max(np.abs(got - rows)))
    same = np.array_equal(got, rows)
    print(f"  vs one-shot rows: max|diff| {d:.3e} of max|base| {np.max(np.abs(base)):.3f}, bit-equal {same}")
    assert d <= 2e-4 * np.max(np.abs(base))
    if unsplit(T):
        # both launches walk every key tile of a query block in one workgroup, on identical f16 operands (a past key goes cache -> f16:
        # the bits the one-shot preparation's f16 of the exact value has), in the same order: the same bits
        assert same
        # ... and they leave the same cache (the same RoPE arithmetic, the same single rounding)
        assert torch_.equal(op.kc.view(torch_.int16 if f16 else torch_.int32), kc2.view(torch_.int16 if f16 else torch_.int32))
        assert torch_.equal(op.vc.view(torch_.int16 if f16 else torch_.int32), vc2.view(torch_.int16 if f16 else torch_.int32))


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("past,n,n_heads,n_kv,max_pos", [(37, 1, 4, 2, 512), (100, 27, 4, 4, 512), (333, 300, 8, 2, 1024), (2047, 130, 20, 5, 2304)])
def test_stale_slots_beyond_the_past_are_never_read(hip, oracle, torch_, past, n, n_heads, n_kv, max_pos, f16):
    """every slot at positions >= past holds large finite garbage before the call (f32: 1e30, an infinity as an f16 operand): the outputs meet
    the same gates, the new positions are overwritten, everything beyond past + n keeps its garbage bit for bit"""
    run_case(hip, oracle, torch_, past, n, n_heads, n_kv, max_pos, f16, "prefill", stale=True)


def test_f16_output_rows_and_a_reused_workspace(hip, oracle, torch_):
    """BITNET_HIP_ATTN_OUT_F16: the same rows rounded once to f16 (what the o-projection's f16 chain reads)"""
    past, n, n_heads, n_kv, max_pos = 130, 70, 20, 5, 256
    rng = np.random.default_rng(5)
    qkv = rng.normal(0, 1.3, (past + n, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    for f16 in (False, True):
        op = Op(hip, oracle, torch_, n_heads, n_kv, max_pos, f16)
        op.prefill(qkv[:past])
        a = op.extend(qkv[past:], past)
        b = op.extend(qkv[past:], past, out_f16=True)  # the same positions again: a repeat rewrites only the new slots, with the same values
        # the kernel rounds o / l to f16 ONCE (a fused multiply-convert), numpy rounds the f32 row a second time: half an f16 ulp + an f32 ulp
        half_ulp = 0.5 * np.spacing(np.abs(a).astype(np.float16)).astype(np.float64)
        assert np.all(np.abs(b.astype(np.float64) - a) <= half_ulp + 2.0 ** -23 * np.abs(a))
    with pytest.raises(Exception, match="KV cache overflow"):
        op.extend(qkv[:60], 200)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("past,n,n_heads,n_kv", [(37, 70, 4, 2), (64, 65, 3, 3)])
def test_misaligned_rows_take_the_query_prep_launch(hip, oracle, torch_, past, n, n_heads, n_kv, f16):
    """q|k|v rows 4 bytes off a 16-byte boundary: k_extend_prep reads them element by element and the query image comes from k_prefill_prep's
    query slabs at the positions k_extend_prep wrote.  The operator's gates against float64 (6e-3, cosine 0.9999), 2e-4 of max|aligned|
    against the aligned call on the same values, and the same caches bit for bit."""
    max_pos, T = 512, past + n
    rng = np.random.default_rng(100 * past + n + (7 if f16 else 0))
    qkv = rng.normal(0, 1.3, (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    outs, ops = [], []
    for misalign in (False, True):
        op = Op(hip, oracle, torch_, n_heads, n_kv, max_pos, f16)
        op.prefill(qkv[:past])
        outs.append(op.extend(qkv[past:], past, misalign=misalign).reshape(n, n_heads, D))
        ops.append(op)
    aligned, got = outs
    pos = np.arange(T)
    _, k_all, v_all = er.split_qkv(qkv, n_heads, n_kv)
    k_all = er.rope_np(k_all, ops[0].sin[pos, None, :], ops[0].cos[pos, None, :])
    want, _, _ = er.extend_f64(qkv[past:], k_all[:past], v_all[:past], n_heads, n_kv, ops[0].sin, ops[0].cos)
    assert np.isfinite(got).all()
    err, c, d = float(np.max(np.abs(got - want))), cosine(got, want), float(np.max(np.abs(got - aligned)))
    print(f"misaligned extend past={past} n={n} heads={n_heads}/{n_kv} f16={f16}: max|diff| vs f64 {err:.3e} cosine {c:.8f}; "
          f"vs aligned {d:.3e} of max|aligned| {np.max(np.abs(aligned)):.3f}")
    assert err <= 6e-3 and c >= 0.9999
    assert d <= 2e-4 * np.max(np.abs(aligned))
    iv = torch_.int16 if f16 else torch_.int32
    assert torch_.equal(ops[1].kc.view(iv), ops[0].kc.view(iv)) and torch_.equal(ops[1].vc.view(iv), ops[0].vc.view(iv))


# ---- the decoder ---------------------------------------------------------------------------------------------------------
SMALL = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=160, eps=1e-5, rope_theta=10000.0)
WIDE = dict(hidden=2560, n_layers=2, n_heads=20, n_kv_heads=5, head_dim=128, ffn=6912, vocab=4096, max_pos=160, eps=1e-5, rope_theta=500000.0)
WIDE4K = dict(WIDE, max_pos=4224)  # tests/test_bench_prefill_instance.py


def models(synth, fmt, cfg):
    glob = synth.make_globals(cfg)
    if fmt == "qk256":
        layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
        return glob, layers, layers
    layers = [synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
    tmap = np.array([0, 1, 0, -1], np.float32)
    olayers = []
    for lay in layers:
        d = {"attn_norm": lay["attn_norm"], "ffn_norm": lay["ffn_norm"], "dense": True}
        for name, (rows, cols) in cfg.shapes().items():
            pk = lay[name].reshape(rows, cols // 4)
            codes = np.stack([(pk >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(rows, cols)
            d[name] = tmap[codes] * np.repeat(lay[name + "_scales"].reshape(rows, cols // 32), 32, axis=1)
        olayers.append(d)
    return glob, layers, olayers


def make_decoder(pkg, cfg, fmt, layers, glob, kv16=False):
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w) if fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
    dec.set_globals(glob)
    dec.reset()
    dec.set_kv_f16(kv16)
    return dec


def oracle_walk(oracle, om, forced, n_greedy, logits_at=()):
    """the oracle's token-by-token model over `forced`, then greedy: -> (sequence of len(forced) + n_greedy tokens, the logits behind each
    greedy token, {position: logits} for the forced positions asked for)"""
    om.reset()
    seq, o_logits, extra = [int(t) for t in forced], [], {}
    n = len(forced)
    for p in range(n + n_greedy - 1):
        want = p >= n - 1 or p in logits_at
        _, logits, _ = om.step(seq[p], want_logits=want)
        if p in logits_at:
            extra[p] = logits.copy()
        if p >= n - 1:
            o_logits.append(logits.copy())
            seq.append(oracle.argmax(logits))
    return seq, o_logits, extra


def check_tail(dec, oracle_logits, seq, n_forced, what):
    """the with-logits step that just ran + the remaining greedy steps against the oracle's logits; then the whole history"""
    n_new = len(oracle_logits)
    for i in range(n_new):
        if i:
            dec.run(1, with_logits=True, use_graph=True)
        c = cosine(dec.last_logits(), oracle_logits[i])
        assert c >= 0.9999, (what, i, c)
        assert dec.position() == n_forced + i
    assert list(dec.history(n_forced + n_new)) == [int(t) for t in seq], what


AB = [(70, 37), (21, 64), (33, 1), (64, 64), (0, 50)]


@pytest.mark.parametrize("kv16", [False, True])
@pytest.mark.parametrize("cfgd,fmt", [(SMALL, "qk256"), (SMALL, "i2s"), (WIDE, "qk256"), (WIDE, "i2s")])
def test_prefill_extend_then_decode_matches_oracle(pkg, oracle, synth, cfgd, fmt, kv16):
    cfg = synth.ModelConfig(**cfgd)
    glob, layers, olayers = models(synth, fmt, cfg)
    om = oracle.OracleModel(cfg, olayers, glob, n_threads=16)
    dec = make_decoder(pkg, cfg, fmt, layers, glob, kv16)
    for a, b in AB:
        prompt = synth.prompt(a + b, cfg.vocab)
        seq, o_logits, _ = oracle_walk(oracle, om, prompt, 4)  # the token behind the prompt + 3 greedy steps
        # digits = 4 once, for the layer loop without the f16 hand-over (f32 attention rows)
        for digits in ((2, 4) if (a, b) == (70, 37) else (2,)):
            dec.reset()
            # the block-scaled format at 4 digits: where the oracle's two best logits behind the prompt lie closer than one f16 rounding of their
            # value (2^-11: the tied head multiplies f16 operands), the pick is not decidable and that ONE pick is forced to the oracle's, so that
            # the steps compare one sequence.  SMALL at 107 rows: 73.09796 / 73.09398, 5.4e-5 apart; the 2-digit chain picks the oracle's token,
            # the 3- / 4-digit planes the other one, on caches that agree with float64 slot by slot (EXPERIMENTS 12.3)
            top = np.sort(o_logits[0])[-2:]
            tie = fmt == "i2s" and digits == 4 and top[1] - top[0] <= 2.0 ** -11 * abs(top[1])
            dec.feed(seq[:a + b + 1] if tie else prompt)
            if a:
                dec.prefill(a, with_logits=False, digits=digits)
                assert dec.position() == a
            dec.extend(b, with_logits=True, digits=digits)
            assert dec.position() == a + b
            check_tail(dec, o_logits, seq, a + b, (a, b, digits))
    # three continuations in a row (30 + 30 + 30), the middle one with logits nobody uses: feed() puts nothing new, the next call overwrites the pick
    prompt = synth.prompt(90, cfg.vocab)
    seq, o_logits, extra = oracle_walk(oracle, om, prompt, 4, logits_at=(59,))
    dec.reset()
    dec.feed(prompt)
    dec.extend(30, with_logits=False)
    assert dec.position() == 30
    dec.extend(30, with_logits=True)
    assert dec.position() == 60 and cosine(dec.last_logits(), extra[59]) >= 0.9999
    assert list(dec.history(60)) == [int(t) for t in prompt[:60]]  # (position 60 is forced: the pick did not replace it)
    assert int(dec.history(61)[60]) == int(prompt[60])
    dec.extend(30, with_logits=True)
    check_tail(dec, o_logits, seq, 90, "30+30+30")
    dec.close()
    om.close()


@pytest.mark.parametrize("kv16", [False, True])
@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
def test_chat_shape_and_rewind_match_oracle(pkg, oracle, synth, fmt, kv16):
    cfg = synth.ModelConfig(**SMALL)
    glob, layers, olayers = models(synth, fmt, cfg)
    om = oracle.OracleModel(cfg, olayers, glob, n_threads=8)
    dec = make_decoder(pkg, cfg, fmt, layers, glob, kv16)
    # ---- chat: a prompt, an answer of 5 greedy tokens, then a second turn of 20 tokens behind the answer ----
    first, turn = synth.prompt(40, cfg.vocab), [int(t) for t in synth.prompt(61, cfg.vocab)[41:]]
    dec.feed(first)
    dec.prefill(40, with_logits=True, digits=2)
    dec.run(4, with_logits=True)  # the prefill picked answer token 1; four steps pick 2 .. 5
    assert dec.position() == 44
    answer = [int(t) for t in dec.history(45)[40:]]
    # the 5th answer token sits unconsumed at history[44]; feed() writes at max(position, fed) = 44: fed again in front of the new tokens
    dec.feed([answer[-1]] + turn)
    assert list(dec.history(45 + 20)) == [int(t) for t in first] + answer + turn
    dec.extend(21, with_logits=True, digits=2)
    assert dec.position() == 65
    seq, o_logits, extra = oracle_walk(oracle, om, list(first) + answer + turn, 4, logits_at=(39, 43))
    assert answer[0] == oracle.argmax(extra[39]) and answer[4] == oracle.argmax(extra[43])  # the decoder's own answer is the oracle's greedy one
    check_tail(dec, o_logits, seq, 65, "chat")
    # ---- rewind: drop B, continue A with C ----
    A, B, C_ = synth.prompt(50, cfg.vocab), synth.prompt(90, cfg.vocab)[50:], [int(t) for t in synth.prompt(140, cfg.vocab)[100:131]]
    dec.reset()
    dec.feed(list(A) + list(B))
    dec.prefill(90, with_logits=True, digits=2)
    assert dec.position() == 90
    dec.rewind(50)
    assert dec.position() == 50 and dec._fed == 50
    dec.feed(C_)
    assert list(dec.history(50 + len(C_))) == [int(t) for t in A] + C_
    dec.extend(len(C_), with_logits=True, digits=2)
    assert dec.position() == 50 + len(C_)
    seq, o_logits, _ = oracle_walk(oracle, om, list(A) + C_, 4)
    check_tail(dec, o_logits, seq, 50 + len(C_), "rewind")
    # rewind to where we are is a no-op; to 0 it makes prefill possible again (reset() stays the full clear)
    p = dec.position()
    dec.rewind(p)
    assert dec.position() == p
    dec.rewind(0)
    assert dec.position() == 0
    dec.feed(A)
    dec.prefill(50, with_logits=False, digits=2)
    assert dec.position() == 50
    dec.close()
    om.close()


def test_guards(pkg, synth):
    cfg = synth.ModelConfig(**dict(SMALL, max_pos=64))
    glob, layers, _ = models(synth, "qk256", cfg)
    dec = make_decoder(pkg, cfg, "qk256", layers, glob)
    prompt = synth.prompt(40, cfg.vocab)
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.extend(4)
    dec.feed(prompt)
    # at position 0 extend IS prefill
    dec.extend(40, with_logits=True, digits=2)
    a, tok_a = dec.last_logits().copy(), int(dec.history(41)[40])
    dec.reset()
    dec.feed(prompt)
    dec.prefill(40, with_logits=True, digits=2)
    assert np.array_equal(dec.last_logits(), a) and int(dec.history(41)[40]) == tok_a
    with pytest.raises(pkg.BitNetHipError, match="fresh sequence"):
        dec.prefill(4)
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.extend(1)  # nothing fed beyond the position (the picked token is not a fed one)
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.extend(0)
    dec.feed(synth.prompt(24, cfg.vocab))  # 40 .. 63: fills the history to max_pos
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.extend(25)
    with pytest.raises(pkg.BitNetHipError, match="KV cache overflow"):
        dec.extend(24)  # 40 + 24 > max_pos - 1
    dec.extend(23, with_logits=True)
    assert dec.position() == 63
    with pytest.raises(pkg.BitNetHipError, match="rewind"):
        dec.rewind(64)
    with pytest.raises(pkg.BitNetHipError, match="rewind"):
        dec.rewind(-1)
    dec.rewind(10)
    assert dec.position() == 10
    dec.close()


def test_sampled_continuation_draws_one_word(pkg, synth):
    cfg = synth.ModelConfig(**SMALL)
    glob, layers, _ = models(synth, "qk256", cfg)
    dec = make_decoder(pkg, cfg, "qk256", layers, glob)
    a, b = 33, 27
    prompt = synth.prompt(a + b, cfg.vocab)
    conf = (0.8, 40, 0.9, 1.1)
    dec.set_sampling(*conf, seed=9)
    ref = sr.RefSampler(*conf, seed=9)
    dec.reset()
    dec.feed(prompt)
    dec.prefill(a, with_logits=False, digits=2)
    assert dec.sampling_draws() == 0
    dec.extend(b, with_logits=True, digits=2)
    assert dec.sampling_draws() == 1 and dec.position() == a + b
    got = int(dec.history(a + b + 1)[a + b])
    want = ref.sample(dec.last_logits(), [])  # nothing generated yet: forced tokens are not counted
    ok, reason = sa.accepts(ref, got)
    assert ok, (got, want, reason)
    assert list(dec.history(a + b)) == [int(t) for t in prompt]
    dec.close()


@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
def test_long_context_on_the_benchmarked_tiles(pkg, hip, oracle, synth, fmt):
    """prefill(2048) + extend(2048) at the 2B-4T widths (2 layers), digits = 2, then 2 decode steps at 4097 / 4098 keys: against the oracle
    walking the 4096 tokens once; f16 KV cache both formats, f32 once.  The continuation takes the chain prefill takes at 2048 rows."""
    cfg = synth.ModelConfig(**WIDE4K)
    glob, layers, olayers = models(synth, fmt, cfg)
    T, half = 4096, 2048
    om = oracle.OracleModel(cfg, olayers, glob, n_threads=16)
    seq, o_logits, _ = oracle_walk(oracle, om, synth.prompt(T, cfg.vocab), 3)
    om.close()
    dec = make_decoder(pkg, cfg, fmt, layers, glob)
    for kv16 in ((True, False) if fmt == "qk256" else (True,)):
        dec.reset()
        dec.set_kv_f16(kv16)
        dec.feed(seq)  # every token forced to the oracle's
        dec.prefill(half, with_logits=False, digits=2)
        path = dec.last_prefill_path()
        dec.extend(half, with_logits=True, digits=2)
        assert dec.last_prefill_path() == path == (0 if fmt == "qk256" else 1)
        assert dec.position() == T
        check_tail(dec, o_logits, seq, T, (fmt, kv16))
    dec.close()
