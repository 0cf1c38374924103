"""GPU parity of the decode step against the CPU oracle's
restatement of the reference transformer (oracle/transformer_oracle.c):
operators one by one, then whole tokens through the C++ host loop (eager and as a
captured hipGraph), greedy tokens identical and per-token logits cosine >= 0.9999
(north_star bar: >= 0.99)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module("bitnet-rs_amd.synth")


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def test_norm_rows(hip, oracle, torch_):
    """LayerNorm without bias, with mean subtraction (T:67-100) and the RMSNorm of
    K/rocm/rmsnorm.rs; reference-style checks: constant row -> 0 (LN), scale invariance."""
    rng = np.random.default_rng(0)
    for hidden in (64, 512, 2560, 6912):
        x = (rng.normal(0.3, 2.0, (3, hidden))).astype(np.float32)
        g = rng.uniform(0.5, 1.5, hidden).astype(np.float32)
        xd, gd = torch_.from_numpy(x).cuda(), torch_.from_numpy(g).cuda()
        for rms in (False, True):
            od = torch_.empty_like(xd)
            hip.norm_rows_dev(xd, gd, od, 3, hidden, 1e-5, rms)
            torch_.cuda.synchronize()
            got = od.cpu().numpy()
            for r in range(3):
                want = oracle.rmsnorm(x[r], g, 1e-5) if rms else oracle.layernorm(x[r], g, 1e-5)
                assert np.allclose(got[r], want, rtol=2e-5, atol=2e-6), (hidden, rms)
        # host-pointer stub signature (K/rocm/rmsnorm.rs:50-60), default eps 1e-6
        got = hip.rmsnorm(x, g, 3, hidden, 1e-6).reshape(3, hidden)
        assert np.allclose(got[1], oracle.rmsnorm(x[1], g, 1e-6), rtol=2e-5, atol=2e-6)
    with pytest.raises(Exception, match="buffer too small"):
        hip.rmsnorm(np.ones(10, np.float32), np.ones(64, np.float32), 1, 64)


def test_embed_and_argmax(hip, torch_):
    rng = np.random.default_rng(1)
    vocab, hidden = 1000, 512
    table = rng.normal(0, 1, (vocab, hidden)).astype(np.float16)
    toks = np.array([0, 999, 17, 17, 500], np.int32)
    td = torch_.from_numpy(table.view(np.int16)).cuda()
    out = torch_.empty(5, hidden, device="cuda")
    hip.embed_f16_dev(td, torch_.from_numpy(toks).cuda(), out, 5, hidden, vocab)
    torch_.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), table[toks].astype(np.float32))  # f16 -> f32 is exact
    # argmax: lowest index on ties, NaN ignored (crates/bitnet-cli/src/sampling.rs:45-49,189-202)
    v = rng.normal(0, 1, 128256).astype(np.float32)
    v[[77, 4000, 100000]] = 9.5
    v[5] = np.nan
    scratch = torch_.empty(2 * 256, dtype=torch_.float32, device="cuda")
    tok = torch_.zeros(1, dtype=torch_.int32, device="cuda")
    hip.argmax_dev(torch_.from_numpy(v).cuda(), v.size, scratch, 256, tok)
    torch_.cuda.synchronize()
    assert int(tok.item()) == 77
    allnan = np.full(300, np.nan, np.float32)
    hip.argmax_dev(torch_.from_numpy(allnan).cuda(), 300, scratch, 4, tok)
    torch_.cuda.synchronize()
    assert int(tok.item()) == 0  # every value -inf: best_idx stays 0


def test_fused_gemv_ln_residual_silu(hip, pkg, oracle, torch_):
    """LN prologue, residual epilogue and silu(gate)*up epilogue of the fused GEMV vs the
    unfused oracle chain (T:1015 -> T:288, T:1073, T:756-781)."""
    rng = np.random.default_rng(2)
    K, N = 2560, 1280
    stride = K // 256 * 64
    qa = rng.integers(0, 256, N * stride, dtype=np.uint8)
    qb = rng.integers(0, 256, N * stride, dtype=np.uint8)
    x = rng.normal(0.1, 1.0, K).astype(np.float32)
    g = (rng.uniform(0.5, 1.5, K) / 80).astype(np.float32)
    res = rng.normal(0, 1, N).astype(np.float32)
    ha, hb = hip.weights_upload_qk256(qa, N, K, stride), hip.weights_upload_qk256(qb, N, K, stride)
    xd, gd, rd = (torch_.from_numpy(a).cuda() for a in (x, g, res))
    xn = oracle.layernorm(x, g, 1e-5)
    ya = oracle.gemv_qk256(qa, xn, N, K, stride)
    yb = oracle.gemv_qk256(qb, xn, N, K, stride)
    tol = lambda want: 3e-5 * np.max(np.abs(want)) + 1e-6
    # LN + residual
    yd = torch_.empty(N, device="cuda")
    hip.gemv_fused_dev(ha, xd, yd, 1, ln_gamma=gd, ln_eps=1e-5, residual=rd)
    torch_.cuda.synchronize()
    assert np.max(np.abs(yd.cpu().numpy() - (ya + res))) <= tol(ya)
    # concat (q|k|v style): rows of a then rows of b
    hc = hip.weights_concat([ha, hb])
    yc = torch_.empty(2 * N, device="cuda")
    hip.gemv_fused_dev(hc, xd, yc, 1, ln_gamma=gd, ln_eps=1e-5)
    torch_.cuda.synchronize()
    assert np.max(np.abs(yc.cpu().numpy() - np.concatenate([ya, yb]))) <= tol(ya)
    # interleaved gate/up + silu*mul
    hg = hip.weights_concat([ha, hb], interleave16=True)
    assert hip.weights_info(hg)[0] == 2 * N
    yh = torch_.empty(N, device="cuda")
    hip.gemv_fused_dev(hg, xd, yh, 1, ln_gamma=gd, ln_eps=1e-5, flags=1)
    torch_.cuda.synchronize()
    want = (ya / (1 + np.exp(-ya.astype(np.float64)))).astype(np.float32) * yb
    assert np.max(np.abs(yh.cpu().numpy() - want)) <= 3e-5 * np.max(np.abs(want)) + 1e-6
    with pytest.raises(pkg.BitNetHipError, match="FUSE_SILU_MUL"):
        hip.gemv_fused_dev(hc, xd, yh, 1, flags=1)
    for h in (ha, hb, hc, hg):
        hip.weights_free(h)


SMALL = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=64, eps=1e-5, rope_theta=10000.0)
WIDE = dict(hidden=2560, n_layers=2, n_heads=20, n_kv_heads=5, head_dim=128, ffn=6912, vocab=4096, max_pos=48, eps=1e-5, rope_theta=500000.0)
# a query group of 3 (the attention records are combined by their own launch: the merging o-projection takes groups 1, 2, 4) on hidden 1536 (the
# guarded <8, 2> instance of the logits head)
GROUP3 = dict(hidden=1536, n_layers=2, n_heads=12, n_kv_heads=4, head_dim=128, ffn=2048, vocab=2048, max_pos=64, eps=1e-5, rope_theta=10000.0)


@pytest.mark.parametrize("cfgd,n_prompt,n_new", [(SMALL, 5, 12), (WIDE, 4, 6), (GROUP3, 4, 6)])
def test_decode_tokens_match_oracle(hip, pkg, oracle, synth, cfgd, n_prompt, n_new):
    cfg = synth.ModelConfig(**cfgd)
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    prompt = synth.prompt(n_prompt, cfg.vocab)
    om = oracle.OracleModel(cfg, layers, glob, n_threads=8)
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w)
    dec.set_globals(glob)

    # oracle: teacher-forced prompt, then greedy
    seq = list(prompt)
    o_logits, o_hidden = [], []
    for p in range(n_prompt + n_new - 1):
        hid, logits, _ = om.step(seq[p])
        o_logits.append(logits)
        o_hidden.append(hid)
        if p + 1 >= n_prompt:
            seq.append(oracle.argmax(logits))

    for use_graph in (False, True):
        dec.reset()
        dec.feed(prompt)
        cosines = []
        for p in range(n_prompt + n_new - 1):
            dec.run(1, with_logits=True, use_graph=use_graph)
            assert dec.position() == p + 1
            got = dec.last_logits()
            c = cosine(got, o_logits[p])
            cosines.append(c)
            assert c >= 0.9999, (use_graph, p, c)
            assert np.max(np.abs(got - o_logits[p])) <= 2e-3 * np.max(np.abs(o_logits[p])), (use_graph, p)
        hist = dec.history(n_prompt + n_new)
        assert list(hist) == [int(t) for t in seq], (use_graph, hist, seq)
    # prompt positions without logits (prefill path) give the same state
    dec.reset()
    dec.feed(prompt)
    dec.run(n_prompt - 1, with_logits=False, use_graph=True)
    dec.run(1, with_logits=True, use_graph=True)
    assert cosine(dec.last_logits(), o_logits[n_prompt - 1]) >= 0.9999
    assert dec.history(n_prompt + 1)[n_prompt] == seq[n_prompt]
    with pytest.raises(pkg.BitNetHipError, match="KV cache overflow"):
        dec.run(cfg.max_pos, with_logits=False)
    dec.close()
    om.close()


LONG = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=320, eps=1e-5, rope_theta=10000.0)


def test_decode_across_chunk_boundaries_teacher_forced(hip, pkg, oracle, synth):
    """Decode steps of a small model through the step graph, the context growing across the 64-position chunk
    boundaries of the attention (64, 128, 192, 256): per-step logits against the oracle, every token forced to the
    oracle's choice so that a near-tie cannot fork the two sequences."""
    cfg = synth.ModelConfig(**LONG)
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    n_prompt, n_total = 10, 270
    om = oracle.OracleModel(cfg, layers, glob, n_threads=8)
    seq = list(synth.prompt(n_prompt, cfg.vocab))
    o_logits = []
    for p in range(n_total - 1):
        _, logits, _ = om.step(seq[p])
        o_logits.append(logits)
        if p + 1 >= n_prompt:
            seq.append(oracle.argmax(logits))
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w)
    dec.set_globals(glob)
    dec.reset()
    dec.feed(seq)  # all forced
    worst = 1.0
    for p in range(n_total - 1):
        dec.run(1, with_logits=True, use_graph=True)
        c = cosine(dec.last_logits(), o_logits[p])
        worst = min(worst, c)
        assert c >= 0.9999, (p, c)
    assert dec.position() == n_total - 1
    # and the unforced greedy run picks the same tokens
    dec.reset()
    dec.feed(seq[:n_prompt])
    dec.run(n_total - 1, with_logits=True, use_graph=True)
    assert list(dec.history(n_total)) == [int(t) for t in seq], worst
    dec.close()
    om.close()


@pytest.mark.parametrize("max_pos,positions,n_heads,n_kv", [
    (512, [0, 1, 62, 63, 64, 65, 127, 128, 129, 300, 511], 8, 2),
    (512, [0, 63, 64, 200], 4, 2),      # query group of 2
    (512, [5, 64, 191], 3, 3),          # no grouping
    (8192, [0, 100, 3071, 3072, 5000, 8100], 8, 2),
    (512, [0, 63, 64, 127, 128, 200], 6, 2)])   # query group of 3: the fourth RoPE wave has no head of its own
@pytest.mark.parametrize("wide", [False, True])
def test_attention_decode_op_vs_f64(hip, oracle, torch_, max_pos, positions, n_heads, n_kv, wide):
    """One-token attention (RoPE + append + GQA softmax) at many context lengths against a f64 numpy
    reference; max_pos 8192 takes the long-context form (several 64-position chunks per workgroup,
    merged online)."""
    D = 128
    group = n_heads // n_kv
    rng = np.random.default_rng(max_pos + n_heads)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    kc = rng.normal(0, 1, (n_kv, D, max_pos)).astype(np.float32)   # logical [kv][D][pos]; the device keeps 64-position tiles
    tiled = lambda a: np.ascontiguousarray(a.reshape(n_kv, D, max_pos // 64, 64).transpose(0, 2, 1, 3))
    untiled = lambda a: a.reshape(n_kv, max_pos // 64, D, 64).transpose(0, 2, 1, 3).reshape(n_kv, D, max_pos)
    vc = rng.normal(0, 1, (n_kv, max_pos, D)).astype(np.float32)
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a)).cuda()
    sb = hip.c.bitnet_hip_attention_scratch_bytes(n_kv, max_pos)
    scratch = torch_.zeros(sb // 4 + 16, device="cuda")
    sin_d, cos_d = dev(sin), dev(cos)
    for pos in positions:
        qkv = rng.normal(0, 1.5, (n_heads + 2 * n_kv) * D).astype(np.float32)
        kc_in = kc.copy()
        kc_in[:, :, pos:] = np.nan    # slots at / past the new token: stale KEYS may hold anything (their scores are replaced)
        vc_in = vc.copy()
        vc_in[:, pos:] *= 1e30        # stale VALUES only have to be finite (zero-filled-cache contract, include/bitnet_hip.h)
        kcd, vcd = dev(tiled(kc_in)), dev(vc_in)
        out = torch_.full((n_heads * D,), float("nan"), device="cuda")
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        # wide: workgroups of 512 threads over 128 positions (bitnet_hip_attention_decode_wide_dev), same value
        (hip.attention_decode_wide_dev if wide else hip.attention_decode_dev)(dev(qkv), sin_d, cos_d, kcd, vcd, n_heads, n_kv, D, max_pos, pos_d, scratch, out)
        torch_.cuda.synchronize()
        got = out.cpu().numpy().reshape(n_heads, D)
        rot = lambda x: np.concatenate([x[..., :64] * cos[pos] - x[..., 64:] * sin[pos], x[..., :64] * sin[pos] + x[..., 64:] * cos[pos]], axis=-1)
        q = rot(qkv[: n_heads * D].reshape(n_heads, D).astype(np.float64))
        kn = rot(qkv[n_heads * D:(n_heads + n_kv) * D].reshape(n_kv, D).astype(np.float64))
        vn = qkv[(n_heads + n_kv) * D:].reshape(n_kv, D).astype(np.float64)
        want = np.zeros((n_heads, D))
        for h in range(n_heads):
            kvh = h // group
            K = np.concatenate([kc[kvh, :, :pos].T.astype(np.float64), kn[kvh][None]], axis=0)
            V = np.concatenate([vc[kvh, :pos].astype(np.float64), vn[kvh][None]], axis=0)
            s = K @ q[h] / np.sqrt(D)
            p = np.exp(s - s.max())
            want[h] = (p / p.sum()) @ V
        assert np.max(np.abs(got - want)) <= 2e-5 * max(1.0, np.abs(want).max()), (max_pos, pos, np.max(np.abs(got - want)))
        # the new key / value were appended at `pos`
        assert np.allclose(untiled(kcd.cpu().numpy())[:, :, pos], kn, atol=1e-5) and np.array_equal(vcd.cpu().numpy()[:, pos], vn.astype(np.float32))


@pytest.mark.parametrize("fmt", ["qk256", "ternary32"])
def test_layernorm_after_product_matches_prologue_form(hip, oracle, torch_, fmt):
    """bitnet_hip_weights_bind_ln: (W (gamma*x) - mean * W gamma) / denom == W LN(x) -- against the oracle
    chain and against the prologue form, incl. an activation row with a large mean (cancellation)."""
    rng = np.random.default_rng(5)
    K, N = 2560, 768
    g = (rng.uniform(0.5, 1.5, K) / 80).astype(np.float32)
    gd = torch_.from_numpy(g).cuda()
    if fmt == "qk256":
        stride = K // 256 * 64
        q = rng.integers(0, 256, N * stride, dtype=np.uint8)
        h = hip.weights_upload_qk256(q, N, K, stride)
        ref = lambda xn: oracle.gemv_qk256(q, xn, N, K, stride)
    else:
        codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(N, K), p=[0.5, 0.25, 0.25])
        packed = (codes[:, 0::4] | codes[:, 1::4] << 2 | codes[:, 2::4] << 4 | codes[:, 3::4] << 6).astype(np.uint8).reshape(-1)
        scales = (2.0 / ((np.arange(N * (K // 32)) % 100) + 1)).astype(np.float16).astype(np.float32)
        h = hip.weights_upload_i2s(packed, scales, N, K, 32)
        ref = lambda xn: oracle.i2s_matmul(xn, packed, scales, 1, N, K, 32)
    res = rng.normal(0, 1, N).astype(np.float32)
    rd = torch_.from_numpy(res).cuda()
    for mean in (0.1, 40.0):
        x = rng.normal(mean, 1.0, K).astype(np.float32)
        xd = torch_.from_numpy(x).cuda()
        want = ref(oracle.layernorm(x, g, 1e-5)) + res
        y1 = torch_.empty(N, device="cuda")
        hip.gemv_fused_dev(h, xd, y1, 1, ln_gamma=gd, ln_eps=1e-5, residual=rd)  # prologue form (nothing bound yet / other gamma)
        torch_.cuda.synchronize()
        hip.weights_bind_ln(h, gd)
        y2 = torch_.empty(N, device="cuda")
        hip.gemv_fused_dev(h, xd, y2, 1, ln_gamma=gd, ln_eps=1e-5, residual=rd)  # LayerNorm after the product
        g2 = gd.clone()
        y3 = torch_.empty(N, device="cuda")
        hip.gemv_fused_dev(h, xd, y3, 1, ln_gamma=g2, ln_eps=1e-5, residual=rd)  # a different gamma buffer: prologue form again
        torch_.cuda.synchronize()
        # the large-mean row loses log2(mean/std) bits in BOTH forms (f32 x - mean); the after-product form adds W.(gamma x) rounding
        tol = (3e-5 if mean < 1 else 2e-3) * np.max(np.abs(want)) + 1e-6
        for y in (y1, y2, y3):
            assert np.max(np.abs(y.cpu().numpy() - want)) <= tol, (fmt, mean)
        assert np.array_equal(y1.cpu().numpy(), y3.cpu().numpy())
        hip.weights_bind_ln(h, g2)  # unbind for the next round: gd no longer matches
    hip.weights_free(h)


@pytest.mark.parametrize("n_heads,n_kv", [(8, 2), (4, 2), (20, 5), (3, 3)])
def test_oproj_merging_the_attention_records_equals_combine_then_project(hip, pkg, oracle, torch_, n_heads, n_kv):
    """bitnet_hip_attention_decode_partial_dev + bitnet_hip_gemv_attn_merge_dev (short contexts: no combine launch)
    against bitnet_hip_attention_decode_dev + bitnet_hip_gemv_fused_dev on the same inputs, contexts of 1..4 chunks."""
    D, max_pos = 128, 512
    cols, rows = n_heads * D, 384
    rng = np.random.default_rng(7 * n_heads + n_kv)
    stride = -(-cols // 256) * 64
    qs = rng.integers(0, 256, rows * stride, dtype=np.uint8)
    w = hip.weights_upload_qk256(qs, rows, cols, stride)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a)).cuda()
    sin_d, cos_d = dev(sin), dev(cos)
    sb = hip.c.bitnet_hip_attention_scratch_bytes(n_kv, max_pos)
    for pos in (0, 1, 63, 64, 127, 128, 200, 255):
        kc = rng.normal(0, 1, n_kv * max_pos * D).astype(np.float32)
        vc = rng.normal(0, 1, n_kv * max_pos * D).astype(np.float32)
        qkv = dev(rng.normal(0, 1.5, (n_heads + 2 * n_kv) * D).astype(np.float32))
        res = dev(rng.normal(0, 1, rows).astype(np.float32))
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        # reference form: attention (two kernels) -> o-projection
        k1, v1 = dev(kc), dev(vc)
        scratch1 = torch_.zeros(sb // 4 + 16, device="cuda")
        att = torch_.zeros(cols, device="cuda")
        y1 = torch_.zeros(rows, device="cuda")
        hip.attention_decode_dev(qkv, sin_d, cos_d, k1, v1, n_heads, n_kv, D, max_pos, pos_d, scratch1, att)
        hip.gemv_fused_dev(w, att, y1, 1, residual=res)
        # merged form
        k2, v2 = dev(kc), dev(vc)
        scratch2 = torch_.zeros(sb // 4 + 16, device="cuda")
        # stale-but-finite records past the context (an earlier, longer sequence) must not matter
        scratch2 += 3.0
        y2 = torch_.zeros(rows, device="cuda")
        hip.attention_decode_partial_dev(qkv, sin_d, cos_d, k2, v2, n_heads, n_kv, D, max_pos, pos_d, scratch2)
        hip.gemv_attn_merge_dev(w, scratch2, n_heads, n_kv, max_pos, pos_d, y2, residual=res)
        torch_.cuda.synchronize()
        a, b = y1.cpu().numpy(), y2.cpu().numpy()
        assert np.max(np.abs(a - b)) <= 2e-5 * max(1.0, np.max(np.abs(a))), (n_heads, n_kv, pos, np.max(np.abs(a - b)))
        assert torch_.equal(k1, k2) and torch_.equal(v1, v2)  # the same cache append
    hip.weights_free(w)


def test_decode_is_bit_reproducible_run_to_run(hip, pkg, synth):
    """No atomics, fixed summation orders: the same token sequence gives bit-identical logits on every run and
    whether the steps are replayed from the step graphs or launched one by one."""
    cfg = synth.ModelConfig(**LONG)
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w)
    dec.set_globals(glob)
    prompt = synth.prompt(12, cfg.vocab)
    runs = []
    for use_graph in (True, True, False):
        dec.reset()
        dec.feed(prompt)
        logits = []
        for _ in range(70):  # crosses the 64-position chunk boundary
            dec.run(1, with_logits=True, use_graph=use_graph)
            logits.append(dec.last_logits().copy())
        runs.append((np.stack(logits), list(dec.history(71))))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert np.array_equal(runs[0][0], runs[2][0]) and runs[0][1] == runs[2][1]
    dec.close()


@pytest.mark.parametrize("max_pos,positions,n_heads,n_kv,wide", [(512, [0, 1, 63, 64, 65, 127, 128, 300, 511], 8, 2, False), (512, [0, 64, 191], 3, 3, False),
                                                                (8192, [0, 100, 3071, 3072, 5000, 8100], 8, 2, True), (4608, [4100, 4223, 4224], 20, 5, True),
                                                                (512, [0, 63, 64, 127, 128, 200], 6, 2, False), (512, [0, 63, 64, 127, 128, 200], 6, 2, True)])  # query group of 3
def test_attention_decode_f16_kv_vs_f64(hip, oracle, torch_, max_pos, positions, n_heads, n_kv, wide):
    """BITNET_HIP_ATTN_KV_F16: the cache holds f16 (K [kv][chunk][64 dim pairs][64 positions][2], V [kv][pos][128]), k / v are
    rounded once when appended.  Against a f64 reference that uses the SAME f16 values: the arithmetic (f32 accumulate) is as
    tight as the f32-cache kernel's."""
    D = 128
    group = n_heads // n_kv
    rng = np.random.default_rng(max_pos + n_heads + 1)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    kc = rng.normal(0, 1, (n_kv, D, max_pos)).astype(np.float16)   # logical [kv][D][pos]
    vc = rng.normal(0, 1, (n_kv, max_pos, D)).astype(np.float16)
    ktile = lambda a: np.ascontiguousarray(a.reshape(n_kv, D // 2, 2, max_pos // 64, 64).transpose(0, 3, 1, 4, 2))   # [kv][chunk][D/2][64][2]
    kuntile = lambda a: a.reshape(n_kv, max_pos // 64, D // 2, 64, 2).transpose(0, 2, 4, 1, 3).reshape(n_kv, D, max_pos)
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a)).cuda()
    sb = hip.c.bitnet_hip_attention_scratch_bytes(n_kv, max_pos)
    scratch = torch_.zeros(sb // 4 + 16, device="cuda")
    sin_d, cos_d = dev(sin), dev(cos)
    for pos in positions:
        qkv = rng.normal(0, 1.5, (n_heads + 2 * n_kv) * D).astype(np.float32)
        kc_in, vc_in = kc.copy(), vc.copy()
        kc_in[:, :, pos:] = np.float16(7.0)     # stale slots: finite bit patterns (zero-filled-cache contract)
        vc_in[:, pos:] = np.float16(-300.0)
        kcd, vcd = dev(ktile(kc_in).view(np.int16)), dev(vc_in.view(np.int16))
        out = torch_.full((n_heads * D,), float("nan"), device="cuda")
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        hip.attention_decode_q_dev(dev(qkv), sin_d, cos_d, kcd, vcd, n_heads, n_kv, D, max_pos, pos_d, scratch, out, None, wide=wide, kv_f16=True)
        torch_.cuda.synchronize()
        got = out.cpu().numpy().reshape(n_heads, D)
        rot = lambda x: np.concatenate([x[..., :64] * cos[pos] - x[..., 64:] * sin[pos], x[..., :64] * sin[pos] + x[..., 64:] * cos[pos]], axis=-1)
        q = rot(qkv[: n_heads * D].reshape(n_heads, D).astype(np.float64))
        kn32 = rot(qkv[n_heads * D:(n_heads + n_kv) * D].reshape(n_kv, D).astype(np.float32))      # RoPE in f32 on the device
        kn = rot(qkv[n_heads * D:(n_heads + n_kv) * D].reshape(n_kv, D).astype(np.float64)).astype(np.float32).astype(np.float16).astype(np.float64)
        vn = qkv[(n_heads + n_kv) * D:].reshape(n_kv, D).astype(np.float16).astype(np.float64)
        want = np.zeros((n_heads, D))
        for h in range(n_heads):
            kvh = h // group
            K = np.concatenate([kc[kvh, :, :pos].T.astype(np.float64), kn[kvh][None]], axis=0)
            V = np.concatenate([vc[kvh, :pos].astype(np.float64), vn[kvh][None]], axis=0)
            s = K @ q[h] / np.sqrt(D)
            p = np.exp(s - s.max())
            want[h] = (p / p.sum()) @ V
        # (the new key's f16 rounding can flip one ulp against this f64-then-f16 reference: 1e-3 of an O(1) score at most)
        assert np.max(np.abs(got - want)) <= 2e-3 * max(1.0, np.abs(want).max()), (max_pos, pos, np.max(np.abs(got - want)))
        # appended: the new key / value, rounded to f16, at `pos`
        kback = kuntile(kcd.cpu().numpy().view(np.float16))
        assert np.allclose(kback[:, :, pos].astype(np.float32), kn32, atol=2e-2, rtol=2e-3)
        assert np.array_equal(vcd.cpu().numpy().view(np.float16).reshape(n_kv, max_pos, D)[:, pos], qkv[(n_heads + n_kv) * D:].reshape(n_kv, D).astype(np.float16))
        # untouched neighbours
        if pos > 0:
            assert np.array_equal(kback[:, :, pos - 1], kc[:, :, pos - 1])


def test_decode_with_f16_kv_cache_at_2k_keys_vs_oracle(hip, pkg, oracle, synth):
    """opt-in f16 KV cache -- a 2,048-token prompt through Decoder.prefill (cache filled with the f16-rounded
    k / v), then decode steps at 2k+ keys through the 128-position chunk form, per-step logits against the oracle (f32 cache):
    cosine >= 0.9999; the same steps with the f32 cache for comparison."""
    cfg = synth.ModelConfig(**dict(SMALL, max_pos=2240))
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    T, n_dec = 2048, 6
    seq = list(synth.prompt(T + n_dec, cfg.vocab))
    om = oracle.OracleModel(cfg, layers, glob, n_threads=8)
    o_logits = []
    for p in range(T + n_dec - 1):
        _, logits, _ = om.step(seq[p], want_logits=p >= T - 1)
        if p >= T - 1:
            o_logits.append(logits)
    om.close()
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w)
    dec.set_globals(glob)
    worst = {}
    for kv16 in (True, False):
        dec.reset()
        dec.set_kv_f16(kv16)
        dec.feed(seq)
        dec.prefill(T, with_logits=True, digits=4)
        cs = [cosine(dec.last_logits(), o_logits[0])]
        for i in range(1, n_dec):
            dec.run(1, with_logits=True, use_graph=True)
            cs.append(cosine(dec.last_logits(), o_logits[i]))
        worst[kv16] = min(cs)
        assert min(cs) >= 0.9999, (kv16, cs)
    with pytest.raises(pkg.BitNetHipError, match="fresh sequence"):
        dec.set_kv_f16(True)
    dec.close()
