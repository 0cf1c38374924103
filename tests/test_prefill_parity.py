"""GPU parity of the prompt (prefill) path: causal attention over a whole prompt and the
host-side prefill loop (tiled matmuls + attention), against the CPU oracle run token by
token (oracle/transformer_oracle.c, T:1482-1504), and against this library's own
single-token path (same KV cache contents, same next tokens)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def rope_np(x, sin, cos):
    half = x.shape[-1] // 2
    x0, x1 = x[..., :half], x[..., half:]
    return np.concatenate([x0 * cos - x1 * sin, x0 * sin + x1 * cos], axis=-1)


@pytest.mark.parametrize("T,n_heads,n_kv", [(1, 4, 2), (37, 4, 2), (64, 4, 4), (200, 20, 5), (333, 8, 2)])
def test_prefill_attention_matches_f64_reference(hip, oracle, torch_, T, n_heads, n_kv):
    D, max_pos = 128, 512
    rng = np.random.default_rng(T)
    qkv = rng.normal(0, 1.5, (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    sin, cos = sin.reshape(max_pos, D // 2), cos.reshape(max_pos, D // 2)
    q = qkv[:, : n_heads * D].reshape(T, n_heads, D).astype(np.float64)
    k = qkv[:, n_heads * D:(n_heads + n_kv) * D].reshape(T, n_kv, D).astype(np.float64)
    v = qkv[:, (n_heads + n_kv) * D:].reshape(T, n_kv, D).astype(np.float64)
    q = rope_np(q, sin[:T, None, :], cos[:T, None, :])
    k = rope_np(k, sin[:T, None, :], cos[:T, None, :])
    want = np.zeros((T, n_heads, D))
    group = n_heads // n_kv
    mask = np.triu(np.ones((T, T), bool), 1)
    for h in range(n_heads):
        s = q[:, h] @ k[:, h // group].T / np.sqrt(D)
        s[mask] = -np.inf
        pm = np.exp(s - s.max(axis=1, keepdims=True))
        want[:, h] = (pm / pm.sum(axis=1, keepdims=True)) @ v[:, h // group]
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    kc = torch_.zeros(n_kv * max_pos * D, device="cuda")  # max_pos is a multiple of 64 here
    vc = torch_.zeros(n_kv * max_pos * D, device="cuda")
    wsb = hip.attention_prefill_workspace_bytes(n_heads, n_kv, T)
    ws = torch_.empty(wsb, dtype=torch_.uint8, device="cuda")
    out = torch_.full((T, n_heads * D), float("nan"), device="cuda")
    hip.attention_prefill_dev(dev(qkv), dev(sin), dev(cos), kc, vc, n_heads, n_kv, D, max_pos, T, ws, wsb, out)
    torch_.cuda.synchronize()
    got = out.cpu().numpy().reshape(T, n_heads, D)
    assert not np.isnan(got).any()
    # f16 operands: 2^-11 relative per element; outputs are averages of O(1) values
    assert np.max(np.abs(got - want)) <= 6e-3, np.max(np.abs(got - want))
    assert cosine(got, want) >= 0.999995
    # the decode cache holds the exact f32 rotated k (transposed) and v
    # K cache: transposed in 64-position tiles [kv][chunk][D][64]  ->  [kv][D][max_pos]
    k_full = kc.cpu().numpy().reshape(n_kv, max_pos // 64, D, 64).transpose(0, 2, 1, 3).reshape(n_kv, D, max_pos)
    assert np.allclose(k_full[:, :, :T].transpose(2, 0, 1), k, rtol=0, atol=2e-6 * np.abs(k).max())
    assert np.array_equal(vc.cpu().numpy().reshape(n_kv, max_pos, D)[:, :T].transpose(1, 0, 2), v.astype(np.float32))
    assert not k_full[:, :, T:].any()
    with pytest.raises(Exception, match="KV cache overflow"):
        hip.attention_prefill_dev(dev(qkv), dev(sin), dev(cos), kc, vc, n_heads, n_kv, D, 16 if T > 16 else 0, T, ws, wsb, out)


def prefill_f64(qkv, sin, cos, n_heads, n_kv):
    """causal GQA attention over a whole prompt in float64 -> [T, heads, D]; sin / cos [max_pos, D / 2]"""
    T, D = qkv.shape[0], 128
    q = qkv[:, : n_heads * D].reshape(T, n_heads, D).astype(np.float64)
    k = qkv[:, n_heads * D:(n_heads + n_kv) * D].reshape(T, n_kv, D).astype(np.float64)
    v = qkv[:, (n_heads + n_kv) * D:].reshape(T, n_kv, D).astype(np.float64)
    q, k = rope_np(q, sin[:T, None, :], cos[:T, None, :]), rope_np(k, sin[:T, None, :], cos[:T, None, :])
    want = np.zeros((T, n_heads, D))
    mask = np.triu(np.ones((T, T), bool), 1)
    for h in range(n_heads):
        s = q[:, h] @ k[:, h // (n_heads // n_kv)].T / np.sqrt(D)
        s[mask] = -np.inf
        pm = np.exp(s - s.max(axis=1, keepdims=True))
        want[:, h] = (pm / pm.sum(axis=1, keepdims=True)) @ v[:, h // (n_heads // n_kv)]
    return want


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("T,n_heads,n_kv", [(70, 4, 2), (130, 3, 3)])
def test_prefill_attention_misaligned_rows(hip, oracle, torch_, T, n_heads, n_kv, f16):
    """q|k|v rows 4 bytes off a 16-byte boundary through bitnet_hip_attention_prefill_flags_dev: k_prefill_prep then prepares the query image
    too (one launch over heads + 2 kv slots, scalar loads) instead of the attention kernel reading the f32 rows.  The operator's gates against
    float64, 2e-4 of max|aligned| against the aligned call on the same values, and the same caches bit for bit."""
    D, max_pos = 128, 512
    rng = np.random.default_rng(10 * T + (7 if f16 else 0))
    qkv = rng.normal(0, 1.5, (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    sin, cos = sin.reshape(max_pos, D // 2), cos.reshape(max_pos, D // 2)
    want = prefill_f64(qkv, sin, cos, n_heads, n_kv)
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    sin_d, cos_d = dev(sin), dev(cos)
    wsb = hip.attention_prefill_workspace_bytes(n_heads, n_kv, T)
    dt, iv = (torch_.float16, torch_.int16) if f16 else (torch_.float32, torch_.int32)

    def run(misalign):
        buf = torch_.zeros(qkv.size + 1, device="cuda")
        buf[1 if misalign else 0:][:qkv.size] = dev(qkv).ravel()
        kc, vc = torch_.zeros(n_kv * max_pos * D, dtype=dt, device="cuda"), torch_.zeros(n_kv * max_pos * D, dtype=dt, device="cuda")
        ws = torch_.full((wsb,), 0xFF, dtype=torch_.uint8, device="cuda")  # NaN patterns: nothing the call did not write may be read
        out = torch_.full((T, n_heads * D), float("nan"), device="cuda")
        hip.attention_prefill_flags_dev(buf.data_ptr() + (4 if misalign else 0), sin_d, cos_d, kc, vc, n_heads, n_kv, D, max_pos, T, ws, wsb, out, 1 if f16 else 0)
        torch_.cuda.synchronize()
        return out.cpu().numpy().reshape(T, n_heads, D), kc.view(iv), vc.view(iv)

    aligned, kc0, vc0 = run(False)
    got, kc1, vc1 = run(True)
    assert np.isfinite(got).all()
    err, c, d = float(np.max(np.abs(got - want))), cosine(got, want), float(np.max(np.abs(got - aligned)))
    print(f"misaligned prefill T={T} heads={n_heads}/{n_kv} f16={f16}: max|diff| vs f64 {err:.3e} cosine {c:.8f}; "
          f"vs aligned {d:.3e} of max|aligned| {np.max(np.abs(aligned)):.3f}")
    assert err <= 6e-3 and c >= 0.9999
    assert d <= 2e-4 * np.max(np.abs(aligned))
    assert torch_.equal(kc1, kc0) and torch_.equal(vc1, vc0)


SMALL = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=160, eps=1e-5, rope_theta=10000.0)
WIDE = dict(hidden=2560, n_layers=2, n_heads=20, n_kv_heads=5, head_dim=128, ffn=6912, vocab=4096, max_pos=96, eps=1e-5, rope_theta=500000.0)


@pytest.mark.parametrize("T,n_heads,n_kv", [(2560, 20, 5), (4096, 20, 5), (2200, 8, 8)])
def test_prefill_attention_long_prompt_rows_match_f64_reference(hip, oracle, torch_, T, n_heads, n_kv):
    """Long prompts (40 - 64 key tiles per query block): the first and last rows of query blocks, rows around the middle of the prompt
    and its last row, against the f64 softmax of the same rows (T:410-533)."""
    D, max_pos = 128, 4096
    rng = np.random.default_rng(T + n_heads)
    qkv = rng.normal(0, 1.2, (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    sin, cos = sin.reshape(max_pos, D // 2), cos.reshape(max_pos, D // 2)
    rows = np.unique(np.concatenate([[0, 31, 32, 63, 64, 2047, 2048, 2079, 2080, 2111, 2112, 2143, T - 65, T - 64, T - 33, T - 32, T - 1],
                                     rng.integers(0, T, 40)]))
    rows = rows[(rows >= 0) & (rows < T)]
    k = qkv[:, n_heads * D:(n_heads + n_kv) * D].reshape(T, n_kv, D).astype(np.float64)
    v = qkv[:, (n_heads + n_kv) * D:].reshape(T, n_kv, D).astype(np.float64)
    k = rope_np(k, sin[:T, None, :], cos[:T, None, :])
    q = rope_np(qkv[rows, : n_heads * D].reshape(len(rows), n_heads, D).astype(np.float64), sin[rows, None, :], cos[rows, None, :])
    group = n_heads // n_kv
    want = np.zeros((len(rows), n_heads, D))
    for i, r in enumerate(rows):
        for h in range(n_heads):
            sc = k[: r + 1, h // group] @ q[i, h] / np.sqrt(D)
            pm = np.exp(sc - sc.max())
            want[i, h] = (pm / pm.sum()) @ v[: r + 1, h // group]
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    kc = torch_.zeros(n_kv * max_pos * D, device="cuda")
    vc = torch_.zeros(n_kv * max_pos * D, device="cuda")
    wsb = hip.attention_prefill_workspace_bytes(n_heads, n_kv, T)
    ws = torch_.empty(wsb, dtype=torch_.uint8, device="cuda")
    out = torch_.full((T, n_heads * D), float("nan"), device="cuda")
    for rep in range(2):  # twice on one workspace
        hip.attention_prefill_dev(dev(qkv), dev(sin), dev(cos), kc, vc, n_heads, n_kv, D, max_pos, T, ws, wsb, out)
        got_all = out.cpu().numpy()
        assert np.isfinite(got_all).all()
        got = got_all[rows].reshape(len(rows), n_heads, D)
        # q, k, v and the probabilities pass through the matrix cores as f16 (2^-11 relative each)
        assert np.max(np.abs(got - want)) <= 6e-3, np.max(np.abs(got - want))
        assert cosine(got, want) >= 0.99999


@pytest.mark.parametrize("cfgd,n_prompt,n_new,fmt", [(SMALL, 70, 6, "qk256"), (SMALL, 21, 4, "i2s"), (WIDE, 33, 4, "qk256")])
def test_prefill_then_decode_matches_oracle(pkg, oracle, synth, cfgd, n_prompt, n_new, fmt):
    cfg = synth.ModelConfig(**cfgd)
    glob = synth.make_globals(cfg)
    if fmt == "qk256":
        layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
        olayers = layers
    else:  # ternary codes + 32-element block scales (f16 values, cols % 256 == 0): the tiled matmul's K = 32 form, k_gemm_mfma<NDIG, TT32, 3, 2, 1>
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
    prompt = synth.prompt(n_prompt, cfg.vocab)
    om = oracle.OracleModel(cfg, olayers, glob, n_threads=8)
    seq = list(prompt)
    o_logits = []
    for p in range(n_prompt + n_new - 1):
        _, logits, _ = om.step(seq[p], want_logits=p >= n_prompt - 1)
        if p >= n_prompt - 1:
            o_logits.append(logits)
            seq.append(oracle.argmax(logits))
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w) if fmt == "qk256" else dec.set_layer_i2s(l, w, 32)
    dec.set_globals(glob)
    for digits in (4, 3):
        dec.reset()
        dec.feed(prompt)
        dec.prefill(n_prompt, with_logits=True, digits=digits)
        assert dec.position() == n_prompt
        c = cosine(dec.last_logits(), o_logits[0])
        assert c >= 0.9999, (digits, c)
        for i in range(1, n_new):
            dec.run(1, with_logits=True, use_graph=True)  # decode continues on the prefilled KV cache
            c = cosine(dec.last_logits(), o_logits[i])
            assert c >= 0.9999, (digits, i, c)
        assert list(dec.history(n_prompt + n_new)) == [int(t) for t in seq], digits
    # prefill without logits + one decode step == the same state
    dec.reset()
    dec.feed(prompt)
    dec.prefill(n_prompt - 1, with_logits=False)
    assert dec.position() == n_prompt - 1
    dec.run(1, with_logits=True, use_graph=False)
    assert cosine(dec.last_logits(), o_logits[0]) >= 0.9999
    # guards
    with pytest.raises(pkg.BitNetHipError, match="fresh sequence"):
        dec.prefill(4)
    dec.reset()
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.prefill(4)
    dec.close()
    om.close()


@pytest.mark.parametrize("batch,heads,seq,causal", [(1, 2, 1, True), (2, 3, 70, True), (1, 4, 130, False)])
def test_host_attention_dropin(hip, batch, heads, seq, causal):
    """bitnet_hip_attention = the reference's fused_attention_hip stub signature (K/rocm/attention.rs:54-65):
    [batch, heads, seq, head_dim] tensors, custom scale, optional causal mask; against a f64 reference."""
    D = 128
    rng = np.random.default_rng(seq)
    q, k, v = (rng.normal(0, 1.2, (batch, heads, seq, D)).astype(np.float32) for _ in range(3))
    scale = 0.11
    s = np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), k.astype(np.float64)) * scale
    if causal:
        s[..., np.triu(np.ones((seq, seq), bool), 1)] = -np.inf
    pm = np.exp(s - s.max(axis=-1, keepdims=True))
    want = np.einsum("bhqk,bhkd->bhqd", pm / pm.sum(axis=-1, keepdims=True), v.astype(np.float64))
    got = hip.attention(q, k, v, seq, heads, D, causal=causal, scale=scale).reshape(batch, heads, seq, D)
    assert np.max(np.abs(got - want)) <= 6e-3
    assert cosine(got, want) >= 0.999995
    with pytest.raises(Exception, match="head_dim 64 unsupported"):
        hip.attention(np.zeros(8 * 64, np.float32), np.zeros(8 * 64, np.float32), np.zeros(8 * 64, np.float32), 1, 8, 64)
    with pytest.raises(Exception, match="must all hold"):
        hip.attention(q, k[:, :1], v, seq, heads, D)


def test_qk256_gemv_batch_dropin(hip, oracle):
    """qk256_gemv_hip_batch (K/rocm/qk256_gemv.rs:67-82): items in order, each = bitnet_hip_qk256_gemv."""
    rng = np.random.default_rng(9)
    items, wants = [], []
    for m, n, k in ((1, 64, 256), (3, 48, 512), (2, 16, 1024)):
        codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(n, k))
        packed = (codes[:, 0::4] | codes[:, 1::4] << 2 | codes[:, 2::4] << 4 | codes[:, 3::4] << 6).astype(np.uint8).reshape(-1)
        scales = rng.uniform(0.1, 1.0, n * (k // 256)).astype(np.float32)
        x = rng.uniform(-2, 2, m * k).astype(np.float32)
        items.append((packed, scales, x, m, n, k))
        wants.append(oracle.i2s_matmul(x, packed, scales, m, n, k, 256))
    outs = hip.qk256_gemv_batch(items)
    for got, want in zip(outs, wants):
        assert np.max(np.abs(got - want)) <= 2e-5 * np.max(np.abs(want)) + 1e-6
    with pytest.raises(Exception, match="multiple of 256"):
        hip.qk256_gemv_batch([(np.zeros(64, np.uint8), np.ones(1, np.float32), np.zeros(100, np.float32), 1, 1, 100)])


def test_prefill_attention_is_causal_and_block_independent(hip, oracle, torch_):
    """Properties at a long sequence (2,000 tokens, 2B-4T head counts): outputs of positions < t do not
    change when tokens >= t change (bit for bit), and a token-parallel call that only holds the first
    1,024 queries (64-row blocks in any order) reproduces those rows (to the rounding of the key-split merge)."""
    n_heads, n_kv, D, T, max_pos = 20, 5, 128, 2000, 2048
    rng = np.random.default_rng(2000)
    qkv = rng.normal(0, 1.2, (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    sin_d, cos_d = dev(sin), dev(cos)
    wsb = hip.attention_prefill_workspace_bytes(n_heads, n_kv, T)
    ws = torch_.empty(wsb, dtype=torch_.uint8, device="cuda")

    def run(x):
        kc = torch_.zeros(n_kv * max_pos * D, device="cuda")
        vc = torch_.zeros(n_kv * max_pos * D, device="cuda")
        out = torch_.empty(T, n_heads * D, device="cuda")
        hip.attention_prefill_dev(dev(x), sin_d, cos_d, kc, vc, n_heads, n_kv, D, max_pos, T, ws, wsb, out)
        torch_.cuda.synchronize()
        return out.cpu().numpy()

    base = run(qkv)
    t = 1217
    changed = qkv.copy()
    changed[t:] = rng.normal(0, 3.0, changed[t:].shape).astype(np.float32)
    got = run(changed)
    assert np.array_equal(got[:t], base[:t])
    assert not np.array_equal(got[t:], base[t:])
    # sharded call: queries 0..1023 as 16 blocks in a shuffled order, full context
    nq = 1024
    order = rng.permutation(nq // 64)
    rows = np.concatenate([np.arange(64 * b, 64 * b + 64) for b in order])
    kv_all = dev(qkv[:, n_heads * D:])
    q_local = dev(qkv[rows][:, : n_heads * D])
    bp = torch_.from_numpy((order * 64).astype(np.int32)).cuda()
    wsb2 = hip.attention_prefill_sharded_workspace_bytes(n_heads, n_kv, nq, T)
    ws2 = torch_.empty(wsb2, dtype=torch_.uint8, device="cuda")
    kc = torch_.zeros(n_kv * max_pos * D, device="cuda")
    vc = torch_.zeros(n_kv * max_pos * D, device="cuda")
    out = torch_.empty(nq, n_heads * D, device="cuda")
    hip.attention_prefill_sharded_dev(q_local, n_heads * D, bp, nq, kv_all, 2 * n_kv * D, T, sin_d, cos_d, kc, vc, n_heads, n_kv, D, max_pos, ws2,
                                      wsb2, out)
    torch_.cuda.synchronize()
    # (the two launches split a query block's key tiles over different numbers of workgroups: equal up to the f32 merge's rounding)
    # the probabilities are rounded to f16 against each key part's own running maximum: observed 6.7e-5 of max|base| when the key-split
    # form landed (gpurun_out/r3_t9.log); the gate is 3x that -- a wrong merge weight shows up at 1e-2 and more
    assert np.max(np.abs(out.cpu().numpy() - base[rows])) <= 2e-4 * np.max(np.abs(base))


MANYKV = dict(hidden=1024, n_layers=2, n_heads=8, n_kv_heads=8, head_dim=128, ffn=1024, vocab=2048, max_pos=2176, eps=1e-5, rope_theta=10000.0)


def test_decode_switches_to_the_wide_attention_form(pkg, oracle, synth):
    """With 8 KV heads the 64-position chunks outnumber the 256 CUs beyond 2048 keys, where the decoder changes to the
    128-position attention workgroups (a third step graph): prefill 2040 tokens, then decode across the switch, every
    step against the oracle (teacher-forced)."""
    cfg = synth.ModelConfig(**MANYKV)
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    n_prompt, n_new = 2040, 16
    om = oracle.OracleModel(cfg, layers, glob, n_threads=8)
    seq = list(synth.prompt(n_prompt, cfg.vocab))
    o_logits = []
    for p in range(n_prompt + n_new - 1):
        _, logits, _ = om.step(seq[p], want_logits=p >= n_prompt - 1)
        if p >= n_prompt - 1:
            o_logits.append(logits)
            seq.append(oracle.argmax(logits))
    dec = pkg.HostDecoder(cfg)
    for l, w in enumerate(layers):
        dec.set_layer_qk256(l, w)
    dec.set_globals(glob)
    dec.reset()
    dec.feed(seq)  # every token forced to the oracle's
    dec.prefill(n_prompt, with_logits=True, digits=4)
    assert cosine(dec.last_logits(), o_logits[0]) >= 0.9999
    for i in range(1, n_new):
        dec.run(1, with_logits=True, use_graph=True)  # keys 2041 .. 2055: crosses 2048
        c = cosine(dec.last_logits(), o_logits[i])
        assert c >= 0.9999, (i, c)
    assert dec.position() == n_prompt + n_new - 1
    dec.close()
    om.close()


@pytest.mark.parametrize("world,T,wire_f16", [(1, 128, False), (2, 256, False), (2, 512, True), (4, 512, False), (8, 1024, True), (8, 8192, True)])
def test_cpp_sharded_prefill_two_ranks_one_gpu(pkg, hip, synth, torch_, world, T, wire_f16):
    """Decoder::prefill_sharded (the C++ host loop + bitnet_hip_attention_prefill_gathered_dev: zigzag chunks, k|v rows read
    in place from the gathered buffer) with `world` decoders = ranks on ONE GPU, each driven from its own host thread, the
    all-gather supplied as a callback that meets at a barrier -- against the unsharded Decoder.prefill."""
    import threading

    # world 8 = the driver's 8-GPU run rehearsed as eight rank threads on one GPU (16 zigzag chunks; 8192 tokens = 512-token
    # chunks, the size bench.py's c5 line uses): its first execution on real ranks must not be the first execution of this indexing
    cfg = synth.ModelConfig(**dict(SMALL, max_pos=max(640, T + 64)))
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    prompt = synth.prompt(T, cfg.vocab)

    def make():
        d = pkg.HostDecoder(cfg)
        for l, w in enumerate(layers):
            d.set_layer_qk256(l, w)
        d.set_globals(glob)
        d.reset()
        d.feed(prompt)
        return d

    ref = make()
    ref.prefill(T, with_logits=True, digits=3)
    want_logits = ref.last_logits()
    ref.run(3, with_logits=True)
    want_tokens = list(ref.history(T + 4))
    ref.close()
    decs = [make() for _ in range(world)]
    slots, bar, errors = [None] * world, threading.Barrier(world), []

    def gather_for(rank):
        def gather(send, recv, nbytes, stream):
            torch_.cuda.synchronize()
            tp_mod = importlib.import_module("bitnet-rs_amd.prefill_parallel")
            slots[rank] = torch_.as_tensor(tp_mod._DevBytes(send, nbytes), device="cuda").clone()
            bar.wait(timeout=60)
            r = torch_.as_tensor(tp_mod._DevBytes(recv, nbytes * world), device="cuda")
            r.copy_(torch_.cat(slots))
            torch_.cuda.synchronize()
            bar.wait(timeout=60)
            return 0
        return gather

    def run(rank):
        try:
            decs[rank].prefill_sharded(T, rank, world, gather_for(rank) if world > 1 else None, with_logits=True, digits=3, wire_f16=wire_f16)
        except Exception as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    d0 = decs[0]
    assert d0.position() == T
    got = d0.last_logits()
    # f16 on the wire rounds the prompt's k|v in the decode cache (not in the prompt attention, which is f16 either way)
    assert cosine(got, want_logits) >= 0.999999 and np.max(np.abs(got - want_logits)) <= 1e-3 * np.max(np.abs(want_logits))
    d0.run(3, with_logits=True)  # decode continues on the cache the shards filled -- on every rank
    assert list(d0.history(T + 4)) == want_tokens or wire_f16
    for d in decs[1:]:
        assert d.position() == T
        # every rank received the last prompt position's row with the closing gather: same logits, and it decodes on from its own cache
        assert np.array_equal(d.last_logits(), got)
    if world > 1:
        decs[-1].run(3, with_logits=True)
        assert list(decs[-1].history(T + 4)) == list(d0.history(T + 4))
    for d in decs:
        d.close()
    with pytest.raises(pkg.BitNetHipError, match="multiple of"):
        dd = make()
        dd.prefill_sharded(100, 0, 2, lambda *a: 0)


@pytest.mark.parametrize("world,T,wire_f16", [(2, 512, True), (4, 1024, False)])
def test_cpp_sharded_prefill_asynchronous_gather_no_host_sync(pkg, hip, synth, torch_, world, T, wire_f16):
    """The all-gather as a collective library issues it: the callback only ENQUEUES work on the stream it is handed (the
    decoder's comm stream) -- device-to-device copies out of every rank's send buffer, ordered by events between the ranks'
    streams -- and returns without a host-device synchronisation.  What orders the pack before the gather, the gather before
    the k / v phase of the attention, and the next layer's pack behind the readers of the send buffer is then ONLY the
    decoder's own event pair (sp_ev_pack_ / sp_ev_gather_) plus the callback's events: the path RCCL takes.
    The host-side barriers only make sure an event has been RECORDED (a host call) before another thread waits on it."""
    import ctypes as C
    import threading

    rt = C.CDLL("libamdhip64.so")
    rt.hipEventCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    rt.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rt.hipEventDestroy.argtypes = [C.c_void_p]
    D2D, NO_TIMING = 3, 2
    cfg = synth.ModelConfig(**dict(SMALL, max_pos=T + 64))
    layers = [synth.make_layer(cfg, l) for l in range(cfg.n_layers)]
    glob = synth.make_globals(cfg)
    prompt = synth.prompt(T, cfg.vocab)

    def make():
        d = pkg.HostDecoder(cfg)
        for l, w in enumerate(layers):
            d.set_layer_qk256(l, w)
        d.set_globals(glob)
        d.reset()
        d.feed(prompt)
        return d

    ref = make()
    ref.prefill(T, with_logits=True, digits=2)  # 2 digits: the f16 hand-over of the attention output and of silu * up, sharded and not
    want_logits = ref.last_logits()
    ref.close()
    decs = [make() for _ in range(world)]

    def event():
        e = C.c_void_p()
        assert rt.hipEventCreateWithFlags(C.byref(e), NO_TIMING) == 0
        return e

    ready = [event() for _ in range(world)]  # rank's send buffer is packed (its comm stream already waits for the pack event)
    done = [event() for _ in range(world)]   # rank has copied out of everybody's send buffer
    sends, bar, errors, host_syncs = [None] * world, threading.Barrier(world), [], []

    def gather_for(rank):
        def gather(send, recv, nbytes, stream):
            sends[rank] = send
            assert rt.hipEventRecord(ready[rank], stream) == 0
            bar.wait(timeout=60)  # every ready[] has been recorded for this layer
            for q in range(world):
                assert rt.hipStreamWaitEvent(stream, ready[q], 0) == 0
                assert rt.hipMemcpyAsync(C.c_void_p(recv + q * nbytes), C.c_void_p(sends[q]), nbytes, D2D, stream) == 0
            assert rt.hipEventRecord(done[rank], stream) == 0
            bar.wait(timeout=60)  # every done[] has been recorded
            for q in range(world):  # like a collective: complete on this rank once nobody reads its send buffer any more
                assert rt.hipStreamWaitEvent(stream, done[q], 0) == 0
            return 0
        return gather

    def run(rank):
        try:
            decs[rank].prefill_sharded(T, rank, world, gather_for(rank), with_logits=True, digits=2, wire_f16=wire_f16)
        except Exception as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    got = decs[0].last_logits()
    assert cosine(got, want_logits) >= 0.999999 and np.max(np.abs(got - want_logits)) <= 1e-3 * np.max(np.abs(want_logits))
    for d in decs:
        assert d.position() == T
        d.close()
    for e in ready + done:
        rt.hipEventDestroy(e)


@pytest.mark.parametrize("wire_f16", [False, True])
def test_gathered_attention_world8_8k_matches_unsharded_and_f64(hip, oracle, torch_, wire_f16):
    """bitnet_hip_attention_prefill_gathered_dev exactly as the 8-GPU run of BASELINE configs[4] calls it: 8192 positions in 16
    zigzag chunks of 512, the k|v rows in rank-major order as ncclAllGather leaves them (f32, or f16 on the wire), 2B-4T head
    counts, one rank's 1024 queries per call (4 key splits: 640 workgroups).  f32 on the wire must reproduce the unsharded
    kernel's rows (to the f32 rounding of the key-split merge) and fill the same cache bit for bit; f16 on the wire is held to the f64 reference (the prompt attention rounds k, v to f16 anyway)."""
    n_heads, n_kv, D, T, world, max_pos = 20, 5, 128, 8192, 8, 8192
    chunk, nq, KD = T // (2 * world), T // world, n_kv * 128
    rng = np.random.default_rng(8192)
    qkv = rng.normal(0, 1.2, (T, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a)).cuda()
    sin_d, cos_d = dev(sin), dev(cos)
    # unsharded: one call over the whole prompt
    wsb = hip.attention_prefill_workspace_bytes(n_heads, n_kv, T)
    ws = torch_.empty(wsb, dtype=torch_.uint8, device="cuda")
    kc0, vc0 = torch_.zeros(n_kv * max_pos * D, device="cuda"), torch_.zeros(n_kv * max_pos * D, device="cuda")
    base_d = torch_.empty(T, n_heads * D, device="cuda")
    hip.attention_prefill_dev(dev(qkv), sin_d, cos_d, kc0, vc0, n_heads, n_kv, D, max_pos, T, ws, wsb, base_d)
    torch_.cuda.synchronize()
    base = base_d.cpu().numpy()
    del ws, base_d
    # the gathered buffer: rank r's block = chunk r, then chunk 2 world - 1 - r; each row = k heads then v heads
    rows_of = lambda r: np.concatenate([np.arange(r * chunk, (r + 1) * chunk), np.arange((2 * world - 1 - r) * chunk, (2 * world - r) * chunk)])
    order = np.concatenate([rows_of(r) for r in range(world)])
    kv = qkv[:, n_heads * D:][order]
    kv_d = dev(kv.astype(np.float16) if wire_f16 else kv)
    wsb2 = hip.attention_prefill_sharded_workspace_bytes(n_heads, n_kv, nq, T)
    ws2 = torch_.empty(wsb2, dtype=torch_.uint8, device="cuda")
    for rank in (0, 3, 7):
        rows = rows_of(rank)
        q_local = dev(qkv[rows][:, : n_heads * D])
        bp = dev(rows[::64].astype(np.int32))
        kc, vc = torch_.zeros(n_kv * max_pos * D, device="cuda"), torch_.zeros(n_kv * max_pos * D, device="cuda")
        out = torch_.full((nq, n_heads * D), float("nan"), device="cuda")
        hip.attention_prefill_gathered_dev(q_local, n_heads * D, bp, nq, kv_d, T, world, wire_f16, sin_d, cos_d, kc, vc, False, n_heads, n_kv, D,
                                           max_pos, ws2, wsb2, out)
        torch_.cuda.synchronize()
        got = out.cpu().numpy()
        assert not np.isnan(got).any()
        if not wire_f16:
            assert np.max(np.abs(got - base[rows])) <= 2e-4 * np.max(np.abs(base)), rank  # key splits differ (8 parts here, 1 there): f16 probabilities against each part's own maximum (observed 6.7e-5)
            assert torch_.equal(kc, kc0) and torch_.equal(vc, vc0), rank  # every rank fills the whole cache
        else:
            assert np.max(np.abs(got - base[rows])) <= 6e-3 and cosine(got, base[rows]) >= 0.99999, rank
            assert float((kc - kc0).abs().max()) <= 2e-3 * float(kc0.abs().max())
    # f64 reference on a sample of rank 7's queries (first chunk 7 = positions 3584.., second chunk 8 = 4096..)
    rows = rows_of(7)[[0, 63, 511, 512, 1000, 1023]]
    q = qkv[:, : n_heads * D].reshape(T, n_heads, D).astype(np.float64)
    k = qkv[:, n_heads * D:(n_heads + n_kv) * D].reshape(T, n_kv, D).astype(np.float64)
    v = qkv[:, (n_heads + n_kv) * D:].reshape(T, n_kv, D).astype(np.float64)
    sin2, cos2 = sin.reshape(max_pos, D // 2), cos.reshape(max_pos, D // 2)
    k = rope_np(k, sin2[:T, None, :], cos2[:T, None, :])
    for t in rows:
        qt = rope_np(q[t], sin2[t][None, :], cos2[t][None, :])
        for h in (0, 7, 19):
            s = k[: t + 1, h // 4] @ qt[h] / np.sqrt(D)
            pm = np.exp(s - s.max())
            want = (pm / pm.sum()) @ v[: t + 1, h // 4]
            assert np.max(np.abs(base[t, h * D:(h + 1) * D] - want)) <= 6e-3, (t, h)
