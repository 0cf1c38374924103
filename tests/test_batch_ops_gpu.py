"""GPU: the decode kernels taking n_seq vectors per launch (csrc/kernels_batch.hip, k_attn_*_batch in csrc/kernels_attn.hip) against the batch-1
entry points they restate, run on private copies of the same inputs.

The batch-1 kernels are pinned to the oracle and to float64 elsewhere (test_decode_parity.py, test_full_depth_parity.py, test_qact_gpu.py,
test_decoder_state_gpu.py).  The batched kernels promise the SAME BITS per vector, so every comparison here is array_equal on raw bit patterns:
there is no tolerance to choose, and the pinning carries over."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """raw bytes of a device tensor (NaN-safe comparison)"""
    return t.contiguous().view(-1).cpu().numpy().view(np.uint8)


def ptr_table(torch_, tensors):
    """int64 device tensor of device pointers; None = idle slot"""
    return torch_.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch_.int64, device="cuda")


# ---------------------------------------------------------------- GEMV
def upload(hip, rng, rows, cols, fmt):
    if fmt == "qk256":
        return hip.weights_upload_qk256(rng.integers(0, 256, rows * cols // 4, dtype=np.uint8), rows, cols, cols // 4)
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(rows, cols), p=[0.5, 0.25, 0.25])
    packed = (codes[:, 0::4] | codes[:, 1::4] << 2 | codes[:, 2::4] << 4 | codes[:, 3::4] << 6).astype(np.uint8).reshape(-1)
    scales = rng.uniform(0.01, 2.0, rows * cols // 32).astype(np.float16).astype(np.float32)  # BitNet32-F16: every scale an f16 value
    return hip.weights_upload_i2s(packed, scales, rows, cols, 32)


def slot_vector(rng, kind, cols):
    if kind == "zeros":
        return np.zeros(cols, np.float32)
    if kind == "1e4":
        return (rng.normal(0, 1, cols) * 1e4).astype(np.float32)
    x = (rng.normal(0.05, 1, cols) * rng.choice([0.01, 1.0, 30.0], cols)).astype(np.float32)
    if kind == "tiny":
        x[32:48] = 1e-30 * rng.choice([-1.0, 1.0], 16)  # a whole 16-group far below the format's smallest scale
    return x


KINDS = ["rand", "zeros", "1e4", "tiny", "rand", "rand", "rand", "rand"]  # slot contents differ on purpose: leakage between slots would show
SHAPES = [(48, 256, False), (272, 512, False), (3840, 2560, False), (2560, 2560, False), (2560, 6912, False), (13824, 2560, True),
          (64, 2560, True), (16, 4352, False)]
# (2560, 6912): four blocks per wave, two copy passes in batch-1, a second copy round for 8 vectors here; (48, 256): fewer row tiles than waves.
# Ring depths (blocks per wave, bitnet_hip_gemv_q_geometry): 2, 2, 2, 2, 4, 5, and the last two for the one that was missing: (64, 2560) paired =
# 10 blocks over 4 K parts, (16, 4352) = 17 blocks over 8 K parts: 3 each.


@pytest.mark.parametrize("fmt", ["qk256", "f16"])
@pytest.mark.parametrize("rows,cols,paired", SHAPES)
def test_gemv_batch_bits_equal_batch1(hip, torch_, rows, cols, paired, fmt):
    rng = np.random.default_rng(rows * 7 + cols + (fmt == "f16"))
    if paired:
        ha, hb = upload(hip, rng, rows // 2, cols, fmt), upload(hip, rng, rows // 2, cols, fmt)
        h = hip.weights_concat([ha, hb], interleave16=True)
    else:
        h = upload(hip, rng, rows, cols, fmt)
    assert hip.gemv_q_supported(h)
    out_rows = rows // 2 if paired else rows
    flags = 1 if paired else 0
    ln_ok = cols <= 4096  # the QAct GEMV's LayerNorm form stops there (batch-1 refuses beyond)
    gamma_in = dev(torch_, (rng.uniform(0.5, 1.5, cols) / (1.58 * np.sqrt(cols))).astype(np.float32))
    if ln_ok:
        hip.weights_bind_ln(h, gamma_in)
    gamma_out = dev(torch_, rng.uniform(0.5, 1.5, out_rows).astype(np.float32))
    qb, sb = hip.qact_bytes(cols), hip.qact_stats_bytes(cols)
    qob, sob = hip.qact_bytes(out_rows), hip.qact_stats_bytes(out_rows)
    option_sets = ["y", "qact"] + (["ln"] if ln_ok else []) + ([] if paired else ["residual"])
    for n_seq in (1, 2, 3, 5, 8):
        xs = [slot_vector(rng, KINDS[b], cols) for b in range(n_seq)]
        res = dev(torch_, rng.normal(0, 1, (n_seq, out_rows)).astype(np.float32))
        for opt in option_sets:
            ln = opt == "ln"
            # inputs: one QAct (+ statistics) per vector, quantised by the library's own producer
            qin = torch_.zeros(n_seq * qb, dtype=torch_.uint8, device="cuda")
            stin = torch_.zeros(n_seq * sb // 8, dtype=torch_.float64, device="cuda")
            for b in range(n_seq):
                hip.quantize_act_dev(dev(torch_, xs[b]), gamma_in if ln else None, cols, qin[b * qb:(b + 1) * qb], stin[b * sb // 8:(b + 1) * sb // 8])
            kw = dict(flags=flags)
            if ln:
                kw.update(ln_gamma=gamma_in, ln_eps=1e-5)
            want_y, want_q, want_s = opt != "qact", opt == "qact", opt == "qact"
            nan = float("nan")
            yb = torch_.full((n_seq, out_rows), nan, device="cuda") if want_y else None
            qo = torch_.full((n_seq * qob,), 0xA5, dtype=torch_.uint8, device="cuda") if want_q else None
            so = torch_.full((n_seq * sob // 8,), nan, dtype=torch_.float64, device="cuda") if want_s else None
            hip.gemv_q_batch_dev(h, n_seq, qin, y=yb, stats_in=stin if ln else None, residual=res if opt == "residual" else None, qact_out=qo,
                                 gamma_out=gamma_out if want_q else None, stats_out=so, **kw)
            # batch-1 on private copies
            qin1, stin1, res1 = qin.clone(), stin.clone(), res.clone()
            y1 = torch_.full((n_seq, out_rows), nan, device="cuda") if want_y else None
            q1 = torch_.full((n_seq * qob,), 0xA5, dtype=torch_.uint8, device="cuda") if want_q else None
            s1 = torch_.full((n_seq * sob // 8,), nan, dtype=torch_.float64, device="cuda") if want_s else None
            for b in range(n_seq):
                hip.gemv_q_dev(h, qin1[b * qb:(b + 1) * qb], y=y1[b] if want_y else None, stats_in=stin1[b * sb // 8:(b + 1) * sb // 8] if ln else None,
                               residual=res1[b] if opt == "residual" else None, qact_out=q1[b * qob:(b + 1) * qob] if want_q else None,
                               gamma_out=gamma_out if want_q else None, stats_out=s1[b * sob // 8:(b + 1) * sob // 8] if want_s else None, **kw)
            torch_.cuda.synchronize()
            tag = (rows, cols, fmt, n_seq, opt)
            if want_y:
                got, want = bits(yb).reshape(n_seq, -1), bits(y1).reshape(n_seq, -1)
                assert not np.isnan(y1.cpu().numpy()).any(), tag
                for b in range(n_seq):
                    assert np.array_equal(got[b], want[b]), (tag, b)
            if want_q:
                got, want = bits(qo).reshape(n_seq, -1), bits(q1).reshape(n_seq, -1)
                for b in range(n_seq):
                    assert np.array_equal(got[b], want[b]), (tag, b, "qact")
                assert np.array_equal(bits(so), bits(s1)), (tag, "stats")
            assert np.array_equal(bits(qin), bits(qin1)) and np.array_equal(bits(res), bits(res1))  # inputs untouched
    hip.weights_free(h)
    if paired:
        hip.weights_free(ha), hip.weights_free(hb)


# ---------------------------------------------------------------- attention
POSITIONS = [0, 63, 64, 127, 128, 191, 200, 319]


@pytest.mark.parametrize("kv_f16", [False, True])
@pytest.mark.parametrize("n_heads,n_kv", [(20, 5), (2, 2), (6, 2)])
def test_attention_batch_bits_equal_batch1(hip, oracle, torch_, n_heads, n_kv, kv_f16):
    D, max_pos, n_seq = 128, 320, 8
    rng = np.random.default_rng(n_heads * 3 + n_kv + kv_f16)
    sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
    sin_d, cos_d = dev(torch_, sin), dev(torch_, cos)
    cols = n_heads * D
    qkv_len = (n_heads + 2 * n_kv) * D
    sbytes = hip.c.bitnet_hip_attention_scratch_bytes(n_kv, max_pos)
    qb = hip.qact_bytes(cols)
    cdt = np.float16 if kv_f16 else np.float32
    qkv = dev(torch_, rng.normal(0, 1.5, (n_seq, qkv_len)).astype(np.float32))
    kc0 = [rng.normal(0, 1, n_kv * max_pos * D).astype(cdt) for _ in range(n_seq)]  # pre-filled with random FINITE values (also past the position)
    vc0 = [rng.normal(0, 1, n_kv * max_pos * D).astype(cdt) for _ in range(n_seq)]
    pos = [torch_.tensor([p], dtype=torch_.int32, device="cuda") for p in POSITIONS]
    # batch-1 on private copies
    k1, v1 = [dev(torch_, a) for a in kc0], [dev(torch_, a) for a in vc0]
    out1 = torch_.full((n_seq, cols), float("nan"), device="cuda")
    q1 = torch_.full((n_seq, qb), 0xA5, dtype=torch_.uint8, device="cuda")
    for b in range(n_seq):
        s1 = torch_.zeros(sbytes // 4, device="cuda")
        hip.attention_decode_q_dev(qkv[b].clone(), sin_d, cos_d, k1[b], v1[b], n_heads, n_kv, D, max_pos, pos[b].clone(), s1, out1[b], q1[b], kv_f16=kv_f16)
    torch_.cuda.synchronize()
    assert not np.isnan(out1.cpu().numpy()).any()
    for idle in ((), (2, 5)):
        k2, v2 = [dev(torch_, a) for a in kc0], [dev(torch_, a) for a in vc0]
        live = [b not in idle for b in range(n_seq)]
        kt = ptr_table(torch_, [k2[b] if live[b] else None for b in range(n_seq)])
        vt = ptr_table(torch_, [v2[b] if live[b] else None for b in range(n_seq)])
        pt = ptr_table(torch_, [pos[b] if live[b] else None for b in range(n_seq)])
        SENT = 0x5A
        scratch = torch_.zeros(n_seq * sbytes, dtype=torch_.uint8, device="cuda")
        out2 = torch_.full((n_seq, cols), float("nan"), device="cuda")
        q2 = torch_.full((n_seq, qb), 0xA5, dtype=torch_.uint8, device="cuda")
        for b in idle:
            scratch[b * sbytes:(b + 1) * sbytes] = SENT
            out2[b].view(torch_.uint8)[:] = SENT
            q2[b] = SENT
        hip.attention_decode_batch_dev(qkv, sin_d, cos_d, kt, vt, pt, n_seq, n_heads, n_kv, D, max_pos, scratch, out2, q2, kv_f16=kv_f16)
        torch_.cuda.synchronize()
        for b in range(n_seq):
            tag = (n_heads, n_kv, kv_f16, idle, b)
            if live[b]:
                assert np.array_equal(bits(out2[b]), bits(out1[b])), tag
                assert np.array_equal(bits(q2[b]), bits(q1[b])), tag
                assert np.array_equal(bits(k2[b]), bits(k1[b])) and np.array_equal(bits(v2[b]), bits(v1[b])), tag
            else:  # an idle slot: caches, records and outputs byte-for-byte unchanged
                assert np.all(bits(out2[b]) == SENT) and np.all(bits(q2[b]) == SENT), tag
                assert np.all(bits(scratch[b * sbytes:(b + 1) * sbytes]) == SENT), tag
                assert np.array_equal(bits(k2[b]), kc0[b].view(np.uint8)) and np.array_equal(bits(v2[b]), vc0[b].view(np.uint8)), tag
        for b in range(n_seq):
            assert int(pos[b].item()) == POSITIONS[b]  # the attention never moves a position


# ---------------------------------------------------------------- embedding gather
def test_embed_batch_bits_equal_batch1(hip, torch_):
    hidden, vocab, n_seq = 512, 100, 6
    rng = np.random.default_rng(4)
    table = dev(torch_, rng.normal(0, 1, (vocab, hidden)).astype(np.float16))
    gamma = dev(torch_, rng.uniform(0.5, 1.5, hidden).astype(np.float32))
    # slot 1 reads an id below 0, slot 3 one >= vocab (both clamped as in batch-1), slot 4 is idle
    hist = [torch_.tensor(h, dtype=torch_.int32, device="cuda") for h in ([5, 17, 3], [9, -3, 4], [99, 0, 1], [1, 2, vocab + 41], [7, 7, 7], [0, 50, 2])]
    posv = [2, 1, 0, 2, 1, 1]
    pos = [torch_.tensor([p], dtype=torch_.int32, device="cuda") for p in posv]
    qb, sb = hip.qact_bytes(hidden), hip.qact_stats_bytes(hidden)
    SENT = 0x5A
    x2 = torch_.full((n_seq, hidden), float("nan"), device="cuda")
    q2 = torch_.full((n_seq, qb), 0xA5, dtype=torch_.uint8, device="cuda")
    s2 = torch_.full((n_seq, sb // 8), float("nan"), dtype=torch_.float64, device="cuda")
    x2[4].view(torch_.uint8)[:] = SENT
    q2[4] = SENT
    s2[4].view(torch_.uint8)[:] = SENT
    ht = ptr_table(torch_, [None if b == 4 else hist[b] for b in range(n_seq)])
    pt = ptr_table(torch_, pos)
    hip.embed_q_batch_dev(table, ht, pt, n_seq, hidden, vocab, x2, gamma, q2, s2)
    torch_.cuda.synchronize()
    for b in range(n_seq):
        if b == 4:
            assert np.all(bits(x2[b]) == SENT) and np.all(bits(q2[b]) == SENT) and np.all(bits(s2[b]) == SENT)
            continue
        x1 = torch_.full((hidden,), float("nan"), device="cuda")
        q1 = torch_.full((qb,), 0xA5, dtype=torch_.uint8, device="cuda")
        s1 = torch_.full((sb // 8,), float("nan"), dtype=torch_.float64, device="cuda")
        hip.embed_q_dev(table, hist[b].clone(), x1, hidden, vocab, gamma, q1, s1, offset=pos[b].clone())
        torch_.cuda.synchronize()
        assert np.array_equal(bits(x2[b]), bits(x1)) and np.array_equal(bits(q2[b]), bits(q1)) and np.array_equal(bits(s2[b]), bits(s1)), b
        tok = int(np.clip(hist[b].cpu().numpy()[posv[b]], 0, vocab - 1))
        assert np.array_equal(x1.cpu().numpy(), table[tok].float().cpu().numpy())


# ---------------------------------------------------------------- logits head + greedy pick
@pytest.mark.parametrize("hidden,vocab", [(512, 1000), (2560, 4096)])
def test_head_batch_bits_equal_batch1(hip, torch_, hidden, vocab):
    rng = np.random.default_rng(hidden + vocab)
    n_seq, n_wg, max_pos = 5, 40, 16
    half = rng.normal(0, 1, (vocab // 2, hidden)).astype(np.float16)
    table = dev(torch_, np.concatenate([half, half]))  # every row twice: every maximum is a tie -> the lowest index wins
    gamma = dev(torch_, rng.uniform(0.5, 1.5, hidden).astype(np.float32))
    xs = rng.normal(0.1, 1.0, (n_seq, hidden)).astype(np.float32)
    xs[1, 37] = np.nan  # slot 1: a NaN column -> every logit NaN -> -inf for the pick
    x = dev(torch_, xs)
    # slot 0 greedy, 1 NaN, 2 at a FORCED position (history kept, position advances), 3 logits only, 4 idle
    p0 = [3, 0, 5, 7, 2]
    forced = [0, 0, 9, 0, 0]
    mk = lambda: dict(pos=[torch_.tensor([p], dtype=torch_.int32, device="cuda") for p in p0],
                      hist=[torch_.full((max_pos,), -7, dtype=torch_.int32, device="cuda") for _ in range(n_seq)],
                      nf=[torch_.tensor([f], dtype=torch_.int32, device="cuda") for f in forced],
                      tok=[torch_.full((1,), -1, dtype=torch_.int32, device="cuda") for _ in range(n_seq)],
                      logits=[torch_.full((vocab,), 123.0, device="cuda") for _ in range(n_seq)])
    one, bat = mk(), mk()
    for b in (0, 1, 2):
        hip.logits_f16_dev(table, x[b].clone(), gamma, 1e-5, hidden, vocab, one["logits"][b], torch_.zeros(2 * n_wg, device="cuda"), n_wg, token=one["tok"][b],
                           pos=one["pos"][b], history=one["hist"][b], n_forced=one["nf"][b])
    hip.logits_f16_dev(table, x[3].clone(), gamma, 1e-5, hidden, vocab, one["logits"][3], torch_.zeros(2 * n_wg, device="cuda"), n_wg)
    pick = lambda key: ptr_table(torch_, [bat[key][b] if b < 3 else None for b in range(n_seq)])
    lt = ptr_table(torch_, [bat["logits"][b] if b < 4 else None for b in range(n_seq)])
    hip.logits_f16_batch_dev(table, x, gamma, 1e-5, hidden, vocab, n_seq, lt, torch_.zeros(2 * n_wg * n_seq, device="cuda"), n_wg, token_ptrs=pick("tok"),
                             pos_ptrs=pick("pos"), history_ptrs=pick("hist"), n_forced_ptrs=pick("nf"))
    torch_.cuda.synchronize()
    for b in range(n_seq):
        for key in ("logits", "pos", "hist", "tok"):
            assert np.array_equal(bits(bat[key][b]), bits(one[key][b])), (b, key)
    lg = one["logits"][0].cpu().numpy()
    assert int(one["tok"][0].item()) == int(np.argmax(lg)) < vocab // 2 and lg[int(np.argmax(lg))] == lg[int(np.argmax(lg)) + vocab // 2]  # the tie, lowest index
    assert int(bat["pos"][0].item()) == 4 and int(bat["hist"][0][4].item()) == int(bat["tok"][0].item())
    assert np.isnan(bat["logits"][1].cpu().numpy()).all() and int(bat["tok"][1].item()) == 0 and int(bat["pos"][1].item()) == 1
    assert int(bat["pos"][2].item()) == 6 and np.all(bat["hist"][2].cpu().numpy() == -7)              # forced: history kept, position advanced
    assert int(bat["pos"][3].item()) == 7 and np.all(bat["hist"][3].cpu().numpy() == -7) and int(bat["tok"][3].item()) == -1  # logits only
    assert np.all(bat["logits"][4].cpu().numpy() == 123.0) and int(bat["pos"][4].item()) == 2          # idle
