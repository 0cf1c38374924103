"""GPU: the wide decode step's kernels (csrc/kernels_wide.hip, k_attn_*_rows in csrc/kernels_attn.hip) against the entry points they share their
arithmetic with, run on private copies of the same inputs.

The rows attention is built on the bodies of the batched and the batch-1 decode attention, and the gather on k_embed_f16's conversion: they promise the
SAME BITS per sequence, so every comparison here is array_equal on raw bit patterns (the batch-1 kernels are pinned to the oracle and to float64
elsewhere: test_decode_parity.py, test_decoder_state_gpu.py).  The hand-over kernel is held to a numpy restatement of its contract.

Head counts of models A and B of tests/test_decoder_state_gpu.py (4 / 2 and 6 / 3, max_pos 300: the last cache tile is padding), both cache types."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_batch_ops_gpu import bits, dev, ptr_table, torch_  # noqa: E402,F401
from test_decoder_state_gpu import MODELS  # noqa: E402

pytestmark = pytest.mark.gpu

D = 128
SPREAD = [0, 1, 63, 64, 65, 127, 128, 298]
SENT = 0x5A
CASES = [(m, k) for m in ("A", "B") for k in (False, True)]
case_id = lambda c: f"{c[0]}-{'kv16' if c[1] else 'kv32'}"


class Ctx:
    """one (model, cache type): rope tables, per-sequence qkv rows and pre-filled caches (random FINITE values, also past the position)"""

    def __init__(self, hip, oracle, torch_, model, kv_f16, n_seq, positions, seed):
        m = MODELS[model]
        self.hip, self.t, self.kv_f16, self.n_seq, self.positions = hip, torch_, kv_f16, n_seq, list(positions)
        self.n_heads, self.n_kv, self.max_pos = m["n_heads"], m["n_kv_heads"], m["max_pos"]
        rng = np.random.default_rng(seed)
        sin, cos = oracle.rope_tables(D, self.max_pos, m["rope_theta"])
        self.sin, self.cos = dev(torch_, sin), dev(torch_, cos)
        self.cols = self.n_heads * D
        self.sbytes = hip.c.bitnet_hip_attention_scratch_bytes(self.n_kv, self.max_pos)
        slots = (self.max_pos + 63) // 64 * 64  # whole 64-position tiles
        cdt = np.float16 if kv_f16 else np.float32
        self.qkv = dev(torch_, rng.normal(0, 1.5, (n_seq, (self.n_heads + 2 * self.n_kv) * D)).astype(np.float32))
        self.kc0 = [rng.normal(0, 1, self.n_kv * slots * D).astype(cdt) for _ in range(n_seq)]
        self.vc0 = [rng.normal(0, 1, self.n_kv * slots * D).astype(cdt) for _ in range(n_seq)]
        self.pos = [torch_.tensor([p], dtype=torch_.int32, device="cuda") for p in self.positions]

    def caches(self):
        return [dev(self.t, a) for a in self.kc0], [dev(self.t, a) for a in self.vc0]

    def rows(self, key_bound, idle=(), out_f16=False):
        """-> (out [n_seq, cols] pre-filled with the sentinel, K caches, V caches, scratch pre-filled with the sentinel in idle / out-of-bound areas)"""
        t, n = self.t, self.n_seq
        k, v = self.caches()
        live = [b not in idle for b in range(n)]
        kt = ptr_table(t, [k[b] if live[b] else None for b in range(n)])
        vt = ptr_table(t, [v[b] if live[b] else None for b in range(n)])
        pt = ptr_table(t, [self.pos[b] if live[b] else None for b in range(n)])
        scratch = t.zeros(n * self.sbytes, dtype=t.uint8, device="cuda")
        for b in range(n):
            if not live[b] or self.positions[b] >= key_bound:
                scratch[b * self.sbytes:(b + 1) * self.sbytes] = SENT
        out = t.full((n, self.cols * (2 if out_f16 else 4)), SENT, dtype=t.uint8, device="cuda")
        self.hip.attention_decode_rows_dev(self.qkv, self.sin, self.cos, kt, vt, pt, n, self.n_heads, self.n_kv, D, self.max_pos, key_bound, scratch, out,
                                           kv_f16=self.kv_f16, out_f16=out_f16)
        t.cuda.synchronize()
        for b in range(n):
            assert int(self.pos[b].item()) == self.positions[b]  # the attention never moves a position
        return out, k, v, scratch

    def untouched(self, b, out, k, v, scratch, tag):
        assert np.all(bits(out[b]) == SENT), (tag, "output row")
        assert np.all(bits(scratch[b * self.sbytes:(b + 1) * self.sbytes]) == SENT), (tag, "records")
        assert np.array_equal(bits(k[b]), self.kc0[b].view(np.uint8)) and np.array_equal(bits(v[b]), self.vc0[b].view(np.uint8)), (tag, "caches")


@pytest.mark.parametrize("n_seq", [1, 2, 8])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rows_attention_bits_equal_the_batched_attention(hip, oracle, torch_, case, n_seq):
    model, kv_f16 = case
    positions = {1: [298], 2: [64, 0], 8: SPREAD}[n_seq]
    c = Ctx(hip, oracle, torch_, model, kv_f16, n_seq, positions, seed=11 * n_seq + kv_f16)
    # the batched entry on private copies
    k1, v1 = c.caches()
    out1 = torch_.full((n_seq, c.cols), float("nan"), device="cuda")
    s1 = torch_.zeros(n_seq * c.sbytes, dtype=torch_.uint8, device="cuda")
    hip.attention_decode_batch_dev(c.qkv, c.sin, c.cos, ptr_table(torch_, k1), ptr_table(torch_, v1), ptr_table(torch_, c.pos), n_seq, c.n_heads, c.n_kv, D, c.max_pos,
                                   s1, out1, None, kv_f16=kv_f16)
    torch_.cuda.synchronize()
    assert not np.isnan(out1.cpu().numpy()).any()
    out2, k2, v2, _ = c.rows(c.max_pos)
    for b in range(n_seq):
        tag = (case, n_seq, b, positions[b])
        assert np.array_equal(bits(out2[b]), bits(out1[b])), tag
        assert np.array_equal(bits(k2[b]), bits(k1[b])) and np.array_equal(bits(v2[b]), bits(v1[b])), tag


@pytest.mark.parametrize("n_seq", [9, 33, 64])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rows_attention_bits_equal_batch1_per_sequence(hip, oracle, torch_, case, n_seq):
    """positions spread over the record boundaries, one idle row; then the f16 rows, the tight key bound and sequences beyond a bound"""
    model, kv_f16 = case
    positions = [SPREAD[(3 * b + b // 8) % 8] for b in range(n_seq)]
    assert set(positions) == set(SPREAD)
    idle = (n_seq // 2,)
    c = Ctx(hip, oracle, torch_, model, kv_f16, n_seq, positions, seed=5 * n_seq + kv_f16)
    # batch-1, 64-position records + combine, on private copies of each sequence alone
    k1, v1 = c.caches()
    out1 = torch_.full((n_seq, c.cols), float("nan"), device="cuda")
    q1 = torch_.zeros((n_seq, hip.qact_bytes(c.cols)), dtype=torch_.uint8, device="cuda")
    for b in range(n_seq):
        s1 = torch_.zeros(c.sbytes // 4, device="cuda")
        hip.attention_decode_q_dev(c.qkv[b].clone(), c.sin, c.cos, k1[b], v1[b], c.n_heads, c.n_kv, D, c.max_pos, c.pos[b].clone(), s1, out1[b], q1[b], kv_f16=kv_f16)
    torch_.cuda.synchronize()
    assert not np.isnan(out1.cpu().numpy()).any()
    out2, k2, v2, s2 = c.rows(c.max_pos, idle=idle)
    for b in range(n_seq):
        tag = (case, n_seq, b, positions[b])
        if b in idle:
            c.untouched(b, out2, k2, v2, s2, tag)
            continue
        assert np.array_equal(bits(out2[b]), bits(out1[b])), tag
        assert np.array_equal(bits(k2[b]), bits(k1[b])) and np.array_equal(bits(v2[b]), bits(v1[b])), tag
    # OUT_F16: every value is the f32 value rounded once to nearest-even; the caches are the same bytes
    out3, k3, v3, _ = c.rows(c.max_pos, idle=idle, out_f16=True)
    want16 = out1.to(torch_.float16)
    for b in range(n_seq):
        if b in idle:
            continue
        assert np.array_equal(bits(out3[b]), bits(want16[b])), (case, n_seq, b, "f16 row")
        assert np.array_equal(bits(k3[b]), bits(k1[b])) and np.array_equal(bits(v3[b]), bits(v1[b])), (case, n_seq, b, "f16 row: caches")
    # key_bound = the largest position + 1: the same bits as key_bound = max_pos
    out4, k4, v4, _ = c.rows(max(positions) + 1, idle=idle)
    for b in range(n_seq):
        assert np.array_equal(bits(out4[b]), bits(out2[b])), (case, n_seq, b, "tight bound")
        assert np.array_equal(bits(k4[b]), bits(k2[b])) and np.array_equal(bits(v4[b]), bits(v2[b])), (case, n_seq, b, "tight bound: caches")
    # a sequence AT or BEYOND the bound is idle for the launch (caches, records and output row keep their bytes); the others are served as before
    for bound in (65, 1, 128):
        out5, k5, v5, s5 = c.rows(bound, idle=idle)
        for b in range(n_seq):
            tag = (case, n_seq, b, positions[b], f"key_bound {bound}")
            if b in idle or positions[b] >= bound:
                c.untouched(b, out5, k5, v5, s5, tag)
            else:
                assert np.array_equal(bits(out5[b]), bits(out2[b])), tag
                assert np.array_equal(bits(k5[b]), bits(k2[b])) and np.array_equal(bits(v5[b]), bits(v2[b])), tag


def test_embed_rows_bits_equal_embed_f16(hip, torch_):
    hidden, vocab, n_seq = 512, 100, 7
    rng = np.random.default_rng(4)
    table = dev(torch_, rng.normal(0, 1, (vocab, hidden)).astype(np.float16))
    # row 1 reads an id below 0, row 3 one >= vocab (both clamped as in embed_f16_dev), row 4 has no history, row 6 no position: idle, zero-filled
    hist = [torch_.tensor(h, dtype=torch_.int32, device="cuda") for h in ([5, 17, 3], [9, -3, 4], [99, 0, 1], [1, 2, vocab + 41], [7, 7, 7], [0, 50, 2], [3, 3, 3])]
    posv = [2, 1, 0, 2, 1, 1, 0]
    pos = [torch_.tensor([p], dtype=torch_.int32, device="cuda") for p in posv]
    x2 = torch_.full((n_seq + 1, hidden), float("nan"), device="cuda")
    ht = ptr_table(torch_, [None if b == 4 else hist[b] for b in range(n_seq)])
    pt = ptr_table(torch_, [None if b == 6 else pos[b] for b in range(n_seq)])
    hip.embed_rows_dev(table, ht, pt, n_seq, hidden, vocab, x2)
    torch_.cuda.synchronize()
    assert np.isnan(x2[n_seq].cpu().numpy()).all()  # nothing beyond row n_seq - 1
    for b in range(n_seq):
        if b in (4, 6):
            assert np.all(bits(x2[b]) == 0), b
            continue
        x1 = torch_.full((hidden,), float("nan"), device="cuda")
        hip.embed_f16_dev(table, hist[b].clone(), x1, 1, hidden, vocab, offset=pos[b].clone())
        torch_.cuda.synchronize()
        assert np.array_equal(bits(x2[b]), bits(x1)), b
        tok = int(np.clip(hist[b].cpu().numpy()[posv[b]], 0, vocab - 1))
        assert np.array_equal(x1.cpu().numpy(), table[tok].float().cpu().numpy())
    for b in range(n_seq):
        assert int(pos[b].item()) == posv[b]


@pytest.mark.parametrize("vocab", [1000, 2047, 4099])
def test_pick_rows_against_a_numpy_restatement(hip, torch_, vocab):
    """row 0 greedy with a tie, 1 an all-NaN row, 2 at a FORCED position, 3 logits only (it samples), 4 idle, 5 greedy without a history, 6 a token
    pointer alone; vocab 1000: the 16-byte copy, 2047 / 4099: the element copy (4099: more than one pass of a block)"""
    rng = np.random.default_rng(vocab)
    n_seq, max_pos = 7, 16
    lg = rng.normal(0, 3, (n_seq, vocab)).astype(np.float32)
    lg[0, 700] = lg[0, 41] = 99.0  # the tie: the head's argmax is the lowest index
    lg[1, :] = np.nan
    am = np.array([41, 0, int(np.argmax(lg[2])), int(np.argmax(lg[3])), 5, int(np.argmax(lg[5])), int(np.argmax(lg[6]))], np.int32)
    p0 = [3, 0, 5, 7, 2, 9, 4]
    forced = [0, 0, 9, 0, 0, 0, 0]
    pos = [torch_.tensor([p], dtype=torch_.int32, device="cuda") for p in p0]
    hist = [torch_.full((max_pos,), -7, dtype=torch_.int32, device="cuda") for _ in range(n_seq)]
    nf = [torch_.tensor([f], dtype=torch_.int32, device="cuda") for f in forced]
    tok = [torch_.full((1,), -1, dtype=torch_.int32, device="cuda") for _ in range(n_seq)]
    rows = [torch_.full((vocab,), 123.0, device="cuda") for _ in range(n_seq)]
    lt = ptr_table(torch_, [None if b == 4 else rows[b] for b in range(n_seq)])
    tt = ptr_table(torch_, [tok[b] if b in (0, 1, 2, 5, 6) else None for b in range(n_seq)])
    pt = ptr_table(torch_, [pos[b] if b in (0, 1, 2, 5) else None for b in range(n_seq)])
    ht = ptr_table(torch_, [hist[b] if b in (0, 1, 2, 3, 6) else None for b in range(n_seq)])
    ft = ptr_table(torch_, [nf[b] if b in (0, 1, 2) else None for b in range(n_seq)])
    hip.pick_rows_dev(dev(torch_, lg), dev(torch_, am), n_seq, vocab, lt, token_ptrs=tt, pos_ptrs=pt, history_ptrs=ht, n_forced_ptrs=ft)
    torch_.cuda.synchronize()
    # ---- the restatement ----
    w_rows = [np.full(vocab, 123.0, np.float32) for _ in range(n_seq)]
    w_tok, w_pos, w_hist = [-1] * n_seq, list(p0), [np.full(max_pos, -7, np.int32) for _ in range(n_seq)]
    for b in range(n_seq):
        if b == 4:
            continue  # no logits pointer: idle
        w_rows[b] = lg[b]
        has_tok, has_pos = b in (0, 1, 2, 5, 6), b in (0, 1, 2, 5)
        if not has_tok and not has_pos:
            continue  # logits only
        if has_tok:
            w_tok[b] = int(am[b])
        if has_pos:
            p = p0[b]
            if b in (0, 1, 2, 3, 6) and not (b in (0, 1, 2) and p + 1 < forced[b]):
                w_hist[b][p + 1] = int(am[b])
            w_pos[b] = p + 1
    for b in range(n_seq):
        assert np.array_equal(bits(rows[b]), w_rows[b].view(np.uint8)), (b, "logits row")
        assert int(tok[b].item()) == w_tok[b] and int(pos[b].item()) == w_pos[b], (b, int(tok[b].item()), int(pos[b].item()))
        assert np.array_equal(hist[b].cpu().numpy(), w_hist[b]), (b, "history")
    assert int(hist[0][4].item()) == 41 and np.all(hist[2].cpu().numpy() == -7) and int(pos[2].item()) == 6  # the tie's lowest index; forced: kept, advanced
    # without any of the optional tables: logits only, for every bound row
    rows2 = [torch_.full((vocab,), 123.0, device="cuda") for _ in range(n_seq)]
    hip.pick_rows_dev(dev(torch_, lg), dev(torch_, am), n_seq, vocab, ptr_table(torch_, rows2))
    torch_.cuda.synchronize()
    for b in range(n_seq):
        assert np.array_equal(bits(rows2[b]), lg[b].view(np.uint8)), b
        assert int(pos[b].item()) == w_pos[b]
