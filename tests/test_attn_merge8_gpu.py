"""GPU: the o-projection that merges up to 8 attention chunk records itself (bitnet_hip_gemv_attn_merge_rec_q_dev, k_gemv_q's
merging prologue with NR = 8) and the decoder form that uses it from 257 keys (Decoder::form_at, form 3).

 1. against attention + combine kernel + plain o-projection: the bounds of test_merging_oproj_on_qact_path_equals_combine_then_project
    (tests/test_qact_gpu.py), contexts of 1..8 records, a record buffer of 16 records with stale finite values and one of 5
    records (the record index clamp);
 2. 8-record entry against the 4-record one while at most 4 records are live: bit-identical (masked records add exact zeros);
    from 5 live records bit-identical to the combine kernel + plain o-projection (case 1 asserts it at >= 257 keys);
 3. the decoder across 256 / 257 keys and across the form's upper bound against Decoder::run_reference on the same tokens."""
import importlib

import numpy as np
import pytest

from tests.qact_ref import dequantize_qact, quantize_qact

pytestmark = pytest.mark.gpu

D, ROWS = 128, 640
POSITIONS = (0, 63, 255, 256, 257, 319, 320, 383, 447, 448, 511)
MERGE8_MAX_KEYS = 512  # Decoder::kMerge8MaxKeys (EXPERIMENTS 15.2)


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module("bitnet-rs_amd.synth")


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(hip, rng, fmt, cols):
    codes = rng.integers(0, 256, ROWS * cols // 4, dtype=np.uint8)
    if fmt == "qk256":
        return hip.weights_upload_qk256(codes, ROWS, cols, cols // 4)
    sc = rng.uniform(0.05, 1.0, ROWS * cols // 32).astype(np.float16).astype(np.float32)
    return hip.weights_upload_i2s(codes, sc, ROWS, cols, 32)


class Case:
    """One (heads, format, cache size): weights, tables and per-position inputs, made once."""

    def __init__(self, hip, oracle, torch_, n_heads, n_kv, fmt, max_pos):
        self.n_heads, self.n_kv, self.max_pos, self.cols = n_heads, n_kv, max_pos, n_heads * D
        rng = np.random.default_rng(131 * n_heads + 7 * n_kv + max_pos)
        self.rng = rng
        self.w = upload(hip, rng, fmt, self.cols)
        assert hip.gemv_q_supported(self.w)
        sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
        self.sin, self.cos = dev(torch_, sin), dev(torch_, cos)
        self.sb = hip.c.bitnet_hip_attention_scratch_bytes(n_kv, max_pos)
        self.gam = dev(torch_, rng.uniform(0.5, 1.5, ROWS).astype(np.float32))
        n = n_kv * max_pos * D
        self.kc, self.vc = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)

    def inputs(self, torch_):
        qkv = dev(torch_, self.rng.normal(0, 1.5, (self.n_heads + 2 * self.n_kv) * D).astype(np.float32))
        res = dev(torch_, self.rng.normal(0, 1, ROWS).astype(np.float32))
        return qkv, res

    def merged(self, hip, torch_, qkv, res, pos, records):
        """partial attention + merging o-projection on a record buffer pre-filled with 3.0 (stale but finite)"""
        z = lambda n, dt=torch_.uint8: torch_.zeros(n, dtype=dt, device="cuda")
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        k, v, s = dev(torch_, self.kc), dev(torch_, self.vc), torch_.zeros(self.sb // 4 + 16, device="cuda") + 3.0
        y, q, st = z(ROWS, torch_.float32), z(hip.qact_bytes(ROWS)), z(ROWS // 16 * 2, torch_.float64)
        hip.attention_decode_partial_dev(qkv, self.sin, self.cos, k, v, self.n_heads, self.n_kv, D, self.max_pos, pos_d, s)
        if records == 0:
            hip.gemv_attn_merge_q_dev(self.w, s, self.n_heads, self.n_kv, self.max_pos, pos_d, y, q, residual=res, gamma_out=self.gam, stats_out=st)
        else:
            hip.gemv_attn_merge_rec_q_dev(self.w, s, self.n_heads, self.n_kv, self.max_pos, pos_d, y, q, records, residual=res, gamma_out=self.gam,
                                          stats_out=st)
        torch_.cuda.synchronize()
        return y.cpu().numpy(), q.cpu().numpy(), st.cpu().numpy(), k, v

    def combined(self, hip, torch_, qkv, res, pos):
        z = lambda n, dt=torch_.uint8: torch_.zeros(n, dtype=dt, device="cuda")
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        k, v, s = dev(torch_, self.kc), dev(torch_, self.vc), torch_.zeros(self.sb // 4 + 16, device="cuda")
        qa, y, q, st = z(hip.qact_bytes(self.cols)), z(ROWS, torch_.float32), z(hip.qact_bytes(ROWS)), z(ROWS // 16 * 2, torch_.float64)
        hip.attention_decode_q_dev(qkv, self.sin, self.cos, k, v, self.n_heads, self.n_kv, D, self.max_pos, pos_d, s, None, qa)
        hip.gemv_q_dev(self.w, qa, y=y, residual=res, qact_out=q, gamma_out=self.gam, stats_out=st)
        torch_.cuda.synchronize()
        return y.cpu().numpy(), q.cpu().numpy(), st.cpu().numpy(), k, v


def test_library_queries(hip):
    assert hip.attention_merge_q_max_keys() == 512
    assert int(hip.c.bitnet_hip_attention_merge_max_keys()) == 256


@pytest.mark.parametrize("max_pos", [1024, 320])
@pytest.mark.parametrize("n_heads,n_kv,fmt", [(8, 2, "qk256"), (4, 2, "qk256"), (20, 5, "f16"), (2, 2, "qk256")])
def test_eight_record_merge_equals_combine_then_project(hip, oracle, torch_, n_heads, n_kv, fmt, max_pos):
    """y within 3e-5 max(1, max|y|), the dequantised QAct within 2e-4, the QAct = quantize_qact of its own y exactly, K / V caches
    equal to the combine path's: the bounds the 4-record form is held to, at 1..8 live records."""
    cs = Case(hip, oracle, torch_, n_heads, n_kv, fmt, max_pos)
    for pos in (p for p in POSITIONS if p < max_pos):
        qkv, res = cs.inputs(torch_)
        a, qa, sa, k1, v1 = cs.combined(hip, torch_, qkv, res, pos)
        b, qb, sb_, k2, v2 = cs.merged(hip, torch_, qkv, res, pos, 8)
        err = np.max(np.abs(a - b))
        print(f"heads {n_heads}/{n_kv} {fmt} max_pos {max_pos} pos {pos}: max|dy| {err:.3e} of max|y| {np.max(np.abs(a)):.3e}")
        assert err <= 3e-5 * max(1.0, np.max(np.abs(a))), (n_heads, n_kv, pos, err)
        da, db = dequantize_qact(qa, ROWS), dequantize_qact(qb, ROWS)
        assert np.max(np.abs(da - db)) <= 2e-4 * max(1.0, np.max(np.abs(da))), (n_heads, n_kv, pos)
        assert np.array_equal(qb, quantize_qact(b, cs.gam.cpu().numpy())), (n_heads, n_kv, pos)
        assert torch_.equal(k1, k2) and torch_.equal(v1, v2)
        if pos >= 256:
            # from 5 live records the prologue takes k_attn_combine's own expf and division (for <= 8 records that kernel is the same
            # two-pass sum in record order), and the GEMV behind it is the same code on the same LDS image: no bit may differ
            assert np.array_equal(a, b) and np.array_equal(qa, qb) and np.array_equal(sa, sb_), (n_heads, n_kv, pos)
    hip.weights_free(cs.w)


@pytest.mark.parametrize("n_heads,n_kv,fmt", [(8, 2, "qk256"), (20, 5, "f16"), (2, 2, "qk256")])
def test_eight_record_entry_is_bit_identical_to_the_four_record_one(hip, oracle, torch_, n_heads, n_kv, fmt):
    cs = Case(hip, oracle, torch_, n_heads, n_kv, fmt, 1024)
    for pos in (0, 63, 64, 130, 255):
        qkv, res = cs.inputs(torch_)
        y4, q4, st4, _, _ = cs.merged(hip, torch_, qkv, res, pos, 0)
        y4r, q4r, st4r, _, _ = cs.merged(hip, torch_, qkv, res, pos, 4)
        y8, q8, st8, _, _ = cs.merged(hip, torch_, qkv, res, pos, 8)
        assert np.array_equal(y4, y8) and np.array_equal(q4, q8) and np.array_equal(st4, st8), (n_heads, pos)
        assert np.array_equal(y4, y4r) and np.array_equal(q4, q4r) and np.array_equal(st4, st4r), (n_heads, pos)
    hip.weights_free(cs.w)


def test_record_bound_is_validated(hip, pkg, oracle, torch_):
    cs = Case(hip, oracle, torch_, 8, 2, "qk256", 512)
    qkv, res = cs.inputs(torch_)
    with pytest.raises(pkg.BitNetHipError, match="max_records must be 4 or 8"):
        cs.merged(hip, torch_, qkv, res, 10, 6)
    hip.weights_free(cs.w)


MODEL = dict(hidden=1024, n_layers=2, n_heads=8, n_kv_heads=2, head_dim=128, ffn=2048, vocab=4096, max_pos=1024, eps=1e-5, rope_theta=10000.0)
CHECK_AT = (250, 256, 257, 320, 511, 512, 529)


@pytest.mark.parametrize("fmt,kv16", [("qk256", False), ("i2s", False), ("i2s", True)])
def test_decoder_across_the_eight_record_form_matches_the_reference_step(pkg, hip, synth, fmt, kv16):
    """530 forced tokens through the step graphs; logits at positions on both sides of 256 / 257 keys and of the form's upper
    bound against Decoder::run_reference (unfused, reference-order kernels, records + combine) on the same tokens."""
    cfg = synth.ModelConfig(**MODEL)
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt, block=32)
        dec.set_layer_i2s(l, w, 32) if fmt == "i2s" else dec.set_layer_qk256(l, w)
    dec.set_globals(synth.make_globals(cfg))
    toks = synth.prompt(531, cfg.vocab)
    # which form each position takes: 4-record merge to 256 keys, 8-record merge for 257..N keys, records + combine beyond
    assert dec.form_at(0) == 1 and dec.form_at(255) == 1
    for keys in range(257, MERGE8_MAX_KEYS + 1):
        assert dec.form_at(keys - 1) == 3, keys
    assert dec.form_at(MERGE8_MAX_KEYS) == 0 and dec.form_at(700) == 0
    runs = []
    for ref in (True, False):
        dec.reset()
        if kv16:
            dec.set_kv_f16(True)
        dec.feed(toks)
        logits, at = [], 0
        for p in CHECK_AT:
            if ref:
                dec.run_reference(p - at, with_logits=False)
                dec.run_reference(1, with_logits=True)
            else:
                dec.run(p - at, with_logits=False, use_graph=True)
                dec.run(1, with_logits=True, use_graph=True)
            at = p + 1
            assert dec.position() == at
            logits.append(dec.last_logits().copy())
        runs.append(logits)
    for p, a, b in zip(CHECK_AT, *runs):
        c = cosine(a, b)
        print(f"{fmt} kv16={kv16} position {p} (form {dec.form_at(p)}): cosine {c:.8f}")
        assert c >= 0.9999, (fmt, kv16, p, c)
    dec.close()
