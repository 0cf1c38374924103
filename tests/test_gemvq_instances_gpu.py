"""GPU: every reachable instance of k_gemv_q (csrc/kernels_gemvq.hip), the decode step's GEMV on producer-quantised activations, by value against
the float64 / int64 model of tests/gemvq_ref.py.  Each case first asserts what bitnet_hip_gemv_q_geometry reports of the launch, then the values:

  exact inputs   small integers with equal group exponents, power-of-two block scales: nothing rounds, the output must EQUAL the model on every
                 element (behind the LayerNorm epilogue: the once-rounded value; behind silu * up: within the bound of its two instructions);
  float inputs   mixed magnitudes per column, a 16-group below the format's smallest scale, a zero vector, a large mean for LayerNorm: every
                 element within the bound gemvq_ref derives (a count of f32 roundings x 2^-24 x the magnitudes that enter them).
Epilogues: y only; residual; QAct out + gamma_out + statistics (with y, and with y null: the same bytes); silu * up on the paired shapes; all with and
without LayerNorm wherever the geometry entry accepts LayerNorm.  y and the QAct / statistics buffers lie between NaN / 0xA5 guards.

Plain instances k_gemv_q<8, RING, SC, LN, NCP>, SC = 0 (qk256), 1 (i2s32: f32 scales), 2 (i2s32h: f16 scales) -- every shape runs all three:

  RING NCP  K split  LN   shape (rows x 256-column blocks; P = interleave16 pair run with silu * up)
   2    1    1       0,1  16 x 1; 144 x 1 (9 tiles, 8 per workgroup: surplus waves); P 160 x 1 (5 pairs, 4 per workgroup)
   2    1    2       0,1  80 x 3 (ranges 1 + 2; 5 tiles, 4 per workgroup); P 96 x 3
   2    1    4       0,1  16 x 5 (ranges 1, 1, 1, 2); P 32 x 5
   2    1    8       0,1  48 x 11 (ranges 1, 1, 2, 1, 1, 2, 1, 2 behind the 11 - wave remap); 16 x 14
   2    2    8       0,1  16 x 15
   3    1    4       0,1  P 32 x 10 (ranges 2, 3, 2, 3); 4112 x 9 (257 tiles: the plain form's first shape off split 8)
   3    2    8       0    16 x 17
   4    1    4       0,1  P 32 x 13
   4    2    4       0,1  P 32 x 15
   4    2    8       0    16 x 25
   4    3    8       0    16 x 29
   5    1    2       0,1  P 8224 x 9 (514 tiles: the first pair off split 4; ranges 4 + 5)
   5    2    4       0    P 32 x 17

Unreachable (no shape the entries accept selects them; removing them is not this file's business):
  RING 2, 3, 5 with NCP 3   three copy passes need 29 .. 32 blocks (the entry stops at 8192 columns), which only split 8 brings under 6 blocks per
                            wave: 4 blocks each;
  LN with NCP 3, and LN with RING 3 or 5 at NCP 2: LayerNorm stops at 4096 columns = 16 blocks; 15 and 16 blocks give 2 (split 8) or 4 (split 4)
                            blocks per wave and nothing else.
That is 18 + 3 + 6 = 27 of the 72; the 45 reachable ones are the 15 (RING, NCP, LN) combinations of the table x 3 scale forms.

Merging instances k_gemv_q<8, 2, SC, 0, 1, NE, NE1, NR> (48 rows, all three scale forms; records from bitnet_hip_attention_decode_partial_dev):
  NE NE1 NR   heads / KV heads (columns, K split)
  1  0   4    8 / 2 (1024, 4)          1  0   8    14 / 7 (1792, 4)
  1  1   4    18 / 9 (2304, 8)         1  1   8    20 / 5 (2560, 8)
  2  0   4    24 / 6 (3072, 8)
at 1, 2, 4 live records (5 and 8 for NR 8), stale finite values in the dead ones, and a record buffer shorter than NR (the index clamp)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemvq_ref as G  # noqa: E402
from qact_ref import quantize_qact  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> rows, 256-column blocks, paired (run with silu * up), LayerNorm accepted, what the geometry entry must report
SHAPES = {
    "16x1": (16, 1, False, True, dict(k_split=1, blocks_per_wave=1, ring=2, copy_passes=1, grid=1)),
    "144x1": (144, 1, False, True, dict(k_split=1, blocks_per_wave=1, ring=2, copy_passes=1, grid=2)),
    "80x3": (80, 3, False, True, dict(k_split=2, blocks_per_wave=2, ring=2, copy_passes=1, grid=2)),
    "16x5": (16, 5, False, True, dict(k_split=4, blocks_per_wave=2, ring=2, copy_passes=1, grid=1)),
    "48x11": (48, 11, False, True, dict(k_split=8, blocks_per_wave=2, ring=2, copy_passes=1, grid=3)),
    "16x14": (16, 14, False, True, dict(k_split=8, blocks_per_wave=2, ring=2, copy_passes=1, grid=1)),
    "16x15": (16, 15, False, True, dict(k_split=8, blocks_per_wave=2, ring=2, copy_passes=2, grid=1)),
    "16x17": (16, 17, False, False, dict(k_split=8, blocks_per_wave=3, ring=3, copy_passes=2, grid=1)),
    "16x25": (16, 25, False, False, dict(k_split=8, blocks_per_wave=4, ring=4, copy_passes=2, grid=1)),
    "16x29": (16, 29, False, False, dict(k_split=8, blocks_per_wave=4, ring=4, copy_passes=3, grid=1)),
    "4112x9": (4112, 9, False, True, dict(k_split=4, blocks_per_wave=3, ring=3, copy_passes=1, grid=129)),
    "P160x1": (160, 1, True, True, dict(k_split=1, blocks_per_wave=1, ring=2, copy_passes=1, grid=2)),
    "P96x3": (96, 3, True, True, dict(k_split=2, blocks_per_wave=2, ring=2, copy_passes=1, grid=2)),
    "P32x5": (32, 5, True, True, dict(k_split=4, blocks_per_wave=2, ring=2, copy_passes=1, grid=1)),
    "P32x10": (32, 10, True, True, dict(k_split=4, blocks_per_wave=3, ring=3, copy_passes=1, grid=1)),
    "P32x13": (32, 13, True, True, dict(k_split=4, blocks_per_wave=4, ring=4, copy_passes=1, grid=1)),
    "P32x15": (32, 15, True, True, dict(k_split=4, blocks_per_wave=4, ring=4, copy_passes=2, grid=1)),
    "P32x17": (32, 17, True, False, dict(k_split=4, blocks_per_wave=5, ring=5, copy_passes=2, grid=1)),
    "P8224x9": (8224, 9, True, True, dict(k_split=2, blocks_per_wave=5, ring=5, copy_passes=1, grid=129)),
}
# heads, KV heads, records -> (NE, NE1, K split)
MERGES = {(8, 2, 4): (1, 0, 4), (14, 7, 8): (1, 0, 4), (18, 9, 4): (1, 1, 8), (20, 5, 8): (1, 1, 8), (24, 6, 4): (2, 0, 8)}
MERGE_ROWS = 48
EPS = 1e-5
WORST = {}  # epilogue kind -> largest error / bound seen (printed; EXPERIMENTS.md keeps the figures of one run)


def seed_of(*parts):
    return sum((i + 1) * sum(map(ord, str(p))) for i, p in enumerate(parts)) % (1 << 31)


def weights_for(name, kind, scales):
    rows, nblk, paired, _, _ = SHAPES[name]
    if not paired:
        return G.make_weights(kind, rows, 256 * nblk, seed_of(name, kind, scales), scales)
    return G.pair(G.make_weights(kind, rows // 2, 256 * nblk, seed_of(name, kind, scales, "gate"), scales),
                  G.make_weights(kind, rows // 2, 256 * nblk, seed_of(name, kind, scales, "up"), scales))


def ln_gamma_for(cols, mode, seed):
    rng = np.random.default_rng(seed)
    if mode == "exact":  # one of two neighbouring powers of two per 16-group: x * gamma and W . gamma are exact
        return np.repeat(rng.choice(np.array([0.25, 0.125], np.float32), cols // 16), 16)
    return (rng.uniform(0.5, 1.5, cols) / (1.58 * np.sqrt(cols))).astype(np.float32)


def vectors(name, mode, ln, ln_gamma, kind=None):
    """[(tag, x f32 [cols])]: what the producer is given"""
    unit = 21 if kind == "i2s32" else -9  # (the exact i2s32 matrices carry block scales of 2^-30, 2^-31)
    rows, nblk, _, _, _ = SHAPES[name]
    cols = 256 * nblk
    if mode == "exact":
        if not ln:
            return [("exact", G.exact_vector(cols, seed_of(name, "x"), None, unit))]
        return [("exact", G.exact_vector(cols, seed_of(name, "x"), ln_gamma[::16].astype(np.float64), unit)[1])]
    kinds = ["mixed", "tiny", "zero"] + (["mean"] if ln else [])
    if rows > 1024:  # the two large shapes: one float vector (their model is 19 M integer products per vector)
        kinds = ["mixed"]
    return [(k, G.float_vector(cols, seed_of(name, k), k)) for k in kinds]


def exact_product(name, kind, ln):
    """the model's product of the exact vector of a case (tests/test_gemvq_ref.py asserts its units from here)"""
    wts = weights_for(name, kind, "pow2")
    g = ln_gamma_for(wts.cols, "exact", seed_of(name, "gamma")) if ln else None
    (_, x), = vectors(name, "exact", ln, g, kind)
    rec, _ = G.producer(x, g)
    return G.product(wts, *G.read_qact(rec, wts.cols), SHAPES[name][4]["k_split"]), wts, g


# ---------------------------------------------------------------- device helpers
@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(hip, wts):
    if "parts" in wts.upload:
        parts = [upload(hip, p) for p in wts.upload["parts"]]
        h = hip.weights_concat(parts, interleave16=True)
        for p in parts:
            hip.weights_free(p)
        return h
    if wts.kind == "qk256":
        return hip.weights_upload_qk256(wts.upload["qs"].reshape(-1), wts.rows, wts.cols, wts.upload["stride"])
    return hip.weights_upload_i2s(wts.upload["packed"].reshape(-1), wts.upload["scales"].reshape(-1), wts.rows, wts.cols, 32)


class Guarded:
    """a device buffer of n elements between two 64-byte guards (NaN for floats, 0xA5 for bytes) that must survive the launch"""

    def __init__(self, torch_, n, dtype, interior):
        self.pad = 64 // {torch_.float32: 4, torch_.float64: 8, torch_.uint8: 1}[dtype]
        self.fill = 0xA5 if dtype == torch_.uint8 else float("nan")
        self.buf = torch_.full((n + 2 * self.pad,), self.fill, dtype=dtype, device="cuda")
        self.view = self.buf[self.pad: self.pad + n]
        self.view.fill_(interior)

    def read(self):
        """the interior as numpy; asserts the guards"""
        a = self.buf.cpu().numpy()
        want = np.full(self.pad, self.fill, a.dtype).view(np.uint8)
        assert np.array_equal(a[: self.pad].view(np.uint8), want) and np.array_equal(a[-self.pad:].view(np.uint8), want), "guard overwritten"
        return a[self.pad: -self.pad].copy()


def hold(got, p, tag, kind):
    """every element within the model's bound; where the bound is 0, equal by value.  -> the worst error / bound"""
    tgt, bound = G.target(p)[0], p.bound[0]
    err = np.abs(got.astype(np.float64) - tgt)
    assert not np.isnan(got).any(), tag
    exact = bound == 0
    assert np.array_equal(got[exact].astype(np.float64), tgt[exact]), (tag, "exact elements differ", int((err[exact] > 0).sum()), float(err[exact].max()))
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print(*tag, f"worst error / bound {ratio:.3f}", f"({int(exact.sum())} of {exact.size} elements exact)")
    assert ratio <= 1.0, (tag, ratio, int(np.argmax(np.where(exact, 0.0, err / np.where(exact, 1.0, bound)))))
    return ratio


def hold_qact(q, s, v, gam, tag):
    """the QAct and statistics the kernel left of its own f32 output v: the quantiser's bits; the pairs are f32 sums over 16 values (15 additions
    of the values, 16 roundings of the squares' sum)"""
    assert np.array_equal(q, quantize_qact(v, gam)), (tag, "qact")  # (bytes no group of v owns were zero before the launch and still are)
    v64 = v.astype(np.float64).reshape(-1, 16)
    st = s.reshape(-1, 2)
    assert np.all(np.abs(st[:, 0] - v64.sum(1)) <= G.R.gamma(15) * np.abs(v64).sum(1) + G.TINY), (tag, "sum")
    assert np.all(np.abs(st[:, 1] - (v64 * v64).sum(1)) <= G.R.gamma(16) * (v64 * v64).sum(1) + 16 * G.TINY), (tag, "sum of squares")


# ---------------------------------------------------------------- the plain instances
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_plain_instance_by_value(hip, pkg, torch_, name, kind):
    rows, nblk, paired, ln_expected, expect = SHAPES[name]
    cols, out_rows, flags = 256 * nblk, rows // 2 if paired else rows, 1 if paired else 0
    rng = np.random.default_rng(seed_of(name, kind, "epilogue"))
    res = rng.normal(0, 1, out_rows).astype(np.float32)
    gam_out = rng.uniform(0.5, 1.5, out_rows).astype(np.float32)
    res_d, gam_d = dev(torch_, res), dev(torch_, gam_out)
    for mode in ("exact", "float"):
        wts = weights_for(name, kind, "pow2" if mode == "exact" else "float")
        h = upload(hip, wts)
        geo = hip.gemv_q_geometry(h, flags=flags)
        assert {k: geo[k] for k in expect} == expect and geo["scale_form"] == G.SCALE_FORM[kind] and geo["blocks"] == nblk and geo["merge_records"] == 0, geo
        try:
            geo_ln = hip.gemv_q_geometry(h, flags=flags, layernorm=True)
        except pkg.BitNetHipError:
            geo_ln = None
        assert (geo_ln is not None) == ln_expected, (name, geo_ln)
        if geo_ln is not None:
            assert geo_ln == dict(geo, layernorm=1)
        for ln in (False, True) if geo_ln is not None else (False,):
            g_np = ln_gamma_for(cols, mode, seed_of(name, "gamma"))
            g_d = dev(torch_, g_np)
            if ln:
                hip.weights_bind_ln(h, g_d)
            for vtag, x in vectors(name, mode, ln, g_np, kind):
                rec, st = G.producer(x, g_np if ln else None)
                rec_d, st_d = dev(torch_, rec), dev(torch_, st.reshape(-1))
                kw = dict(flags=flags)
                if ln:
                    kw.update(stats_in=st_d, ln_gamma=g_d, ln_eps=EPS)
                base = G.launch(wts, rec, expect["k_split"], ln=(st, EPS, g_np) if ln else None, silu=paired)
                tag = (name, kind, mode, "ln" if ln else "--", vtag)
                # y only
                y = Guarded(torch_, out_rows, torch_.float32, float("nan"))
                hip.gemv_q_dev(h, rec_d, y=y.view, **kw)
                torch_.cuda.synchronize()
                v = y.read()
                hold(v, base, tag + ("silu" if paired else "y",), ("silu" if paired else "product") + ("+ln" if ln else ""))
                # residual (the paired form has none)
                if not paired:
                    y = Guarded(torch_, out_rows, torch_.float32, float("nan"))
                    hip.gemv_q_dev(h, rec_d, y=y.view, residual=res_d, **kw)
                    torch_.cuda.synchronize()
                    hold(y.read(), G.add_residual(base, res), tag + ("residual",), "residual" + ("+ln" if ln else ""))
                # QAct out + gamma_out + statistics, with y and with y null
                outs = []
                for with_y in (True, False):
                    y = Guarded(torch_, out_rows, torch_.float32, float("nan"))
                    q = Guarded(torch_, hip.qact_bytes(out_rows), torch_.uint8, 0)
                    s = Guarded(torch_, out_rows // 16 * 2, torch_.float64, float("nan"))
                    hip.gemv_q_dev(h, rec_d, y=y.view if with_y else None, qact_out=q.view, gamma_out=gam_d, stats_out=s.view, **kw)
                    torch_.cuda.synchronize()
                    outs.append((y.read(), q.read(), s.read()))
                (v2, q2, s2), (v3, q3, s3) = outs
                assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)), (tag, "y changes with the QAct output")
                assert np.isnan(v3).all(), (tag, "y null but written")
                assert np.array_equal(q2, q3) and np.array_equal(s2.view(np.uint64), s3.view(np.uint64)), (tag, "QAct output changes with y null")
                hold_qact(q2, s2, v, gam_out, tag)
                assert np.array_equal(rec_d.cpu().numpy(), rec), (tag, "input overwritten")
        hip.weights_free(h)
    print("worst error / bound so far:", {k: round(r, 3) for k, r in sorted(WORST.items())})


# ---------------------------------------------------------------- the merging instances
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("n_heads,n_kv,nr", list(MERGES))
def test_merging_instance_by_value(hip, oracle, torch_, n_heads, n_kv, nr, kind):
    D, cols, rows = 128, n_heads * 128, MERGE_ROWS
    ne, ne1, k_split = MERGES[(n_heads, n_kv, nr)]
    wts = G.make_weights(kind, rows, cols, seed_of("merge", n_heads, kind))
    h = upload(hip, wts)
    geo = hip.gemv_q_geometry(h, merge_records=nr)
    assert (geo["merge_slots4"], geo["merge_slots1"], geo["merge_records"], geo["ring"], geo["copy_passes"], geo["layernorm"]) == (ne, ne1, nr, 2, 1, 0), geo
    assert geo["scale_form"] == G.SCALE_FORM[kind] and geo["k_split"] == k_split and geo["blocks_per_wave"] <= 2, geo
    rng = np.random.default_rng(seed_of("merge", n_heads, n_kv, nr, kind))
    res = rng.normal(0, 1, rows).astype(np.float32)
    gam = rng.uniform(0.5, 1.5, rows).astype(np.float32)
    res_d, gam_d = dev(torch_, res), dev(torch_, gam)
    # (max_pos, pos): 1, 2, 4 live records (5, 8 for NR 8); a buffer of 2 records, shorter than NR: records 2 .. NR - 1 are read from its last one
    runs = [(512, 10), (512, 100), (512, 255)] + ([(512, 300), (512, 511)] if nr == 8 else []) + [(128, 100)]
    for max_pos, pos in runs:
        sin, cos = oracle.rope_tables(D, max_pos, 10000.0)
        sb = hip.c.bitnet_hip_attention_scratch_bytes(n_kv, max_pos)
        kc = dev(torch_, rng.normal(0, 1, n_kv * max_pos * D).astype(np.float32))
        vc = dev(torch_, rng.normal(0, 1, n_kv * max_pos * D).astype(np.float32))
        qkv = dev(torch_, rng.normal(0, 1.5, (n_heads + 2 * n_kv) * D).astype(np.float32))
        pos_d = torch_.tensor([pos], dtype=torch_.int32, device="cuda")
        scratch = torch_.zeros(sb // 4 + 16, device="cuda") + 3.0  # stale but finite records past the context
        hip.attention_decode_partial_dev(qkv, dev(torch_, sin), dev(torch_, cos), kc, vc, n_heads, n_kv, D, max_pos, pos_d, scratch)
        torch_.cuda.synchronize()
        records = scratch.cpu().numpy()
        y = Guarded(torch_, rows, torch_.float32, float("nan"))
        q = Guarded(torch_, hip.qact_bytes(rows), torch_.uint8, 0)
        s = Guarded(torch_, rows // 16 * 2, torch_.float64, float("nan"))
        hip.gemv_attn_merge_rec_q_dev(h, scratch, n_heads, n_kv, max_pos, pos_d, y.view, q.view, nr, residual=res_d, gamma_out=gam_d, stats_out=s.view)
        torch_.cuda.synchronize()
        assert np.array_equal(scratch.cpu().numpy(), records), "records overwritten"
        v, delta = G.merge_records(records, pos, n_heads, n_kv, -(-max_pos // 64), nr)
        rec, spread = G.quant_interval(v, delta)
        p = G.add_residual(G.product(wts, *G.read_qact(rec, cols), geo["k_split"], spread=spread), res)
        got = y.read()
        tag = ("merge", f"{n_heads}/{n_kv}", f"NR{nr}", kind, f"max_pos {max_pos}", f"pos {pos}")
        hold(got, p, tag, "merge")
        hold_qact(q.read(), s.read(), got, gam, tag)
    hip.weights_free(h)
    print("worst error / bound so far:", {k: round(r, 3) for k, r in sorted(WORST.items())})
