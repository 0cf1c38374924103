"""CPU: tests/gemvq_ref.py, the model tests/test_gemvq_instances_gpu.py holds k_gemv_q's instances against.

1. the model is the oracle's operation: quantise -> [LayerNorm after the product] -> product -> [silu * up] against oracle.layernorm ->
   oracle.gemv_qk256 / i2s_matmul on the same f32 inputs, at the gates tests/test_qact_gpu.py uses for the device chain (cosine >= 0.99999 per output
   vector, max error <= 2e-4 of the largest output); the record reader against qact_ref.dequantize_qact.
2. the bounds are tight enough to catch real faults: each fault of gemvq_ref.FAULTS, planted in the model, must leave the derived bound behind
   TENFOLD in at least one output (where the bound is 0 -- exact inputs -- it must change an output).
3. the exact inputs ARE exact: for every case of the GPU file the largest partial sum any order can reach stays below 2^24 units, and the model
   draws the same conclusion (bound 0); the LayerNorm vector of the exact cases gives an exact g_r."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemvq_ref as G  # noqa: E402
import test_gemvq_instances_gpu as T  # noqa: E402  (its case table and input generators; nothing there touches a GPU at import)
from qact_ref import dequantize_qact, quantize_qact  # noqa: E402


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


# ---------------------------------------------------------------- 1. against the oracle
def oracle_product(oracle, wts, x):
    if wts.kind == "qk256":
        return oracle.gemv_qk256(wts.upload["qs"].reshape(-1), x, wts.rows, wts.cols, wts.upload["stride"]).astype(np.float64)
    return oracle.i2s_matmul(x, wts.upload["packed"].reshape(-1), wts.upload["scales"].reshape(-1), 1, wts.rows, wts.cols, 32).reshape(-1).astype(np.float64)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("rows,nblk,k_split", [(48, 1, 1), (32, 3, 2), (64, 5, 4), (32, 11, 8)])
def test_model_matches_the_oracle(oracle, kind, rows, nblk, k_split):
    cols = 256 * nblk
    wts = G.make_weights(kind, rows, cols, rows + nblk)
    rng = np.random.default_rng(cols)
    x = rng.normal(0.05, 1.0, cols).astype(np.float32)
    rec, _ = G.producer(x)
    p = G.launch(wts, rec, k_split)
    want = oracle_product(oracle, wts, x)
    assert cosine(p.want[0], want) >= 0.99999 and np.max(np.abs(p.want[0] - want)) <= 2e-4 * np.max(np.abs(want))
    assert np.allclose(p.want[0], G.launch(wts, rec, 1).want[0], rtol=0, atol=1e-12 * p.mag[0].max())  # the K split moves roundings, not the value
    # LayerNorm after the product against LayerNorm before it
    g = (rng.uniform(0.5, 1.5, cols) / (1.58 * np.sqrt(cols))).astype(np.float32)
    rec, st = G.producer(x, g)
    p = G.launch(wts, rec, k_split, ln=(st, 1e-5, g))
    want = oracle_product(oracle, wts, oracle.layernorm(x, g, 1e-5))
    assert cosine(p.want[0], want) >= 0.99999 and np.max(np.abs(p.want[0] - want)) <= 2e-4 * np.max(np.abs(want))
    # silu(gate) * up on the interleaved pair
    up = G.make_weights(kind, rows, cols, rows + nblk + 1)
    ps = G.launch(G.pair(wts, up), rec, min(k_split, 4), ln=(st, 1e-5, g), silu=True)
    gate, u = want, oracle_product(oracle, up, oracle.layernorm(x, g, 1e-5))
    want_h = gate / (1.0 + np.exp(-gate)) * u
    assert cosine(ps.want[0], want_h) >= 0.99999 and np.max(np.abs(ps.want[0] - want_h)) <= 3e-4 * np.max(np.abs(want_h))


def test_record_reader_and_ranges():
    x = G.float_vector(768, 4, "tiny")
    rec = quantize_qact(x)
    assert np.array_equal(G.dequantised(rec, 768), dequantize_qact(rec, 768))
    d0, d1, as_ = G.read_qact(rec, 768)
    assert np.abs(d0).max() <= 128 and np.abs(256 * d1 + d0).max() <= 1 << 14 and np.all(np.frexp(as_)[0] == 0.5)
    for nblk in range(1, 33):
        for ks in (1, 2, 4, 8):
            r = G.k_ranges(nblk, ks)
            assert r[0][0] == 0 and r[-1][1] == nblk and all(a[1] == b[0] for a, b in zip(r, r[1:]))  # the parts tile the blocks
    assert [b - a for a, b in G.k_ranges(11, 8)] == [1, 1, 2, 1, 1, 2, 1, 2] and G.product_roundings(11, 8) == 1 + 4 + 2 + 7


# ---------------------------------------------------------------- 2. the bounds catch real faults
F_ROWS, F_NBLK, F_KS = 64, 5, 4  # four row tiles (two pairs), K ranges of 1, 1, 1 and 2 blocks


def fault_case(fault, kind, mode):
    """-> (p, bad): the model's launch and its output under the fault (None: the form has nothing the fault could touch)"""
    cols = 256 * F_NBLK
    scales = "pow2" if mode == "exact" else "float"
    wts = G.make_weights(kind, F_ROWS, cols, T.seed_of("fault", kind), scales)
    res = np.random.default_rng(7).normal(0, 1, F_ROWS).astype(np.float32)
    if fault in ("live_ignored", "dead_included"):
        n_heads, n_kv, nr, chunks_max = cols // 128, cols // 256, 4, 8
        rng = np.random.default_rng(T.seed_of("records", kind))
        scratch = np.full(n_kv * chunks_max * G.REC_FLOATS, 3.0, np.float32)  # stale finite values in the dead records
        pos = 255 if fault == "live_ignored" else 100
        for kv in range(n_kv):
            for c in range((pos + 64) >> 6):
                r = scratch[(kv * chunks_max + c) * G.REC_FLOATS:][:G.REC_FLOATS]
                l_ = rng.uniform(1.0, 40.0, 4)
                r[0:8:2], r[1:8:2] = rng.normal(0, 2, 4), l_
                r[8:] = (rng.normal(0, 1, (4, 128)) * l_[:, None]).reshape(-1)
        v, delta = G.merge_records(scratch, pos, n_heads, n_kv, chunks_max, nr)
        rec, spread = G.quant_interval(v, delta)
        p = G.product(wts, *G.read_qact(rec, cols), 8, spread=spread)
        vb, _ = G.merge_records(scratch, pos, n_heads, n_kv, chunks_max, nr, fault)
        return p, G.product(wts, *G.read_qact(quantize_qact(vb.astype(np.float32)), cols), 8).want
    ln = fault == "g_row"
    silu = fault == "silu_on_up"
    if mode == "exact":
        g = T.ln_gamma_for(cols, "exact", 3)
        unit = 21 if kind == "i2s32" else -9
        x = G.exact_vector(cols, 5, g[::16].astype(np.float64), unit)[1] if ln else G.exact_vector(cols, 5, None, unit)
    else:
        g = T.ln_gamma_for(cols, "float", 3)
        x = G.float_vector(cols, 5, "mean" if ln else "mixed")
    rec, st = G.producer(x, g if ln else None)
    kw = dict(ln=(st, 1e-5, g) if ln else None, silu=silu, residual=res if fault == "residual_row" else None)
    if silu:
        wts = G.pair(wts, G.make_weights(kind, F_ROWS, cols, T.seed_of("fault", kind, "up"), scales))
    if fault == "scale_pair" and wts.scale is None:
        return None, None
    return G.launch(wts, rec, F_KS, **kw), G.launch(wts, rec, F_KS, fault=fault, **kw).want


@pytest.mark.parametrize("mode", ["float", "exact"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_every_fault_leaves_the_bound_behind_tenfold(kind, mode):
    for fault in G.FAULTS:
        if mode == "exact" and fault in ("live_ignored", "dead_included"):
            continue  # the merge has no exact inputs: its weights are exponentials
        p, bad = fault_case(fault, kind, mode)
        if p is None:
            continue
        tgt = G.target(p)
        assert np.all(np.abs(p.want - tgt) <= p.bound + G.U * np.abs(p.want))  # (the exact value is the want, rounded once)
        with np.errstate(over="ignore"):
            got = bad.astype(np.float32).astype(np.float64)  # what an f32 buffer would hold
        err = np.abs(got - tgt)
        caught = ~(err <= 10.0 * p.bound)
        print(kind, mode, fault, "outputs beyond 10 x bound:", int(caught.sum()), "of", caught.size, "largest error / bound",
              float((err / np.maximum(p.bound, 1e-300)).max()))
        assert caught.any(), (kind, mode, fault)


# ---------------------------------------------------------------- 3. the exact inputs are exact
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("name", list(T.SHAPES))
def test_exact_inputs_stay_below_2_24_units(name, kind):
    ln_ok = T.SHAPES[name][3]
    p, wts, _ = T.exact_product(name, kind, False)
    print(name, kind, "largest partial sum:", float(p.units.max()), "units")
    assert p.units.max() < G.R.EXACT_UNITS and not p.bound.any()
    assert np.array_equal(p.exact32.astype(np.float64), p.want)  # nothing to round: the f32 value IS the exact one
    if ln_ok:
        g = T.ln_gamma_for(wts.cols, "exact", T.seed_of(name, "gamma"))
        (_, x), = T.vectors(name, "exact", True, g, kind)
        (_, u), = T.vectors(name, "exact", False, None, kind)
        assert np.array_equal((x * g).astype(np.float32), u)  # the LayerNorm producer quantises the same integers
        _, bg = G.g_rows(wts, g)
        assert not bg.any()
        _, bg = G.g_rows(wts, T.ln_gamma_for(wts.cols, "float", 1))
        assert bg.all()


def test_the_case_table_covers_the_45_reachable_plain_instances():
    """what the GPU file's header counts: 15 (RING, NCP, LN) combinations x 3 scale forms, K splits 1, 2, 4, 8, and an unequal K range at every split > 1"""
    seen = set()
    for rows, nblk, paired, ln_ok, geo in T.SHAPES.values():
        assert geo["ring"] == max(2, geo["blocks_per_wave"]) == max(2, max(b - a for a, b in G.k_ranges(nblk, geo["k_split"])))
        assert geo["copy_passes"] == -(-G.QREC * nblk // 8192) and geo["grid"] == -(-(rows // 16) // (8 // geo["k_split"]))
        for ln in (0, 1) if ln_ok else (0,):
            seen.add((geo["ring"], geo["copy_passes"], ln))
    assert len(seen) == 15 and {r for r, _, _ in seen} == {2, 3, 4, 5} and {n for _, n, _ in seen} == {1, 2, 3}
    assert {g["k_split"] for *_, g in T.SHAPES.values()} == {1, 2, 4, 8}
    for ks in (2, 4, 8):
        assert any(len({b - a for a, b in G.k_ranges(nblk, g["k_split"])}) > 1 for _, nblk, _, _, g in T.SHAPES.values() if g["k_split"] == ks), ks
    assert {(ne, ne1, nr) for (_, _, nr), (ne, ne1, _) in T.MERGES.items()} == {(1, 0, 4), (1, 1, 4), (2, 0, 4), (1, 0, 8), (1, 1, 8)}
