"""CPU checks of tests/attn_decode_ref.py, the float64 model behind tests/test_attn_decode_instances_gpu.py: the model against a direct
softmax(Q K^T / sqrt d) V, the conditions the input families must meet (from the model, never from the kernel), the float32 emulation of the
kernel's chunk algorithm under the tolerance (output rows and records, both record sizes, both cache types), and the seeded faults.

Which family catches which fault (EXPOSES; `out` = the output row exceeds tol(), `rec` = a record exceeds rec_tol()):
  mask_tail     sunk, gauss, newtok (out)       -- the stale key's score (8 q' . q', or NaN in an f32 cache) takes the row
  new_twice     newtok, needle, gauss (out)     -- the weight meets the stale value slot; invisible in oldonly with an f16 cache (weight e^-30)
  enew_dropped  newtok, needle, gauss (out)     -- invisible in oldonly
  merge_swap    ramp12, fall12, gauss, needle (out)
  dead_record   gauss, ramp12, sunk, needle (out)
  half_m        needle (out: exp(m1 - m0) overflows), ramp12 and gauss (rec: m is not the record's maximum); invisible in fall12 (m0 IS the maximum)
  head_map      every family; needle and gauss named (out)
  v_class       gauss, ramp12, fall12, oldonly, needle (out); invisible in newtok (the mass is on enew)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_decode_ref as dr  # noqa: E402

D = 128
MAX_POS = 4224
N_HEADS, N_KV = 4, 2
SIZES = [1, 63, 64, 65, 128, 129, 513, 1100, 4161]  # keys (the new token included)


@pytest.fixture(scope="module")
def tables(oracle):
    sin, cos = oracle.rope_tables(D, MAX_POS, 10000.0)
    return sin.reshape(MAX_POS, D // 2), cos.reshape(MAX_POS, D // 2)


_cases = {}


def case(tables, name, keys, kv_f16):
    """one family at `keys` keys: inputs, model and tolerance (cached: the reference is computed once and left unchanged)"""
    key = (name, keys, bool(kv_f16))
    if key not in _cases:
        sin, cos = tables
        pos = keys - 1
        rng = np.random.default_rng(dr.seed_of("ref", *key))
        m = dr.master(name, rng, keys, N_KV)
        q1, kn1, vn, t = dr.token(m, rng, pos, N_HEADS)
        qkv = dr.raw_qkv(q1, kn1, vn, pos, sin, cos)
        kc, vc = dr.host_caches(m, q1, pos, (keys + 63) // 64 * 64 + 64, kv_f16)
        ex = dr.exact(qkv, kc, vc, pos, sin, cos, N_HEADS, N_KV, kv_f16)
        tl = dr.tol(ex)
        for a in (qkv, kc, vc, tl, ex["out"], ex["p"], ex["s"], ex["ds"], ex["K"], ex["V"]):
            a.setflags(write=False)
        _cases[key] = dict(qkv=qkv, kc=kc, vc=vc, pos=pos, ex=ex, tol=tl, t=t, q1=q1, kn1=kn1, vn=vn, m=m, kv_f16=bool(kv_f16))
    return _cases[key]


def run_walk(tables, c, rec, fault=None):
    """-> (max err / tol of the output rows, max err / tol of the records, the rows)"""
    out, (m, l, o) = dr.walk(c["qkv"], c["kc"], c["vc"], c["pos"], *tables, N_HEADS, N_KV, c["kv_f16"], rec, fault=fault)
    return dr.ratio(out, c["ex"]["out"], c["tol"]), dr.rec_ratio(c["ex"], rec, m, l, o), out


@pytest.mark.parametrize("kv_f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("name", dr.FAMILIES)
def test_exact_against_a_direct_softmax(tables, name, kv_f16):
    """the operands are the construction's (the query and the new key survive unrope -> f32 -> rope to f32 rounding, the past is the cache's own
    values, the f16 new key is the construction's nearest f16 or its neighbour), and on them out = softmax(Q K^T / sqrt d) V written directly;
    the records recombine to the same rows"""
    for keys in (1, 65, 200):
        c = case(tables, name, keys, kv_f16)
        ex, pos = c["ex"], c["pos"]
        assert np.max(np.abs(ex["q"] - c["q1"])) <= 2.0 ** -22 * np.max(np.abs(c["q1"]))
        assert np.array_equal(ex["K"][:, :pos], c["kc"][:, :pos].astype(np.float64)) and np.array_equal(ex["V"][:, :pos], c["vc"][:, :pos].astype(np.float64))
        assert not ex["K"][:, keys:].any() and not ex["V"][:, keys:].any()
        if kv_f16:
            assert np.all(np.abs(ex["K"][:, pos] - c["kn1"]) <= np.spacing(np.abs(c["kn1"]).astype(np.float16)).astype(np.float64))
            assert np.array_equal(ex["V"][:, pos], c["vn"].astype(np.float32).astype(np.float16).astype(np.float64))
        else:
            assert np.max(np.abs(ex["K"][:, pos] - c["kn1"])) <= 2.0 ** -22 * np.max(np.abs(c["kn1"]))
            assert np.array_equal(ex["V"][:, pos], c["vn"].astype(np.float32).astype(np.float64))
        group = N_HEADS // N_KV
        for h in range(N_HEADS):
            K, V = ex["K"][h // group, :keys], ex["V"][h // group, :keys]
            z = (ex["q"][h][None] @ K.T / np.sqrt(128.0))[0]
            w = np.exp(z - z.max())
            want = (w / w.sum()) @ V
            assert np.all(np.abs(ex["out"][h] - want) <= 1e-13 * (np.abs(V).max() + 1.0))
            assert np.all(np.abs(ex["s"][h] - z) <= 1e-12 * (1.0 + np.abs(z)))
            for rec in (64, 128):
                m, l, o = (x[h] for x in ex["rec"][rec])
                assert m.shape[0] == (keys + rec - 1) // rec
                f = np.exp(m - z.max())
                assert np.all(np.abs((f[:, None] * o).sum(0) / (f * l).sum() - want) <= 1e-12 * (np.abs(V).max() + 1.0))


@pytest.mark.parametrize("keys", [65, 513, 4161])
@pytest.mark.parametrize("name", dr.FAMILIES)
def test_families_meet_their_conditions(tables, name, keys):
    for kv_f16 in (False, True):
        c = case(tables, name, keys, kv_f16)
        ex, pos = c["ex"], c["pos"]
        s, p = ex["s"], ex["p"]
        group = N_HEADS // N_KV
        # stale slots: hostile and finite values everywhere behind the context; keys finite in f16 caches and in `sunk`
        assert np.isfinite(c["vc"][:, pos:].astype(np.float64)).all() and np.min(np.abs(c["vc"][:, pos:].astype(np.float64))) >= 6.0e4
        assert np.isfinite(c["kc"][:, pos:].astype(np.float64)).all() == (kv_f16 or name == "sunk")
        if name == "needle":
            assert np.array_equal(ex["V"][:, :keys], c["m"]["v"].transpose(1, 0, 2))  # the 1/64 grid survives either cache type
            assert pos in c["t"] and len(set(c["t"])) > 1
            for h in range(N_HEADS):
                assert p[h, c["t"][h]] >= 1.0 - 2.0 ** -60
                assert np.all(np.abs(ex["out"][h] - ex["V"][h // group, c["t"][h]]) <= 2.0 ** -60)
        if name == "ramp12":  # every later whole record has the larger maximum, by about 12 per 64 positions; the mass is at the end
            m = ex["rec"][64][0]
            assert np.all(np.diff(m[:, :-1], axis=1) > 8.0) and np.all(p[:, -65:].sum(1) > 0.99)
        if name == "fall12":  # record 0 dominates; at 4161 keys the last records' weights are below the f32 range
            m = ex["rec"][64][0]
            assert np.all(np.diff(m[:, :-1], axis=1) < -8.0) and np.all(p[:, :64].sum(1) > 0.99)
            assert keys < 4161 or np.all(m[:, -1] - m[:, 0] < -110.0)
        if name == "newtok":
            assert np.all(s[:, pos] - np.delete(s, pos, axis=1).max(1) > 25.0) if pos else True
        if name == "oldonly" and pos:
            assert np.all(s[:, pos] - np.delete(s, pos, axis=1).min(1) < -25.0)
        if name == "sunk":  # a stale key (8 q') would outscore every real one by far more than the f32 exp range
            assert np.max(s) < -25.0
            stale_score = np.einsum("hd,hd->h", ex["q"], c["kc"][:, pos + 1].astype(np.float64)[np.arange(N_HEADS) // group]) * dr.SCALE
            assert np.all(stale_score[::group] > 100.0)


@pytest.mark.parametrize("keys", SIZES)
@pytest.mark.parametrize("name", dr.FAMILIES)
def test_walk_without_a_fault_stays_within_the_tolerance(tables, name, keys):
    """output rows and records, 64- and 128-position records, f32 and f16 caches; needle rows equal v[t(h)] to the last bit"""
    for kv_f16 in (False, True):
        c = case(tables, name, keys, kv_f16)
        for rec in (64, 128):
            r, rr, out = run_walk(tables, c, rec)
            print(f"{name} keys={keys} kv16={int(kv_f16)} rec={rec}: walk max(err/tol) rows {r:.3f} records {rr:.3f}")
            assert r <= 1.0 and rr <= 1.0, (name, keys, kv_f16, rec, r, rr)
            if name == "needle":
                for h in range(N_HEADS):
                    assert np.array_equal(out[h], c["ex"]["V"][h // (N_HEADS // N_KV), c["t"][h]]), (keys, kv_f16, rec, h)


# fault -> [(family, keys, record size, f16 cache, what exceeds its bound)]
EXPOSES = {
    "mask_tail": [("sunk", 65, 64, False, "out"), ("sunk", 513, 128, True, "out"), ("gauss", 129, 64, False, "out"), ("newtok", 200, 128, True, "out")],
    "new_twice": [("newtok", 65, 64, False, "out"), ("newtok", 513, 128, True, "out"), ("needle", 129, 64, True, "out"), ("gauss", 200, 128, False, "out")],
    "enew_dropped": [("newtok", 65, 64, False, "out"), ("newtok", 513, 128, True, "out"), ("needle", 129, 64, True, "out"), ("gauss", 200, 128, False, "out")],
    "merge_swap": [("ramp12", 513, 64, False, "out"), ("ramp12", 1100, 128, True, "out"), ("fall12", 513, 64, True, "out"), ("gauss", 1100, 64, False, "out"),
                   ("needle", 1100, 128, False, "out")],
    "dead_record": [("gauss", 65, 64, False, "out"), ("ramp12", 513, 128, True, "out"), ("sunk", 1100, 64, True, "out"), ("needle", 129, 128, False, "out")],
    "half_m": [("needle", 129, 128, False, "out"), ("needle", 513, 128, True, "out"), ("ramp12", 513, 128, False, "rec"), ("gauss", 200, 128, True, "rec")],
    "head_map": [("needle", 65, 64, False, "out"), ("gauss", 513, 128, True, "out"), ("ramp12", 129, 64, True, "out"), ("sunk", 200, 128, False, "out")],
    "v_class": [("gauss", 65, 64, False, "out"), ("gauss", 513, 128, True, "out"), ("ramp12", 129, 64, True, "out"), ("fall12", 200, 128, False, "out"),
                ("oldonly", 513, 64, True, "out"), ("needle", 200, 64, True, "out")],
}
# fault -> [(family, keys, record size, f16 cache)] where the rows stay WITHIN the tolerance: why the other families exist
BLIND = {
    "new_twice": [("oldonly", 513, 64, True)],
    "enew_dropped": [("oldonly", 513, 64, False), ("oldonly", 129, 128, True)],
    "half_m": [("fall12", 513, 128, False), ("gauss", 513, 128, False), ("ramp12", 513, 128, True)],
    "v_class": [("newtok", 513, 64, True)],
}


def test_every_fault_is_listed():
    assert set(EXPOSES) == set(dr.FAULTS)


@pytest.mark.parametrize("fault", dr.FAULTS)
def test_every_seeded_fault_exceeds_the_tolerance_on_its_families(tables, fault):
    for name, keys, rec, kv_f16, what in EXPOSES[fault]:
        c = case(tables, name, keys, kv_f16)
        clean, clean_rec, _ = run_walk(tables, c, rec)
        assert clean <= 1.0 and clean_rec <= 1.0
        r, rr, _ = run_walk(tables, c, rec, fault=fault)
        print(f"{fault} on {name} keys={keys} rec={rec} kv16={int(kv_f16)}: max(err/tol) rows {r:.3g} records {rr:.3g}")
        assert (r if what == "out" else rr) > 1.0, (fault, name, keys, rec, kv_f16, r, rr)


@pytest.mark.parametrize("fault", list(BLIND))
def test_the_families_that_do_not_see_a_fault(tables, fault):
    for name, keys, rec, kv_f16 in BLIND[fault]:
        r, _, _ = run_walk(tables, case(tables, name, keys, kv_f16), rec, fault=fault)
        assert r <= 1.0, (fault, name, keys, rec, kv_f16, r)
