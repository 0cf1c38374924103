"""CPU: the model tests/gemv_mfma_ref.py holds k_gemv_mfma to, checked without a GPU -- and the selection the kernel's launcher takes its
instance from (csrc/gemv_instance.hpp), against the selection as launch_gemv_mfma made it before it moved there.

  selection    tests/host/gemv_instance_sweep.cpp (host compiler, no HIP) prints gemv_mfma_instance over rows {16, 48, 4112, 8208, 16400} x blocks
               1..32 x paired / unpaired x LN 0, 1, 2 x every scale form; old_selection below restates launch_gemv_mfma's own lines once.
  the model    equals a float64 W @ x with the epilogues in float64 within its own bound plus the quantisation it models (half a step 2^(be - 156)
               per element), on every input family, for every shape of the GPU table with rows <= 160.
  faults       for every fault of gemv_mfma_ref.FAULTS one named case on which the faulty model leaves the bound by a factor of 4, or differs
               where the bound is 0: the GPU file's inputs can see what they are meant to see.
  digits       the balanced digits and the quantiser against Python integers at the corners.
  exact cases  every plane-vector case of the GPU table has bound 0 on all of its elements; the table's case count and its docstring."""
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_mfma_ref as M  # noqa: E402
import gemvq_ref as Q  # noqa: E402
import test_gemv_mfma_instances_gpu as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = T.EPS


# ---------------------------------------------------------------- the selection
def div_ceil(a, b):
    return -(-a // b)


def old_pick_ksplit(rows, cols, paired, nw=8):
    n_tiles, nblk = div_ceil(rows, 16), div_ceil(cols, 256)
    ks_max = 4 if paired else 8
    ks = ks_max
    while ks >= 1:
        if not (ks > nblk or div_ceil(nblk, ks) > 5) and div_ceil(n_tiles * ks, nw) <= 256:
            return ks
        ks >>= 1
    ks = 1
    while ks < ks_max and (n_tiles * ks < 8 * 256 or div_ceil(nblk, ks) > 5) and ks * 2 <= nblk:
        ks *= 2
    return ks


def old_selection(rows, cols, silu, ln, sc, merge=False):
    """launch_gemv_mfma as it chose before gemv_mfma_instance: gemv_geometry, nv, the BH_PICK chain over (RING, NV) in its order, the merging
    override, the LDS size -> None (refused) or the tuple the sweep prints"""
    nw = 8
    ks = old_pick_ksplit(rows, cols, silu, nw)
    lg = {1: 0, 2: 1, 4: 2, 8: 3}[ks]
    nblk = div_ceil(cols, 256)
    ring = div_ceil(nblk, ks)
    ring_t = 2 if ring <= 2 else ring
    tiles = nw // ks
    grid = div_ceil(div_ceil(rows, 16), tiles)
    nv = div_ceil(cols // 4, nw * 64) if ln else 1
    if ring > 5 or nv > 4:
        return None
    kfn = None
    if merge:
        if ln or ring > 2 or cols % 128:
            return None
        kfn = (2, 1, 0, 1)
    for R_, NV_ in ((2, 2), (2, 4), (3, 2), (3, 4), (4, 2), (4, 4), (5, 2), (5, 4)):
        if ring <= R_ and nv <= NV_ and kfn is None:
            kfn = (R_, NV_, 2, 0) if ln == 2 else (R_, NV_, 1, 0) if ln else (R_, 1, 0, 0)
    if kfn is None:
        return None
    lds = nw * (5 if sc else 4) * (ring_t * 256 + 16) + 2 * nw * 8 + nw * 16 * 4 + (cols * 4 if ln == 1 else 0)
    return (ks, lg, nblk, ring, kfn[0], kfn[1], kfn[2], kfn[3], tiles, grid, lds, int(lds > 64 * 1024))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_selection_is_what_the_launcher_chose_before(tmp_path):
    exe = str(tmp_path / "gemv_instance_sweep")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/bitnet-rs_amd/csrc", os.path.join(ROOT, "tests", "host", "gemv_instance_sweep.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    rows = [16, 48, 4112, 8208, 16400]
    out = subprocess.run([exe, *map(str, rows), "x", "1", "32"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    plain = [ln for ln in lines if not ln.startswith("merge")]
    merge = [ln for ln in lines if ln.startswith("merge")]
    assert len(plain) == len(rows) * 32 * 2 * 3 * 4 and len(merge) == 32 * 3
    taken = set()
    for line in plain:
        key, val = line.split("|")
        r, cols, paired, ln, sc, wscale = map(int, key.split())
        got = tuple(map(int, val.split()))
        want = old_selection(r, cols, bool(paired), ln, sc)
        assert got == ((0,) if want is None else (1,) + want), line
        if want is not None:
            taken.add((want[4], want[5], want[6], sc))
    for line in merge:
        key, val = line.split("|")
        _, nblk, sc = key.split()
        got = tuple(map(int, val.split()))
        want = old_selection(48, int(nblk) * 256, False, 0, int(sc), merge=True)
        assert got == ((0,) if want is None else (1, want[0], want[3], want[4], want[5], want[7], want[10])), line
    # the sweep itself walks every reachable plain instance: 12 + 21 + 21
    assert len(taken) == 54, sorted(taken)


# ---------------------------------------------------------------- the table
def test_case_table_counts_and_docstring():
    assert len(T.CASES) == T.N_CASES == 54 and len(set(T.CASES)) == 54 and len(T.LEAVES_MFMA) == 2
    assert [k for n, k in T.CASES if n == "16x300c"] == ["qk256"]
    # the docstring's table, row by row, against SHAPES and the selection
    rows = re.findall(r"^  (P?\d+x\d+c?) +(\d+) x (\d+) +(\d) +((?:\d )+) +(\d) +(\d) +(\d) +(\d) +(\d+)", T.__doc__, re.M)
    assert [r[0] for r in rows] == list(T.SHAPES)
    reached = set()
    for name, r, c, ks, ranges, bpw, ring, nv, tiles, grid in rows:
        rows_, cols, paired, expect, nv_ = T.SHAPES[name]
        assert (int(r), int(c)) == (rows_, cols) and int(nv) == nv_
        assert dict(k_split=int(ks), blocks=div_ceil(cols, 256), blocks_per_wave=int(bpw), ring=int(ring), tiles_per_workgroup=int(tiles), grid=int(grid)) == expect
        assert [b1 - b0 for b0, b1 in Q.k_ranges(div_ceil(cols, 256), int(ks))] == list(map(int, ranges.split())), name
        for kind in M.KINDS:
            if (name, kind) not in T.CASES:
                continue
            for ln in (0, 1, 2):
                sel = old_selection(rows_, cols, paired, ln, M.SCALE_FORM[kind])
                assert sel[:4] == (int(ks), {1: 0, 2: 1, 4: 2, 8: 3}[int(ks)], expect["blocks"], int(bpw)) and sel[4] == int(ring) and sel[5] == (nv_ if ln else 1)
                assert sel[10] == T.lds_bytes(name, kind, ln)
                reached.add((sel[4], sel[5], ln, M.SCALE_FORM[kind]))
    assert len(reached) == 54  # + the 3 merging instances = the docstring's 57 of 63
    assert "57 of 63" in T.__doc__
    for (n_heads, n_kv), ks in T.MERGES.items():
        assert old_selection(T.MERGE_ROWS, n_heads * 128, False, 0, 0, merge=True)[0] == ks


# ---------------------------------------------------------------- digits and the quantiser
CORNERS = [0, 1, 127, 128, 129, 2 ** 15, 2 ** 23 + 2 ** 15 + 2 ** 7, 2 ** 30 - 1]


def test_digits_at_the_corners():
    qs = sorted({s * q for q in CORNERS for s in (1, -1)} | {2 ** 30})
    d = M.digits(np.array(qs, np.int64))
    for i, q in enumerate(qs):
        di = [int(d[j, i]) for j in range(4)]
        assert sum(di[j] * 256 ** j for j in range(4)) == q, (q, di)
        assert all(-128 <= v <= 127 for v in di[:3]) and -64 <= di[3] <= 64, (q, di)
    # a carry runs through: 128 = -128 + 1 * 256; 2^23 + 2^15 + 2^7 = -128 - 127 * 256 - 127 * 65536 + 1 * 2^24
    assert [int(v) for v in M.digits(np.array([128]))[:, 0]] == [-128, 1, 0, 0]
    assert [int(v) for v in M.digits(np.array([2 ** 23 + 2 ** 15 + 2 ** 7]))[:, 0]] == [-128, -127, -127, 1]
    # the planted fault reads the same bytes without the carry: it must differ exactly where a low byte is 128 or more
    bad = M.digits(np.array(qs, np.int64), "carry")
    for i, q in enumerate(qs):
        low_bytes = [(q & 0xFFFFFFFF) >> (8 * j) & 0xFF for j in range(3)]
        assert (sum(int(bad[j, i]) * 256 ** j for j in range(4)) != q) == any(b >= 128 for b in low_bytes), q


@pytest.mark.parametrize("e", [-100, -3, 0, 17, 96])
def test_quantiser_at_power_of_two_maxima(e):
    """am exactly 2^e: q of the maximum is 2^29; am one ulp below 2^(e + 1): q = 2^30 - 64; every other element against exact rationals"""
    rng = np.random.default_rng(e + 200)
    for top in (np.float32(2.0 ** e), np.nextafter(np.float32(2.0 ** (e + 1)), np.float32(0))):
        x = (rng.uniform(-1, 1, 64) * float(top)).astype(np.float32)
        x[5], x[6], x[7] = top, -top, np.float32(float(top) * 2.0 ** -31)
        be, q = M.quantise(x)
        assert be == max(32, 127 + e)
        sc = Fraction(2) ** (156 - be)
        for xi, qi in zip(x, q):
            v = Fraction(float(xi)) * sc + Fraction(1, 2)
            assert int(qi) == v.numerator // v.denominator
        assert int(q[5]) == -int(q[6])
        if 127 + e >= 32:
            assert int(q[5]) == (2 ** 29 if top == np.float32(2.0 ** e) else 2 ** 30 - 64)
    # the exponent clamp: below 2^-95 every range takes be = 32, and the digits die out instead of the scale leaving the normal range
    be, q = M.quantise(np.array([2.0 ** -100, -2.0 ** -124, 2.0 ** -125, 1e-45], np.float32))
    assert be == 32 and [int(v) for v in q] == [2 ** 24, -1, 1, 0]


# ---------------------------------------------------------------- the model against float64
SMALL = [(n, k) for n, k in T.CASES if T.SHAPES[n][0] <= 160]


def quantisation(wts, x, ks):
    """sum_k |W_k| times half a step of the K range of k: how far the model's integers lie from x"""
    half = np.zeros(wts.cols)
    for c0, c1 in M.column_ranges(wts.cols, ks):
        if c1 > c0:
            half[c0:c1] = 2.0 ** (max(32, M.biased_exponent(np.abs(x[c0:c1]).max())) - 157)
    return wts.abs_row_sums(half)


def silu64(t):
    t = t.reshape(-1, 2, 16)
    with np.errstate(over="ignore"):
        return (t[:, 0] / (1.0 + np.exp(-t[:, 0])) * t[:, 1]).reshape(-1)


@pytest.mark.parametrize("name,kind", SMALL)
def test_model_equals_float64_within_its_bound(name, kind):
    rows, cols, paired, expect, _ = T.SHAPES[name]
    ks = expect["k_split"]
    rng = np.random.default_rng(T.seed_of(name, kind, "cpu"))
    res = rng.normal(0, 1, rows // 2 if paired else rows).astype(np.float32)
    for mode in ("exact", "float"):
        wts = T.weights_for(name, kind, "pow2" if mode == "exact" else "float")
        g_np = T.ln_gamma_for(cols, mode, T.seed_of(name, "gamma"))
        for ln in (0, 1, 2):
            if ln == 1 and mode == "exact":
                continue
            for vtag, x in T.vectors(name, kind, mode, ln, g_np):
                x64 = x.astype(np.float64)
                tag = (name, kind, mode, ln, vtag)
                if ln == 0:
                    a64 = x64
                    ref = wts.dot(a64)
                    p = M.product(wts, x, ks)
                    tol = p.bound[0] + quantisation(wts, x, ks)
                else:
                    mean, var = x64.mean(), x64.var()
                    denom = np.sqrt(var + EPS)
                    a64 = (x64 - mean) / denom * g_np.astype(np.float64)
                    ref = wts.dot(a64)
                    p = M.launch(wts, x, ks, ln=(ln, g_np, EPS, old_pick_ksplit(rows, cols, False)))
                    # what the float64 LayerNorm and the kernel's (f32 mean, f32 denominator: 2 u each, relatively; f32(x gamma): u) differ by,
                    # carried through the product, and the quantisation of the row the kernel quantises
                    mean32, denom32 = Q.ln_statistics(M.element_statistics(x), cols, EPS, M.STAT_DEPTH)
                    a_k = (x64 - mean32) / denom32 * g_np.astype(np.float64)
                    moved = wts.abs_row_sums(np.abs(a_k - a64) + 4 * M.U * (np.abs(a_k) + abs(mean32) / denom32 * np.abs(g_np)))
                    act = a_k.astype(np.float32) if ln == 1 else (x * g_np)
                    tol = p.bound[0] + moved + quantisation(wts, act, ks) / (1.0 if ln == 1 else denom32)
                err = np.abs(M.target(p)[0] - ref)
                assert np.all(err <= tol), (tag, float((err / np.maximum(tol, 1e-300)).max()))
                if mode == "exact" and ln == 0:
                    assert np.all(p.bound[0] == 0) and np.array_equal(p.want[0], ref), tag  # the plane vectors: the model IS the float64 product
                if ln == 0 and paired:
                    ps = Q.silu_mul(p)
                    g_, u_ = ref.reshape(-1, 2, 16)[:, 0].reshape(-1), ref.reshape(-1, 2, 16)[:, 1].reshape(-1)
                    tq = tol.reshape(-1, 2, 16)
                    with np.errstate(over="ignore"):
                        sg = np.abs(g_ / (1.0 + np.exp(-g_)))
                    tol_s = ps.bound[0] + 1.1 * tq[:, 0].reshape(-1) * (np.abs(u_) + tq[:, 1].reshape(-1)) + sg * tq[:, 1].reshape(-1) + 2e-7 * np.abs(silu64(ref))
                    assert np.all(np.abs(ps.want[0] - silu64(ref)) <= tol_s), tag
                if ln == 0 and not paired:
                    pr = Q.add_residual(p, res)
                    assert np.all(np.abs(M.target(pr)[0] - (ref + res)) <= pr.bound[0] + tol + M.U * np.abs(ref + res)), tag


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("name,kind", [c for c in T.CASES if c[0] not in T.LARGE])
def test_plane_vectors_are_exact_on_every_element(name, kind):
    """100 % of the output elements of every plane-vector case carry bound 0 (the product of the vector, of vector * gamma behind LN 2, and of
    gamma itself for g = W . gamma), and the value is the float64 product: nothing rounds on the way"""
    prods = T.exact_products(name, kind)
    assert len(prods) == 11
    for tag, p in prods:
        assert np.all(p.bound[0] == 0), (name, kind, tag, float(p.units.max()))
        assert np.array_equal(p.exact32[0].astype(np.float64), p.want[0]), (name, kind, tag)


# ---------------------------------------------------------------- fault sensitivity
def leaves(good, bad, margin=4.0):
    """the faulty answer lies outside the bound of the good one by `margin` on some element, or differs where the bound is 0"""
    tg, tb, b = M.target(good)[0], M.target(bad)[0], good.bound[0]
    diff = np.abs(tg - tb)
    return bool(np.any((b == 0) & (diff > 0)) or np.any((b > 0) & (diff > margin * (b + bad.bound[0]))))


def plane_case(name, kind, plane, **kw):
    return vector_case(name, kind, f"plane{plane}", **kw)


def vector_case(name, kind, vtag, **kw):
    wts = T.weights_for(name, kind, "pow2")
    x = dict(T.vectors(name, kind, "exact", 0, None))[vtag]
    ks = T.SHAPES[name][3]["k_split"]
    return lambda fault=None: M.launch(wts, x, ks, fault=fault, silu=T.SHAPES[name][2], **kw)


def float_case(name, kind, vtag, ln):
    wts = T.weights_for(name, kind, "float")
    rows, cols, paired, expect, _ = T.SHAPES[name]
    g = T.ln_gamma_for(cols, "float", T.seed_of(name, "gamma"))
    x = dict(T.vectors(name, kind, "float", ln, g))[vtag]
    lnarg = (ln, g, EPS, old_pick_ksplit(rows, cols, False)) if ln else None
    return lambda fault=None: M.launch(wts, x, expect["k_split"], ln=lnarg, silu=paired, fault=fault)


def merge_case(fault, live_pos, n_heads=4, n_kv=2, kind="qk256"):
    rng = np.random.default_rng(T.seed_of("merge", "cpu", fault))
    wts = Q.make_weights(kind, T.MERGE_ROWS, n_heads * 128, 7, any_shape=True)
    records = T.write_records(rng, n_kv, n_heads // n_kv, 4, (live_pos + 64) >> 6, 40.0)

    def run(f=None):
        v, delta = M.merged_row(records, live_pos, n_heads, n_kv, 4, f)
        return M.product(wts, v, T.MERGES[(n_heads, n_kv)], spread=delta)
    return run


# fault -> the case that exposes it (shape, kind, vector), as a function fault -> Product
EXPOSED_BY = {
    "plane_dropped_0": lambda: plane_case("48x11", "qk256", 0),
    "plane_dropped_1": lambda: plane_case("48x11", "i2s32", 1),
    "plane_dropped_2": lambda: plane_case("48x11", "i2s32h", 2),
    "plane_dropped_3": lambda: plane_case("48x11", "i2s256", 3),
    "planes_swapped": lambda: plane_case("16x17", "qk256", 1),
    "plane_weight": lambda: plane_case("16x17", "i2s32", 1),
    "carry": lambda: plane_case("33x5", "qk256", 0),
    "part_dropped": lambda: plane_case("48x11", "qk256", 2),
    "parts_swapped": lambda: plane_case("48x11", "i2s32", 0),
    "clamped_twice": lambda: plane_case("48x11", "qk256", 1),
    "tail_unmasked": lambda: plane_case("48x2564c", "qk256", 0),
    "scale_pair": lambda: plane_case("33x5", "i2s32", 0),
    "scale_half": lambda: plane_case("33x5", "i2s32h", 0),
    "wscale_block": lambda: plane_case("48x11", "i2s256", 0),
    "g_row": lambda: float_case("P32x10", "qk256", "mean", 2),
    "mean_kept": lambda: float_case("48x11", "qk256", "mean", 1),
    "silu_on_up": lambda: float_case("P32x10", "i2s32", "mixed", 0),
    "dead_record": lambda: merge_case("dead_record", 100),
    "record_head": lambda: merge_case("record_head", 255),
    "rpi_in_f32": lambda: vector_case("48x11", "i2s32", "rpi"),
}


@pytest.mark.parametrize("fault", M.FAULTS)
def test_every_fault_is_exposed_by_a_named_case(fault):
    if fault == "surplus_tile_stored":  # 33 rows in 48 slots: the good launch leaves NaN behind row 33, the faulty one does not
        wts = T.weights_for("33x5", "qk256", "pow2")
        p = M.product(wts, dict(T.vectors("33x5", "qk256", "exact", 0, None))["plane0"], 4)
        good, bad = M.stored_rows(wts, p), M.stored_rows(wts, p, fault)
        assert np.isnan(good[33:]).all() and good.size == 48 and not np.isnan(bad[33:]).any()
        return
    if fault == "residual_row":  # m = 3 on 33x5: rows 1 and 2 take their own residual rows
        wts = T.weights_for("33x5", "i2s256", "float")
        xs = np.stack([x for _, x in T.vectors("33x5", "i2s256", "float", 0, None)[:3]])
        res = np.random.default_rng(5).normal(0, 1, (3, 33)).astype(np.float32)
        good, bad = M.launch_rows(wts, xs, 4, residual=res), M.launch_rows(wts, xs, 4, residual=res, fault=fault)
        assert not leaves(good[0], bad[0]) and leaves(good[1], bad[1]) and leaves(good[2], bad[2])
        return
    run = EXPOSED_BY[fault]()
    good, bad = run(), run(fault)
    assert leaves(good, bad), fault
    assert not leaves(good, run()), fault  # (and the model is a function of its inputs)


def test_fault_list_is_the_documented_one():
    assert set(EXPOSED_BY) | {"surplus_tile_stored", "residual_row"} == set(M.FAULTS) and len(M.FAULTS) == 22
