"""CPU: the numpy restatement of the context shift (tests/shift_ref.py) against its float64 target and the bound derived in that file's docstring,
four injected faults against the same bound, and the host-side arithmetic of Decoder::shift as pure functions.

max_pos 4096, rope_theta 5e5, n = 4095 (a sequence at the wall), 2 KV heads, standard-normal keys; (keep, discard) = (4, 2046), (0, 1), (64, 3000).
f32 cache: raw keys r (float64 normals), stored key = the f32 rotation of r by table row j + discard (the rounding a cache write has), target = the
float64 rotation of r by table row j.  f16 cache: the STORED f16 key is the random datum and the raw key is its exact inverse image
(shift_ref.unrotate_f64), so term 1 of the bound is zero and the f16 addend covers the one rounding of the result, as the bound counts it.
Faults must exceed the bound more than tenfold somewhere.  The row-`discard` fault's 2e-4 relative error is below ten times the 2^-11 an f16
rounding is allowed, so on the f16 cache it is held to the f32 part of the bound, on the result before its rounding to f16."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shift_ref as sr  # noqa: E402

MAX_POS, THETA, N, N_KV = 4096, 5e5, 4095, 2
CASES = [(4, 2046), (0, 1), (64, 3000)]
HALF = sr.HALF


@pytest.fixture(scope="module")
def tables():
    return sr.rope_tables(MAX_POS, THETA)


def make(tables, f16, seed):
    """-> (stored K [N, kv, D] in the cache's dtype, V likewise, raw keys [N, kv, D] float64 by slot)"""
    sin, cos = tables
    rng = np.random.default_rng(seed)
    pos = np.arange(N)
    v = rng.standard_normal((N, N_KV, sr.D)).astype(np.float16 if f16 else np.float32)
    if f16:
        k = rng.standard_normal((N, N_KV, sr.D)).astype(np.float16)
        return k, v, sr.unrotate_f64(k, sin[pos], cos[pos])
    raw = rng.standard_normal((N, N_KV, sr.D))
    r32 = raw.astype(np.float32)
    raw = r32.astype(np.float64)  # the projection's output is an f32 number
    s, c = sin[pos][:, None, :], cos[pos][:, None, :]
    r0, r1 = r32[..., :HALF], r32[..., HALF:]
    k = np.concatenate([(r0 * c - r1 * s).astype(np.float32), (r0 * s + r1 * c).astype(np.float32)], axis=-1)
    return k, v, raw


def excess(got, target, f16):
    """worst |got - target| / bound"""
    return float((np.abs(np.asarray(got, np.float64) - target) / sr.bound(target, f16)).max())


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("keep,discard", CASES)
def test_the_restatement_stays_inside_the_bound(tables, keep, discard, f16):
    sin, cos = tables
    k, v, raw = make(tables, f16, 1000 * keep + discard)
    k2, v2 = sr.shift_f32(k, v, sin, cos, keep, discard, N)
    j = np.arange(keep, N - discard)
    target = sr.target_f64(raw, sin, cos, keep, discard, N)
    worst = excess(k2[j], target, f16)
    units = float((np.abs(k2[j].astype(np.float64) - target) / (sr.bound(target) / sr.BOUND_UNITS)).max())
    print(f"shift_ref keep={keep} discard={discard} f16={f16}: worst / bound {worst:.3f}; worst in u (|k0| + |k1|): {units:.2f}")
    assert worst <= 1.0
    assert np.array_equal(v2[j].view(np.uint16 if f16 else np.uint32), v[j + discard].view(np.uint16 if f16 else np.uint32))
    # everything else keeps its bits
    rest = np.ones(N, bool)
    rest[j] = False
    for a, b in ((k2, k), (v2, v)):
        assert np.array_equal(a[rest].view(np.uint8), b[rest].view(np.uint8))


def faulty(name, k, v, sin, cos, keep, discard, n):
    """shift_ref.shift_f32 with one thing wrong"""
    f = np.float32
    j = np.arange(keep, n - discard)
    x = np.asarray(k[j + discard], f)
    x0, x1 = x[..., :HALF], x[..., HALF:]
    sa, ca, sb, cb = (t[:, None, :] for t in (sin[j + discard], cos[j + discard], sin[j], cos[j]))
    c, s = (ca * cb + sa * sb).astype(f), (sa * cb - ca * sb).astype(f)
    k2, v2 = k.copy(), v.copy()
    v2[j] = v[j + discard]
    if name == "row_discard":  # the obvious formula: turn back by table row `discard`
        c, s = np.broadcast_to(cos[discard], c.shape), np.broadcast_to(sin[discard], s.shape)
    if name == "sign_of_s":
        s = -s
    if name == "adjacent_pairs":  # the pair (i, i + 1) in place of (i, i + 64)
        e, o = x[..., 0::2], x[..., 1::2]
        c2, s2 = c[..., : HALF], s[..., : HALF]
        y = np.empty_like(x)
        y[..., 0::2], y[..., 1::2] = e * c2 + o * s2, o * c2 - e * s2
        k2[j] = y.astype(k.dtype)
        return k2, v2
    if name == "v_rotated":
        v2[j] = sr.rerotate_f32(np.asarray(v[j + discard], f), sin[j + discard], cos[j + discard], sin[j], cos[j]).astype(v.dtype)
    k2[j] = np.concatenate([x0 * c + x1 * s, x1 * c - x0 * s], axis=-1).astype(k.dtype)
    return k2, v2


FAULTS = [(f, h) for f in ("row_discard", "sign_of_s", "adjacent_pairs", "v_rotated") for h in (False, True) if not (f == "row_discard" and h)]


@pytest.mark.parametrize("keep,discard", CASES)
@pytest.mark.parametrize("fault,f16", FAULTS, ids=[f"{f}-{'kv16' if h else 'kv32'}" for f, h in FAULTS])
def test_injected_faults_break_the_bound_tenfold(tables, fault, keep, discard, f16):
    sin, cos = tables
    k, v, raw = make(tables, f16, 1000 * keep + discard)
    j = np.arange(keep, N - discard)
    k2, v2 = faulty(fault, k, v, sin, cos, keep, discard, N)
    if fault == "v_rotated":
        want = v[j + discard].astype(np.float64)
        worst = float((np.abs(v2[j].astype(np.float64) - want) / (2.0 ** -24 * (np.abs(want) + 1e-30))).max())  # V is a bit copy: any bound is zero
        assert not np.array_equal(v2[j], v[j + discard]) and worst > 10.0
        return
    worst = excess(k2[j], sr.target_f64(raw, sin, cos, keep, discard, N), f16)
    print(f"fault {fault} keep={keep} discard={discard} f16={f16}: worst / bound {worst:.1f}")
    assert worst > 10.0


@pytest.mark.parametrize("keep,discard", CASES)
def test_row_discard_on_an_f16_cache_breaks_the_f32_part_of_the_bound(tables, keep, discard):
    """the f16 cache's share of the row-`discard` fault: the stored f16 keys, widened exactly, through the faulty formula, taken BEFORE the one
    rounding to f16 and held to the bound without its f16 addend.  The right formula on the same keys stays inside that part, so the rounding
    allowance is all that hides the fault in the whole bound."""
    sin, cos = tables
    k, v, raw = make(tables, True, 1000 * keep + discard)
    wide_k, wide_v = k.astype(np.float32), v.astype(np.float32)
    j = np.arange(keep, N - discard)
    target = sr.target_f64(raw, sin, cos, keep, discard, N)
    right, _ = sr.shift_f32(wide_k, wide_v, sin, cos, keep, discard, N)
    wrong, _ = faulty("row_discard", wide_k, wide_v, sin, cos, keep, discard, N)
    ok, worst = excess(right[j], target, False), excess(wrong[j], target, False)
    print(f"f16 keys before rounding, keep={keep} discard={discard}: right / bound {ok:.3f}, row_discard / bound {worst:.1f}")
    assert ok <= 1.0 and worst > 10.0


def test_two_shifts_compose(tables):
    """a second shift works on the first one's output: within twice the bound of the raw keys' final slots (each shift adds one bound)"""
    sin, cos = tables
    k, v, raw = make(tables, False, 7)
    k1, v1 = sr.shift_f32(k, v, sin, cos, 4, 1000, N)
    k2, v2 = sr.shift_f32(k1, v1, sin, cos, 4, 500, N - 1000)
    j = np.arange(4, N - 1500)
    target = sr.rotate_f64(raw[j + 1500], sin[j], cos[j])
    assert float((np.abs(k2[j].astype(np.float64) - target) / sr.bound(target)).max()) <= 2.0
    assert np.array_equal(v2[j], v[j + 1500])


def shift_state_slow(pos, forced, history, keep, discard, max_pos):
    """Decoder::shift's loops, entry by entry"""
    out = [0] * len(history)
    for i in range(keep):
        out[i] = int(history[i])
    for i in range(keep + discard, max_pos):
        out[i - discard] = int(history[i])
    f = forced if forced <= keep else (keep if forced <= keep + discard else forced - discard)
    return pos - discard, f, out


def test_history_forced_count_and_records_follow_the_shift():
    rng = np.random.default_rng(3)
    max_pos = 300
    for _ in range(200):
        pos = int(rng.integers(1, max_pos))
        keep = int(rng.integers(0, pos))
        discard = int(rng.integers(1, pos - keep + 1))
        forced = int(rng.integers(0, max_pos + 1))
        hist = np.zeros(max_pos + 2, np.int32)
        hist[:max(pos + 1, forced)] = rng.integers(1, 2048, max(pos + 1, forced))
        p2, f2, h2 = sr.shift_state(pos, forced, hist, keep, discard, max_pos)
        assert (p2, f2, list(h2)) == shift_state_slow(pos, forced, hist, keep, discard, max_pos)
        assert p2 == pos - discard and h2[p2] == hist[pos]                      # the unconsumed token travels
        assert np.array_equal(h2[:keep], hist[:keep]) and np.array_equal(h2[keep:p2], hist[keep + discard:pos])
        assert not h2[max_pos - discard:].any()
        assert f2 == (forced if forced <= keep else keep if forced <= keep + discard else forced - discard)
        rec = rng.integers(0, 255, (max_pos, 12)).astype(np.uint8)  # no 0xFF byte in a live record
        r2 = sr.shift_records(rec, pos, keep, discard)
        for q in range(max_pos):
            if q <= keep:
                assert np.array_equal(r2[q], rec[q])
            elif q <= pos - discard:
                assert np.array_equal(r2[q], rec[q + discard])
            else:
                assert (r2[q] == 0xFF).all()
    # the three branches of the forced count, at their edges
    assert [sr.shift_forced(f, 4, 10) for f in (0, 4, 5, 14, 15, 20)] == [0, 4, 4, 4, 5, 10]
