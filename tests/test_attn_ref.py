"""CPU checks of tests/attn_ref.py, the float64 model behind tests/test_prefill_attn_instances_gpu.py: the model against the existing
float64 prompt reference, the conditions every input family must meet (from the model, never from the kernel), the float32 emulation of the
kernel's loop under the tolerance, and the seeded faults -- which of them which family exposes, and that Gaussian inputs expose neither of
the alpha faults: the reason the families exist."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
from test_prefill_parity import prefill_f64  # noqa: E402

D = 128
MAX_POS = 512


@pytest.fixture(scope="module")
def tables(oracle):
    sin, cos = oracle.rope_tables(D, MAX_POS, 10000.0)
    return sin.reshape(MAX_POS, D // 2), cos.reshape(MAX_POS, D // 2)


_cases = {}


def case(tables, name, T, n_heads=2, n_kv=1, causal=True):
    """-> the f32 inputs and f16 operands of one family at T positions (cached: the reference is computed once and left unchanged)"""
    key = (name, T, n_heads, n_kv, causal)
    if key not in _cases:
        sin, cos = tables
        rng = np.random.default_rng(ar.seed_of("ref", *key))
        pos = np.arange(T)
        q1, k1, v, t = ar.family(name, rng, pos, T, n_heads, n_kv, causal)
        q_in, k_in, v_in = ar.unrope(q1, pos, sin, cos), ar.unrope(k1, pos, sin, cos), v.astype(np.float32)
        qh, kh, vh = ar.operands_q(q_in, pos, sin, cos), ar.operands_k(k_in, pos, sin, cos), ar.operands_v(v_in)
        want, tl, p = ar.model(qh, kh, vh, pos, causal)
        for a in (q_in, k_in, v_in, qh, kh, vh, want, tl, p):
            a.setflags(write=False)
        _cases[key] = dict(q_in=q_in, k_in=k_in, v_in=v_in, qh=qh, kh=kh, vh=vh, want=want, tol=tl, p=p, t=t, pos=pos, q1=q1, k1=k1)
    return _cases[key]


def walk_ratio(c, h=0, **kw):
    got, cnt = ar.walk(c["qh"][:, h], c["kh"][:, 0], c["vh"][:, 0], c["pos"], **kw)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - c["want"][:, h]) / c["tol"][:, h])), cnt


def test_the_scale_constant():
    assert ar.QMUL == np.float32(np.float32(1.4426950408889634) * np.float32(0.08838834764831845))
    assert abs(float(ar.QMUL) - np.log2(np.e) / np.sqrt(128.0)) <= 2.0 ** -24 * 0.2


@pytest.mark.parametrize("T", [1, 65, 130])
def test_model_agrees_with_the_existing_f64_reference_within_operand_rounding(tables, T):
    """exact() on the f16 operands against prefill_f64 on the unrounded ones.  q and k are each rounded by at most 2^-11 relative, so a natural
    -log score moves by at most ds = (2^-10 + 2^-22) sum_d |q_d k_d| / sqrt(128) (+ the f32 rounding of QMUL, 2^-24); probabilities then
    move by a factor within e^(+-2 ds) and v by 2^-11 relative: |difference| <= (e^(2 ds) - 1 + 2^-11 e^(2 ds)) sum_j p_j |v_jd|."""
    sin, cos = tables
    n_heads, n_kv = 4, 2
    c = case(tables, "gauss", T, n_heads, n_kv)
    qkv = np.concatenate([c["q_in"].reshape(T, -1), c["k_in"].reshape(T, -1), c["v_in"].reshape(T, -1)], axis=1)
    base = prefill_f64(qkv, sin, cos, n_heads, n_kv)
    q, k = np.abs(ar.rope(c["q_in"], c["pos"], sin, cos)), np.abs(ar.rope(c["k_in"], c["pos"], sin, cos))
    for h in range(n_heads):
        g = h // (n_heads // n_kv)
        ds = ((2.0 ** -10 + 2.0 ** -22 + 2.0 ** -23) * (q[:, h] @ k[:, g].T) / np.sqrt(D) * ar.visible(c["pos"], T)).max(axis=1, keepdims=True)
        bound = (np.expm1(2 * ds) + 2.0 ** -11 * np.exp(2 * ds)) * (c["p"][h] @ np.abs(c["vh"][:, g])) * (1 + 2.0 ** -9) + 1e-12
        assert np.all(np.abs(c["want"][:, h] - base[:, h]) <= bound)
    # and the rounding is there: the two references are not the same numbers
    assert T == 1 or np.max(np.abs(c["want"] - base)) > 1e-6


@pytest.mark.parametrize("T", [130, 200, 333, 512])
@pytest.mark.parametrize("name", ar.FAMILIES)
def test_families_meet_their_conditions(tables, name, T):
    sin, cos = tables
    c = case(tables, name, T)
    # the f32 inputs reproduce the post-RoPE construction (rope(unrope(x)) = x to f32 rounding)
    back = ar.rope(c["k_in"], c["pos"], sin, cos)
    assert np.max(np.abs(back - c["k1"])) <= 2.0 ** -22 * np.max(np.abs(c["k1"]))
    s = ar.scores(c["qh"], c["kh"], c["pos"])
    if name != "needle":
        assert np.max(np.abs(s)) <= 128.0, np.max(np.abs(s))
    else:
        rows = np.arange(T)
        for h in range(c["qh"].shape[1]):
            w = c["p"][h][rows, c["t"][:, h]]
            assert np.all(c["t"][:, h] <= c["pos"])  # a visible key
            assert np.min(w) >= 1.0 - 2.0 ** -20, np.min(w)
            # v sits on a 1/64 grid, so the f16 rounding leaves it alone and the expected row IS the target's v
            assert np.array_equal(c["vh"], c["v_in"].astype(np.float64))
            assert np.all(np.abs(c["want"][:, h] - c["vh"][c["t"][:, h], 0]) <= 2.0 ** -20 * np.max(np.abs(c["vh"])))
    if name == "sunk":
        vis = ar.visible(c["pos"], T)
        assert np.max(s) <= -20.0  # a zero-padded key (score 0) would outweigh every real one by 2^20
        assert vis.sum() * c["qh"].shape[1] == s.size
    if name == "steep":  # the mass sits on the last few visible keys
        r = T - 1
        assert c["p"][0][r, max(0, r - 15):r + 1].sum() >= 0.99 if T <= 128 else c["p"][0][r, r - 63:r + 1].sum() >= 0.99
    if name == "fall12" and T > 130:  # later probabilities underflow (f32: 2^-149)
        assert c["p"][0][T - 1, 2 * 64:].max() < 2.0 ** -12


@pytest.mark.parametrize("heads", [(4, 1), (8, 2), (4, 2), (6, 1), (3, 3), (5, 1)], ids=lambda h: f"{h[0]}x{h[1]}")
def test_f32_rope_on_the_device_costs_at_most_half_the_tolerance(tables, heads):
    """The tolerance is twice the rounding bound of the probabilities; the walk uses at most half of it (below).  The other half is for what the
    model does not restate: the device rotates q and k in f32, so a few operands round to the other f16 neighbour.  On the inputs of the GPU
    module's whole-prompt cases (same seeds), with either f32 arithmetic a compiler may emit, the expected rows move by at most 0.5 tol."""
    import test_prefill_attn_instances_gpu as gpu

    sin, cos = tables
    n_heads, n_kv = heads
    for T in (130, 200):
        pos = np.arange(T)
        for name in ar.FAMILIES:
            q_in, k_in, v_in, _ = gpu.inputs(sin, cos, name, "fresh", pos, T, n_heads, n_kv)
            qh, kh, vh = ar.operands_q(q_in, pos, sin, cos), ar.operands_k(k_in, pos, sin, cos), ar.operands_v(v_in)
            want, tl, _ = ar.model(qh, kh, vh, pos)
            for fused in (False, True):
                q32 = ar.f16((ar.rope_f32(q_in, pos, sin, cos, fused).astype(np.float32) * ar.QMUL).astype(np.float64))
                k32 = ar.f16(ar.rope_f32(k_in, pos, sin, cos, fused))
                alt, _, _ = ar.model(q32, k32, vh, pos)
                r = float(np.max(np.abs(alt - want) / tl))
                print(f"{name} {heads} T={T} fused={fused}: {int((q32 != qh).sum())} q / {int((k32 != kh).sum())} k operands differ, max(shift/tol) {r:.3f}")
                assert r <= 0.5, (name, T, fused, r)


@pytest.mark.parametrize("T", [130, 200])
@pytest.mark.parametrize("name", ar.FAMILIES)
def test_walk_without_a_fault_stays_under_half_the_tolerance(tables, name, T):
    c = case(tables, name, T)
    for h in range(2):
        r, _ = walk_ratio(c, h)
        print(f"{name} T={T} head {h}: walk max(err/tol) {r:.3f}")
        assert r <= 0.5, r


@pytest.mark.parametrize("T", [130, 200, 512])
@pytest.mark.parametrize("name", ar.FAMILIES)
def test_walk_split_into_parts_equals_the_unsplit_walk(tables, name, T):
    c = case(tables, name, T)
    whole, _ = ar.walk(c["qh"][:, 0], c["kh"][:, 0], c["vh"][:, 0], c["pos"])
    for parts in range(1, 9):
        for qg in (32, 64, 128):
            got, _ = ar.walk(c["qh"][:, 0], c["kh"][:, 0], c["vh"][:, 0], c["pos"], parts=parts, split_tiles=1, qg=qg)
            assert np.isfinite(got).all()
            assert np.all(np.abs(got - whole) <= c["tol"][:, 0]), (parts, qg)
            assert np.all(np.abs(got - c["want"][:, 0]) <= c["tol"][:, 0]), (parts, qg)


def test_path_counters(tables):
    """which inputs reach which branch of the loop: the reference moves mid-prompt on ramp12 / steep / needle, never on sunk / fall12, and on
    ramp6 it is left stale (a tile's maximum above it, by no more than 8) before it moves"""
    for T in (130, 200):
        for name in ("ramp12", "steep", "needle"):
            _, cnt = walk_ratio(case(tables, name, T))
            assert cnt["grow_mid"] >= 1, (name, T, cnt)
        for name in ("sunk", "fall12"):
            _, cnt = walk_ratio(case(tables, name, T))
            assert cnt["grow_mid"] == 0, (name, T, cnt)
        _, cnt = walk_ratio(case(tables, "ramp6", T))  # 6 per tile: stale at the second tile, moved at the third or fourth (T = 200)
        assert cnt["stale"] > 0 and (cnt["grow_mid"] >= 1 or T < 200), cnt
    # ramp12 moves it in every tile behind the first that a row sees whole (12 per tile against the 8 of the rule; a diagonal tile with
    # few visible keys gains less)
    _, cnt = walk_ratio(case(tables, "ramp12", 200))
    assert cnt["grow_mid"] >= sum(max(0, (r + 1) // 64 - 1) for r in range(200)), cnt
    # a key-split share whose tiles lie wholly above a row's limit leaves that row's reference unset past the share's first tile: query blocks
    # at positions 192 and 0 in ONE 128-row workgroup (the token-parallel prefill), 4 tiles in 2 shares
    c = case(tables, "ramp12", 256)
    rows = np.concatenate([np.arange(192, 256), np.arange(0, 64)])
    got, cnt = ar.walk(c["qh"][rows, 0], c["kh"][:, 0], c["vh"][:, 0], c["pos"][rows], parts=2, split_tiles=1, qg=128)
    assert cnt["unset_mid"] >= 64, cnt
    assert np.all(np.abs(got - c["want"][rows, 0]) <= 0.5 * c["tol"][rows, 0])


EXPOSES = {
    "alpha_l": ("ramp12", "ramp6", "steep"),
    "alpha_o": ("ramp12", "ramp6", "steep", "needle"),
    "mask": ("gauss", "ramp12", "steep", "sunk"),
}


@pytest.mark.parametrize("fault", list(EXPOSES))
def test_every_seeded_fault_exceeds_the_tolerance_on_its_families(tables, fault):
    for name in EXPOSES[fault]:
        for T in ((200,) if name == "ramp6" else (130, 200)):  # (ramp6 first moves the reference past 192 keys)
            r, _ = walk_ratio(case(tables, name, T), fault=fault)
            print(f"{fault} on {name} T={T}: max(err/tol) {r:.3g}")
            assert r > 1.0, (fault, name, T, r)


def test_a_merge_that_ignores_m_exceeds_the_tolerance(tables):
    for name in ("ramp12", "steep", "fall12", "needle"):
        c = case(tables, name, 200)
        r, _ = walk_ratio(c, parts=3, split_tiles=1, fault="merge_m")
        print(f"merge_m on {name}: max(err/tol) {r:.3g}")
        assert r > 1.0, (name, r)
        ok, _ = walk_ratio(c, parts=3, split_tiles=1)
        assert ok <= 1.0


def test_gaussian_inputs_do_not_see_the_alpha_faults(tables):
    """why the families exist: on Gaussian scores the reference is set in the first tile and does not move at T = 130, so a loop that forgets
    alpha gives the correct walk's numbers"""
    c = case(tables, "gauss", 130)
    clean, cnt = ar.walk(c["qh"][:, 0], c["kh"][:, 0], c["vh"][:, 0], c["pos"])
    assert cnt["grow_mid"] == 0
    for fault in ("alpha_l", "alpha_o"):
        got, _ = ar.walk(c["qh"][:, 0], c["kh"][:, 0], c["vh"][:, 0], c["pos"], fault=fault)
        assert np.array_equal(got, clean), fault
        assert np.all(np.abs(got - c["want"][:, 0]) <= c["tol"][:, 0])
