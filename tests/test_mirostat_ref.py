"""CPU: the Mirostat restatement (tests/mirostat_ref.py) and its per-draw rule (tests/mirostat_accept.py).

The restatement is held to cases whose f32 arithmetic is exact by construction and to the reference's own unit tests
(crates/bitnet-sampling/src/strategies.rs: mu is 2 * tau at creation and after reset, the token is valid, the same seed gives the same
token).  The rule is held to a numpy MODEL of the kernel's arithmetic (`dev_model`: fixed-point sums, the g > mu - ln S form, the f32 update;
not a second restatement) on the seeded inputs the GPU tests use -- every call of the model must pass -- and to planted faults in that
model, each of which must be rejected on at least one case; the test prints which case catches which.  The loose-draw cap is checked here for
the restatement alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirostat_accept as ma  # noqa: E402
import mirostat_cases as mc  # noqa: E402
import mirostat_ref as mr  # noqa: E402
import sampler_ref as sr  # noqa: E402

F = np.float32
NINF = F(-np.inf)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 5, 10])
def test_equal_logits_give_exactly_one_over_n(k):
    n = 1 << k
    rec = mr.mirostat(np.full(n, F(1.25)), 100.0, 5.0, 0.1, sr.ChaCha20Rng(3))
    assert np.all(rec["p"] == F(1.0 / n)) and rec["S"] == n and not rec["fallback"]
    assert np.all(rec["q"] == F(1.0 / n)) and rec["sum2"] == 1
    assert rec["token"] == int(np.ceil(float(rec["u"]) * n)) - 1 if rec["u"] > 0 else rec["token"] == 0
    assert rec["surprise"] == F(-np.log(F(1.0 / n)))


def test_one_finite_entry_has_surprise_zero():
    x = np.full(300, NINF)
    x[17] = F(-3.5)
    for mu in (0.0, 1.0, 7.25):
        rec = mr.mirostat(x, mu, 3.0, 0.25, sr.ChaCha20Rng(1))
        assert rec["p"][17] == 1 and rec["token"] == 17 and not rec["fallback"] and rec["words"] == 1
        assert rec["surprise"] == 0 and rec["mu_after"] == F(F(mu) + F(0.25) * F(3.0))  # mu' = mu + eta * tau
    rec = mr.mirostat(x, -0.5, 3.0, 0.25, sr.ChaCha20Rng(1))  # surprise 0 > mu: removed, the fallback; the same token and update
    assert rec["fallback"] and rec["token"] == 17 and rec["words"] == 0 and rec["mu_after"] == F(F(-0.5) + F(0.75))


def test_the_reference_unit_tests():
    """strategies.rs tests: mu starts at 2 * tau and returns there on reset; the token is valid; the same seed gives the same token"""
    logits = np.array([2.0, 1.0, 0.5, -1.0, -2.0], F)
    a, b = mr.MirostatRef(5.0, 0.1, seed=42), mr.MirostatRef(5.0, 0.1, seed=42)
    assert a.mu == F(10.0)
    ta, tb = [a.sample(logits, []) for _ in range(8)], [b.sample(logits, []) for _ in range(8)]
    assert ta == tb and all(0 <= t < 5 for t in ta)
    assert a.mu != F(10.0)
    a.reset()
    assert a.mu == F(10.0)


def test_the_fallback_takes_the_last_maximum_and_draws_no_word():
    x = mc.tie_row(500, [3, 250, 499])
    rng = sr.ChaCha20Rng(9)
    rec = mr.mirostat(x, -1.0, 0.5, 0.1, rng)
    assert rec["fallback"] and rec["token"] == 499 and rec["words"] == 0 and rng.draws == 0
    assert sr.argmax(x) == 3  # the greedy pick's rule is the opposite one
    assert rec["surprise"] == F(-np.log(rec["p"][499]))
    rec = mr.mirostat(x, 50.0, 0.5, 0.1, rng)
    assert not rec["fallback"] and rng.draws == 1


@pytest.mark.parametrize("name", ["all-neg-inf", "all-nan", "pos-inf"])
def test_a_row_with_no_finite_maximum_is_uniform(name):
    x = {"all-neg-inf": np.full(64, NINF), "all-nan": np.full(64, F(np.nan)), "pos-inf": np.r_[np.zeros(60, F), F(np.inf), np.zeros(3, F)].astype(F)}[name]
    ref = mr.MirostatRef(5.0, 0.1, seed=2)
    ref.sample(x, [])
    rec = ref.last
    assert rec["uniform"] and np.all(rec["p"] == F(1 / 64)) and not rec["fallback"]  # -ln(1 / 64) = 4.16 <= mu = 10
    assert np.all(rec["kept"]) and rec["token"] == int(np.ceil(float(rec["u"]) * 64)) - 1
    ref.sample(x, [], mu=4.0)  # every entry removed: the fallback, the last maximum
    assert ref.last["fallback"] and ref.last["token"] == (60 if name == "pos-inf" else 63)
    assert ref.last["surprise"] == F(-np.log(F(1 / 64)))


class FixedU:
    def __init__(self, u):
        self.u, self.draws = F(u), 0

    def random_f32(self):
        self.draws += 1
        return self.u


def test_the_ends_of_the_walk():
    x = np.array([NINF, 0.0, 0.0, -40.0], F)  # entry 0 has no mass; entry 3 is removed at mu = 5
    rec = mr.mirostat(x, 5.0, 2.0, 0.1, FixedU(0.0))
    assert rec["token"] == 0 and rec["q"][0] == 0 and rec["surprise"] == F(2.0) and rec["mu_after"] == F(5.0)  # u <= 0 at id 0: tau
    rec = mr.mirostat(x, 5.0, 2.0, 0.1, FixedU(0.5))
    assert rec["token"] == 1  # u <= cumulative: `<=`, the sum is exactly 0.5 at id 1
    rec = mr.mirostat(np.array([0.0, 0.0, 0.0, -40.0], F), 5.0, 2.0, 0.1, FixedU(np.nextafter(F(1), F(0))))
    # three thirds in f32 end at or above u or not; either way the walk's end is n - 1 = 3, removed: tau
    if rec["cum"][-1] < rec["u"]:
        assert rec["token"] == 3 and rec["surprise"] == F(2.0)
    fell = 0
    for k in range(1, 200):  # rows whose f32 total ends below u = 1 - 2^-24: the walk falls through to n - 1, which the filter removed
        x = np.array([0.0, -0.5, -1.0] * k + [-40.0], F)
        rec = mr.mirostat(x, 8.0, 2.0, 0.1, FixedU(np.nextafter(F(1), F(0))))
        if rec["cum"][-1] < rec["u"]:
            fell += 1
            assert rec["token"] == x.size - 1 and not rec["kept"][-1] and rec["surprise"] == F(2.0) and rec["mu_after"] == F(8.0)
        else:
            assert rec["kept"][rec["token"]]
    assert fell > 0


# ---- a numpy model of the kernel's arithmetic, with planted faults ---------------------------------------------------------------------
def dev_model(x, mu, tau, eta, u, fault=None):
    """csrc/kernels_sample.hip mirostat_finish in numpy -> (token, mu_after, words)"""
    x = np.asarray(x, F)
    n = x.size
    mu, tau, eta = F(mu), F(tau), F(eta)
    M = F(x.max())
    finite = bool(np.isfinite(M))
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        if finite:
            g = (M - x).astype(F)
            e = np.exp((x - M).astype(F)).astype(F)
            mass = np.rint(e.astype(np.float64) * 2.0 ** 40)
            S = F(mass.sum() * 2.0 ** -40)
            lnS = F(np.log(S))
            thr = F(mu - lnS)
            fallback = bool(F(0) >= thr) if fault == "ge" else bool(F(0) > thr)
            removed = (g >= thr) if fault == "ge" else (g > thr)
        else:
            lnS = F(-np.log(F(F(1) / F(n))))
            fallback = bool(lnS >= mu) if fault == "ge" else bool(lnS > mu)
        words, sur = 0, lnS
        if fallback:
            hits = np.flatnonzero(x == M)
            tok = int(hits[0] if fault == "first" else hits[-1])
            words = 1 if fault == "word" else 0
        elif not finite:
            words = 1
            tok = 0 if u == 0 else min(n - 1, int(np.ceil(float(u) * n)) - 1)
        else:
            words = 1
            km = np.where(removed, 0.0, mass)
            Sk = F(km.sum() * 2.0 ** -40)
            C = np.cumsum(km) / km.sum()
            hit = np.flatnonzero((float(u) <= C) & (km > 0))
            tok = 0 if u == 0 else (int(hit[0]) if hit.size else n - 1)
            if fault == "chunk":
                tok = tok + 1024 if tok + 1024 < n else (tok - 1024 if tok >= 1024 else tok)
            q = F(0) if removed[tok] else F(e[tok] / (S if fault == "unfiltered" else Sk))
            sur = F(-np.log(q)) if q > 0 else tau
        if fault == "swap":
            mu_after = F(mu - F(tau * F(sur - eta)))
        elif fault == "sign":
            mu_after = F(mu + F(eta * F(sur - tau)))
        else:
            mu_after = F(mu - F(eta * F(sur - tau)))
    return tok, mu_after, words


def walk(case, fault=None, row=None, mu0=None, steps=None):
    """a case's chained calls: the model is the device, the restatement judges from the model's mu -> list of verdicts"""
    x = mc.row(case) if row is None else row
    ref = mr.MirostatRef(**mc.ref_kwargs(case))
    mu = ref.mu if mu0 is None else F(mu0)
    draws, hist, out = 0, [], []
    for _ in range(case["steps"] if steps is None else steps):
        ref.rng.draws = draws
        ref.sample(x, hist, mu=mu)
        rec = ref.last
        u = ma.u_of(ref.rng, draws)
        tok, mu_after, words = dev_model(rec["x"], mu, case["tau"], case["eta"], u, fault)
        v = ma.judge(rec, u, tok, mu_after, words)
        v["rec"] = rec
        out.append(v)
        mu, draws, hist = mu_after, draws + words, hist + [tok]
    return out


@pytest.fixture(scope="module")
def verdicts():
    return {c["id"]: walk(c) for c in mc.CASES}


def test_the_model_of_the_kernel_passes_the_rule_on_every_seeded_call(verdicts):
    for cid, vs in verdicts.items():
        for i, v in enumerate(vs):
            assert v["ok"], (cid, i, v["reason"])
            if v["mode"] == "draw":
                assert v["rec"]["_an"]["draw"]["base_ok"], (cid, i, "the restatement's kept set lies outside the derived band")


def test_the_regimes_are_the_ones_the_cases_name(verdicts):
    def share(cid):
        return sum(v["mode"] == "fallback" for v in verdicts[cid]) / len(verdicts[cid])

    for c in mc.CASES:
        if c["vocab"] >= 257 and c["tau"] == 0.5:
            assert share(c["id"]) == 1.0, c["id"]
            assert float(verdicts[c["id"]][-1]["rec"]["mu_after"]) < 0, c["id"]  # mu runs negative
        if c["vocab"] >= 32000 and c["tau"] == 3.0:
            assert share(c["id"]) == 1.0, c["id"]
        if c["vocab"] >= 257 and c["tau"] == 8.0:
            assert share(c["id"]) == 0.0 and np.mean(verdicts[c["id"]][0]["rec"]["kept"]) > 0.9, c["id"]
        if c["vocab"] >= 4099 and c["tau"] == 5.0:
            kept = [int(np.count_nonzero(v["rec"]["kept"])) for v in verdicts[c["id"]] if v["mode"] == "draw"]
            assert kept and 20 <= np.median(kept) <= 2000, (c["id"], kept)


def test_the_loose_cap_holds_for_the_restatement_alone():
    """at most 1/8 of a case's draws have an ambiguous mass above 1e-4 of the kept mass"""
    for c in mc.CASES:
        x, ref = mc.row(c), mr.MirostatRef(**mc.ref_kwargs(c))
        hist, draws, loose = [], 0, 0
        for _ in range(c["steps"]):
            d0 = ref.rng.draws
            tok = ref.sample(x, hist)
            rec = ref.last
            if not rec["fallback"]:
                v = ma.judge(rec, rec["u"], tok, rec["mu_after"], 1)
                draws += 1
                loose += v["loose"]
                assert ma.analyse(rec)["draw"]["admit"][tok]
            assert ref.rng.draws - d0 == rec["words"]
            hist.append(tok)
        print(f"{c['id']}: {loose} loose of {draws} draws")
        assert loose <= mc.LOOSE_CAP * max(draws, 1), (c["id"], loose, draws)


EXACT = dict(id="single-finite-mu0", vocab=300, tau=3.0, eta=0.25, sigma=0.0, temperature=1.0, seed=1, steps=1, **mc.PEN_OFF)


def planted(fault):
    """-> ids of the cases that reject the fault"""
    caught = []
    single = np.full(300, NINF)
    single[17] = F(-3.5)
    # surprise 0 against mu 0, every rounding absent: `>` keeps the entry and draws, `>=` removes it and falls back
    if not all(v["ok"] for v in walk(EXACT, fault, row=single, mu0=0.0)):
        caught.append(EXACT["id"])
    tie = dict(EXACT, id="tied-maxima-fallback", vocab=3000, tau=0.5, eta=0.1, steps=4)
    if not all(v["ok"] for v in walk(tie, fault, row=mc.tie_row(3000, [5, 1500, 2999]))):
        caught.append(tie["id"])
    for c in mc.CASES:
        if c["vocab"] in (4099, 32003) and not all(v["ok"] for v in walk(c, fault)):
            caught.append(c["id"])
    return caught


@pytest.mark.parametrize("fault", ["ge", "first", "word", "unfiltered", "swap", "sign", "chunk"])
def test_the_rule_rejects_planted_faults(fault):
    """`>=` for `>` in the filter; first-index fallback; a word drawn on fallback; mu updated from the unfiltered p; tau and eta swapped; the
    update's sign; a chunk off by one in the scan"""
    assert all(v["ok"] for v in walk(EXACT, None, row=np.r_[np.full(17, NINF), F(-3.5), np.full(282, NINF)].astype(F), mu0=0.0))
    caught = planted(fault)
    print(f"fault {fault}: rejected on {caught}")
    assert caught, fault
    must = {"ge": "single-finite-mu0", "first": "tied-maxima-fallback", "word": "tied-maxima-fallback"}.get(fault)
    assert must is None or must in caught, (fault, caught)
