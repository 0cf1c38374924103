"""CPU checks of the chain's per-draw acceptance rule (tests/sampler_chain_accept.py) over exactly the case lists the GPU runs
(tests/sampler_chain_cases.py), after tests/test_sampler_accept.py:

  * an exact sampler -- `Exact` below, an independent float64 implementation of the chain with the same filters, tie rules and u --
    is accepted on every case;
  * copies of it that are wrong in one way (MUTANTS) are each rejected on at least one named case;
  * the restatement's own token passes by construction, its min-p prefix and its typical-p kept set lie inside the admissible range;
  * at most 2 % of the min-p-only F draws and at most 10 % of the F typical-p draws are undecided (a deciding comparison inside the
    derived tolerance).

The typical-p mutants meet rows whose sums are exact (all entries equal) on both paths."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
import sampler_chain_accept as ca  # noqa: E402
import sampler_chain_cases as cc  # noqa: E402
import sampler_chain_ref as cr  # noqa: E402
import sampler_ref as sr  # noqa: E402

MUTANTS = ["minp_ignored", "minp_le", "typ_gt", "typ_one_more", "typ_one_fewer", "typ_ties_desc", "freq_uses_exponent"]
MUTANT_MAX_VOCAB = 2049
UNDECIDED_CAP_MINP = 0.02
UNDECIDED_CAP_TYP = 0.10


class Exact:
    """The chain with exact sums: f32 where the reference is elementwise (penalties, temperature, x - max), float64 for every sum."""

    def __init__(self, cfg, ex, seed, mutant=None):
        t, k, p, rp = cfg
        self.t, self.k, self.p, self.rp = np.float32(t), int(k), np.float32(p), np.float32(rp)
        self.mp = min(max(float(np.float32(ex["min_p"])), 0.0), 1.0)
        self.ty = min(max(float(np.float32(ex["typical_p"])), 0.0), 1.0)
        self.fp, self.pp = np.float32(ex["frequency_penalty"]), np.float32(ex["presence_penalty"])
        self.key = sr.pcg32_key(seed)
        self.n_draws = 0
        self.exp = collections.Counter()
        self.m = mutant

    def _u(self):
        w = sr.chacha20_block(self.key, self.n_draws // 16)[self.n_draws % 16]
        self.n_draws += 1
        return float(w >> 8) * 2.0 ** -24

    def sample(self, logits, generated):
        m = self.m
        self.exp.update(int(g) for g in generated)
        occ = collections.Counter(int(g) for g in generated)
        x = np.array(logits, np.float32)
        n = x.size
        greedy = self.t == 0 or (self.t == 1 and self.k == 0 and self.p == 1 and self.mp <= 0 and self.ty >= 1)
        with np.errstate(all="ignore"):
            if self.fp != 0 or self.pp != 0:
                for tok, c in occ.items():
                    if tok < n:
                        c = self.exp[tok] if m == "freq_uses_exponent" else c
                        x[tok] = np.float32(np.float32(x[tok] - np.float32(self.fp * np.float32(c))) - self.pp)
            if self.rp != 1:
                for tok, c in self.exp.items():
                    if tok < n:
                        pen = sr.powi(self.rp, c)
                        x[tok] = np.float32(x[tok] * pen) if (x[tok] <= 0 or np.isnan(x[tok])) else np.float32(x[tok] / pen)
            x[np.isnan(x)] = -np.inf
            if greedy:
                mx = x.max()
                return 0 if mx == -np.inf else int(np.flatnonzero(x == mx)[0])
            if self.t != 1:
                x = (x / self.t).astype(np.float32)
            kept = np.ones(n, bool)
            if 0 < self.k < n:
                kth = np.partition(x, n - self.k)[n - self.k]
                above = x > kth
                ties = np.flatnonzero(x == kth)
                kept = above.copy()
                kept[ties[: self.k - int(above.sum())]] = True
            x = np.where(kept, x, np.float32(-np.inf)).astype(np.float32)
            M = x.max()
            finite = bool(np.isfinite(M))
            if self.p < 1 and finite:
                e = np.exp((x - M).astype(np.float32).astype(np.float64))
                order = np.argsort(-x, kind="stable")
                over = np.flatnonzero(np.cumsum(e[order]) / float(e.sum()) > float(self.p))
                keep2 = np.zeros(n, bool)
                keep2[order[: int(over[0]) + 1 if over.size else n]] = True
                x = np.where(keep2, x, np.float32(-np.inf)).astype(np.float32)
            if self.mp > 0 and finite and m != "minp_ignored":
                e = np.exp((x - M).astype(np.float32).astype(np.float64))
                gone = e <= self.mp if m == "minp_le" else e < self.mp
                x = np.where(gone, np.float32(-np.inf), x).astype(np.float32)
            if self.ty < 1 and finite and np.isfinite(x.max()):
                e = np.exp((x - x.max()).astype(np.float32).astype(np.float64))
                p = e / e.sum()
                idx = np.flatnonzero(p > 0)
                ln = np.log(p[idx])
                H = float(-(p[idx] * ln).sum())
                d = np.abs(-ln - H)
                order = np.lexsort((-idx if m == "typ_ties_desc" else idx, d))
                cum = np.cumsum(p[idx][order])
                over = np.flatnonzero(cum > self.ty if m == "typ_gt" else cum >= self.ty)
                cutoff = int(over[0]) + 1 if over.size else idx.size
                cutoff = min(idx.size, max(1, cutoff + {"typ_one_more": 1, "typ_one_fewer": -1}.get(m, 0)))
                keep3 = np.zeros(n, bool)
                keep3[idx[order[:cutoff]]] = True
                x = np.where(keep3, x, np.float32(-np.inf)).astype(np.float32)
            u = self._u()
            M = x.max()
            if not np.isfinite(M):
                return n - 1
            e = np.exp((x - M).astype(np.float32).astype(np.float64))
            over = np.flatnonzero(np.cumsum(e) / float(e.sum()) > u)
            return int(over[0]) if over.size else n - 1


def _relevant(mutant, case):
    ex = case["ex"]
    if mutant.startswith("minp"):
        return ex["min_p"] > 0
    if mutant.startswith("typ"):
        return ex["typical_p"] < 1
    return ex["frequency_penalty"] != 0


def make_ref(case):
    return cr.ChainRef(*case["cfg"], seed=case["seed"], **case["ex"])


@pytest.fixture(scope="module")
def walked():
    out = []
    killed: dict[str, str] = {}
    for case in cc.ALL:
        x = sc.row(case)
        ref = make_ref(case)
        ex = Exact(case["cfg"], case["ex"], case["seed"])
        muts = {}
        if case["vocab"] <= MUTANT_MAX_VOCAB:
            muts = {m: Exact(case["cfg"], case["ex"], case["seed"], m) for m in MUTANTS if m not in killed and _relevant(m, case)}
        hist = sc.gen(case)
        for step in range(case["steps"]):
            want = ref.sample(x, hist)
            got = ex.sample(x, hist)
            ok, reason = ca.accepts(ref, got)
            s = dict(id=case["id"], step=step, path=ref.last_path, want=want, exact=got, ok=ok, reason=reason, undecided=ref.last["undecided"],
                     minp_only=case in cc.MINP_ONLY, typ=case in cc.FULL_TYP)
            for m, mu in muts.items():
                mg = mu.sample(x, hist)
                if m not in killed and not ca.accepts(ref, mg)[0]:
                    killed[m] = f"{case['id']} step {step}: want {want}, mutant {mg}: {ca.accepts(ref, mg)[1]}"
            if ref.last_path == "F":
                an = ca.analyse(ref)
                s["nan_row"] = an["nan_row"]
                if not an["nan_row"]:
                    s.update(cut_ok=an["cut_ok"], minp_ok=an.get("minp_ok", True), prefix_ok=an.get("minp_prefix_ok", True), typ_ok=an.get("typ_ok", True), n_amb=an.get("n_amb", 0), tol=an["tol"], T=an["T"],
                             dist_want=float(an["dist"][want]), width_want=float(an["width"][want]), u=an["u"], f32_total=an["f32_total"],
                             n_admit=int(an["admit"].sum()), n_kept=an["n_kept"])
            out.append(s)
            hist = hist + [want]
    return out, killed


def test_the_reference_token_passes_by_construction(walked):
    calls, _ = walked
    n = 0
    for s in calls:
        if s["path"] != "F" or s["nan_row"]:
            continue
        n += 1
        assert s["cut_ok"] and s["minp_ok"] and s["prefix_ok"] and s["typ_ok"], s
        if s["width_want"] > 0 and s["u"] < s["f32_total"]:
            assert s["dist_want"] <= s["tol"], s
        else:
            assert s["u"] >= s["f32_total"] and s["u"] >= 1 - s["tol"], s
    assert n > 150


def test_the_exact_sampler_is_accepted_on_every_case(walked):
    calls, _ = walked
    per = collections.Counter((s["path"], s["exact"] == s["want"]) for s in calls)
    print(f"\nexact chain sampler: {len(calls)} calls; (path, equal): {dict(per)}")
    bad = [s for s in calls if not s["ok"]]
    assert not bad, bad[:5]


def test_every_mutant_is_rejected_by_a_named_case(walked):
    _, killed = walked
    print()
    for m in MUTANTS:
        print(f"mutant {m}: {killed.get(m, 'NOT REJECTED')}")
    assert not [m for m in MUTANTS if m not in killed]


def test_undecided_draws_stay_under_the_cap(walked):
    calls, _ = walked
    minp = [s for s in calls if s["minp_only"] and s["path"] == "F"]
    und = [s for s in minp if s["undecided"]]
    print(f"\nmin-p-only F draws: {len(minp)}, undecided {len(und)} ({len(und) / len(minp):.2%})")
    assert len(minp) >= 150
    assert len(und) <= UNDECIDED_CAP_MINP * len(minp), und[:5]
    typ = [s for s in calls if s["typ"] and s["path"] == "F"]
    undt = [s for s in typ if s["undecided"]]
    by = collections.Counter(s["id"].rsplit("-sig", 1)[0] for s in undt)
    print(f"F typical-p draws: {len(typ)}, undecided {len(undt)} ({len(undt) / len(typ):.2%}); by case {dict(by)}")
    assert len(typ) >= 100
    assert len(undt) <= UNDECIDED_CAP_TYP * len(typ), undt[:5]


def test_the_rule_admits_few_tokens(walked):
    calls, _ = walked
    f = [s for s in calls if s["path"] == "F" and not s["nan_row"] and not s["undecided"]]
    # never more than the kept set, and where min-p leaves a handful of entries, a handful at the most
    assert all(s["n_admit"] <= s["n_kept"] + 2 for s in f), [s for s in f if s["n_admit"] > s["n_kept"] + 2][:3]
    assert np.median([s["n_admit"] for s in f]) <= 3


def test_case_lists_cover_what_they_claim():
    labels = collections.Counter()
    for c in cc.ALL:
        r = make_ref(c)
        labels["G" if r.is_greedy() else "S" if 0 < r.k <= sr.SMALL_K and r.k < c["vocab"] else "F"] += 1
        if c["row"] == ("normal", 2.0):
            assert c["ex"]["min_p"] >= 0.02, c["id"]  # flat rows only behind min-p
    assert labels["G"] >= 5 and labels["S"] >= 30 and labels["F"] >= 40, labels
    assert {c["vocab"] for c in cc.FULL} == {1025, 2049, 32000, 128256}
    assert sc.geometry(1025)[0] == 2 and sc.geometry(2049)[0] == 3
    for c in cc.FULL_TYP:  # at 128256: typical_p <= 0.5, or min-p in front
        assert c["vocab"] < 128256 or c["ex"]["typical_p"] <= 0.5 or c["ex"]["min_p"] >= 0.02, c["id"]
