"""CPU checks of the per-draw acceptance rule (tests/sampler_accept.py) over exactly the case lists the GPU runs
(tests/sampler_cases.py).  What makes the rule trustworthy:

  * the reference's own token lies within `tol` of its float64 interval on every case (by construction of `tol`);
  * an exact sampler -- `Exact` below, an independent float64 implementation with the same filters, tie rules and u: what an ideal
    device returns -- is accepted on every case, the flat 128k rows where it lands far from the reference included;
  * copies of the exact sampler that are wrong in one way (MUTANTS) are each rejected on at least one named case;
  * the rule admits few tokens: never more than 2 * ceil(T / smallest kept probability) + 1, and exactly the reference's token
    when one probability exceeds 0.5 and u is more than tol inside its interval.

One mutant differs from the issue's wording: "the wrong keystream word" takes word n + 1 for draw n.  A greedy call that consumed
a word could not show through tokens alone, because bitnet_hip_sampler_configure (the only way from a greedy config to a
sampling one) restarts the stream; the GPU tests hold the draw counter after every G call instead.

Sequences (steps > 1) feed every sampler the reference's own growing list, so each step is one comparable call.
Wall time of this module: about 20 s on the development machine (tests/test_sampler_ref.py: 4 s); EXPERIMENTS.md section 9."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_accept as sa  # noqa: E402
import sampler_cases as sc  # noqa: E402
import sampler_ref as sr  # noqa: E402

MUTANTS = ["topk_tie_last", "negzero_below", "topp_ge", "topp_one_fewer", "topp_one_more", "draw_sorted_order", "penalty_plain_count",
           "penalty_mul_positive", "nan_before_penalty", "temperature_after_topk", "u_shift_9", "keystream_word_off_by_one",
           "fallthrough_last_kept"]
MUTANT_MAX_VOCAB = 65537  # the mutants run on the smaller cases only: every one of them is rejected there


def _desc_order(x, negzero_below=False):
    key = x.astype(np.float32).copy()
    if negzero_below:
        key[(key == 0) & np.signbit(key)] = np.float32(-1e-45)
    return np.argsort(-key, kind="stable"), key


class Exact:
    """The sampler with exact sums: f32 where the reference is elementwise (penalty, temperature, x - max), float64 for every sum
    (numpy's pairwise float64 sums: error about 1e-16 * log2(n), nine orders below any tolerance here)."""

    def __init__(self, cfg, seed, mutant=None):
        t, k, p, rp = cfg
        self.t, self.k, self.p, self.rp = np.float32(t), int(k), np.float32(p), np.float32(rp)
        self.key = sr.pcg32_key(seed)
        self.n_draws = 0
        self.exp = collections.Counter()
        self.m = mutant

    def _u(self):
        n = self.n_draws + (1 if self.m == "keystream_word_off_by_one" else 0)
        w = sr.chacha20_block(self.key, n // 16)[n % 16]
        self.n_draws += 1
        return float(w >> (9 if self.m == "u_shift_9" else 8)) * 2.0 ** -24

    def sample(self, logits, generated):
        m = self.m
        if m == "penalty_plain_count":
            self.exp = collections.Counter(int(g) for g in generated)  # occurrences in the list, not compounded over the calls
        else:
            self.exp.update(int(g) for g in generated)
        x = np.array(logits, np.float32)
        n = x.size
        greedy = self.t == 0 or (self.t == 1 and self.k == 0 and self.p == 1)
        with np.errstate(all="ignore"):
            if m == "nan_before_penalty":
                x[np.isnan(x)] = -np.inf
            if self.rp != 1:
                for tok, c in self.exp.items():
                    if tok < n:
                        pen = sr.powi(self.rp, c)  # the square-and-multiply loop itself is pinned in test_sampler_ref.py
                        x[tok] = np.float32(x[tok] * pen) if (x[tok] <= 0 or np.isnan(x[tok]) or m == "penalty_mul_positive") else np.float32(x[tok] / pen)
            if np.isnan(x).any():
                if m == "nan_before_penalty" and not greedy and not 0 < self.k < n and not self.p < 1:
                    self._u()  # a NaN left in the row poisons the softmax: every probability NaN, the draw falls through
                    return n - 1
                x[np.isnan(x)] = -np.inf
            if greedy:
                mx = x.max()
                return 0 if mx == -np.inf else int(np.flatnonzero(x == mx)[0])
            if self.t != 1 and m != "temperature_after_topk":
                x = (x / self.t).astype(np.float32)
            kept = np.ones(n, bool)
            nzb = m == "negzero_below"
            if 0 < self.k < n:
                _, key = _desc_order(x, nzb)
                kth = np.partition(key, n - self.k)[n - self.k]
                above = key > kth
                ties = np.flatnonzero(key == kth)
                r = self.k - int(above.sum())
                kept = above.copy()
                kept[ties[-r:] if m == "topk_tie_last" else ties[:r]] = True
            if self.t != 1 and m == "temperature_after_topk":
                x = (x / self.t).astype(np.float32)
            x = np.where(kept, x, np.float32(-np.inf)).astype(np.float32)
            if self.p < 1:
                M = x.max()
                if np.isfinite(M):
                    e = np.exp((x - M).astype(np.float32).astype(np.float64))
                    order, _ = _desc_order(x, nzb)
                    cs = np.cumsum(e[order]) / float(e.sum())
                    over = np.flatnonzero(cs >= float(self.p) if m == "topp_ge" else cs > float(self.p))
                    cut = int(over[0]) + 1 if over.size else n
                    cut = min(n, max(1, cut + {"topp_one_fewer": -1, "topp_one_more": 1}.get(m, 0)))
                    keep2 = np.zeros(n, bool)
                    keep2[order[:cut]] = True
                    kept &= keep2
                    x = np.where(kept, x, np.float32(-np.inf)).astype(np.float32)
            u = self._u()
            M = x.max()
            if not np.isfinite(M):
                if m == "fallthrough_last_kept" and M == -np.inf:
                    return int(np.flatnonzero(kept)[-1])
                return n - 1
            e = np.exp((x - M).astype(np.float32).astype(np.float64))
            tot = float(e.sum())
            if m == "draw_sorted_order":
                order, _ = _desc_order(x)
                over = np.flatnonzero(np.cumsum(e[order]) / tot > u)
                return int(order[over[0]]) if over.size else n - 1
            over = np.flatnonzero(np.cumsum(e) / tot > u)
            return int(over[0]) if over.size else n - 1


def _relevant(mutant, case):
    t, k, p, rp = case["cfg"]
    v = case["vocab"]
    if mutant in ("topk_tie_last", "temperature_after_topk"):
        return 0 < k < v
    if mutant.startswith("topp"):
        return p < 1
    if mutant.startswith("penalty") or mutant == "nan_before_penalty":
        return rp != 1
    if mutant == "fallthrough_last_kept":
        return case["row"][0] == "all_neginf" and k > sc.SMALL_K  # an F case: top-k keeps the first k of the tie, the last of them is not vocab - 1
    return True


@pytest.fixture(scope="module")
def walked():
    """One pass over every case: per call, a small summary (the records themselves are too large to keep)."""
    out = []
    killed: dict[str, str] = {}
    for case in sc.ALL:
        x = sc.row(case)
        ref = sr.RefSampler(*case["cfg"], seed=case["seed"])
        ex = Exact(case["cfg"], case["seed"])
        muts = {}
        if case["vocab"] <= MUTANT_MAX_VOCAB:
            muts = {m: Exact(case["cfg"], case["seed"], m) for m in MUTANTS if m not in killed and _relevant(m, case)}
        hist = sc.gen(case)
        for step in range(case["steps"]):
            want = ref.sample(x, hist)
            got = ex.sample(x, hist)
            ok, reason = sa.accepts(ref, got)
            s = dict(id=case["id"], step=step, path=ref.last_path, k=ref.k, want=want, exact=got, ok=ok, reason=reason, verdict=dict(ref.last["verdict"]),
                     flat=case["row"][0] != "planted")
            for m, mu in muts.items():
                mg = mu.sample(x, hist)
                if m not in killed and not sa.accepts(ref, mg)[0]:
                    killed[m] = f"{case['id']} step {step}: want {want}, mutant {mg}: {sa.accepts(ref, mg)[1]}"
            if ref.last_path == "F":
                an = sa.analyse(ref)
                s["nan_row"] = an["nan_row"]
                if not an["nan_row"]:
                    s.update(tol=an["tol"], T=an["T"], cut_ok=an.get("cut_ok", True), dist_want=float(an["dist"][want]), width_want=float(an["width"][want]),
                             u=an["u"], n_admit=int(an["admit"].sum()), cap=sa.admitted_cap(ref), pmax=an["pmax"], f32_total=an["f32_total"],
                             inside=min(an["u"] - float(an["lo"][want]), float(an["hi"][want]) - an["u"]))
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
        assert s["cut_ok"], s
        if s["width_want"] > 0 and s["u"] < s["f32_total"]:
            assert s["dist_want"] <= s["tol"], s  # its f32 interval holds u; the f64 endpoints are within the drift
        else:
            assert s["u"] >= s["f32_total"] and s["u"] >= 1 - s["tol"], s  # the fall-through: the f32 sums ended at or below u
    assert n > 300


def test_the_exact_sampler_is_accepted_on_every_case(walked):
    calls, _ = walked
    bad = [s for s in calls if not s["ok"]]
    per = collections.Counter((s["path"], s["exact"] == s["want"]) for s in calls)
    far = max(calls, key=lambda s: s["verdict"]["idx"])
    worst = max((s for s in calls if s["verdict"]["T"] > 0), key=lambda s: s["verdict"]["dist"] / s["verdict"]["T"])
    print(f"\nexact sampler: {len(calls)} calls; (path, equal): {dict(per)}; largest index distance {far['verdict']['idx']} ({far['id']}); "
          f"largest dist / T {worst['verdict']['dist'] / worst['verdict']['T']:.3f} ({worst['id']})")
    assert not bad, bad[:5]
    # the flat 128k row: the exact sampler lands far from the reference and is accepted
    flat = [s for s in calls if s["id"].startswith("adv-v128256-equal-F") and s["exact"] != s["want"]]
    assert flat and max(s["verdict"]["idx"] for s in flat) >= 20, flat


def test_every_mutant_is_rejected_by_a_named_case(walked):
    _, killed = walked
    print()
    for m in MUTANTS:
        print(f"mutant {m}: {killed.get(m, 'NOT REJECTED')}")
    assert not [m for m in MUTANTS if m not in killed]


def test_the_rule_admits_few_tokens(walked):
    calls, _ = walked
    f = [s for s in calls if s["path"] == "F" and not s["nan_row"]]
    over = [s for s in f if s["n_admit"] > s["cap"]]
    assert not over, over[:5]
    sure = [s for s in f if s["pmax"] > 0.5 and s["width_want"] > 0.5 and s["inside"] > s["tol"]]
    assert len(sure) >= 20
    assert not [s for s in sure if s["n_admit"] != 1]
    print(f"\nF calls {len(f)}; admitted tokens: median {int(np.median([s['n_admit'] for s in f]))}, max {max(s['n_admit'] for s in f)}; "
          f"{len(sure)} calls with one probability above 0.5 and u inside it admit exactly the reference's token")


def test_the_hard_coded_seeds_put_u_at_the_ends():
    lo = sr.ChaCha20Rng(sc.SEED_U_LOW).random_f32()
    hi = sr.ChaCha20Rng(sc.SEED_U_HIGH).random_f32()
    assert 0 <= lo < 2.0 ** -16 and 1 - 2.0 ** -16 <= hi < 1
    # the fall-through case: the reference's f32 total of that row ends below 1 and below u
    case = next(c for c in sc.ENDS if c["id"].startswith("ends-past-total"))
    ref = sr.RefSampler(*case["cfg"], seed=case["seed"])
    assert ref.sample(sc.row(case), []) == case["vocab"] - 1
    assert ref.last["cum"][-1] < 1 and ref.last["u"] >= ref.last["cum"][-1] and ref.last["probs"][-1] > 0


def test_case_lists_cover_what_they_claim():
    assert {c["vocab"] for c in sc.SWEEP} == set(sc.SWEEP_VOCABS) and sc.SWEEP_VOCABS[-1] == 1 << 20
    for v in (1024, 1025, 65536, 65537, 1 << 20):
        nwg, sl = sc.geometry(v)
        assert nwg * sl >= v > (nwg - 1) * sl
    assert sc.geometry(1024) == (1, 1024) and sc.geometry(1025) == (2, 513) and sc.geometry(65536) == (64, 1024) and sc.geometry(65537) == (64, 1025)
    labels = collections.Counter()
    for c in sc.ALL:
        r = sr.RefSampler(*c["cfg"])
        labels["G" if r.is_greedy() else "S" if 0 < r.k <= sr.SMALL_K and r.k < c["vocab"] else "F"] += 1
    assert labels["G"] >= 20 and labels["S"] >= 80 and labels["F"] >= 300, labels
    # the duplicated k-th value straddles every slice boundary
    case = next(c for c in sc.ADVERSARIAL if c["id"].startswith("adv-v128256-kth_dup-F2"))
    x = sc.row(case)
    nwg, sl = sc.geometry(case["vocab"])
    kth = np.sort(x)[::-1][case["cfg"][1] - 1]
    assert (x == kth).sum() >= 200 and all(x[b - 1] == kth and x[b] == kth for b in range(sl, case["vocab"], sl))
    # the penalty edges reach inf and 0
    assert sr.powi(np.float32(2.0), 200) == np.inf and sr.powi(np.float32(0.5), 200) == 0 and sr.powi(np.float32(1e10), 3) < np.inf
