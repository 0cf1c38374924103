"""CPU checks of the chain restatement (tests/sampler_chain_ref.py): the reference's own known answers (tests/golden/sampler_chain_kats.json),
and with neutral values the token and the record of `RefSampler` on every case of tests/sampler_cases.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
import sampler_chain_ref as cr  # noqa: E402
import sampler_ref as sr  # noqa: E402

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_chain_kats.json")))


@pytest.mark.parametrize("kat", KATS["min_p"], ids=lambda k: k["note"][:40])
def test_min_p_known_answers(kat):
    keep, _ = cr.min_p_keep(np.array(kat["probs"], np.float32), kat["min_p"])
    p = np.array(kat["probs"], np.float32)
    assert [int(i) for i in np.flatnonzero(keep & (p > 0))] == kat["keep"]


@pytest.mark.parametrize("kat", KATS["typical"], ids=lambda k: k["note"][:40])
def test_typical_known_answers(kat):
    p = np.array(kat["probs"], np.float32)
    t = cr.typical_keep(p, kat["typical_p"])
    keep = np.flatnonzero(p > 0) if t is None else np.flatnonzero(t["keep"])
    assert kat["count"][0] <= keep.size <= kat["count"][1]  # what the reference's test asserts
    assert [int(i) for i in keep] == kat["keep"]


def test_clamps_and_penalty_known_answers():
    for v, want in KATS["clamp"]["min_p"]:
        assert cr.ChainRef(1.0, 0, 1.0, 1.0, min_p=v).mp == np.float32(want)
    for v, want in KATS["clamp"]["typical_p"]:
        assert cr.ChainRef(1.0, 0, 1.0, 1.0, typical_p=v).ty == np.float32(want)
    for kat in KATS["penalty"]:
        x = cr.additive(np.array(kat["logits"], np.float32), [tuple(c) for c in kat["counts"]], kat["frequency_penalty"], kat["presence_penalty"])
        assert np.all(np.abs(x - np.array(kat["expect"], np.float32)) <= kat["abs"] + 1e-12), (x, kat)


def test_stage_rules_on_exact_rows():
    # typical-p: ties in ascending id, the entry that crosses is kept, `>=`
    p = np.full(64, 1 / 64, np.float32)
    t = cr.typical_keep(p, 0.5)
    assert t["cutoff"] == 32 and np.array_equal(np.flatnonzero(t["keep"]), np.arange(32))
    assert np.flatnonzero(cr.typical_keep(p, 0.0)["keep"]).tolist() == [0]
    # an entry whose probability is 0 is neither kept nor counted
    q = np.array([0.5, 0.0, 0.5], np.float32)
    assert np.flatnonzero(cr.typical_keep(q, 0.99)["keep"]).tolist() == [0, 2]
    # NaN: both comparisons are false
    nan = np.full(4, np.nan, np.float32)
    assert cr.min_p_keep(nan, 0.5)[0].all() and cr.typical_keep(nan, 0.5) is None
    # min_p 1 keeps exactly the entries tied at the maximum
    assert np.flatnonzero(cr.min_p_keep(np.array([0.3, 0.2, 0.3, 0.2], np.float32), 1.0)[0]).tolist() == [0, 2]


def test_the_greedy_shortcut_needs_every_stage_off():
    assert cr.ChainRef(1.0, 0, 1.0, 1.1).is_greedy() and cr.ChainRef(0.0, 0, 1.0, 1.0, min_p=0.3, typical_p=0.2).is_greedy()
    assert not cr.ChainRef(1.0, 0, 1.0, 1.0, min_p=0.1).is_greedy() and not cr.ChainRef(1.0, 0, 1.0, 1.0, typical_p=0.9).is_greedy()
    assert cr.ChainRef(1.0, 0, 1.0, 1.0, min_p=-1.0, typical_p=2.0, frequency_penalty=0.5).is_greedy()  # penalties do not leave path G
    # path G with the penalties: 10 - 0.5 * 2 - 0.3 = 8.7 < 9
    r = cr.ChainRef(0.0, 0, 1.0, 1.0, frequency_penalty=0.5, presence_penalty=0.3)
    x = np.zeros(8, np.float32)
    x[:2] = [10.0, 9.0]
    assert r.sample(x, [0]) == 0 and r.sample(x, [0, 0]) == 1 and r.rng.draws == 0


def test_neutral_values_give_ref_sampler_on_every_case():
    n = 0
    for case in sc.ALL:
        x = sc.row(case)
        a, b = sr.RefSampler(*case["cfg"], seed=case["seed"]), cr.ChainRef(*case["cfg"], seed=case["seed"])
        hist = sc.gen(case)
        for _ in range(case["steps"]):
            wa, wb = a.sample(x, hist), b.sample(x, hist)
            assert wa == wb and a.last_path == b.last_path and a.last_margin == b.last_margin and a.rng.draws == b.rng.draws, case["id"]
            for key, va in a.last.items():
                vb = b.last[key]
                if isinstance(va, np.ndarray):
                    assert np.array_equal(va, vb, equal_nan=True), (case["id"], key)
                else:
                    assert va == vb or (va is None and vb is None), (case["id"], key)
            hist = hist + [wa]
            n += 1
    assert n == sum(c["steps"] for c in sc.ALL)
