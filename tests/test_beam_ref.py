"""CPU: the beam search rule.  tests/beam_ref.py (numpy, float32 operations in the stated order) is held to a brute-force float64 search over a tiny
table language model; every property of the rule is shown on a crafted input, with an assertion that the case really occurred; the compiled header
(csrc/beam_rule.hpp, the code k_beam_select runs) is run stand-alone under the address and undefined-behaviour sanitizers
(tests/host/beam_rule_check.cpp) and its output held EQUAL, step by step, to beam_ref.py on 200 seeded random searches; three planted faults are each
caught by a named case.  Nothing is loaded into Python under a sanitizer."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cases as bc  # noqa: E402
import beam_ref as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- a tiny table LM: the next-token log-probabilities depend on the whole prefix --------------------------------------------------------
V, DEPTH, EOS = 5, 4, 0


def table_lm(seed):
    rng = np.random.default_rng(seed)
    table = {}
    for n in range(DEPTH):
        for prefix in itertools.product(range(1, V), repeat=n):
            l = rng.normal(size=V) * 1.5
            table[prefix] = l - np.log(np.exp(l).sum())
    return table


def exhaustive(table):
    """every hypothesis: a prefix of non-EOS tokens ended by EOS (length <= DEPTH) or DEPTH non-EOS tokens -> [(score f64, tokens)] best first"""
    out = []
    for n in range(DEPTH + 1):
        for prefix in itertools.product(range(1, V), repeat=n):
            s = sum(table[prefix[:i]][prefix[i]] for i in range(n))
            if n < DEPTH:
                out.append((s + table[prefix][EOS], list(prefix) + [EOS]))
            else:
                out.append((s, list(prefix)))
    return sorted(out, key=lambda t: -t[0])


def run_table(table, B, cls=br.BeamRef):
    ref = cls(B, EOS, DEPTH, br.len_weights(DEPTH, 0.0))
    p = 0
    while not ref.done:
        lse, ids, logits = [], [], []
        # rows as a tap with top_n = 2B leaves them: the V entries by descending logit, then -inf entries under ids no token has (never EOS); a beam
        # that is dead (score -inf: a copy nobody continued) gets a row of those alone
        pad = list(range(V, V + 2 * B))
        for b in range(B):
            if ref.score[b] > -np.inf:
                row = table[tuple(ref.beam_tokens[b])]
                order = sorted(range(V), key=lambda t: (-row[t], t))
                ids.append((order + pad)[:2 * B]), logits.append(([row[t] for t in order] + [-np.inf] * (2 * B))[:2 * B])
            else:
                ids.append(pad), logits.append([-np.inf] * (2 * B))
            lse.append(0.0)
        ref.step(lse, ids, logits, p)
        p += 1
    return ref


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_against_the_exhaustive_search(seed):
    table = table_lm(seed)
    best = exhaustive(table)
    assert best[0][0] - best[1][0] > 1e-4  # float32 sums cannot swap the two best
    for B in (V ** 3, V ** 3 + 5):
        ref = run_table(table, B)
        tokens, score_bits, _ = ref.hypotheses()[0]
        assert tokens == best[0][1]
        assert abs(float(np.uint32(score_bits).view(np.float32)) - best[0][0]) < 1e-5
    # B = 1 is the greedy path: the argmax token of every row until EOS or the budget
    ref = run_table(table, 1)
    greedy, prefix = [], ()
    while len(greedy) < DEPTH:
        t = int(np.argmax(table[prefix]))
        greedy.append(t)
        if t == EOS:
            break
        prefix += (t,)
    assert ref.hypotheses()[0][0] == greedy and ref.pool_n == 1


# ---- crafted cases (inputs: tests/beam_cases.py): each asserts the rule's answer and that the case occurred --------------------------------
def play(name, cls):
    """-> (ref, step): step() runs the next step of the crafted search"""
    search = bc.CRAFTED[name]
    ref = bc.new_ref(search, cls)
    it = iter(range(len(search["steps"])))
    return ref, lambda: bc.ref_step(ref, search, next(it))


def case_tie_orders(cls=br.BeamRef):
    """equal scores: ascending j inside a beam (step 0), ascending b across beams (step 1)"""
    ref, step = play("tie_orders", cls)
    step()
    assert [w[1:] for w in ref.walk] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert list(ref.token[:2]) == [5, 6] and list(ref.parent[:2]) == [0, 0] and ref.score[0] == ref.score[1] == F(-1)
    step()
    assert [w[1:] for w in ref.walk] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert list(ref.token[:2]) == [10, 11] and list(ref.parent[:2]) == [0, 0]
    return ref


def case_non_finite_last(cls=br.BeamRef):
    """NaN and -inf candidates read as -inf and come last, in (b, j) order; a NaN lse sinks a whole beam"""
    ref, step = play("non_finite_last", cls)
    step()
    assert list(ref.score[:2]) == [F(-0.25), F(-0.5)]
    step()
    assert [w[1:] for w in ref.walk] == [(0, 1), (0, 3), (0, 0), (0, 2)]
    assert list(ref.token[:2]) == [6, 8] and list(ref.score[:2]) == [F(-1.25), F(-2.25)]
    step()  # +inf - 0 = +inf stays; +inf - +inf = NaN -> -inf; finite - +inf = -inf
    assert [w[1:] for w in ref.walk] == [(0, 3), (0, 0), (0, 1), (0, 2)]
    assert ref.score[0] == F(np.inf) and ref.score[1] == br.NEG_INF and list(ref.token[:2]) == [8, 5]
    return ref


def case_eos_walk_index(cls=br.BeamRef):
    """an EOS at walk index 0 < B is pooled, an EOS at walk index 2 >= B is skipped"""
    ref, step = play("eos_walk_index", cls)
    step()
    step()
    assert [w[1:] for w in ref.walk] == [(0, 0), (1, 0), (1, 1), (0, 1)]
    assert ("eos_pooled", 0) in ref.events and ("eos_skipped", 2) in ref.events
    assert ref.pool_n == 1 and ref.done == 0 and ref.pool_tokens[0] == [5, 9] and ref.pool_len[0] == 2
    assert ref.pool_score[0] == F(-1) + F(-0.1)
    assert list(ref.parent[:2]) == [1, 0] and list(ref.token[:2]) == [5, 5]
    return ref


def case_pool_replaces_worst(cls=br.BeamRef):
    """a full pool replaces its worst entry for a strictly greater key, and the search ends by the pool"""
    ref, step = play("pool_replaces_worst", cls)
    step()
    assert ref.events[:2] == [("eos_pooled", 2), ("pool_add", 0)] and ref.pool_key[0] == F(-12) and ref.pool_score[0] == F(-3)
    assert list(ref.token[:3]) == [1, 2, 3] and ref.done == 0
    step()
    assert [e for e in ref.events if e[0].startswith("pool")] == [("pool_add", 1), ("pool_add", 2), ("pool_replace", 0)]
    assert list(ref.pool_key[:3]) == [F(-4.125), F(-1.125), F(-2.125)] and list(ref.pool_order[:3]) == [3, 1, 2]
    assert ref.done == br.DONE_POOL and ref.pool_n == 3
    assert [h[0] for h in ref.hypotheses()] == [[1, 9], [2, 9], [3, 9]]
    return ref


def case_done_by_budget(cls=br.BeamRef):
    ref, step = play("done_by_budget", cls)
    step()
    assert ref.done == 0
    step()
    assert ref.done == br.DONE_BUDGET and ref.pool_n == 2 and list(ref.pool_len[:2]) == [2, 2]
    assert list(ref.pool_key[:2]) == [F(-2) * F(0.5), F(-2.5) * F(0.5)]
    assert [h[0] for h in ref.hypotheses()] == [[5, 1], [6, 1]]
    return ref


def case_from_is_div_before(cls=br.BeamRef):
    """three steps of two beams whose lineages part at step 0 and are replaced at step 2: from[] is read from div BEFORE the step"""
    ref, step = play("from_is_div_before", cls)
    step()
    assert list(ref.frm[:2]) == [10, 10] and ref.div[0, 1] == 11
    step()  # each beam continues itself: parents (0, 1)
    assert list(ref.parent[:2]) == [0, 1] and ref.div[0, 1] == 11 and list(ref.frm[:2]) == [11, 11]
    step()  # both from beam 1
    assert list(ref.parent[:2]) == [1, 1]
    assert list(ref.frm[:2]) == [11, 12]  # beam 0 takes beam 1's slots from where they parted; beam 1 is its own parent
    assert ref.div[0, 1] == 13
    return ref


CASES = [case_tie_orders, case_non_finite_last, case_eos_walk_index, case_pool_replaces_worst, case_done_by_budget, case_from_is_div_before]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_crafted_case(case):
    case()


def test_pool_worst_among_equal_keys_is_the_latest_inserted():
    ref = br.BeamRef(3, 9, 8, br.len_weights(8, 0.0))
    for i, s in enumerate([-2.0, -2.0, -1.0]):
        ref._pool_add(F(s), 1, 0, 9, [i])
    ref._pool_add(F(-2.0), 1, 0, 9, [3])  # not strictly greater: dropped
    assert ref.events[-1] == ("pool_drop", 1) and [t[0] for t in ref.pool_tokens[:3]] == [0, 1, 2]
    ref._pool_add(F(-1.5), 1, 0, 9, [4])  # replaces the LATER of the two -2 entries
    assert ref.events[-1] == ("pool_replace", 1) and [t[0] for t in ref.pool_tokens[:3]] == [0, 4, 2]
    assert [h[0] for h in ref.hypotheses()] == [[2], [4], [0]]


# ---- planted faults: each is caught by a named case --------------------------------------------------------------------------------------
class TieReversed(br.BeamRef):
    TIE_REVERSED = True


class FromNew(br.BeamRef):
    FROM_NEW = True


class EosAtBAccepted(br.BeamRef):
    EOS_SLACK = 1


@pytest.mark.parametrize("mutant,case", [(TieReversed, case_tie_orders), (FromNew, case_from_is_div_before), (EosAtBAccepted, case_eos_walk_index)],
                         ids=["wrong tie order", "from taken from div_new", "EOS at walk index B accepted"])
def test_planted_fault_is_caught(mutant, case):
    case()  # the rule passes ...
    with pytest.raises(AssertionError):
        case(mutant)  # ... and the fault does not


# ---- random searches ---------------------------------------------------------------------------------------------------------------------
def ref_lines(search, cls=br.BeamRef):
    ref = bc.new_ref(search, cls)
    lines = []
    for s in range(len(search["steps"])):
        if ref.done:
            break
        bc.ref_step(ref, search, s)
        lines.append((ref.words(), [list(ref.pool_tokens[i]) for i in range(ref.pool_n)]))
    return ref, lines


def test_div_recurrence_against_the_beams_token_prefixes():
    """div[b][c] from the recurrence == the first slot at which the two beams' tokens can have led to different cache contents: token k of a beam
    is consumed into slot P + 1 + k, so two beams share every slot up to and including P + (their common prefix length), and the slots just
    filled (<= p) at the most"""
    rng = np.random.default_rng(77)
    seen_deep = 0
    for _ in range(60):
        search = dict(bc.random_search(rng), eos=-1)  # no EOS: every search runs its whole budget
        B, P = search["B"], search["P"]
        ref = bc.new_ref(search)
        for s in range(len(search["steps"])):
            bc.ref_step(ref, search, s)
            p = P + s
            for b in range(B):
                for c in range(B):
                    tb, tc = ref.beam_tokens[b], ref.beam_tokens[c]
                    lcp = next((k for k in range(len(tb)) if tb[k] != tc[k]), len(tb))
                    assert ref.div[b, c] == min(P + 1 + lcp, p + 1), (b, c, tb, tc)
                    seen_deep += P + 1 + lcp < p + 1
    assert seen_deep > 100  # beams that parted more than one step ago occurred


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("beam") / "beam_rule_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'bitnet-rs_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "host", "beam_rule_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe


def test_compiled_header_equals_the_restatement_on_200_random_searches(check_exe, tmp_path):
    rng = np.random.default_rng(20240521)
    searches = [bc.random_search(rng) for _ in range(200)]
    u = lambda a: " ".join(str(int(x)) for x in np.asarray(a, F).reshape(-1).view(np.uint32))
    text = [str(len(searches))]
    for q in searches:
        text.append(f"{q['B']} {q['eos']} {q['max_new']} {q['P']}")
        text.append(u(q["lw"]))
        for step in q["steps"]:
            for lse, ids, logits in step:
                text.append(u(lse) + " " + " ".join(str(int(t)) for t in ids) + " " + u(logits))
    path = tmp_path / "searches.txt"
    path.write_text("\n".join(text) + "\n")
    run = subprocess.run([check_exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "beam_rule_check: ok" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = run.stdout.splitlines()[:-1]
    want, kinds = [], set()
    for search in searches:
        ref, lines = ref_lines(search)
        kinds.add(ref.done)
        for words, pool in lines:
            want.append(" ".join(str(w) for w in words) + " " + "".join("| " + "".join(f"{t} " for t in toks) for toks in pool))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.split() == w.split(), f"line {i}"
    assert {br.DONE_POOL, br.DONE_BUDGET} <= kinds  # both endings occurred


def test_the_random_searches_tell_the_planted_faults_too(check_exe):
    """the 200 searches are not blind to the faults either: each mutant's lines differ from the rule's somewhere"""
    rng = np.random.default_rng(20240521)
    searches = [bc.random_search(rng) for _ in range(200)]
    for mutant in (TieReversed, FromNew, EosAtBAccepted):
        assert any(ref_lines(s, mutant)[1] != ref_lines(s)[1] for s in searches), mutant.__name__
