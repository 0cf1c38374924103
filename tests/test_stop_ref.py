"""tests/stop_ref.py, the restatement the GPU stop tests are held to, against the contract in the words of this file: after a token is placed,
a stop id beats EOS, EOS beats the budget, the budget beats a stop sequence; the lowest index reports when several entries match; the token that
reaches the budget counts; a sequence may reach back exactly as far as tokens were counted since the last arm and no further; prompt tokens
neither stop nor count; a stopped sequence is put back on its stop position by every later launch and its forced count says "everything is
forced".  Every expectation below is written out by hand.  Six planted faults (stop_ref.FAULTS) must each be caught by the case named for it.
CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stop_ref as R  # noqa: E402
from stop_ref import Config, State, Words


def _gen(cfg, prompt, generated, fault=None, capacity=16, steps_over_prompt=False):
    """a generation: the prompt at slots 0.., then `generated` placed one per step; returns (states per step, words, state)"""
    hist = list(prompt) + [0] * (capacity - len(prompt))
    st = State()
    if steps_over_prompt:  # single-token steps through the prompt: the launches at forced positions run too
        w = Words(pos=0, history=hist, n_forced=len(prompt), token=0)
        toks = [99] * (len(prompt) - 1) + list(generated)
    else:  # a prompt forward: the first launch sees the first generated token
        w = Words(pos=len(prompt) - 1, history=hist, n_forced=len(prompt), token=0)
        toks = list(generated)
    return R.run(cfg, st, w, toks, fault=fault), w, st


def case_stop_id_beats_eos(fault=None):
    states, _, _ = _gen(Config(stop_ids=(7,), eos=7, max_tokens=1, sequences=((7,),)), [1, 2], [7], fault)
    return states[-1]


def case_eos_beats_budget(fault=None):
    states, _, _ = _gen(Config(eos=5, max_tokens=1, sequences=((5,),)), [1, 2], [5], fault)
    return states[-1]


def case_budget_beats_sequence(fault=None):
    states, _, _ = _gen(Config(max_tokens=2, sequences=((4, 5),)), [1, 2], [4, 5], fault)
    return states[-1]


def case_lowest_stop_id_index(fault=None):
    states, _, _ = _gen(Config(stop_ids=(9, 4, 4)), [1, 2], [3, 4], fault)
    return states[-1]


def case_lowest_sequence_index_not_longest(fault=None):
    states, _, _ = _gen(Config(sequences=((3, 4), (4,), (2, 3, 4))), [1], [2, 3, 4], fault)
    return states[-1]


def case_budget_of_one(fault=None):
    states, _, _ = _gen(Config(max_tokens=1), [1, 2, 3], [8, 9], fault)
    return states


def case_budget_of_three(fault=None):
    states, _, _ = _gen(Config(max_tokens=3), [1, 2], [5, 6, 7, 8], fault)
    return [s[0] for s in states], states[-1][4]


def case_sequence_as_long_as_the_window(fault=None):
    states, _, _ = _gen(Config(sequences=((3, 4, 5),)), [1, 2], [3, 4, 5], fault)
    return states[-1]


def case_sequence_one_longer_than_the_window(fault=None):
    states, _, _ = _gen(Config(sequences=((2, 3, 4, 5),)), [1, 2], [3, 4, 5], fault)
    return states[-1]


def case_sequence_across_an_arm(fault=None):
    cfg = Config(sequences=((3, 4),))
    hist = [1, 2] + [0] * 8
    w, st = Words(pos=1, history=hist, n_forced=2, token=0), State()
    R.run(cfg, st, w, [3], fault=fault)
    st.arm(keep_generated=True)
    return R.run(cfg, st, w, [4], fault=fault)[-1]


def case_prompt_tokens_neither_stop_nor_count(fault=None):
    # the prompt holds the stop id and would fill the budget; three steps run over it before the first token is generated
    states, _, _ = _gen(Config(stop_ids=(2,), max_tokens=3), [1, 2, 2, 3], [5, 6, 7], fault, steps_over_prompt=True)
    return states


def case_frozen_steps_restore_the_position(fault=None):
    states, w, st = _gen(Config(eos=6), [1, 2], [5, 6, 7, 7, 7], fault)
    return states[-1], w.pos, w.token, w.history[:6]


def case_stop_raises_the_forced_count(fault=None):
    states, w, st = _gen(Config(eos=6), [1, 2], [5, 6, 7, 8], fault)
    return w.n_forced, w.history[:6]


CASES = {
    case_stop_id_beats_eos: (R.TOKEN, 0, 7, 2, 1, 0),
    case_eos_beats_budget: (R.EOS, 0, 5, 2, 1, 0),
    case_budget_beats_sequence: (R.MAX_TOKENS, 0, 5, 3, 2, 0),
    case_lowest_stop_id_index: (R.TOKEN, 1, 4, 3, 2, 0),
    case_lowest_sequence_index_not_longest: (R.SEQUENCE, 0, 4, 3, 3, 0),
    case_budget_of_one: [(R.MAX_TOKENS, 0, 8, 3, 1, 0), (R.MAX_TOKENS, 0, 8, 3, 1, 1)],
    case_budget_of_three: ([R.NONE, R.NONE, R.MAX_TOKENS, R.MAX_TOKENS], 3),
    case_sequence_as_long_as_the_window: (R.SEQUENCE, 0, 5, 4, 3, 0),
    case_sequence_one_longer_than_the_window: (R.NONE, 0, 0, 0, 3, 0),
    case_sequence_across_an_arm: (R.NONE, 0, 0, 0, 2, 0),
    case_prompt_tokens_neither_stop_nor_count: [(R.NONE, 0, 0, 0, 0, 0)] * 3 + [(R.NONE, 0, 0, 0, 1, 0), (R.NONE, 0, 0, 0, 2, 0), (R.MAX_TOKENS, 0, 7, 6, 3, 0)],
    case_frozen_steps_restore_the_position: ((R.EOS, 0, 6, 3, 2, 3), 3, 6, [1, 2, 5, 6, 0, 0]),
    case_stop_raises_the_forced_count: (0x7FFFFFFF, [1, 2, 5, 6, 0, 0]),
}

# the case that must catch each planted fault
CATCHES = {
    "match_into_prompt": case_sequence_one_longer_than_the_window,
    "longest_sequence": case_lowest_sequence_index_not_longest,
    "budget_off_by_one": case_budget_of_three,
    "forced_counted": case_prompt_tokens_neither_stop_nor_count,
    "position_not_restored": case_frozen_steps_restore_the_position,
    "n_forced_left": case_stop_raises_the_forced_count,
}


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: c.__name__)
def test_restatement_meets_the_contract(case):
    assert case() == CASES[case]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_caught_by_its_named_case(fault):
    case = CATCHES[fault]
    assert case(fault) != CASES[case], f"{case.__name__} does not notice {fault}"


def test_every_fault_has_a_case():
    assert set(CATCHES) == set(R.FAULTS) and len(R.FAULTS) == 6


def test_a_garbage_position_is_a_no_op():
    cfg = Config(stop_ids=(0,), eos=0, max_tokens=1, sequences=((0,),))
    for P in (0, -5, 8, 9):
        w, st = Words(pos=P, history=[0] * 8, n_forced=0, token=3), State()
        before = w.copy()
        R.launch(cfg, st, w)
        assert w == before and st == State(), P


def test_the_empty_config_counts_and_never_stops():
    states, w, st = _gen(Config(), [1], list(range(2, 12)), capacity=16)
    assert [s[0] for s in states] == [R.NONE] * 10 and st.generated == 10 and w.n_forced == 1


def test_first_stop_names_the_step():
    hist = [1, 2, 3, 10, 11, 12, 13, 14]
    assert R.first_stop(Config(stop_ids=(12,)), hist, 3, 5)[0] == 3
    k, st = R.first_stop(Config(sequences=((11, 12, 13),)), hist, 3, 5)
    assert k == 4 and st.public() == (R.SEQUENCE, 0, 13, 6, 4, 0)
    assert R.first_stop(Config(eos=10), hist, 3, 5)[0] == 1
    assert R.first_stop(Config(eos=99), hist, 3, 5)[0] is None
