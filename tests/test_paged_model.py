"""CPU: the Python model of PagedBatch's page bookkeeping (tests/paged_model.py) on hand-worked cases, and the coverage the seeded walk of
tests/test_paged_lifecycle_gpu.py must reach -- both from the model alone, so they hold before anything runs on a GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_model as pm  # noqa: E402


def model(n_pages=12):
    return pm.PagedModel(n_pages, 8, 2, 300)


def test_three_holders_of_one_first_append_page_make_two_copies():
    m = model()
    m.admit(0, 70)  # pages 0, 1
    m.fork(0, 1)
    m.fork(0, 2)
    assert m.in_use == 2 and [p.holders for p in m.seq[0]] == [3, 3]
    assert m.need_step(1) == 2  # every sharer of page 1 but the last
    assert m.step(1) == 2 and m.in_use == 1 + 3
    assert [m.seq[b][0] is m.seq[0][0] for b in (1, 2)] == [True, True] and len({id(m.seq[b][1]) for b in range(3)}) == 3
    assert m.seq[2][1].holders == 1 and m.need_step(1) == 0 and m.step(1) == 0  # the last holder kept the page; nobody shares an append page now
    # two of the three listed for a prefill, the third holds the page too: two copies all the same
    m = model()
    m.admit(0, 70)
    m.fork(0, 1)
    m.fork(0, 2)
    assert m.need_prefill([1, 2], [3, 60]) == 2 + 1  # two copies, and slot 2 reaches page 2
    assert m.prefill([1, 2], [3, 60]) == 2 and m.in_use == 2 + 2 + 1 and m.seq[0][1].holders == 1


def test_a_fork_at_a_multiple_of_64_needs_no_copy():
    for at in (64, 128):
        m = model()
        m.admit(0, at)
        m.fork(0, 1)
        assert m.in_use == at // 64 and m.need_step(1) == 2  # a fresh page each
        assert m.step(1) == 0 and m.in_use == at // 64 + 2
    m = model()
    m.admit(0, 63)
    m.fork(0, 1)
    assert m.need_step(2) == 1 + 2  # one copy of page 0, then a fresh page 1 each
    assert m.step(2) == 1 and m.in_use == 2 + 2


def test_a_step_that_grows_a_table_by_two_pages():
    m = model()
    m.admit(0, 60)
    assert m.need_step(70) == 2 and m.step(70) == 0 and m.in_use == 3 and m.pos[0] == 130


def test_the_run_is_capped_by_the_shortest_member():
    m = model(16)
    m.admit(0, 130)  # pages 0, 1, 2
    m.fork(0, 1)
    m.fork(0, 2)
    assert m.groups(1) == [([0, 1, 2], 2)] and m.groups(2) == [([0, 1, 2], 2)] and m.groups(3) == []
    m2 = model(16)
    m2.admit(0, 70)
    m2.fork(0, 3)
    m2.prefill([0], [60])  # slot 0 goes on to 130 on a private page 1; slot 3 stays at 70
    m2.fork(0, 1)
    m2.fork(0, 2)
    assert m2.groups(1) == [([0, 1, 2, 3], 1)]  # page 0 alone is common, and 70 >> 6 = 1 caps it besides
    assert m2.groups(2) == []  # the whole first-page group is ungrouped, the three with two common pages included
    m2.set_share(1)
    m2.step(1)
    assert m2.shared_rows == 4 * 2
    m2.set_share(2)
    m2.step(1)
    assert m2.shared_rows == 0
    # a member at exactly 128 holds nothing but the run
    m3 = model(16)
    m3.admit(0, 128)
    m3.fork(0, 1)
    m3.set_share(1)
    m3.step(1)
    assert m3.last_groups == [([0, 1], 2)] and m3.in_use == 4
    # below one page nothing is shared: the only common page takes the appends
    m4 = model()
    m4.admit(0, 30)
    m4.fork(0, 1)
    m4.set_share(1)
    m4.step(1)
    assert m4.shared_rows == 0 and m4.in_use == 2


def test_refusals_change_nothing():
    m = model(3)
    m.admit(0, 70)
    m.fork(0, 1)
    m.open(2)
    with pytest.raises(pm.Refused, match="too few free pages for this prefill"):
        m.prefill([2], [130])
    with pytest.raises(pm.Refused, match="listed twice"):
        m.prefill([0, 0], [1, 1])
    with pytest.raises(pm.Refused, match="taken"):
        m.open(1)
    with pytest.raises(pm.Refused, match="empty"):
        m.release(5)
    m.release(2)
    assert m.need_step(60) == 1 + 2 > m.free  # a copy of page 1, and page 2 for both
    with pytest.raises(pm.Refused, match="too few free pages for"):
        m.step(60)
    assert m.in_use == 2 and m.pos == {0: 70, 1: 70} and m.copies == 0
    m.release(0)
    m.release(1)
    assert m.in_use == 0
    with pytest.raises(pm.Refused, match="no member to step"):
        m.step(1)
    m = model(8)
    m.admit(0, 130)
    with pytest.raises(pm.Refused, match="KV cache overflow"):
        m.step(170)
    assert m.step(169) == 0 and m.pos[0] == 299


@pytest.mark.parametrize("seed", pm.SEEDS)
def test_need_is_what_the_reservations_take(seed):
    """the counting rule of the two comments against the reservations themselves, along the walks: replayed on a pool with pages to spare, every
    advance takes exactly the pages counted before it"""
    ops, _ = pm.walk(seed)
    big = pm.PagedModel(64, pm.WALK["n_slots"], pm.WALK["n_layers"], pm.WALK["max_pos"])
    for e in ops:
        if e["op"] == "open":
            big.open(e["slot"])
        elif e["op"] == "fork":
            big.fork(e["src"], e["slot"])
        elif e["op"] == "release":
            big.release(e["slot"])
        elif e["op"] == "prefill" and not e["refused"]:
            need, had = big.need_prefill(e["slots"], e["n"]), big.in_use
            big.prefill(e["slots"], e["n"])
            assert big.in_use - had == need, e
        elif e["op"] == "step" and not e["refused"]:
            need, had = big.need_step(e["n"]), big.in_use
            big.step(e["n"])
            assert big.in_use - had == need, e


def test_the_walks_are_a_pure_function_of_the_seed_and_cover_what_they_must():
    total = {}
    for seed in pm.SEEDS:
        ops, stats = pm.walk(seed)
        again, _ = pm.walk(seed)
        assert ops == again
        assert sum(e["op"] == "checkpoint" for e in ops) == 2 and ops[-1]["op"] == "checkpoint"
        assert all(0 <= e["in_use"] <= pm.WALK["n_pages"] for e in ops if "in_use" in e)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + int(v)
    print("walk coverage over seeds", pm.SEEDS, total)
    assert total["copies"] >= 3
    assert total["refusals"] >= 2
    assert total["slot_reuses"] >= 2
    assert total["hole_steps"] >= 2
    assert total["wide_group_steps"] >= 1
    assert total["two_page_growths"] >= 1
