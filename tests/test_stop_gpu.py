"""GPU, no model: bitnet_hip_stop_dev / bitnet_hip_stop_batch_dev (csrc/kernels_stop.hip) on hand-made position, history, forced-count and token
words against tests/stop_ref.py, launch by launch.  Every comparison is on integers: after each launch the position, the token word, the
whole history, the forced count, the six state words and the guard words around all of them must be the restatement's.  tests/test_stop_ref.py
holds the restatement to the contract."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stop_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

G = 4
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


class Lane:
    """one Stop object with the device words a launch takes -- token, position, forced count, history[capacity] -- in one int32 arena, each
    between guard words, and the restatement's copy of the same words"""

    def __init__(self, torch, pkg, hip, cfg: R.Config, history, pos, n_forced, capacity=None, token=-1):
        self.torch = torch
        self.cfg = cfg
        self.cap = len(history) if capacity is None else capacity
        self.stop = pkg.Stop(hip, **cfg.kwargs())
        n = len(history)
        # G guards | token | G | position | G | forced count | G | history[n] | G
        self.o_tok, self.o_pos, self.o_nf, self.o_hist = G, 2 * G + 1, 3 * G + 2, 4 * G + 3
        self.arena = torch.full((self.o_hist + n + G,), GUARD, dtype=torch.int32, device="cuda")
        self.tok, self.pos, self.nf = (self.arena[o:o + 1] for o in (self.o_tok, self.o_pos, self.o_nf))
        self.hist = self.arena[self.o_hist:self.o_hist + n]
        self.w = R.Words(pos=pos, history=list(history), n_forced=n_forced, token=token)
        self.st = R.State()
        self.upload()

    def upload(self):
        host = np.full(self.arena.numel(), GUARD, np.int32)
        host[self.o_tok], host[self.o_pos], host[self.o_nf] = self.w.token, self.w.pos, self.w.n_forced
        host[self.o_hist:self.o_hist + len(self.w.history)] = self.w.history
        self.arena.copy_(self.torch.from_numpy(host))

    def expected(self):
        host = np.full(self.arena.numel(), GUARD, np.int64)
        host[self.o_tok], host[self.o_pos], host[self.o_nf] = self.w.token, self.w.pos, self.w.n_forced
        host[self.o_hist:self.o_hist + len(self.w.history)] = self.w.history
        return host.astype(np.int32)

    def launch_alone(self):
        self.stop.launch(self.pos, self.hist, self.cap, self.nf, self.tok)

    def bind(self, table, slot):
        table.set(slot, self.stop, self.pos, self.hist, self.cap, self.nf, self.tok)

    def ref_launch(self):
        R.launch(self.cfg, self.st, self.w, capacity=self.cap)

    def check(self, what=""):
        self.torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        want = self.expected()
        assert np.array_equal(got, want), (what, np.nonzero(got != want)[0].tolist(), got.tolist(), want.tolist())
        assert self.stop.state().astuple() == self.st.public(), (what, self.stop.state(), self.st)

    def step(self, token, what=""):
        """the pick in front of the launch, applied to both sides (a host write stands in for the pick kernel), then one launch"""
        R.pick(self.w, token)
        self.upload()
        self.launch_alone()
        self.ref_launch()
        self.check(what)

    def arm(self, keep_generated=False):
        self.stop.arm(keep_generated)
        self.st.arm(keep_generated)

    def close(self):
        self.stop.close()


def run_case(torch, pkg, hip, cfg, prompt, generated, capacity=None, steps_over_prompt=False):
    capacity = capacity or len(prompt) + len(generated) + 2
    hist = list(prompt) + [0] * (capacity - len(prompt))
    lane = Lane(torch, pkg, hip, cfg, hist, 0 if steps_over_prompt else len(prompt) - 1, len(prompt))
    toks = ([99] * (len(prompt) - 1) if steps_over_prompt else []) + list(generated)
    for i, t in enumerate(toks):
        lane.step(t, f"step {i}")
    st = lane.st.public()
    lane.close()
    return st


def test_smallest_and_largest_valid_position(torch_, pkg, hip):
    # P = 1: one prompt token, the first generated token is EOS
    assert run_case(torch_, pkg, hip, R.Config(eos=9), [3], [9], capacity=4) == (R.EOS, 0, 9, 1, 1, 0)
    # P = capacity - 1: the last history slot
    assert run_case(torch_, pkg, hip, R.Config(sequences=((7, 8),)), [3], [5, 6, 7, 8], capacity=5) == (R.SEQUENCE, 0, 8, 4, 4, 0)


@pytest.mark.parametrize("P", [8, -5, 0, 0x7FFFFFFF, -0x80000000])
def test_a_garbage_position_is_a_no_op(torch_, pkg, hip, P):
    cfg = R.Config(stop_ids=(0, 4), eos=4, max_tokens=1, sequences=((4,), (0,)))
    lane = Lane(torch_, pkg, hip, cfg, [4] * 8, P, 0, token=77)
    lane.launch_alone()
    lane.ref_launch()
    assert lane.st == R.State() and lane.w.pos == P  # the restatement left everything alone ...
    lane.check(f"P = {P}")  # ... and so did the device: every word, every guard, the state
    lane.close()


def test_sequences_of_length_1_and_32(torch_, pkg, hip):
    assert run_case(torch_, pkg, hip, R.Config(sequences=((6,),)), [1, 2], [5, 6]) == (R.SEQUENCE, 0, 6, 3, 2, 0)
    long = tuple(range(100, 132))
    # 31 of the 32 tokens, then a break, then all 32: only the full run stops; and 32 tokens behind a 1-token window do not
    gen = list(long[:31]) + [7] + list(long)
    assert run_case(torch_, pkg, hip, R.Config(sequences=(long,)), [1, 2], gen) == (R.SEQUENCE, 0, 131, 65, 64, 0)
    assert run_case(torch_, pkg, hip, R.Config(sequences=(long,)), [1] + list(long[:31]), [131, 5])[0] == R.NONE
    # a mismatch in each quarter of the 32 (lanes 4 s + q compare 8 tokens each)
    for j in (0, 9, 18, 31):
        seq = list(long)
        seq[j] += 1
        assert run_case(torch_, pkg, hip, R.Config(sequences=(tuple(seq),)), [1, 2], list(long))[0] == R.NONE, j


def test_sixteen_sequences_all_matching_report_the_lowest(torch_, pkg, hip):
    seqs = tuple(tuple(range(50 - L, 50)) for L in range(16, 0, -1))  # every one a suffix of ..., 48, 49; the longest first
    assert run_case(torch_, pkg, hip, R.Config(sequences=seqs), [1], list(range(30, 50)))[:2] == (R.SEQUENCE, 0)
    # the same with the longest LAST: still index 0, which is now the shortest
    st = run_case(torch_, pkg, hip, R.Config(sequences=seqs[::-1]), [1], list(range(30, 50)))
    assert st[:2] == (R.SEQUENCE, 0) and st[2] == 49
    # only sequence 15 matches
    only = tuple((900 + s,) for s in range(15)) + ((48, 49),)
    assert run_case(torch_, pkg, hip, R.Config(sequences=only), [1], [47, 48, 49])[:2] == (R.SEQUENCE, 15)


def test_thirty_two_stop_ids_match_in_the_last(torch_, pkg, hip):
    ids = tuple(range(200, 232))
    assert run_case(torch_, pkg, hip, R.Config(stop_ids=ids), [1, 2], [5, 231]) == (R.TOKEN, 31, 231, 3, 2, 0)
    assert run_case(torch_, pkg, hip, R.Config(stop_ids=ids + ()), [1, 2], [5, 200])[:2] == (R.TOKEN, 0)
    assert run_case(torch_, pkg, hip, R.Config(stop_ids=(8, 7, 7, 7)), [1, 2], [7])[:2] == (R.TOKEN, 1)


def test_priority_order(torch_, pkg, hip):
    assert run_case(torch_, pkg, hip, R.Config(stop_ids=(3, 7), eos=7, max_tokens=1, sequences=((7,),)), [1, 2], [7])[:2] == (R.TOKEN, 1)
    assert run_case(torch_, pkg, hip, R.Config(eos=5, max_tokens=1, sequences=((5,),)), [1, 2], [5])[0] == R.EOS
    assert run_case(torch_, pkg, hip, R.Config(max_tokens=2, sequences=((4, 5),)), [1, 2], [4, 5])[0] == R.MAX_TOKENS
    assert run_case(torch_, pkg, hip, R.Config(max_tokens=3, sequences=((4, 5),)), [1, 2], [4, 5])[0] == R.SEQUENCE
    assert run_case(torch_, pkg, hip, R.Config(max_tokens=1), [1, 2, 3], [8]) == (R.MAX_TOKENS, 0, 8, 3, 1, 0)


def test_a_match_straddling_the_forced_count_is_none(torch_, pkg, hip):
    assert run_case(torch_, pkg, hip, R.Config(sequences=((2, 3, 4),)), [1, 2], [3, 4])[0] == R.NONE
    # single-token steps over the prompt: the launches at forced positions run, see the stop id and the sequence there, and pass
    st = run_case(torch_, pkg, hip, R.Config(stop_ids=(2,), max_tokens=3, sequences=((1, 2),)), [1, 2, 2, 3], [5, 6, 7], steps_over_prompt=True)
    assert st == (R.MAX_TOKENS, 0, 7, 6, 3, 0)


def test_a_match_straddling_an_arm_is_none(torch_, pkg, hip):
    lane = Lane(torch_, pkg, hip, R.Config(sequences=((3, 4),), max_tokens=5), [1, 2] + [0] * 8, 1, 2)
    lane.step(3)
    lane.arm(keep_generated=True)
    lane.check("armed")
    lane.step(4, "behind the arm")
    assert lane.st.public() == (R.NONE, 0, 0, 0, 2, 0)
    lane.step(3)
    lane.step(4, "inside the new window")
    assert lane.st.public() == (R.SEQUENCE, 0, 4, 5, 4, 0)
    lane.close()
    lane = Lane(torch_, pkg, hip, R.Config(sequences=((3, 4),), max_tokens=3), [1, 2] + [0] * 8, 1, 2)
    lane.step(3)
    lane.arm(keep_generated=True)
    lane.step(4)
    lane.step(3, "the kept count reaches the budget")
    assert lane.st.public() == (R.MAX_TOKENS, 0, 3, 4, 3, 0)
    lane.arm(keep_generated=False)
    lane.check("armed, count dropped")
    assert lane.st.public() == (R.NONE, 0, 0, 0, 0, 0)
    lane.close()


def test_the_empty_config_counts_and_never_stops(torch_, pkg, hip):
    assert run_case(torch_, pkg, hip, R.Config(), [0], [0] * 12) == (R.NONE, 0, 0, 0, 12, 0)


def test_configure_is_followed_without_a_new_object(torch_, pkg, hip):
    lane = Lane(torch_, pkg, hip, R.Config(), [1, 2] + [0] * 6, 1, 2)
    lane.step(5)
    lane.cfg = R.Config(eos=6)
    lane.stop.configure(**lane.cfg.kwargs())
    lane.step(6)
    assert lane.st.public() == (R.EOS, 0, 6, 3, 2, 0)  # the count went on: configure leaves the state alone
    lane.close()


def test_frozen_launches_hold_the_sequence(torch_, pkg, hip):
    lane = Lane(torch_, pkg, hip, R.Config(eos=6), [1, 2] + [0] * 10, 1, 2)
    lane.step(5)
    lane.step(6)
    assert lane.st.reason == R.EOS and lane.w.n_forced == R.FROZEN_FORCED
    held = list(lane.w.history)
    for i in range(5):  # each preceded by *pos += 1, as the pick does at a forced position
        lane.step(40 + i, f"frozen {i}")
        assert lane.w.pos == 3 and lane.w.token == 6 and lane.w.history == held
    assert lane.st.public() == (R.EOS, 0, 6, 3, 2, 5)
    lane.close()


def test_null_token_pointer(torch_, pkg, hip):
    lane = Lane(torch_, pkg, hip, R.Config(eos=6), [1, 2] + [0] * 4, 1, 2, token=-3)
    lane.w.token = None
    for t in (5, 6, 7, 8):
        R.pick(lane.w, t)
        lane.w.token = -3
        lane.upload()
        lane.w.token = None
        lane.stop.launch(lane.pos, lane.hist, lane.cap, lane.nf, None)
        lane.ref_launch()
        lane.w.token = -3
        lane.check(f"token {t}")
        lane.w.token = None
    assert lane.st.public() == (R.EOS, 0, 6, 3, 2, 2)
    lane.close()


def test_batched_form_leaves_the_single_form_s_bits(torch_, pkg, hip):
    """slots 1, 8 and 64 of a 64-slot table (indices 0, 7, 63), idle slots between them, against twins that go through bitnet_hip_stop_dev"""
    specs = [(R.Config(eos=6), [1, 2], [5, 6, 7, 7, 7, 7]), (R.Config(sequences=((7, 8),), stop_ids=(3,)), [1], [9, 7, 8, 2, 2, 2]),
             (R.Config(max_tokens=5), [1, 2, 3], [4, 4, 4, 4, 4, 4])]
    mk = lambda c, p: Lane(torch_, pkg, hip, c, list(p) + [0] * 10, len(p) - 1, len(p))
    lanes, twins = [mk(c, p) for c, p, _ in specs], [mk(c, p) for c, p, _ in specs]
    table = pkg.StopBatch(hip, 64)
    assert table.live() == 0
    for slot, lane in zip((0, 7, 63), lanes):
        lane.bind(table, slot)
    assert table.live() == 3
    lives = []
    for i in range(6):
        for lane, twin, (_, _, gen) in zip(lanes, twins, specs):
            for x in (lane, twin):
                R.pick(x.w, gen[i])
                x.upload()
            twin.launch_alone()
        table.launch()
        for lane, twin in zip(lanes, twins):
            lane.ref_launch()
            twin.ref_launch()
            lane.check(f"table, step {i}")
            twin.check(f"alone, step {i}")
            assert np.array_equal(lane.arena.cpu().numpy(), twin.arena.cpu().numpy())
            assert lane.stop.state().astuple() == twin.stop.state().astuple()
        lives.append(table.live())
    # stops: lane 0 at step 1 (EOS), lane 1 at step 2 (sequence), lane 2 at step 4 (budget of 5)
    assert lives == [3, 2, 1, 1, 0, 0]
    assert [l.st.public() for l in lanes] == [(R.EOS, 0, 6, 3, 2, 4), (R.SEQUENCE, 0, 8, 3, 3, 3), (R.MAX_TOKENS, 0, 4, 7, 5, 1)]
    # arm recounts; an emptied slot is idle and leaves its words alone
    lanes[0].arm()
    assert table.live() == 1
    table.set(0, None)
    assert table.live() == 0
    before = lanes[0].arena.cpu().numpy().copy()
    table.launch()
    torch_.cuda.synchronize()
    assert np.array_equal(lanes[0].arena.cpu().numpy(), before)
    # refusals that need live objects: a slot beyond the table, an object bound to two slots
    small = pkg.StopBatch(hip, 4)
    with pytest.raises(pkg.BitNetHipError, match="slot 4 out of range") as e:
        lanes[0].bind(small, 4)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.BitNetHipError, match="already bound to slot 7"):
        lanes[1].bind(table, 9)
    with pytest.raises(pkg.BitNetHipError, match="already bound to slot 7 of another table"):
        lanes[1].bind(small, 1)
    lanes[1].bind(table, 7)  # the same slot again is a re-bind
    small.close()
    table.close()
    for x in lanes + twins:
        x.close()


def random_case(rng):
    """one history of the sweep: a config and a generation over a 4-letter alphabet, so stop ids and sequences match often"""
    n_prompt = int(rng.integers(1, 5))
    n_gen = int(rng.integers(1, 14))
    cfg = R.Config(
        stop_ids=tuple(int(t) for t in rng.integers(0, 6, int(rng.integers(0, 3)))) if rng.random() < 0.4 else (),
        eos=int(rng.integers(0, 6)) if rng.random() < 0.3 else None,
        max_tokens=int(rng.integers(1, 12)) if rng.random() < 0.4 else 0,
        sequences=tuple(tuple(int(t) for t in rng.integers(0, 4, int(rng.integers(1, 5)))) for _ in range(int(rng.integers(0, 5)))),
    )
    prompt = [int(t) for t in rng.integers(0, 4, n_prompt)]
    gen = [int(t) for t in rng.integers(0, 4, n_gen)]
    return cfg, prompt, gen, bool(rng.random() < 0.3), int(rng.integers(0, n_gen + 1))


def sweep(torch, pkg, hip, n, seed=2024):
    """n random histories, launch by launch; returns how many ended on each reason"""
    rng = np.random.default_rng(seed)
    reasons = [0] * 5
    for c in range(n):
        cfg, prompt, gen, over_prompt, arm_at = random_case(rng)
        cap = len(prompt) + len(gen) + int(rng.integers(0, 3))  # the last step may sit at capacity - 1, or at capacity itself (a no-op)
        cap = max(cap, len(prompt) + 1)
        hist = list(prompt) + [0] * (len(prompt) + len(gen) + 2 - len(prompt))
        lane = Lane(torch, pkg, hip, cfg, hist, 0 if over_prompt else len(prompt) - 1, len(prompt), capacity=cap)
        toks = ([9] * (len(prompt) - 1) if over_prompt else []) + gen
        for i, t in enumerate(toks):
            if i == arm_at and lane.st.reason == R.NONE:
                lane.arm(keep_generated=bool(i & 1))
            lane.step(t, f"case {c}, step {i}: {cfg}, prompt {prompt}, generated {gen}")
        reasons[lane.st.reason] += 1
        lane.close()
    return reasons


def test_random_sweep(torch_, pkg, hip):
    reasons = sweep(torch_, pkg, hip, 300)
    assert sum(reasons) == 300 and all(r >= 15 for r in reasons), reasons  # every reason, and running on, occurs often
