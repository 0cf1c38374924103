"""GPU: the lifecycle of a PagedBatch (host/paged_batch.hpp) -- which page is whose, which table row the device sees, which dense row is which
slot, when a page is copied, who forms a share group -- on model A of tests/test_decoder_state_gpu.py (qk256; 5 table entries per member), pools
of 8 to 16 pages, 8 slots.  Every batch runs beside the Python model of the bookkeeping (tests/paged_model.py), which says before each call
whether it fits, how many pages are in use afterwards and how many rows a step sends through the shared pass.

Reference: for each member the float64 whole-prompt forward (tests/model_ref.py) over the member's OWN history, whatever the device picked: the
pages must hold the K / V of those tokens, so a near-tie cannot fail a test.  Gates, all the project's own:
  G1  extract() into a scratch decoder, then check_values of tests/test_decoder_state_gpu.py over every position below the member's, every layer:
      rel <= 4 u_l (+ 2^-11 on f16 pools), u_l = mr.yardstick over the member's own tokens.  KVTABLE paths paged-step / paged-churn / paged-share.
  G2  last_logits cosine >= 0.9999 against the float64 logits row (members whose last call computed logits).
  G3  pages_in_use / pages_free / shared_rows == the model's, exactly.
Equalities without a tolerance:
  B1  a member's extracted rows below its position keep their bits across any operation on other members.
  B2  forks' extracted rows below the fork point are each other's, bit for bit.
  B3  a refused call leaves counts, positions, histories and every member's extracted bits as they were.

Scenes: (a) a pool and slots that held other sequences, against a fresh twin bit for bit; (b) occupied slots 1, 4, 6, 7 against 0..3 bit for bit;
(c) forks at 64 / 128 / 63, a step(70) that grows a table by two pages and ends at max_pos - 1, the overflow refusal; (d) a fork of a fork, the
original released, its slot reused, prefill behind step; (e) share groups capped by the shortest member, dropped by min_pages, a member with
every page in the run, holes in the slots; (f) a step / prefill that needs exactly the free pages, and one page more; the other refusals.
Then a seeded walk of about 40 operations drawn from the model (paged_model.walk), three seeds.  Observed on an MI355X: EXPERIMENTS.md 48."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402
import model_ref as mr  # noqa: E402
import paged_model as pm  # noqa: E402
from test_decoder_state_gpu import check_values, cosine, snapshot, worlds  # noqa: E402,F401

pytestmark = pytest.mark.gpu

N_SLOTS = 8
KV = pytest.mark.parametrize("kv16", (False, True), ids=("kv32", "kv16"))
WORST = {"cosine": 1.0}


@pytest.fixture(scope="module", autouse=True)
def worst_cosine():
    yield
    print(f"\npaged lifecycle: worst last_logits cosine against float64 {WORST['cosine']:.6f}")


def stream(W, k, n):
    """token stream k: the prompt shifted per stream"""
    return ((W.prompt[:n].astype(np.int64) + 37 * k + 1) % W.cfg.vocab).astype(np.int32)


def reference(W, tokens):
    """-> (the float64 forward over `tokens`, u_l per layer); computed once per token sequence, never changed"""
    memo = W.__dict__.setdefault("_lifecycle_refs", {})
    key = tuple(int(t) for t in tokens)
    if key not in memo:
        ref = W.forward(list(key))
        memo[key] = (ref, mr.yardstick(ref, W.forward(list(key), rnd=mr.f16)))
    return memo[key]


def same_rows(a, b, n=None):
    """two extracted snapshots ([(k, v)] per layer, already cut to their rows): the same bits below n"""
    return all(np.array_equal(x[:n], y[:n]) for la, lb in zip(a, b) for x, y in zip(la, lb))


class Scene:
    """a PagedBatch beside its model: every call goes to both, and G3 follows every call"""

    def __init__(self, pkg, W, kv16, owner, n_pages, path):
        self.pkg, self.W, self.kv16, self.owner, self.path = pkg, W, kv16, owner, path
        self.batch = pkg.HostPagedBatch(owner, n_pages, N_SLOTS)
        self.model = pm.PagedModel(n_pages, N_SLOTS, W.cfg.n_layers, W.cfg.max_pos)
        self.members, self.logits, self.forced, self.stages = {}, {}, {}, {}
        self.dst = self.shared()

    def shared(self):
        d = self.owner.shared()
        d.set_kv_f16(self.kv16)
        return d

    def close(self):
        for d in list(self.members.values()) + [self.batch, self.dst] + list(self.stages.values()):
            d.close()

    # ---- G3 ----
    def counts(self, what=""):
        got = (self.batch.pages_in_use(), self.batch.pages_free())
        assert got == (self.model.in_use, self.model.free), (what, "pages in use / free", got, "the model", (self.model.in_use, self.model.free))
        for b, m in self.members.items():
            assert m.position() == self.model.pos[b], (what, "position of slot", b)

    # ---- the calls ----
    def _seat(self, slot, fed, forced):
        m = self.members[slot] = self.batch.member(slot)
        self.logits[slot], self.forced[slot] = False, forced
        self.feed(slot, fed)
        return m

    def feed(self, slot, toks):
        """Decoder::feed appends behind max(position, tokens fed so far); the count is kept here as the decoder keeps it"""
        if len(toks):
            self.members[slot].feed(toks)
            self.forced[slot] = max(self.model.pos[slot], self.forced[slot]) + len(toks)

    def ensure_fed(self, slot, n, k):
        """feed from stream k what a prefill of n tokens still lacks"""
        have = max(0, self.forced[slot] - self.model.pos[slot])
        self.feed(slot, stream(self.W, k, max(0, n - have)))

    def open(self, slot, fed=()):
        self.model.open(slot)
        self.batch.open(slot)
        self.counts(f"open({slot})")
        return self._seat(slot, fed, 0)

    def admit(self, slot, k, n):
        """the first n tokens of stream k from a staging decoder; the stream's next token is fed behind them"""
        if (k, n) not in self.stages:
            s = self.stages[(k, n)] = self.shared()
            s.feed(stream(self.W, k, n))
            s.prefill(n, with_logits=False, digits=2)
        self.model.admit(slot, n)
        self.batch.admit(slot, self.stages[(k, n)], n)
        self.counts(f"admit({slot}, {n})")
        return self._seat(slot, stream(self.W, k, n + 1)[n:], n)

    def fork(self, src, slot, fed=()):
        self.model.fork(src, slot)
        self.batch.fork(src, slot)
        self.counts(f"fork({src}, {slot})")
        return self._seat(slot, fed, min(self.forced[src], self.model.pos[src]))

    def release(self, slot):
        self.model.release(slot)
        self.batch.release(slot)
        self.members.pop(slot).close()
        self.counts(f"release({slot})")

    def prefill(self, slots, n, fed=None):
        """fed: per listed member the tokens to feed first"""
        for b, t in zip(slots, fed or ()):
            self.feed(b, t)
        copies = self.model.prefill(slots, n)
        self.batch.prefill(slots, n)
        for b in slots:
            self.logits[b] = True
        self.counts(f"prefill({slots}, {n})")
        return copies

    def step(self, n):
        copies = self.model.step(n)
        self.batch.step(n, 2)
        for b in self.members:
            self.logits[b] = True
        self.counts(f"step({n})")
        got = self.batch.shared_rows()
        assert got == self.model.shared_rows, (f"step({n})", "shared_rows", got, "the model", self.model.shared_rows, self.model.last_groups)
        return copies

    def set_share(self, v):
        self.model.set_share(v)
        self.batch.set_share(v)

    # ---- what a member holds ----
    def tokens(self, slot):
        m = self.members[slot]
        return m.history(m.position() + 1).copy()

    def rows(self, slot):
        """the extracted caches below the member's position, as bits: [(k, v)] per layer"""
        p = self.members[slot].position()
        if p == 0:
            return []
        self.batch.extract(slot, self.dst)
        assert self.dst.position() == p
        return [(kv.bits(k[:p]).copy(), kv.bits(v[:p]).copy()) for k, v in snapshot(self.dst, self.W, self.kv16)]

    def state(self):
        return {"counts": (self.batch.pages_in_use(), self.batch.pages_free()), **{b: (self.tokens(b), self.rows(b)) for b in sorted(self.members)}}

    def same_state(self, before, what, only=None):
        """B3 (all members) / B1 (only: the members that must not have changed)"""
        now = self.state()
        if only is None:
            assert now["counts"] == before["counts"] and set(now) == set(before), (what, "counts / members changed")
        for b in (sorted(self.members) if only is None else only):
            assert np.array_equal(now[b][0], before[b][0]), (what, "position / history of slot", b)
            assert len(now[b][1]) == len(before[b][1]) and same_rows(now[b][1], before[b][1]), (what, "extracted rows of slot", b)

    def refused(self, call, text, what):
        """B3 around a call that must be refused with `text`"""
        before = self.state()
        with pytest.raises(self.pkg.BitNetHipError, match=text):
            call()
        self.same_state(before, what + ": refused, yet something changed")
        self.counts(what)

    def keeps(self, others, call, what):
        """B1: `call` works on other members; `others` keep position, history and extracted bits"""
        before = {b: (self.tokens(b), self.rows(b)) for b in others}
        out = call()
        self.same_state(before, what, only=others)
        return out

    # ---- G1, G2 ----
    def check(self, slot, what):
        m, W = self.members[slot], self.W
        p = m.position()
        if p == 0:
            return
        toks = self.tokens(slot)
        ref, u = reference(W, toks[:p])
        self.batch.extract(slot, self.dst)
        assert self.dst.position() == p and np.array_equal(self.dst.history(p + 1), toks), (what, slot)
        check_values(W, snapshot(self.dst, W, self.kv16), ref, u, self.kv16, slice(0, p), self.path, f"{what}, slot {slot} at {p}")
        if self.logits[slot]:
            c = cosine(m.last_logits(), ref.logits[p - 1])
            WORST["cosine"] = min(WORST["cosine"], c)
            print(f"{self.path} kv16={self.kv16} {what} slot {slot} at {p}: last logits cosine against float64 {c:.6f}")
            assert c >= 0.9999, (what, slot, c)

    def check_all(self, what):
        for b in sorted(self.members):
            self.check(b, what)

    def outcome(self, order):
        """what a twin run must repeat bit for bit: per member (in `order`) tokens, last_logits bits, extracted bits"""
        return [(self.tokens(b), self.members[b].last_logits().view(np.uint32).copy(), self.rows(b)) for b in order]


def same_outcome(a, b, what):
    assert len(a) == len(b)
    for i, ((ta, la, ra), (tb, lb, rb)) in enumerate(zip(a, b)):
        assert np.array_equal(ta, tb), (what, "tokens of dense row", i)
        assert np.array_equal(la, lb), (what, "last_logits bits of dense row", i)
        assert len(ra) == len(rb) and same_rows(ra, rb), (what, "extracted rows of dense row", i)


@pytest.fixture
def scenes(pkg, worlds):
    W = worlds("A", "qk256")
    made = []

    def make(kv16, n_pages, path):
        owner = made[0].owner if made else W.decoder(pkg, kv16)  # (one cache type per test)
        made.append(Scene(pkg, W, kv16, owner, n_pages, path))
        return made[-1]

    yield W, make
    for s in reversed(made):
        s.close()
    if made:
        made[0].owner.close()


def little_scene(S, slots, what):
    """the scene of (a) and (b) in `slots` = (s0, s1, s2, s3): open + prefill(70), admit at 130, open + prefill(21), step(3), a fork of the 130
    member into s3 fed a token of its own, step(2); G1 to G3 at the end"""
    s0, s1, s2, s3 = slots
    W = S.W
    S.open(s0, stream(W, 1, 71))
    S.prefill([s0], [70])
    S.admit(s1, 2, 130)
    S.open(s2, stream(W, 3, 22))
    S.prefill([s2], [21])
    S.step(3)
    S.fork(s1, s3, [7])
    assert S.step(2) == 1  # the fork and its source diverge on page 2: one copy, the last holder keeps the page
    assert not np.array_equal(S.tokens(s1), S.tokens(s3)), "the fork did not diverge"
    S.check_all(what)
    return S.outcome(slots)


# ---- (a) dirty pool, reused slots --------------------------------------------------------------------------------------------------------
@KV
def test_a_recycled_pages_and_table_rows_hold_what_a_fresh_batch_holds(scenes, kv16):
    W, make = scenes
    S = make(kv16, 12, "paged-churn")
    for b in range(4):
        S.open(b, stream(W, 10 + b, 191))
        S.prefill([b], [190])
    assert S.batch.pages_free() == 0  # four members of three pages: the whole pool
    S.step(2)
    for b in range(4):
        S.release(b)
    assert S.batch.pages_in_use() == 0
    dirty = little_scene(S, (0, 1, 2, 3), "on recycled pages and table rows")
    fresh = little_scene(make(kv16, 12, "paged-churn"), (0, 1, 2, 3), "the fresh twin")
    same_outcome(dirty, fresh, "recycled against fresh")


# ---- (b) holes -----------------------------------------------------------------------------------------------------------------------------
@KV
def test_b_holes_in_the_slots_change_nothing(scenes, kv16):
    W, make = scenes
    S = make(kv16, 12, "paged-step")
    for b in (0, 3):  # two others, seated first and gone before the first step
        S.open(b, stream(W, 20 + b, 31))
        S.prefill([b], [30])
    S.open(1, stream(W, 1, 71))
    S.release(0)
    S.release(1)  # (and seated again by the scene: a released slot between occupied ones)
    S.release(3)
    holes = little_scene(S, (1, 4, 6, 7), "slots 1, 4, 6, 7")
    dense = little_scene(make(kv16, 12, "paged-step"), (0, 1, 2, 3), "slots 0 .. 3")
    same_outcome(holes, dense, "slots 1, 4, 6, 7 against slots 0 .. 3")


# ---- (c) boundaries ------------------------------------------------------------------------------------------------------------------------
@KV
def test_c_forks_at_page_boundaries(scenes, kv16):
    W, make = scenes
    S = make(kv16, 16, "paged-step")
    S.admit(0, 1, 64)
    S.fork(0, 1, [7])
    S.admit(2, 2, 128)
    S.fork(2, 3, [11])
    S.admit(4, 3, 63)
    S.fork(4, 5, [13])
    assert S.model.in_use == 1 + 2 + 1  # a fork adds no page
    pairs = [S.rows(b) for b in range(6)]
    assert same_rows(pairs[0], pairs[1]) and same_rows(pairs[2], pairs[3]) and same_rows(pairs[4], pairs[5])  # B2
    assert S.step(1) == 1 and S.model.in_use == 4 + 2 + 2 + 1  # at 64 and at 128: a fresh page each, no copy; at 63: one copy of page 0
    assert S.step(1) == 0 and S.model.in_use == 9 + 2          # the forks at 63 cross into a fresh page 1 each
    S.check_all("forks at 64, 128 and 63, two steps")
    now = [S.rows(b) for b in range(6)]
    for a, b, n in ((0, 1, 64), (2, 3, 128), (4, 5, 63)):
        assert same_rows(now[a], now[b], n) and same_rows(now[a], pairs[a], n), ("below the fork point", a, b)
        assert not np.array_equal(S.tokens(a), S.tokens(b)), "the forks did not diverge"
    S.step(3)
    S.check_all("three steps on")


@KV
def test_c_two_new_table_entries_in_one_step_and_the_last_position(scenes, kv16):
    W, make = scenes
    S = make(kv16, 8, "paged-step")
    S.open(2, stream(W, 1, 61))
    S.prefill([2], [60])
    S.admit(5, 2, 229)
    assert S.model.in_use == 1 + 4
    assert S.step(70) == 0 and S.model.in_use == 3 + 5  # 60 -> 130: pages 1 and 2 in one call; 229 -> 299: page 4
    assert S.members[2].position() == 130 and S.members[5].position() == W.cfg.max_pos - 1
    S.check_all("step(70)")  # G1 over all 130 / 299 rows
    S.refused(lambda: S.batch.step(1, 2), "KV cache overflow", "a step beyond max_pos - 1")
    with pytest.raises(pm.Refused, match="KV cache overflow"):
        S.model.step(1)
    S.release(5)
    S.step(1)
    S.check_all("the other member steps on alone")


# ---- (d) fork tree -------------------------------------------------------------------------------------------------------------------------
@KV
def test_d_fork_of_a_fork_outlives_the_original_whose_slot_is_reused(scenes, kv16):
    W, make = scenes
    S = make(kv16, 16, "paged-churn")
    S.admit(0, 1, 130)
    S.fork(0, 1, [7])
    S.fork(1, 2, [11])
    first = [S.rows(b) for b in range(3)]
    assert same_rows(first[0], first[1]) and same_rows(first[0], first[2])  # B2
    assert S.model.in_use == 3
    S.keeps([1, 2], lambda: S.release(0), "release of the original")
    assert S.model.in_use == 3  # its forks hold every page
    assert S.step(2) == 1 and S.model.in_use == 4  # two holders of page 2: one copy, the last holder keeps the page
    assert not np.array_equal(S.tokens(1), S.tokens(2)), "the forks did not diverge"
    S.keeps([1, 2], lambda: S.fork(2, 0), "fork into the released slot")
    W40 = stream(W, 5, 80)
    S.keeps([1, 2], lambda: S.prefill([0], [40], [W40[:40]]), "the reused slot continues by prefill")  # 132 .. 171: a copy of page 2
    assert S.model.in_use == 5
    S.keeps([1, 2], lambda: S.prefill([0], [40], [W40[40:]]), "and on across 192")  # 172 .. 211: a fresh page 3
    assert S.model.in_use == 6 and S.members[0].position() == 212
    S.check_all("behind the prefills")
    S.step(3)
    S.check_all("three steps for all")
    now = [S.rows(b) for b in range(3)]
    for b in range(3):
        assert same_rows(now[b], first[0], 130), ("below the fork point", b)  # B2, and B1 across everything above
    assert same_rows(now[0], now[2], 132)  # the second fork's point


# ---- (e) share groups ----------------------------------------------------------------------------------------------------------------------
def share_run(S, share, with_short):
    """slots 1, 3, 4 of one prompt (1 at exactly 128, 3 and 4 at 130), slot 6 forked from it at 70 (page 0 in common), slot 7 unrelated; step(3)"""
    W = S.W
    toks = stream(W, 1, 129)
    S.open(1, toks)
    S.prefill([1], [70])
    if with_short:
        S.fork(1, 6, [7])
    assert S.prefill([1], [58]) == int(with_short)  # to 128: page 1 is copied when slot 6 holds it too
    S.fork(1, 3)
    S.fork(1, 4)
    assert S.prefill([3, 4], [2, 2], [[11, 12], [13, 14]]) == 0  # forks at 128: a fresh page each
    S.admit(7, 2, 30)
    S.set_share(share)
    S.step(3)
    return S.batch.shared_rows(), S.batch.pages_in_use()


@KV
def test_e_share_groups_capped_dropped_and_with_a_member_wholly_in_the_run(scenes, kv16):
    W, make = scenes
    NL = W.cfg.n_layers
    for with_short, cases in ((True, ((1, 4 * NL), (2, 0))), (False, ((2, 3 * NL), (3, 0)))):
        off = make(kv16, 16, "paged-share")
        rows_off, pages_off = share_run(off, 0, with_short)
        assert rows_off == 0
        for share, want_rows in cases:
            S = make(kv16, 16, "paged-share")
            rows, pages = share_run(S, share, with_short)
            # with the member at 70 the run is capped at its one full page, and min_pages 2 drops the whole first-page group, the three members with
            # two common pages included; without it the run is 2 = every page the member at 128 had
            assert rows == want_rows == S.model.shared_rows, (with_short, share, rows, S.model.last_groups)
            assert pages == pages_off
            S.check_all(f"set_share({share}), member at 70: {with_short}")
            a, b = S.outcome([7]), off.outcome([7])
            same_outcome(a, b, "the unrelated member against the share-off twin")
        off.check_all("share off")


# ---- (f) all or nothing --------------------------------------------------------------------------------------------------------------------
def three_holders(S, extra):
    S.admit(0, 1, 126)
    S.fork(0, 1, [7])
    S.fork(0, 2, [11])
    S.admit(3, 2, 130)
    if extra:
        S.admit(4, 3, 5)


@KV
def test_f_a_step_takes_exactly_the_free_pages_or_nothing(scenes, kv16):
    W, make = scenes
    S = make(kv16, 10, "paged-step")
    three_holders(S, False)
    assert S.model.need_step(3) == S.batch.pages_free() == 5  # two copies of page 1 for its three holders, page 2 for each
    assert S.step(3) == 2 and S.batch.pages_free() == 0
    S.check_all("a step that takes every free page")
    S = make(kv16, 10, "paged-step")
    three_holders(S, True)
    assert S.model.need_step(3) == 5 == S.batch.pages_free() + 1
    S.refused(lambda: S.batch.step(3, 2), "too few free pages for 3 more positions", "a step one page short")
    with pytest.raises(pm.Refused, match="too few free pages for"):
        S.model.step(3)
    assert S.step(2) == 2  # to 128: the copies alone
    S.check_all("the step that fits, behind the refusal")


@KV
def test_f_a_prefill_takes_exactly_the_free_pages_or_nothing(scenes, kv16):
    W, make = scenes
    fed = [stream(W, 5, 60), stream(W, 6, 60)]

    def population(S, extra):
        S.admit(0, 1, 70)
        S.fork(0, 1)
        S.fork(0, 2)
        S.admit(3, 2, 290)
        if extra:
            S.admit(4, 3, 5)
        for b in (1, 2):
            S.feed(b, fed[b - 1])

    S = make(kv16, 11, "paged-step")
    population(S, False)
    assert S.model.need_prefill([1, 2], [60, 60]) == S.batch.pages_free() == 4  # two copies of the page slot 0 holds too, page 2 for each
    assert S.keeps([0, 3], lambda: S.prefill([1, 2], [60, 60]), "a prefill that takes every free page") == 2
    assert S.batch.pages_free() == 0
    S.check_all("a prefill that takes every free page")
    S = make(kv16, 11, "paged-step")
    population(S, True)
    S.refused(lambda: S.batch.prefill([1, 2], [60, 60]), "too few free pages for this prefill", "a prefill one page short")
    with pytest.raises(pm.Refused, match="too few free pages for this prefill"):
        S.model.prefill([1, 2], [60, 60])
    assert S.keeps([0, 3, 4], lambda: S.prefill([1, 2], [50, 50]), "the prefill that fits") == 2  # to 120: the copies alone
    S.check_all("the prefill that fits, behind the refusal")


@KV
def test_f_the_other_refusals_change_nothing(scenes, kv16):
    W, make = scenes
    S = make(kv16, 8, "paged-step")
    S.refused(lambda: S.batch.step(1, 2), "no member to step", "a step of an empty batch")
    S.admit(0, 1, 70)
    S.fork(0, 1, [7])
    S.step(1)
    S.feed(0, [9])  # (a member's own span is checked before the next listed slot is looked at)
    b = S.batch
    for call, text in ((lambda: b.prefill([0, 0], [1, 1]), "listed twice"), (lambda: b.prefill([5], [1]), "the slot is empty"), (lambda: b.release(5), "the slot is empty"),
                       (lambda: b.fork(5, 6), "the slot is empty"), (lambda: b.extract(5, S.dst), "the slot is empty"), (lambda: b.open(0), "the slot is taken"),
                       (lambda: b.fork(0, 1), "the slot is taken"), (lambda: b.admit(1, S.stages[(1, 70)], 70), "the slot is taken"),
                       (lambda: b.open(N_SLOTS), "slot index out of range"), (lambda: b.step(0, 2), "at least 1"), (lambda: b.set_share(-1), "min_pages")):
        S.refused(call, text, text)
    S.step(1)
    S.check_all("behind the refusals")


# ---- the seeded walk -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", pm.SEEDS)
@KV
def test_seeded_walk(scenes, kv16, seed):
    W, make = scenes
    ops, _ = pm.walk(seed)
    S = make(kv16, pm.WALK["n_pages"], "paged-churn")
    fresh = iter(range(100, 10 ** 6))  # a token stream of its own for everything fed
    for i, e in enumerate(ops):
        op, what = e["op"], f"seed {seed} op {i} {e}"
        if op == "checkpoint":
            S.check_all(f"seed {seed} checkpoint at op {i}")
            continue
        if op == "open":
            S.open(e["slot"])
        elif op == "fork":
            S.fork(e["src"], e["slot"], [next(fresh) % W.cfg.vocab])
        elif op == "release":
            S.release(e["slot"])
        elif op == "share":
            S.set_share(e["min_pages"])
        elif op == "prefill":
            for b, n in zip(e["slots"], e["n"]):
                S.ensure_fed(b, n, next(fresh))
            if e["refused"]:
                S.refused(lambda: S.batch.prefill(e["slots"], e["n"]), e["refused"], what)
                with pytest.raises(pm.Refused):
                    S.model.prefill(e["slots"], e["n"])
            else:
                assert S.prefill(e["slots"], e["n"]) == e["copies"], what
        elif op == "step":
            if e["refused"]:
                S.refused(lambda: S.batch.step(e["n"], 2), e["refused"], what)
                with pytest.raises(pm.Refused):
                    S.model.step(e["n"])
            else:
                assert S.step(e["n"]) == e["copies"] and S.model.shared_rows == e["shared_rows"], what
        assert S.model.in_use == e["in_use"], what
        S.counts(what)
