"""The page bookkeeping of a PagedBatch in plain Python, written from the prose of host/kv_pool.hpp and host/paged_batch.hpp (tests only).

A sequence is a list of abstract Page objects (identity, a holder count; no ids): page i holds positions [64 i, 64 i + 64).  fork() shares every
page of the source.  reserve(upto) appends fresh pages up to page upto // 64 and, when that page has more than one holder, replaces it by a
private one: a copy.  release() drops the sequence's references; a page nobody holds is free again.  A call that does not fit changes nothing.

need_step(n) / need_prefill(slots, n) count as the two comments in host/paged_batch.cpp say: fresh pages up to the last new position, plus one
copy of the page of the first append for every sharer of it but the last.  groups(min_pages) is set_share's rule: members (in slot order) with
the same first page; the run is their longest common leading run of pages, capped at min over the members of position >> 6; fewer than 2
members or a run below min_pages = ungrouped.

The model predicts, per operation: pages_in_use afterwards, whether the call is refused (Refused, carrying a piece of the refusal's text), how
many page copies it makes, and shared_rows of a step (grouped members x n_layers).

walk(seed) draws the operation list of the seeded lifecycle walk (tests/test_paged_lifecycle_gpu.py) from the model alone: no GPU is involved,
so its coverage is asserted in tests/test_paged_model.py."""
from __future__ import annotations

import random

PAGE = 64


class Refused(Exception):
    """the model says the call does not fit; str(e) is a piece of the text the batch must refuse with"""


class Page:
    __slots__ = ("holders",)

    def __init__(self):
        self.holders = 1


class PagedModel:
    def __init__(self, n_pages, n_slots, n_layers, max_pos):
        self.n_pages, self.n_slots, self.n_layers, self.max_pos = n_pages, n_slots, n_layers, max_pos
        self.seq = {}  # slot -> [Page]
        self.pos = {}  # slot -> position
        self.in_use = 0
        self.share_min = 0
        self.copies = 0       # page copies since creation
        self.shared_rows = 0  # of the last step
        self.last_groups = []  # of the last step: [(member slots, run)]

    # ---- the pool ----
    @property
    def free(self):
        return self.n_pages - self.in_use

    def slots(self):
        return sorted(self.seq)

    def _fresh(self):
        assert self.in_use < self.n_pages, "the model took a page it had not counted"
        self.in_use += 1
        return Page()

    def reserve(self, slot, upto):
        """room for positions [0, upto] -> (fresh pages appended, 1 if the page of upto was copied)"""
        pages, want = self.seq[slot], upto // PAGE + 1
        fresh = max(0, want - len(pages))
        for _ in range(fresh):
            pages.append(self._fresh())
        copied = 0
        if not fresh and pages[want - 1].holders > 1:
            pages[want - 1].holders -= 1
            pages[want - 1] = self._fresh()
            copied = 1
            self.copies += 1
        return fresh, copied

    def _need(self, slots, n):
        need, left = 0, {}
        for b, k in zip(slots, n):
            pages, p = self.seq[b], self.pos[b]
            need += max(0, (p + k - 1) // PAGE + 1 - len(pages))
            if p // PAGE < len(pages) and pages[p // PAGE].holders > 1:
                page = pages[p // PAGE]
                left.setdefault(id(page), page.holders)
                if left[id(page)] > 1:  # the last sharer keeps the page
                    need += 1
                    left[id(page)] -= 1
        return need

    def need_step(self, n):
        return self._need(self.slots(), [n] * len(self.seq))

    def need_prefill(self, slots, n):
        return self._need(list(slots), list(n))

    # ---- the operations ----
    def _empty(self, slot):
        if not 0 <= slot < self.n_slots:
            raise Refused("slot index out of range")
        if slot in self.seq:
            raise Refused("the slot is taken")

    def _member(self, slot):
        if not 0 <= slot < self.n_slots:
            raise Refused("slot index out of range")
        if slot not in self.seq:
            raise Refused("the slot is empty")

    def open(self, slot):
        self._empty(slot)
        self.seq[slot], self.pos[slot] = [], 0

    def admit(self, slot, n):
        self._empty(slot)
        if (n + PAGE - 1) // PAGE > self.free:
            raise Refused("too few free pages")
        self.seq[slot], self.pos[slot] = [], n
        self.reserve(slot, n - 1)

    def fork(self, src, dst):
        self._member(src)
        self._empty(dst)
        for page in self.seq[src]:
            page.holders += 1
        self.seq[dst], self.pos[dst] = list(self.seq[src]), self.pos[src]

    def release(self, slot):
        self._member(slot)
        for page in self.seq.pop(slot):
            page.holders -= 1
            self.in_use -= page.holders == 0
        del self.pos[slot]

    def _advance(self, slots, n):
        """-> copies made"""
        copies = 0
        for b, k in zip(slots, n):
            copies += self.reserve(b, self.pos[b])[1]
            self.reserve(b, self.pos[b] + k - 1)
        for b, k in zip(slots, n):
            self.pos[b] += k
        return copies

    def prefill(self, slots, n):
        slots, n = list(slots), list(n)
        if not slots:
            raise Refused("listed members")
        for i, b in enumerate(slots):
            self._member(b)
            if b in slots[:i]:
                raise Refused("a slot is listed twice")
            if n[i] > self.max_pos - 1 - self.pos[b]:
                raise Refused("KV cache overflow")
        if self.need_prefill(slots, n) > self.free:
            raise Refused("too few free pages for this prefill")
        return self._advance(slots, n)

    def set_share(self, min_pages):
        self.share_min = min_pages

    def groups(self, min_pages, pos=None):
        """-> [(member slots, run)] of the grouped members; pos: the positions the cap is taken from (default: now)"""
        pos = self.pos if pos is None else pos
        by_first = {}
        for b in self.slots():
            if self.seq[b]:
                by_first.setdefault(id(self.seq[b][0]), []).append(b)
        out = []
        for members in by_first.values():
            run = min(pos[b] // PAGE for b in members)
            lead = self.seq[members[0]]
            for b in members:
                k = 0
                while k < min(run, len(self.seq[b])) and self.seq[b][k] is lead[k]:
                    k += 1
                run = k
            if len(members) >= 2 and run >= min_pages:
                out.append((members, run))
        return out

    def step(self, n):
        """-> copies made; shared_rows is set"""
        if not self.seq:
            raise Refused("no member to step")
        for b in self.slots():
            if n > self.max_pos - 1 - self.pos[b]:
                raise Refused("KV cache overflow")
        if self.need_step(n) > self.free:
            raise Refused("too few free pages for")
        before = dict(self.pos)
        copies = self._advance(self.slots(), [n] * len(self.seq))
        # the groups are found behind the reservation and the copies, from the positions the step starts at
        self.last_groups = self.groups(self.share_min, before) if self.share_min > 0 else []
        self.shared_rows = sum(len(m) for m, _ in self.last_groups) * self.n_layers
        return copies


# ---- the seeded walk -------------------------------------------------------------------------------------------------------------------
WALK = dict(n_pages=10, n_slots=8, n_layers=2, max_pos=300, n_ops=40)
SEEDS = (2, 18, 33)


def walk(seed, n_pages=WALK["n_pages"], n_slots=WALK["n_slots"], n_layers=WALK["n_layers"], max_pos=WALK["max_pos"], n_ops=WALK["n_ops"]):
    """-> (ops, stats).  ops: [dict(op=..., args..., refused=None | text, copies=c, in_use=pages afterwards, shared_rows=of a step)], with two
    checkpoints, one of them last.  A refused open + prefill is followed by the release of the still empty member.  stats: the coverage counts."""
    rng = random.Random(seed)
    m = PagedModel(n_pages, n_slots, n_layers, max_pos)
    ops, released = [], set()
    stats = dict(copies=0, refusals=0, slot_reuses=0, hole_steps=0, wide_group_steps=0, two_page_growths=0)

    def record(op, call, **args):
        """-> True when the model lets the call through"""
        before = {b: len(p) for b, p in m.seq.items()}
        e = dict(op=op, refused=None, copies=0, **args)
        try:
            e["copies"] = call() or 0
        except Refused as why:
            e["refused"] = str(why)
            stats["refusals"] += 1
        e["in_use"] = m.in_use
        stats["copies"] += e["copies"]
        if not e["refused"]:
            stats["two_page_growths"] += any(len(m.seq[b]) - before[b] >= 2 for b in before if b in m.seq)
        ops.append(e)
        return not e["refused"]

    def seat(slot):
        stats["slot_reuses"] += slot in released
        released.discard(slot)

    for i in range(n_ops):
        if i == n_ops // 2:
            ops.append(dict(op="checkpoint"))
        taken, empty = m.slots(), [b for b in range(n_slots) if b not in m.seq]
        kinds = ["open"] * 3 * bool(empty) + ["fork"] * 3 * bool(empty and taken) + ["prefill"] * 2 * bool(taken) + ["release"] * 2 * bool(taken)
        kinds += ["step"] * 4 * bool(taken) + ["share"]
        kind = rng.choice(kinds)
        if kind == "open":
            b, n = rng.choice(empty), rng.choice((5, 21, 63, 64, 65, 100, 128, 130, 190))
            record("open", lambda: m.open(b), slot=b)
            seat(b)
            if not record("prefill", lambda: m.prefill([b], [n]), slots=[b], n=[n]):
                record("release", lambda: m.release(b), slot=b)
                released.add(b)
        elif kind == "fork":
            a, b = rng.choice(taken), rng.choice(empty)
            record("fork", lambda: m.fork(a, b), src=a, slot=b)
            seat(b)
        elif kind == "prefill":
            listed = rng.sample(taken, rng.randint(1, min(3, len(taken))))
            n = [min(rng.choice((1, 7, 40, 64, 70)), max_pos - 1 - m.pos[b]) for b in listed]
            listed, n = [b for b, k in zip(listed, n) if k > 0], [k for k in n if k > 0]
            if not listed:
                continue
            record("prefill", lambda: m.prefill(listed, n), slots=listed, n=n)
        elif kind == "release":
            b = rng.choice(taken)
            record("release", lambda: m.release(b), slot=b)
            released.add(b)
        elif kind == "step":
            n = rng.randint(1, 3)
            if record("step", lambda: m.step(n), n=n):
                ops[-1]["shared_rows"] = m.shared_rows
                lowest_empty = min(b for b in range(n_slots + 1) if b not in m.seq)
                stats["hole_steps"] += lowest_empty < max(m.seq)
                stats["wide_group_steps"] += any(len(g) >= 3 for g, _ in m.last_groups)
        else:
            v = rng.randint(0, 1)
            record("share", lambda: m.set_share(v), min_pages=v)
    ops.append(dict(op="checkpoint"))
    return ops, stats
