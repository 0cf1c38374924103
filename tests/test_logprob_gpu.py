"""GPU: the logits tap's kernel (csrc/kernels_logprob.hip) through bitnet_hip_logprob_dev / _batch_dev on torch tensors, against the numpy /
float64 restatement (tests/logprob_ref.py).

token, n_top, top_id and the bits of top_logit and logit are exact; entries >= n_top keep the bytes the test planted; lse is equal where
infinite and elsewhere within logprob_ref.lse_bound: 2 * (D + 4) * 2^-24 * max(1, |lse|), D = the longest chain of f32 additions the kernel
performs for that vocabulary, read off the code (logprob_ref.chain: per-thread run ceil(slice / 512), wave tree 6, eight waves 7, merge 2 + 6;
vocab 128256: slice 2004, D = 25).  The bound is derived from the kernel as written, doubled; it is no number read off its outputs.

Vocabularies: the issue's list; the slice width is 1024 up to 65536 entries (1023 / 1024 / 1025 sit around it; 2047 / 2048 / 2049 around two
slices), 65537 and 65540 are the first sizes with wider slices (1028), 128256 has 64 slices of 2004."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

VOCABS = [1, 2, 19, 20, 21, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 65536, 65537, 65540, 128256]
TOPS = [0, 1, 5, 20]
SENTINEL = 0xA5


def rows(V):
    """name -> row: the issue's list, built around this vocabulary's slices"""
    rng = np.random.default_rng(1000 + V)
    S, nwg = ref.geometry(V)
    normal = rng.standard_normal(V).astype(np.float32)
    out = {"normal": normal, "all equal": np.full(V, 1.5, np.float32)}
    r = normal.copy()
    a, b = (S - 1, S) if V > S else (V - 1, 0)  # the last lane of one slice and the first of the next
    r[a] = r[b] = 9.0
    out["maximum on both sides of a slice boundary"] = r
    r = normal.copy()
    r[np.unique(np.linspace(0, V - 1, 25).astype(np.int64))] = 8.0  # 25 equal maxima spread over the slices
    out["25 equal maxima"] = r
    out["descending ramp"] = np.linspace(5.0, -5.0, V).astype(np.float32)
    out["ascending ramp"] = np.linspace(-5.0, 5.0, V).astype(np.float32)
    r = normal.copy()
    r[int(np.argmax(r))] = np.nan
    out["NaN at the argmax"] = r
    r = normal.copy()
    r[V // 3] = np.inf
    out["one +inf"] = r
    out["all -inf"] = np.full(V, -np.inf, np.float32)
    out["all NaN"] = np.full(V, np.nan, np.float32)
    r = -np.abs(normal)
    r[::2] = -0.0
    r[1::4] = 0.0
    out["-0.0 against +0.0"] = r.astype(np.float32)
    return out


class Entry:
    """one bitnet_hip_logprob_args with its tensors: `capacity` records between two guard records, all planted with SENTINEL bytes"""

    def __init__(self, pkg, hip, V, capacity=4):
        import torch

        self.pkg, self.hip, self.V, self.capacity, self.torch = pkg, hip, V, capacity, torch
        self.logits = torch.zeros(V, dtype=torch.float32, device="cuda")
        self.pos = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.history = torch.zeros(capacity + 2, dtype=torch.int32, device="cuda")
        self.records = torch.full(((capacity + 2) * 176,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.scratch = torch.zeros(hip.logprob_scratch_bytes(V), dtype=torch.uint8, device="cuda")

    def set(self, row, token, q):
        torch = self.torch
        self.logits.copy_(torch.from_numpy(np.ascontiguousarray(row, np.float32)))
        self.pos.fill_(int(q))
        if 0 <= q < self.capacity:
            self.history[q] = int(token)
        self.records.fill_(SENTINEL)

    def args(self, top_n, empty=False):
        return self.pkg.LogprobArgs.make(self.logits, self.pos, self.history, None if empty else self.records.data_ptr() + 176, self.scratch, self.capacity, top_n)

    def launch(self, top_n):
        self.hip.logprob_dev(self.args(top_n), self.V)
        self.torch.cuda.synchronize()

    def read(self):
        """(records [capacity], the two guards' bytes)"""
        raw = self.records.cpu().numpy()
        return raw[176:-176].view(self.pkg.LOGPROB_DTYPE), (raw[:176], raw[-176:])


def guards_intact(guards):
    return all((g == SENTINEL).all() for g in guards)


def check(rec, want, V, what):
    s32 = np.uint32(0xA5A5A5A5)
    assert int(rec["token"]) == want.token and int(rec["n_top"]) == want.n_top, (what, rec["token"], rec["n_top"])
    assert np.array_equal(rec["top_id"][:want.n_top], want.top_id), (what, rec["top_id"][:want.n_top], want.top_id)
    assert ref.same_bits(rec["top_logit"][:want.n_top], want.top_logit), what
    assert (rec["top_id"][want.n_top:].view(np.uint32) == s32).all() and (rec["top_logit"][want.n_top:].view(np.uint32) == s32).all(), (what, "entries >= n_top")
    assert ref.same_bits(rec["logit"], want.logit) or (np.isnan(want.logit) and np.isnan(rec["logit"])), (what, rec["logit"], want.logit)
    got = float(rec["lse"])
    if np.isinf(want.lse):
        assert got == want.lse, (what, got, want.lse)
    else:
        err, bound = abs(got - want.lse), ref.lse_bound(V, want.lse)
        print(f"{what}: lse {got!r} float64 {want.lse!r} |diff| {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, got, want.lse, err, bound)


@pytest.mark.parametrize("V", VOCABS)
def test_record_equals_the_restatement(pkg, hip, V):
    e = Entry(pkg, hip, V)
    rng = np.random.default_rng(V)
    for name, row in rows(V).items():
        order = ref.top_order(row)
        for top_n in TOPS:
            token, q = int(rng.integers(0, V)), int(rng.integers(0, e.capacity))
            e.set(row, token, q)
            e.launch(top_n)  # the same scratch, launch after launch: every one of them needs the hand-over re-armed
            recs, guards = e.read()
            check(recs[q], ref.record(row, token, top_n, order), V, (V, name, top_n))
            untouched = np.delete(np.arange(e.capacity), q)
            assert (recs[untouched].view(np.uint8) == SENTINEL).all() and guards_intact(guards), (V, name, top_n, "other records")
    assert int(e.scratch[:4].view(e.torch.int32)[0]) == 0  # the ticket is back at 0


@pytest.mark.parametrize("V", [21, 4099, 128256])
def test_position_bounds_and_rearm(pkg, hip, V):
    e = Entry(pkg, hip, V, capacity=3)
    row = rows(V)["normal"]
    order = ref.top_order(row)
    e.set(row, 7 % V, e.capacity - 1)  # the last record
    e.launch(5)
    recs, guards = e.read()
    check(recs[-1], ref.record(row, 7 % V, 5, order), V, (V, "last record"))
    assert guards_intact(guards) and (recs[:-1].view(np.uint8) == SENTINEL).all()
    for q in (e.capacity, -1, e.capacity + 1000, -(2 ** 31)):  # nothing is written ...
        e.set(row, 0, q)
        e.launch(5)
        recs, guards = e.read()
        assert (recs.view(np.uint8) == SENTINEL).all() and guards_intact(guards), (V, q)
    e.set(row, 3 % V, 0)  # ... and the hand-over was re-armed all the same: the next launch on this scratch is right
    e.launch(20)
    recs, guards = e.read()
    check(recs[0], ref.record(row, 3 % V, 20, order), V, (V, "after the out-of-range launches"))
    assert guards_intact(guards)


@pytest.mark.parametrize("V", [64, 4099])
def test_token_out_of_range_gives_nan_logit_and_the_rest_intact(pkg, hip, V):
    e = Entry(pkg, hip, V)
    row = rows(V)["normal"]
    for token in (V, -1, 2 ** 31 - 1):
        e.set(row, token, 1)
        e.launch(5)
        recs, guards = e.read()
        want = ref.record(row, token, 5)
        assert np.isnan(want.logit) and np.isnan(recs[1]["logit"])
        check(recs[1], want, V, (V, "token", token))
        assert guards_intact(guards)


def test_repeated_launches_give_identical_bytes(pkg, hip):
    V = 128256
    e = Entry(pkg, hip, V)
    e.set(rows(V)["normal"], 11, 2)
    seen = set()
    for _ in range(5):
        e.launch(20)
        seen.add(e.records.cpu().numpy().tobytes() + e.scratch.cpu().numpy().tobytes())
    assert len(seen) == 1


def table_of(torch, entries):
    return torch.from_numpy(np.frombuffer(b"".join(bytes(a) for a in entries), np.uint8).copy()).cuda()


@pytest.mark.parametrize("V", [2049, 128256])
def test_batch_equals_single_launches(pkg, hip, V):
    import torch

    R = rows(V)
    names = list(R)
    rng = np.random.default_rng(V + 1)
    tops = [0, 1, 5, 20, 20, 7, 25, 3]  # 25: the kernel clamps a table entry's top_n to the maximum
    empty = {2, 5}
    singles, batch = [Entry(pkg, hip, V) for _ in range(8)], [Entry(pkg, hip, V) for _ in range(8)]
    for b in range(8):
        row, token, q = R[names[b % len(names)]], int(rng.integers(0, V)), int(rng.integers(0, 4))
        singles[b].set(row, token, q)
        batch[b].set(row, token, q)
        if b not in empty:
            singles[b].launch(min(tops[b], 20))
    table = table_of(torch, [batch[b].args(tops[b], empty=b in empty) for b in range(8)])
    hip.logprob_batch_dev(table, 8, V)
    torch.cuda.synchronize()
    for b in range(8):
        got, want = batch[b].records.cpu().numpy(), singles[b].records.cpu().numpy()
        assert np.array_equal(got, want), (V, "slot", b, "records")
        assert np.array_equal(batch[b].scratch.cpu().numpy(), singles[b].scratch.cpu().numpy()), (V, "slot", b, "scratch")
        if b in empty:
            assert (got == SENTINEL).all() and not batch[b].scratch.any()  # an empty entry: nothing read or written
        else:
            assert (got[176:-176] != SENTINEL).any()
    # a table of one, and an all-empty table
    one = Entry(pkg, hip, V)
    one.set(R["normal"], 5 % V, 0)
    hip.logprob_batch_dev(table_of(torch, [one.args(5)]), 1, V)
    torch.cuda.synchronize()
    recs, guards = one.read()
    check(recs[0], ref.record(R["normal"], 5 % V, 5), V, (V, "table of one"))
    assert guards_intact(guards)
    one.set(R["normal"], 5 % V, 0)
    hip.logprob_batch_dev(table_of(torch, [one.args(5, empty=True) for _ in range(8)]), 8, V)
    torch.cuda.synchronize()
    assert (one.records.cpu().numpy() == SENTINEL).all()
