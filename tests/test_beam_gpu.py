"""GPU: the two beam search launches on raw buffers, no decoder.

bitnet_hip_beam_select_dev: crafted and random record tables (tests/beam_cases.py); after every launch EVERY word of the state, the pool's tokens,
every position and every history entry equal tests/beam_ref.py.  Between two launches the test does what a batched step does to the members: the
positions go up by one, a greedy pick lands in history[position] and the tap writes record [position].

bitnet_hip_kv_permute_dev: 2 layers x 2 KV heads, max_pos 300 (five chunks, the last padded), f32 and f16 caches filled with random 32-bit patterns
(NaN payloads, infinities and denormals planted); the expected arena is a numpy gather over the layout formulas (tests/extend_ref.py: k_index for K,
[kv][C * 64][D] for V) read from the ORIGINAL arena -- the permutation is simultaneous -- and the comparison is over the whole arena: moved slots,
slots below from[b] and at or above n, the padding slots, untouched beams and the guard words between the caches, in one equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cases as bc  # noqa: E402
import beam_ref as br  # noqa: E402
import extend_ref as er  # noqa: E402
import kv_read  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


# ---- select ------------------------------------------------------------------------------------------------------------------------------
class Rig:
    """B members' records, positions and histories on the device and their model on the host; GUARD entries behind every member's `capacity`"""
    GUARD = 8

    def __init__(self, torch, hip, pkg, search, capacity):
        self.torch, self.pkg, self.search = torch, pkg, search
        B = self.B = search["B"]
        self.capacity = capacity
        rng = np.random.default_rng(1234 + B)
        self.rec = np.frombuffer(rng.integers(0, 256, size=B * (capacity + self.GUARD) * pkg.LOGPROB_DTYPE.itemsize, dtype=np.uint8).tobytes(),
                                 pkg.LOGPROB_DTYPE).reshape(B, capacity + self.GUARD).copy()
        self.pos = np.full(B, search["P"], np.int32)
        self.hist = rng.integers(0, 1000, size=(B, capacity + self.GUARD)).astype(np.int32)
        self.hist[:, :search["P"] + 1] = self.hist[0, :search["P"] + 1]  # one prompt
        self.rec_dev = torch.from_numpy(self.rec.view(np.uint8).reshape(B, -1).copy()).cuda()
        self.pos_dev = torch.from_numpy(self.pos.copy()).cuda()
        self.hist_dev = torch.from_numpy(self.hist.copy()).cuda()
        row = (capacity + self.GUARD)
        members = (pkg.BeamMember * B)(*[pkg.BeamMember(self.rec_dev.data_ptr() + b * row * pkg.LOGPROB_DTYPE.itemsize, self.pos_dev.data_ptr() + 4 * b,
                                                         self.hist_dev.data_ptr() + 4 * b * row, capacity, 0) for b in range(B)])
        self.members = torch.from_numpy(np.frombuffer(bytes(members), np.uint8).copy()).cuda()
        self.beam = pkg.Beam(hip, B, search["eos"], search["max_new"], search["lw"])
        self.beam.reset(search["P"])
        self.ref = bc.new_ref(search)

    def batched_step(self, s):
        """what a step leaves in front of the select launch; the record only where the search has one"""
        self.pos += 1
        for b in range(self.B):
            q = int(self.pos[b])
            if q < self.capacity:
                self.hist[b, q] = 5000 + b  # the greedy pick the select overwrites
                if s < len(self.search["steps"]):
                    lse, ids, logits = self.search["steps"][s][b]
                    r = self.rec[b, q]
                    r["lse"], r["top_id"][:ids.size], r["top_logit"][:ids.size] = lse, ids, logits
        self.rec_dev.copy_(self.torch.from_numpy(self.rec.view(np.uint8).reshape(self.B, -1)))
        self.pos_dev.copy_(self.torch.from_numpy(self.pos))
        self.hist_dev.copy_(self.torch.from_numpy(self.hist))

    def select_and_compare(self, what):
        self.beam.select(self.members)
        st, tok = self.beam.read()
        self.ref.select(lambda b, q: (self.rec[b, q]["lse"], self.rec[b, q]["top_id"], self.rec[b, q]["top_logit"]), self.pos, self.hist, self.capacity)
        assert st.words() == self.ref.words(), what
        for i in range(self.ref.pool_n):
            assert list(tok[i, :self.ref.pool_len[i]]) == self.ref.pool_tokens[i], (what, i)
        assert np.array_equal(self.pos_dev.cpu().numpy(), self.pos), what
        assert np.array_equal(self.hist_dev.cpu().numpy(), self.hist), what
        assert np.array_equal(self.rec_dev.cpu().numpy().reshape(-1), self.rec.view(np.uint8).reshape(-1)), what  # the records are only read
        return st

    def run(self, extra=2):
        """every step of the search, then `extra` more launches (frozen if the search is done); -> steps that ran the rule"""
        ran = 0
        for s in range(len(self.search["steps"]) + extra):
            was_done = self.ref.done
            self.batched_step(s)
            if not was_done and s >= len(self.search["steps"]):
                break  # the search ran out of crafted records before it ended: nothing more to feed
            st = self.select_and_compare(f"step {s}")
            ran += st.stepped
            assert st.stepped == (0 if was_done else 1)
        return ran


@pytest.mark.parametrize("name", sorted(bc.CRAFTED))
def test_select_crafted_case(hip, pkg, torch_, name):
    search = bc.CRAFTED[name]
    rig = Rig(torch_, hip, pkg, search, capacity=search["P"] + search["max_new"] + 4)
    assert rig.run() == len(search["steps"])
    if rig.ref.done:
        assert rig.ref.frozen_steps == 2  # the frozen launches happened and were compared


@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_select_random_searches(hip, pkg, torch_, B):
    rng = np.random.default_rng(99 + B)
    longest, endings = 0, set()
    for _ in range(6):
        search = bc.random_search(rng, B)
        rig = Rig(torch_, hip, pkg, search, capacity=search["P"] + search["max_new"] + 4)
        longest = max(longest, rig.run())
        endings.add(rig.ref.done)
        assert rig.ref.done and rig.ref.frozen_steps >= 2
    assert longest >= 3  # three consecutive steps and more


def test_select_refuses_an_out_of_range_record_index(hip, pkg, torch_):
    """the step that would read record [capacity] sets the error bit and touches nothing; the search is frozen from then on.  Unequal positions
    are refused the same way."""
    search = dict(bc.CRAFTED["from_is_div_before"])
    rig = Rig(torch_, hip, pkg, search, capacity=search["P"] + 2)  # records 11 exist, record 12 does not
    rig.batched_step(0)
    rig.select_and_compare("step 0")
    assert rig.ref.done == 0
    rig.batched_step(1)
    st = rig.select_and_compare("step 1: q == capacity")
    assert st.done == br.ERR_RANGE and st.stepped == 0 and st.gen_len == 1
    rig.batched_step(2)
    st = rig.select_and_compare("frozen behind the error")
    assert st.frozen_steps == 1
    rig = Rig(torch_, hip, pkg, search, capacity=64)
    rig.batched_step(0)
    rig.pos[1] += 1
    rig.pos_dev.copy_(torch_.from_numpy(rig.pos))
    st = rig.select_and_compare("unequal positions")
    assert st.done == br.ERR_RANGE


# ---- permute ------------------------------------------------------------------------------------------------------------------------------
N_LAYERS, N_KV, D, MAX_POS, B = 2, 2, er.D, 300, 4
GUARD = 64
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000, 0xFFFFFFFF, 0x7BFF7E01, 0x0001FC00],
                    np.uint32)
PARENTS = {"identity": [0, 1, 2, 3], "swap": [1, 0, 2, 3], "cycle3": [1, 2, 0, 3], "all_from_one": [2, 2, 2, 2], "mixed_out_of_range": [3, -1, 7, 0]}


def slot_words(f16):
    """-> (K, V) [slots][words]: the 32-bit words of ONE cache that each slot occupies (every KV head)"""
    per_word = 2 if f16 else 1
    slots = er.chunks(MAX_POS) * 64
    head = slots * D  # elements per KV head
    d, pos = np.meshgrid(np.arange(D), np.arange(slots), indexing="ij")
    out = []
    for idx in (er.k_index(d, pos, f16), pos * D + d):  # [D][slots] element indices inside one head
        full = (np.arange(N_KV)[:, None, None] * head + idx[None]) // per_word  # [kv][D][slots] word indices
        words = np.sort(full.transpose(2, 0, 1).reshape(slots, -1), axis=1)
        words = words[:, ::per_word]  # an f16 word holds two elements of ONE slot: each word once
        assert np.unique(words).size == words.size == N_KV * slots * D // per_word
        out.append(words)
    return out


class PermuteRig:
    def __init__(self, torch, hip, pkg, f16):
        self.torch, self.hip, self.pkg, self.f16 = torch, hip, pkg, f16
        rng = np.random.default_rng(7 + int(f16))
        self.words = N_KV * er.chunks(MAX_POS) * 64 * D // (2 if f16 else 1)
        self.count = 2 * B * N_LAYERS  # cache index: (is_v * B + beam) * N_LAYERS + layer
        self.host = rng.integers(0, 1 << 32, size=GUARD + self.count * (self.words + GUARD), dtype=np.uint32)
        for i in range(self.count):
            v = self.view(self.host, i)
            v[rng.choice(self.words, size=4 * SPECIALS.size, replace=False)] = np.tile(SPECIALS, 4)
        self.pristine = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        self.dev = self.pristine.clone()
        table = lambda is_v: torch.tensor([self.dev.data_ptr() + 4 * self.offset(self.index(is_v, b, l)) for b in range(B) for l in range(N_LAYERS)],
                                          dtype=torch.int64, device="cuda")
        self.k_table, self.v_table = table(0), table(1)
        self.kw, self.vw = slot_words(f16)
        self.beam = pkg.Beam(hip, B, -1, 4, np.ones(5, np.float32))
        self.state_ptr = self.beam.done_ptr() - pkg.BeamState.done.offset

    def index(self, is_v, b, l):
        return (is_v * B + b) * N_LAYERS + l

    def offset(self, i):
        return GUARD + i * (self.words + GUARD)

    def view(self, host, i):
        return host[self.offset(i):self.offset(i) + self.words]

    def set_state(self, parent, frm, n_slots, stepped=1):
        st, _ = self.beam.read()
        for b in range(B):
            st.parent[b], st.from_[b] = parent[b], frm[b]
        st.n_slots, st.stepped = n_slots, stepped
        rt = kv_read.runtime()
        assert rt.hipMemcpy(C.c_void_p(self.state_ptr), C.byref(st), C.sizeof(st), 1) == 0  # hipMemcpyHostToDevice

    def expected(self, parent, frm, n, moved=True):
        want = self.host.copy()
        if not moved:
            return want
        for b in range(B):
            par = parent[b]
            if par < 0 or par >= B or par == b:
                continue
            f = min(max(frm[b], 0), n)
            for is_v, words in ((0, self.kw), (1, self.vw)):
                idx = words[f:n].reshape(-1)
                for l in range(N_LAYERS):
                    self.view(want, self.index(is_v, b, l))[idx] = self.view(self.host, self.index(is_v, par, l))[idx]
        return want

    def launch_and_compare(self, key_bound, want, what):
        torch = self.torch
        self.dev.copy_(self.pristine)
        self.hip.kv_permute_dev(self.k_table, self.v_table, self.beam, N_LAYERS, B, N_KV, D, MAX_POS, key_bound, kv_f16=self.f16)
        torch.cuda.synchronize()
        want_dev = torch.from_numpy(want.view(np.int32)).cuda()
        if not torch.equal(self.dev, want_dev):
            bad = np.flatnonzero(self.dev.cpu().numpy().view(np.uint32) != want)
            raise AssertionError((what, f"{bad.size} words differ, first at arena word {bad[0]}"))


@pytest.mark.parametrize("pattern", sorted(PARENTS))
@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
def test_permute_moves_the_diverged_slots_and_nothing_else(hip, pkg, torch_, f16, pattern):
    rig = PermuteRig(torch_, hip, pkg, f16)
    parent = PARENTS[pattern]
    moved_words = 0
    for n in (1, 63, 64, 65, 130, 300):
        froms = sorted({f for f in (0, 1, 63, 64, n - 1, n) if 0 <= f <= n})
        for rot in range(len(froms)):
            frm = [froms[(rot + b) % len(froms)] for b in range(B)]  # every beam its own start slot
            if pattern == "mixed_out_of_range" and rot == 0:
                frm[0], frm[3] = -3, n + 5  # clamped into [0, n]
            rig.set_state(parent, frm, n)
            want = rig.expected(parent, frm, n)
            moved_words += int((want != rig.host).sum())
            for key_bound in (n, MAX_POS):
                rig.launch_and_compare(key_bound, want, (pattern, n, frm, key_bound))
    assert (moved_words > 0) == (pattern != "identity")


def test_permute_writes_nothing_behind_a_frozen_step_and_clamps_n(hip, pkg, torch_):
    rig = PermuteRig(torch_, hip, pkg, False)
    rig.set_state([1, 0, 3, 2], [0, 0, 0, 0], 130, stepped=0)
    rig.launch_and_compare(MAX_POS, rig.expected(None, None, 0, moved=False), "stepped == 0")
    rig.set_state([1, 0, 3, 2], [5, 70, 0, 64], 140, stepped=1)  # n_slots beyond key_bound reads as key_bound
    rig.launch_and_compare(130, rig.expected([1, 0, 3, 2], [5, 70, 0, 64], 130), "n_slots > key_bound")
    rig.set_state([1, 0, 3, 2], [5, 70, 0, 64], -4, stepped=1)
    rig.launch_and_compare(130, rig.expected(None, None, 0, moved=False), "n_slots < 0")
