"""GPU: bitnet_hip_sample_batch_* (csrc/kernels_sample.hip, k_sample_batch) -- every bound slot of a table sampled in ONE launch -- against
TWIN samplers of the same configs and seeds that take the same logits through bitnet_hip_sample_dev, one by one.

The criterion is equality: both kernels run one body, so per slot the token, the history entry, the position and the ChaCha20 word counter
must be the twin's, call after call (the repetition penalty makes every later call depend on the counts the earlier ones left).  No
tolerance is involved.  k_sample itself is held to the reference's sampler by tests/test_sampling_gpu.py.

Every slot's token word, position, history, forced count and logits sit between guard words, checked after every launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# G with penalty, S, F, top_k = 1, top_k = 100 (the F path with a top-k)
CONFIGS = [(1.0, 0, 1.0, 1.1), (0.7, 40, 0.95, 1.1), (0.7, 0, 0.95, 1.1), (0.8, 1, 0.9, 1.1), (0.7, 100, 0.95, 1.1)]
HIST, G = 40, 4
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def planted_logits(rng, vocab, k):
    """a peaked row with a NaN, a -inf, both zeros, duplicates, and ties at the k-th value (the stable tie rule decides which survive)"""
    x = (4.0 * rng.standard_normal(vocab)).astype(np.float32)
    idx = rng.choice(vocab, 12, replace=False)
    x[idx[0]] = np.nan
    x[idx[1]] = -np.inf
    x[idx[2]] = 0.0
    x[idx[3]] = -0.0
    x[idx[4:6]] = x[idx[6]]
    if 0 < k < vocab:
        kth = np.sort(np.where(np.isnan(x), -np.inf, x))[::-1][k - 1]
        x[idx[7:10]] = kth
    return x


class Lane:
    """one sampler with the device words sample_dev takes, each between guard words"""

    def __init__(self, torch, hip, vocab, cfg, seed, pos0=0, n_forced=0):
        self.torch, self.vocab, self.cfg = torch, vocab, cfg
        self.smp = hip.sampler(vocab, *cfg, seed=seed)
        n = G + 1 + G + 1 + G + HIST + G + 1 + G
        self.arena = torch.full((n,), GUARD, dtype=torch.int32, device="cuda")
        o = G
        self.tok = self.arena[o:o + 1]
        o += 1 + G
        self.pos = self.arena[o:o + 1]
        o += 1 + G
        self.hist = self.arena[o:o + HIST]
        o += HIST + G
        self.nf = self.arena[o:o + 1]
        self.tok.fill_(-1)
        self.pos.fill_(pos0)
        self.hist.fill_(-1)
        self.nf.fill_(n_forced)
        self.larena = torch.zeros(vocab + 2 * G, dtype=torch.float32, device="cuda")
        self.larena.view(torch.int32)[:G] = GUARD
        self.larena.view(torch.int32)[-G:] = GUARD
        self.logits = self.larena[G:G + vocab]
        self.mask = torch.ones(n, dtype=torch.bool, device="cuda")
        for v in (self.tok, self.pos, self.hist, self.nf):
            self.mask[v.storage_offset():v.storage_offset() + v.numel()] = False

    def load(self, x):
        self.logits.copy_(self.torch.from_numpy(x))

    def guards_ok(self):
        li = self.larena.view(self.torch.int32)
        return bool((self.arena[self.mask] == GUARD).all()) and bool((li[:G] == GUARD).all()) and bool((li[-G:] == GUARD).all())

    def words(self):
        p = int(self.pos.item())
        return dict(tok=int(self.tok.item()), pos=p, hist=self.hist.cpu().numpy().copy())

    def bind(self, table, slot):
        table.set(slot, self.smp, self.logits, self.tok, self.pos, self.hist, self.nf)

    def alone(self):
        self.smp.sample_dev(self.logits, self.tok, self.pos, self.hist, self.nf)

    def close(self):
        self.smp.close()


def pair(torch, hip, vocab, i, **kw):
    cfg = CONFIGS[i % len(CONFIGS)]
    return Lane(torch, hip, vocab, cfg, seed=100 + 7 * i, **kw), Lane(torch, hip, vocab, cfg, seed=100 + 7 * i, **kw)


def feed(rng, lanes):
    """fresh planted logits of its own for one slot: the member and its twin read the same row"""
    x = planted_logits(rng, lanes[0].vocab, lanes[0].cfg[1])
    for l in lanes:
        l.load(x)


def assert_equal(m, t, what):
    a, b = m.words(), t.words()
    assert a["tok"] == b["tok"], (what, "token", a["tok"], b["tok"])
    assert a["pos"] == b["pos"], (what, "position", a["pos"], b["pos"])
    assert np.array_equal(a["hist"], b["hist"]), (what, "history", a["hist"], b["hist"])
    assert m.guards_ok() and t.guards_ok(), (what, "guard words")


@pytest.mark.parametrize("n_slots", [1, 3, 8])
@pytest.mark.parametrize("vocab", [1000, 2500, 128256])  # 1 workgroup per slot (a ticket of one), 3 with a ragged last slice, 64
def test_every_slot_equals_its_twin_over_twelve_calls(hip, torch_, vocab, n_slots):
    torch = torch_
    rng = np.random.default_rng(1000 * n_slots + vocab)
    pairs = [pair(torch, hip, vocab, i, pos0=i) for i in range(n_slots)]
    table = hip.sample_batch(vocab, n_slots)
    for b, (m, _) in enumerate(pairs):
        m.bind(table, b)
    tokens = set()
    for call in range(12):
        for p in pairs:
            feed(rng, p)
        table.launch()
        for _, t in pairs:
            t.alone()
        torch.cuda.synchronize()
        for b, (m, t) in enumerate(pairs):
            assert_equal(m, t, (vocab, n_slots, "call", call, "slot", b))
            w = m.words()
            assert w["pos"] == b + call + 1 and w["hist"][w["pos"]] == w["tok"] and 0 <= w["tok"] < vocab
            tokens.add(w["tok"])
    for b, (m, t) in enumerate(pairs):
        want = 0 if m.cfg == CONFIGS[0] else 12  # the greedy shortcut takes no RNG word
        assert m.smp.draws() == t.smp.draws() == want, (vocab, n_slots, "draws of slot", b)
    assert len(tokens) > 1
    table.close()
    for p in pairs:
        for l in p:
            l.close()


def test_empty_slots_touch_nothing_and_a_rebound_slot_continues(hip, torch_):
    """8 entries, empty ones in the middle (2, 5) and at the end (7); slot 3 is emptied after six calls and bound again after eight: while it is
    empty none of its words, logits or guard words changes and its sampler draws nothing; afterwards it continues as a twin that skipped
    those two calls."""
    torch = torch_
    vocab = 2500
    rng = np.random.default_rng(7)
    bound = [0, 1, 3, 4, 6]
    pairs = {b: pair(torch, hip, vocab, b, pos0=2) for b in bound}
    table = hip.sample_batch(vocab, 8)
    for b in bound:
        pairs[b][0].bind(table, b)
    for call in range(12):
        away = 6 <= call < 8
        if call == 6:
            table.set(3, None)
        if call == 8:
            pairs[3][0].bind(table, 3)
        for b in bound:
            feed(rng, pairs[b])
        m3 = pairs[3][0]
        before = (m3.arena.clone(), m3.larena.view(torch.int32).clone(), m3.smp.draws()) if away else None
        table.launch()
        for b in bound:
            if not (away and b == 3):
                pairs[b][1].alone()
        torch.cuda.synchronize()
        for b in bound:
            assert_equal(*pairs[b], ("call", call, "slot", b))
        if away:
            assert torch.equal(m3.arena, before[0]) and torch.equal(m3.larena.view(torch.int32), before[1]) and m3.smp.draws() == before[2]
    for b in bound:
        m, t = pairs[b]
        assert m.smp.draws() == t.smp.draws(), b
    assert pairs[3][0].words()["pos"] == 2 + 10 and pairs[0][0].words()["pos"] == 2 + 12
    # a table with every slot empty still launches, and nothing moves
    for b in bound:
        table.set(b, None)
    snap = {b: pairs[b][0].arena.clone() for b in bound}
    table.launch()
    torch.cuda.synchronize()
    for b in bound:
        assert torch.equal(pairs[b][0].arena, snap[b])
    table.close()
    for p in pairs.values():
        for l in p:
            l.close()


def test_a_forced_position_draws_and_counts_nothing(hip, torch_):
    """slot 1 stands at p + 1 < n_forced for two calls: the token word receives the prompt token, the position advances, draws() does not move"""
    torch = torch_
    vocab = 2500
    rng = np.random.default_rng(11)
    pairs = [pair(torch, hip, vocab, i, pos0=3, n_forced=6 if i == 1 else 0) for i in range(3)]
    for l in pairs[1]:
        l.hist[4], l.hist[5] = 77, 78
    table = hip.sample_batch(vocab, 3)
    for b, (m, _) in enumerate(pairs):
        m.bind(table, b)
    for call in range(5):
        for p in pairs:
            feed(rng, p)
        table.launch()
        for _, t in pairs:
            t.alone()
        torch.cuda.synchronize()
        for b, (m, t) in enumerate(pairs):
            assert_equal(m, t, ("call", call, "slot", b))
        m = pairs[1][0]
        w = m.words()
        assert w["pos"] == 4 + call
        if call < 2:  # p + 1 = 4, 5 < 6: a prompt token sits there
            assert w["tok"] == 77 + call and list(w["hist"][4:6]) == [77, 78] and m.smp.draws() == 0
        else:
            assert m.smp.draws() == call - 1 and w["hist"][w["pos"]] == w["tok"]
    assert pairs[1][0].smp.draws() == pairs[1][1].smp.draws() == 3  # S config: one word per sampled call
    assert pairs[2][0].smp.draws() == 5
    table.close()
    for p in pairs:
        for l in p:
            l.close()


def test_a_sampler_moves_between_the_table_and_sample_dev(hip, torch_):
    """three calls through the table, three through sample_dev after its slot was emptied, three through the table again: the hand-over is left
    re-armed either way, and the sampler goes on as a twin that took all nine through sample_dev"""
    torch = torch_
    vocab = 2500
    rng = np.random.default_rng(13)
    pairs = [pair(torch, hip, vocab, i + 1) for i in range(2)]  # S and F
    table = hip.sample_batch(vocab, 2)
    pairs[1][0].bind(table, 1)
    for call in range(9):
        if call == 0 or call == 6:
            pairs[0][0].bind(table, 0)
        if call == 3:
            table.set(0, None)
        for p in pairs:
            feed(rng, p)
        table.launch()
        if 3 <= call < 6:
            pairs[0][0].alone()
        for _, t in pairs:
            t.alone()
        torch.cuda.synchronize()
        for b, (m, t) in enumerate(pairs):
            assert_equal(m, t, ("call", call, "slot", b))
    for m, t in pairs:
        assert m.smp.draws() == t.smp.draws() == 9
    table.close()
    for p in pairs:
        for l in p:
            l.close()


def test_refusals_leave_the_table_unchanged(hip, pkg, torch_):
    torch = torch_
    vocab = 1000
    rng = np.random.default_rng(17)
    (m, t), (other, other_t) = pair(torch, hip, vocab, 2), pair(torch, hip, vocab, 1)
    foreign = Lane(torch, hip, 999, CONFIGS[1], seed=1)
    table = hip.sample_batch(vocab, 3)
    m.bind(table, 0)
    with pytest.raises(pkg.BitNetHipError, match="slot 3 out of range") as e:
        other.bind(table, 3)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.BitNetHipError, match="sample_batch_set: vocab 1000, the sampler was made for 999"):
        foreign.bind(table, 1)
    with pytest.raises(pkg.BitNetHipError, match="already bound to slot 0"):
        m.bind(table, 2)
    with pytest.raises(pkg.BitNetHipError, match="Null pointer"):
        table.set(1, other.smp, None, other.tok, other.pos, other.hist, other.nf)
    m.bind(table, 0)  # the same sampler into its own slot again is no refusal
    feed(rng, (m, t))
    feed(rng, (other, other_t))
    snap = (other.arena.clone(), foreign.arena.clone())
    table.launch()
    t.alone()
    torch.cuda.synchronize()
    assert_equal(m, t, "the bound slot after the refusals")
    assert torch.equal(other.arena, snap[0]) and torch.equal(foreign.arena, snap[1])  # slots 1 and 2 stayed empty
    assert other.smp.draws() == 0 and foreign.smp.draws() == 0 and m.smp.draws() == 1
    for n_slots in (0, 9):
        with pytest.raises(pkg.BitNetHipError, match="n_slots must be in 1..8"):
            hip.sample_batch(vocab, n_slots)
    table.close()
    for l in (m, t, other, other_t, foreign):
        l.close()
