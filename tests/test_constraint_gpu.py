"""GPU: the sampler's CONSTRAINTS stage (bitnet_hip_sampler_set_constraints, csrc/kernels_sample.hip) -- logit bias, bans, an allowed set,
an EOS hold-off, an n-gram block -- held by an EQUIVALENCE, bit for bit, with no tolerance:

    sampler A has constraints and samples the raw row L;
    sampler B has the same config and seed and NO constraints, and is given L' = apply(L, cfg, g, seq) (tests/constraint_ref.py), uploaded.

At every step the two must agree in token, history, position, ChaCha20 word counter and Mirostat's mu; the per-token counts are held through
what they do: the G cases run a repetition penalty and both additive penalties (every later token depends on the counts the earlier ones
left), and after the last step both samplers take one common config with strong penalties, constraints off, and must go on agreeing.

Constrained ids sit at 0, at vocab - 1 and at both edges of a workgroup slice (the launch geometry is restated in `geometry`)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
STEPS, CAP = 12, 64
VOCABS = [1, 2, 63, 64, 65, 1000, 4097]
BIG = 128256

# name -> (sampler kwargs, mirostat).  G: greedy with the penalties; S: the one-lane path; F: the full-vocabulary path; M: Mirostat
PATHS = {
    "G-repetition": (dict(temperature=0.0, repetition_penalty=1.3), None),
    "G-additive": (dict(temperature=0.0, frequency_penalty=0.4, presence_penalty=0.2), None),
    "S-topk8": (dict(temperature=0.8, top_k=8, repetition_penalty=1.1), None),
    "F-temperature": (dict(temperature=0.7), None),
    "F-top_p": (dict(temperature=0.7, top_p=0.9, repetition_penalty=1.1), None),
    "F-min_p": (dict(temperature=0.9, min_p=0.05), None),
    "F-typical_p": (dict(temperature=0.9, typical_p=0.9), None),
    "M-mirostat": (dict(temperature=0.9, frequency_penalty=0.1), (5.0, 0.1)),
}


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def geometry(vocab):
    """(workgroups, slice) of a sampling launch: csrc/kernels_sample.hip `geometry`"""
    nwg = min(64, (vocab + 1023) // 1024)
    return nwg, (vocab + nwg - 1) // nwg


def edge_ids(vocab):
    """0, vocab - 1, and both sides of the first and the last boundary between two workgroups' slices"""
    nwg, sl = geometry(vocab)
    ids = {0, vocab - 1, vocab // 2}
    if nwg > 1:
        ids |= {sl - 1, sl, (nwg - 1) * sl - 1, (nwg - 1) * sl}
    return sorted(i for i in ids if 0 <= i < vocab)


_ROWS = {}


def rows(vocab):
    """three peaked rows per vocabulary, made once and shared; the edge ids carry the largest logits of row 0, so that constraints on them decide"""
    if vocab not in _ROWS:
        rng = np.random.default_rng(7000 + vocab)
        out = []
        for r in range(3):
            x = (2.5 * rng.standard_normal(vocab)).astype(F)
            e = edge_ids(vocab)
            if r == 0:
                x[e] = (9.0 + 0.25 * np.arange(len(e))).astype(F)
            elif r == 1:
                x[e[::2]] = F(8.5)
            if vocab > 16:
                x[vocab // 3] = np.nan
                x[vocab // 3 + 1] = -np.inf
                x[vocab // 3 + 2] = -0.0
            out.append(x)
        _ROWS[vocab] = out
    return _ROWS[vocab]


def configs(vocab):
    """two constraint configs for a vocabulary, on the edge ids"""
    e = edge_ids(vocab)
    vals = [6.0, -np.inf, -2.5, 3.0, 0.75, -np.inf, 1.5]
    bias = [(t, vals[k % len(vals)]) for k, t in enumerate(e)]
    bias = bias + [(e[0], -1.0), (e[-1], 4.0)]  # duplicates: the last entry wins
    first = dict(bias=bias, hold=[e[-1], e[len(e) // 2]], min_tokens=5, no_repeat_ngram=2)
    allowed = sorted(set(e) | {t for t in (1, 2, vocab // 3, vocab // 3 + 1, vocab - 2) if 0 <= t < vocab})
    second = dict(allowed=allowed, bias=[(e[0], 2.0), (e[-1], -0.5)], no_repeat_ngram=1 if vocab > 8 else 0, hold=[e[0]], min_tokens=3)
    return [("bias-hold-ngram2", first), ("allowed-bias-ngram1", second)]


class Lane:
    def __init__(self, torch, hip, vocab, kw, miro, prompt, seed=77):
        self.torch, self.vocab = torch, vocab
        self.smp = hip.sampler(vocab, seed=seed, **kw)
        if miro:
            self.smp.set_mirostat(*miro)
        self.tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.hist = torch.full((CAP,), -1, dtype=torch.int32, device="cuda")
        if len(prompt):
            self.hist[:len(prompt)] = torch.tensor(prompt, dtype=torch.int32)
        self.pos = torch.full((1,), len(prompt) - 1, dtype=torch.int32, device="cuda")
        self.nf = torch.full((1,), len(prompt), dtype=torch.int32, device="cuda")
        self.logits = torch.zeros(vocab, dtype=torch.float32, device="cuda")

    def step(self, x, stream=0):
        self.logits.copy_(self.torch.from_numpy(np.ascontiguousarray(x)))
        self.smp.sample_dev(self.logits, self.tok, self.pos, self.hist, self.nf, stream=stream)
        self.torch.cuda.synchronize()

    def seq(self):
        p = int(self.pos.item())
        return self.hist[:p + 1].cpu().numpy().tolist()

    def words(self):
        mu, fb = self.smp.mirostat_state()
        return dict(tok=int(self.tok.item()), pos=int(self.pos.item()), hist=self.hist.cpu().numpy().tolist(), draws=self.smp.draws(),
                    mu=F(mu).tobytes(), fallbacks=fb)

    def close(self):
        self.smp.close()


def assert_same(a, b, what):
    wa, wb = a.words(), b.words()
    for k in wa:
        assert wa[k] == wb[k], (what, k, wa[k], wb[k])


def equivalence(torch, hip, vocab, kw, miro, cfg, prompt, steps=STEPS, tag="", row_list=None):
    """A (constrained, raw rows) against B (unconstrained, rows edited by the restatement); returns A's tokens"""
    xs = row_list or rows(vocab)
    A, B = Lane(torch, hip, vocab, kw, miro, prompt), Lane(torch, hip, vocab, kw, miro, prompt)
    A.smp.set_constraints(**cfg)
    toks, edited = [], 0
    for i in range(steps):
        x = xs[i % len(xs)]
        g, seq = A.smp.chosen(), A.seq()
        assert g == i
        y = cr.apply(x, cfg, g, seq)
        edited += y.tobytes() != x.tobytes()
        A.step(x)
        B.step(y)
        assert_same(A, B, (tag, vocab, "step", i))
        toks.append(int(A.tok.item()))
    assert A.smp.chosen() == steps and B.smp.chosen() == 0
    assert edited > 0, (tag, "the constraints never changed a row")
    # the counts both hold, through what they do: one common config with strong penalties, constraints off
    A.smp.set_constraints()
    for s in (A, B):
        s.smp.set_mirostat(None)
        s.smp.configure(0.0, 0, 1.0, 1.7, 5, frequency_penalty=0.9, presence_penalty=0.3)
    for i in range(3):
        A.step(xs[0])
        B.step(xs[0])
        assert_same(A, B, (tag, vocab, "counts probe", i))
    assert A.smp.chosen() == steps  # launches with constraints off do not count
    A.close()
    B.close()
    return toks


def prompt_for(vocab):
    e = edge_ids(vocab)
    return [e[0], e[-1], e[0], e[-1]] if vocab > 1 else [0]


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("path", list(PATHS))
def test_constrained_equals_unconstrained_on_the_edited_row(hip, torch_, path, vocab):
    kw, miro = PATHS[path]
    for name, cfg in configs(vocab):
        equivalence(torch_, hip, vocab, kw, miro, cfg, prompt_for(vocab), tag=(path, name))


@pytest.mark.parametrize("path", ["G-repetition", "S-topk8", "F-top_p", "M-mirostat"])
def test_the_full_vocabulary(hip, torch_, path):
    kw, miro = PATHS[path]
    name, cfg = configs(BIG)[0]
    equivalence(torch_, hip, BIG, kw, miro, cfg, prompt_for(BIG), tag=(path, name))


V4 = 4097  # five workgroups of 820 entries
NGRAM_CASES = [
    # name, history, n, the tokens the block must ban
    ("shorter-than-n-1", [5], 3, set()),
    ("exactly-n-1", [5, 6], 3, set()),
    ("empty-history-n1", [], 1, set()),
    ("match-at-j0", [5, 6, 7, 1, 5, 6], 3, {7}),
    ("match-at-the-last-j", [1, 2, 4, 4], 2, {4}),
    ("overlapping", [7, 7, 7, 7], 3, {7}),
    ("two-matches", [5, 6, 7, 5, 6, 8, 5, 6], 3, {7, 8}),
    ("another-slice", [3, 4, 4000, 9, 3, 4], 3, {4000}),
    ("slice-edges", [819, 820, 11, 820, 819, 12, 819], 2, {820, 12}),
    ("n1", [0, 4096, 819, 820, 17], 1, {0, 4096, 819, 820, 17}),
    ("n8", [1, 2, 3, 4, 5, 6, 7, 4096, 9, 1, 2, 3, 4, 5, 6, 7], 8, {4096}),
    ("n8-one-short", [1, 2, 3, 4, 5, 6, 7], 8, set()),
    ("out-of-vocabulary", [5000, -3, 9, 5000, -3, 5000, 5000, -3], 3, {9}),  # such ids take part in a match; as the banned token they are skipped
]


@pytest.mark.parametrize("name,history,n,banned", NGRAM_CASES, ids=[c[0] for c in NGRAM_CASES])
def test_ngram_block(hip, torch_, name, history, n, banned):
    """a greedy sampler on a row whose largest entries are the tokens the block should ban (and three it should not): the token is the argmax
    of the edited row, and the banned set is the one written down here"""
    assert cr.ngram_banned(history, n, V4) == banned
    x = np.full(V4, -1.0, F)
    decoys = [2048, 33, 4095]
    for k, t in enumerate(sorted(banned)):
        x[t] = F(20.0 + k)
    for k, t in enumerate(decoys):
        x[t] = F(10.0 - k)
    cfg = dict(no_repeat_ngram=n)
    y = cr.apply(x, cfg, 0, history)
    assert set(np.flatnonzero(y != x).tolist()) == banned and int(np.argmax(y)) == 2048
    if banned:
        assert int(np.argmax(x)) in banned  # without the block a banned token would win
    A, B = (Lane(torch_, hip, V4, dict(temperature=0.0), None, history) for _ in range(2))
    A.smp.set_constraints(**cfg)
    A.step(x)
    B.step(y)
    assert int(A.tok.item()) == 2048
    assert_same(A, B, name)
    A.close()
    B.close()


def test_hold_off_counts_chosen_tokens_only(hip, torch_):
    """EOS held with min_tokens = 5: -inf for the first five chosen tokens, live from the sixth; a forced position in the middle does not count"""
    torch = torch_
    V, E, second = 1000, 999, 500
    x = np.zeros(V, F)
    x[E], x[second] = 9.0, 8.0
    A = Lane(torch, hip, V, dict(temperature=0.0), None, [1, 2])
    A.smp.set_constraints(hold=[E], min_tokens=5)
    got = []
    for i in range(8):
        if i == 2:  # a token fed into the running generation: position p + 1 is forced
            p = int(A.pos.item())
            A.hist[p + 1] = 77
            A.nf.fill_(p + 2)
        g = A.smp.chosen()
        A.step(x)
        got.append((int(A.tok.item()), g, A.smp.chosen()))
    assert [t for t, _, _ in got] == [second, second, 77, second, second, second, E, E]
    assert [(b, a) for _, b, a in got] == [(0, 1), (1, 2), (2, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]
    A.smp.reset()
    assert A.smp.chosen() == 0
    A.close()
    # the same through the equivalence, sampled
    equivalence(torch, hip, V, dict(temperature=0.8, top_k=8), None, dict(hold=[E, second], min_tokens=5), [1, 2], row_list=[x], tag="hold")


@pytest.mark.parametrize("path", list(PATHS))
def test_a_row_on_which_everything_is_banned(hip, torch_, path):
    kw, miro = PATHS[path]
    V = 1000
    cfg = dict(bias=[(t, -np.inf) for t in range(V)])
    x = rows(V)[0]
    assert np.all(cr.apply(x, cfg, 0, []) == -np.inf)
    equivalence(torch_, hip, V, kw, miro, cfg, [3, 4], steps=4, tag=(path, "all-banned"))
    equivalence(torch_, hip, 65, kw, miro, dict(allowed=[7], bias=[(7, -np.inf)]), [3, 4], steps=4, tag=(path, "all-banned-allowed"))


@pytest.mark.parametrize("path", ["G-repetition", "G-additive", "S-topk8", "F-top_p", "M-mirostat"])
def test_sample_host_applies_the_same_stage(hip, path):
    """bitnet_hip_sample_host with constraints == apply, then the unconstrained sample_host: g = the list's length, the list is the sequence"""
    kw, miro = PATHS[path]
    V = 4097
    name, cfg = configs(V)[0]
    A, B = hip.sampler(V, seed=9, **kw), hip.sampler(V, seed=9, **kw)
    for s in (A, B):
        if miro:
            s.set_mirostat(*miro)
    A.set_constraints(**cfg)
    gen = [0, 4096, 0]
    for i in range(STEPS):
        x = rows(V)[i % 3]
        a = A.sample_host(x, gen)
        b = B.sample_host(cr.apply(x, cfg, len(gen), gen), gen)
        assert a == b and A.draws() == B.draws() and A.mirostat_state() == B.mirostat_state(), (path, i, a, b)
        gen = gen + [a]
    assert A.chosen() == 0  # the host path's count is the length of its list
    A.close()
    B.close()


def test_refusals_that_need_the_vocabulary_change_nothing(hip, pkg, torch_):
    V = 1000
    A = Lane(torch_, hip, V, dict(temperature=0.0), None, [1])
    A.smp.set_constraints(bias={5: -np.inf})
    x = np.zeros(V, F)
    x[5], x[6], x[999] = 3.0, 2.0, 1.0
    for bad in (dict(bias={V: 1.0}), dict(allowed=[3, V]), dict(hold=[V + 5], min_tokens=1), dict(bias={1: float("nan")}), dict(no_repeat_ngram=9)):
        with pytest.raises(pkg.BitNetHipError) as e:
            A.smp.set_constraints(**bad)
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT
        A.step(x)
        assert int(A.tok.item()) == 6  # the config in force is still the first one
    A.smp.set_constraints(off=True)
    A.step(x)
    assert int(A.tok.item()) == 5
    A.close()


def test_a_captured_graph_follows_set_constraints(hip, torch_):
    """four launches captured once with constraints off; replayed off, then under constraints, then under others, then off again -- each time
    the words an eager twin leaves.  chosen() counts the constrained launches and stays when constraints go off."""
    torch = torch_
    V = 4097
    kw = dict(temperature=0.8, top_p=0.9, repetition_penalty=1.1)
    x = rows(V)[0]
    G_, T_ = Lane(torch, hip, V, kw, None, [0, 4096]), Lane(torch, hip, V, kw, None, [0, 4096])
    for l in (G_, T_):
        l.logits.copy_(torch.from_numpy(x))
    n = 4
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        G_.smp.sample_dev(G_.logits, G_.tok, G_.pos, G_.hist, G_.nf, stream=stream.cuda_stream)  # warm-up: one real call
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(n):
                G_.smp.sample_dev(G_.logits, G_.tok, G_.pos, G_.hist, G_.nf, stream=stream.cuda_stream)
    T_.step(x)
    assert_same(G_, T_, "warm-up")
    first, second = configs(V)
    chosen = 0
    for cfg in (None, first[1], second[1], None):
        for l in (G_, T_):
            l.smp.set_constraints(**cfg) if cfg else l.smp.set_constraints()
        graph.replay()
        torch.cuda.synchronize()
        for _ in range(n):
            T_.step(x)
        chosen += n if cfg else 0
        assert_same(G_, T_, ("replay", cfg))
        assert G_.smp.chosen() == T_.smp.chosen() == chosen
    # and the twin's constrained steps were the restatement's: an unconstrained sampler on the edited rows lands on the same history
    R = Lane(torch, hip, V, kw, None, [0, 4096])
    R.step(x)
    g = 0
    for cfg in (None, first[1], second[1], None):
        for _ in range(n):
            R.step(cr.apply(x, cfg, g, R.seq()) if cfg else x)
            g += 1 if cfg else 0
    assert R.words()["hist"] == T_.words()["hist"] and R.smp.draws() == T_.smp.draws()
    for l in (G_, T_, R):
        l.close()


def test_batch_slots_equal_sample_dev_alone(hip, torch_):
    """k_sample_batch shares the body: eight slots with different constraints and paths each leave what sample_dev alone leaves, and an
    unconstrained slot beside constrained ones keeps the tokens of a sampler that never met constraints"""
    torch = torch_
    V = 4097
    names = list(PATHS)
    first, second = configs(V)

    def lane_cfg(i):
        base = dict((first, second)[i % 2][1])
        base["no_repeat_ngram"] = 1 + i % 3
        base["min_tokens"] = 2 + i
        return base

    members = [Lane(torch, hip, V, *PATHS[names[i]], prompt_for(V), seed=50 + i) for i in range(8)]
    twins = [Lane(torch, hip, V, *PATHS[names[i]], prompt_for(V), seed=50 + i) for i in range(8)]
    for i in range(8):
        members[i].smp.set_constraints(**lane_cfg(i))
        twins[i].smp.set_constraints(**lane_cfg(i))
    table = hip.sample_batch(V, 8)
    for i, m in enumerate(members):
        table.set(i, m.smp, m.logits, m.tok, m.pos, m.hist, m.nf)
    plain = Lane(torch, hip, V, *PATHS["S-topk8"], prompt_for(V), seed=50)
    plain_twin = Lane(torch, hip, V, *PATHS["S-topk8"], prompt_for(V), seed=50)
    for step in range(8):
        if step == 4:  # an unconstrained sampler takes slot 0, beside seven constrained ones
            table.set(0, plain.smp, plain.logits, plain.tok, plain.pos, plain.hist, plain.nf)
        x = rows(V)[step % 3]
        live = ([plain] if step >= 4 else [members[0]]) + members[1:]
        for m in live:
            m.logits.copy_(torch.from_numpy(x))
        table.launch()
        torch.cuda.synchronize()
        for i in range(8):
            if i == 0 and step >= 4:
                plain_twin.step(x)
                assert_same(plain, plain_twin, ("plain slot", step))
            else:
                twins[i].step(x)
                assert_same(members[i], twins[i], ("slot", i, step))
                assert members[i].smp.chosen() == twins[i].smp.chosen() == step + 1
    assert plain.smp.chosen() == 0
    table.close()
    for l in members + twins + [plain, plain_twin]:
        l.close()
