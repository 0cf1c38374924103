"""GPU: the sampler's GRAMMAR stage (bitnet_hip_sampler_set_grammar, csrc/kernels_sample.hip) -- a token automaton whose state moves with every
chosen token -- held by the constraints' method, an EQUIVALENCE bit for bit, with no tolerance:

    sampler A has the grammar and samples the raw row L;
    sampler B has the same config and seed and NO grammar, and is given L' = apply(L, desc, s) (tests/grammar_ref.py), s from the restatement's walk.

At every step the two must agree in token, history, position, ChaCha20 word counter and Mirostat's mu, and A's (state, steps, violations) must be
the restatement's.  After the last step both take one common config with strong penalties, grammar off, and must go on agreeing: that holds the
per-token counts.  Banned and allowed ids sit at 0, at vocab - 1 and at both sides of a workgroup slice boundary (tests/grammar_cases.py restates
the launch geometry).  The masked rows of path F are judged by the chain's acceptance rule on sampler B alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grammar_cases as gc  # noqa: E402
import grammar_ref as gr  # noqa: E402
import sampler_chain_accept as ca  # noqa: E402
import sampler_chain_ref as cref  # noqa: E402
import test_constraint_gpu as tcg  # noqa: E402
from test_constraint_gpu import PATHS, Lane, assert_same  # noqa: E402
from test_sampler_chain_gpu import UNDECIDED_CAP_MINP, UNDECIDED_CAP_TYP  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
STEPS = 12
VOCABS = [1, 2, 63, 64, 65, 1000, 4097]
BIG = 128256
CLASS_COUNTS = [1, 31, 32, 33, 2049, 16384]


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def amax(y):
    """the greedy pick: NaN read as -inf, the lowest index of the maximum"""
    return int(np.argmax(np.where(np.isnan(y), -np.inf, y)))


_AUTOMATA = {}


def automaton(vocab, C, S=6, p_ban=0.45, seed=0):
    """one random automaton per (vocab, C, ...), made once and shared; the edge ids of the launch get classes of their own first"""
    key = (vocab, C, S, p_ban, seed)
    if key not in _AUTOMATA:
        rng = np.random.default_rng(8000 + 31 * vocab + C + seed)
        _AUTOMATA[key] = gr.random_automaton(rng, S, C, vocab, p_ban, pinned=gc.edge_ids(vocab))
    return _AUTOMATA[key]


class Model:
    """the restatement's own (state, steps, violations), moved by the tokens the device chose"""

    def __init__(self, desc, start):
        self.desc, self.s, self.steps, self.viol = desc, int(start), 0, 0

    def take(self, tok):
        n = gr.step(self.desc, self.s, tok)
        if n >= 0:
            self.s, self.steps = n, self.steps + 1
        else:
            self.viol += 1

    def words(self):
        return (self.s, self.steps, self.viol)


def equivalence(torch, hip, vocab, kw, miro, desc, start, prompt, steps=STEPS, tag="", row_list=None, constraints=None, expect_edit=True):
    """A (grammar, raw rows) against B (no grammar, rows edited by the restatement); returns (A's tokens, the model, rows the mask changed)"""
    xs = row_list or tcg.rows(vocab)
    g = hip.grammar(*desc)
    A, B = Lane(torch, hip, vocab, kw, miro, prompt), Lane(torch, hip, vocab, kw, miro, prompt)
    A.smp.set_grammar(g, start)
    if constraints:
        for l in (A, B):
            l.smp.set_constraints(**constraints)  # both stages on: the constraints run in both samplers, the grammar's bans add up in A
    m = Model(desc, start)
    toks, edited = [], 0
    for i in range(steps):
        x = xs[i % len(xs)]
        assert A.smp.grammar_state() == m.words(), (tag, "before step", i)
        y = gr.apply(x, desc, m.s)
        edited += y.tobytes() != x.tobytes()
        A.step(x)
        B.step(y)
        assert_same(A, B, (tag, vocab, "step", i))
        t = int(A.tok.item())
        m.take(t)
        toks.append(t)
    assert A.smp.grammar_state() == m.words() and B.smp.grammar_state() == (-1, 0, 0), tag
    assert m.steps + m.viol == steps
    if expect_edit:
        assert edited > 0, (tag, "the grammar never changed a row")
    # the counts both hold, through what they do: one common config with strong penalties, grammar (and constraints) off
    A.smp.set_grammar(None)
    for s in (A, B):
        s.smp.set_constraints()
        s.smp.set_mirostat(None)
        s.smp.configure(0.0, 0, 1.0, 1.7, 5, frequency_penalty=0.9, presence_penalty=0.3)
    for i in range(3):
        A.step(xs[0])
        B.step(xs[0])
        assert_same(A, B, (tag, vocab, "counts probe", i))
    assert A.smp.grammar_state() == (-1, 0, 0)
    A.close()
    B.close()
    g.close()
    return toks, m, edited


def classes_for(vocab):
    return max(1, min(33, vocab))


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("path", list(PATHS))
def test_grammar_equals_no_grammar_on_the_edited_row(hip, torch_, path, vocab):
    kw, miro = PATHS[path]
    desc, single = automaton(vocab, classes_for(vocab))
    S = desc[1].shape[0]
    for start in (0, S - 2):  # a random state, and the state that allows one token
        toks, m, _ = equivalence(torch_, hip, vocab, kw, miro, desc, start, tcg.prompt_for(vocab), tag=(path, start), expect_edit=vocab > 2)
        if start == S - 2 and vocab >= 2 and classes_for(vocab) >= 2:
            assert toks[0] == single and m.steps >= 1  # one live entry: every path picks it


@pytest.mark.parametrize("path", ["G-repetition", "S-topk8", "F-top_p", "M-mirostat"])
def test_the_full_vocabulary(hip, torch_, path):
    kw, miro = PATHS[path]
    desc, _ = automaton(BIG, 2049)
    equivalence(torch_, hip, BIG, kw, miro, desc, 0, tcg.prompt_for(BIG), steps=8, tag=(path, "big"))


@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_class_counts_across_the_bitmap_words(hip, torch_, C):
    """the state's class bitmap: one word, exactly one word, one bit into the second, many words, the maximum"""
    V = 4097 if C < 2049 else 40000
    desc, _ = automaton(V, C, S=4)
    assert int(desc[0].max()) == C - 1  # the last class is in use
    for path in ("G-repetition", "F-top_p"):
        kw, miro = PATHS[path]
        equivalence(torch_, hip, V, kw, miro, desc, 0, tcg.prompt_for(V), steps=8, tag=(path, "classes", C), expect_edit=C > 1)


def test_edge_ids_banned_and_allowed(hip, torch_):
    """a row that carries its largest logits at the edge ids (0, vocab - 1, both sides of a slice boundary): a state that bans exactly those,
    then one that allows exactly those, under a greedy sampler whose token is read off the edited row"""
    for V in (4097, 65, BIG):
        e = gc.edge_ids(V)
        tc = np.zeros(V, np.uint16)
        tc[e] = 1
        desc = (tc, np.array([[1, -1], [-1, 1]], np.int32))  # state 0 bans the edge ids and moves to state 1, which allows only them
        x = np.array(tcg.rows(V)[0])
        x[e] = (20.0 + 0.25 * np.arange(len(e))).astype(F)  # the edge ids carry the largest logits, whatever the vocabulary
        assert amax(x) in e and amax(gr.apply(x, desc, 0)) not in e and amax(gr.apply(x, desc, 1)) in e
        toks, m, edited = equivalence(torch_, hip, V, dict(temperature=0.0), None, desc, 0, [3], steps=4, row_list=[x], tag=("edges", V))
        assert toks[0] not in e and all(t in e for t in toks[1:]) and m.words() == (1, 4, 0) and edited == 4
        for path in ("S-topk8", "F-temperature"):
            kw, miro = PATHS[path]
            toks, m, _ = equivalence(torch_, hip, V, kw, miro, desc, 0, [3], steps=6, tag=("edges", path, V))
            assert toks[0] not in e and all(t in e for t in toks[1:])


@pytest.mark.parametrize("path", list(PATHS))
def test_the_empty_state(hip, torch_, path):
    """a state that allows nothing: one violation per step, the state stays, the token is B's on the all -inf row"""
    kw, miro = PATHS[path]
    V = 1000
    desc, _ = automaton(V, 33)
    S = desc[1].shape[0]
    assert np.all(gr.apply(tcg.rows(V)[0], desc, S - 1) == -np.inf)
    toks, m, _ = equivalence(torch_, hip, V, kw, miro, desc, S - 1, [3, 4], steps=4, tag=(path, "empty"))
    assert m.words() == (S - 1, 0, 4)


def test_forced_positions_do_not_move_the_state(hip, torch_):
    V = 1000
    desc, _ = automaton(V, 33)
    g = hip.grammar(*desc)
    A = Lane(torch_, hip, V, dict(temperature=0.8, top_k=8), None, [1, 2, 3, 4])
    A.pos.fill_(-1)  # the prompt of 4 is consumed through the sampler: positions 0..3 are forced
    A.smp.set_grammar(g, 0)
    x = tcg.rows(V)[0]
    m = Model(desc, 0)
    for i in range(8):
        A.step(x)
        t = int(A.tok.item())
        if i < 4:
            assert t == i + 1 and A.smp.grammar_state() == (0, 0, 0), i  # forced: the prompt token, nothing moves
        else:
            assert gr.allowed(desc, m.s)[t] or not gr.allowed(desc, m.s).any()
            m.take(t)
            assert A.smp.grammar_state() == m.words(), i
    assert m.steps + m.viol == 4 and A.smp.draws() == 4
    A.close()
    g.close()


def test_reset_and_set_grammar_state(hip, pkg, torch_):
    V = 1000
    desc, single = automaton(V, 33)
    S = desc[1].shape[0]
    g = hip.grammar(*desc)
    A = Lane(torch_, hip, V, dict(temperature=0.0), None, [1])
    A.smp.set_grammar(g, 2)
    x = tcg.rows(V)[0]
    m = Model(desc, 2)
    for _ in range(3):
        A.step(x)
        m.take(int(A.tok.item()))
    assert A.smp.grammar_state() == m.words() and m.steps + m.viol == 3
    A.smp.set_grammar_state(S - 2)  # the state word alone: the counters stay
    assert A.smp.grammar_state() == (S - 2, m.steps, m.viol)
    A.step(x)
    assert int(A.tok.item()) == single
    for other in ("configure", "mirostat", "constraints"):  # the other setters leave all of it alone
        before = A.smp.grammar_state()
        if other == "configure":
            A.smp.configure(0.9, 0, 1.0, 1.0, 3)
        elif other == "mirostat":
            A.smp.set_mirostat(4.0, 0.2)
            A.smp.set_mirostat(None)
        else:
            A.smp.set_constraints(bias={5: -1.0})
            A.smp.set_constraints()
        assert A.smp.grammar_state() == before, other
        A.pos.fill_(0)
        A.step(x)  # and the stage is still on: the token is allowed from the state before
        assert gr.allowed(desc, before[0])[int(A.tok.item())] or not gr.allowed(desc, before[0]).any(), other
    A.smp.reset()  # back to the bound start state, counters 0
    assert A.smp.grammar_state() == (2, 0, 0)
    A.close()
    g.close()


def test_grammar_and_constraints_both_on(hip, torch_):
    V = 4097
    desc, _ = automaton(V, 33)
    name, cfg = tcg.configs(V)[0]
    for path in ("G-additive", "S-topk8", "F-top_p", "M-mirostat"):
        kw, miro = PATHS[path]
        # the constraints run in both samplers (their own suite holds them); the grammar's bans add up in A and are edited into B's rows
        equivalence(torch_, hip, V, kw, miro, desc, 0, tcg.prompt_for(V), constraints=cfg, tag=(path, "both"))


def test_a_captured_graph_follows_set_grammar(hip, torch_):
    """four launches captured once with the grammar off; replayed off, under a grammar, under a second handle, and off again -- each time the
    words an eager twin leaves"""
    torch = torch_
    V = 4097
    kw = dict(temperature=0.8, top_p=0.9, repetition_penalty=1.1)
    x = tcg.rows(V)[0]
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
    d1, d2 = automaton(V, 33)[0], automaton(V, 2049, S=5, seed=1)[0]
    g1, g2 = hip.grammar(*d1), hip.grammar(*d2)
    R = Lane(torch, hip, V, kw, None, [0, 4096])  # no grammar, edited rows: the restatement's lane
    R.step(x)
    for g, desc, start in ((None, None, 0), (g1, d1, 0), (g2, d2, 1), (None, None, 0)):
        for l in (G_, T_):
            l.smp.set_grammar(g, start)
        graph.replay()
        torch.cuda.synchronize()
        m = Model(desc, start) if desc else None
        for _ in range(n):
            T_.step(x)
            R.step(gr.apply(x, desc, m.s) if m else x)
            if m:
                m.take(int(R.tok.item()))
        assert_same(G_, T_, ("replay", start))
        assert_same(T_, R, ("restatement", start))
        assert G_.smp.grammar_state() == T_.smp.grammar_state() == (m.words() if m else (-1, 0, 0))
    for l in (G_, T_, R):
        l.close()
    g1.close()
    g2.close()


def test_batch_slots_share_one_handle_at_different_states(hip, torch_):
    """k_sample_batch shares the body: eight slots on ONE grammar handle, each at its own state and path, leave what sample_dev alone leaves"""
    torch = torch_
    V = 4097
    desc, _ = automaton(V, 33, S=9)
    g = hip.grammar(*desc)
    names = list(PATHS)
    members = [Lane(torch, hip, V, *PATHS[names[i]], tcg.prompt_for(V), seed=50 + i) for i in range(8)]
    twins = [Lane(torch, hip, V, *PATHS[names[i]], tcg.prompt_for(V), seed=50 + i) for i in range(8)]
    models = [Model(desc, i) for i in range(8)]
    for i in range(8):
        members[i].smp.set_grammar(g, i)
        twins[i].smp.set_grammar(g, i)
    table = hip.sample_batch(V, 8)
    for i, mb in enumerate(members):
        table.set(i, mb.smp, mb.logits, mb.tok, mb.pos, mb.hist, mb.nf)
    for step in range(8):
        x = tcg.rows(V)[step % 3]
        for mb in members:
            mb.logits.copy_(torch.from_numpy(x))
        table.launch()
        torch.cuda.synchronize()
        for i in range(8):
            twins[i].step(x)
            assert_same(members[i], twins[i], ("slot", i, step))
            models[i].take(int(members[i].tok.item()))
            assert members[i].smp.grammar_state() == twins[i].smp.grammar_state() == models[i].words(), (i, step)
    assert len({mm.s for mm in models}) > 1
    table.close()
    for l in members + twins:
        l.close()
    g.close()


@pytest.mark.parametrize("path", ["G-repetition", "S-topk8", "F-top_p", "M-mirostat"])
def test_sample_host_is_list_defined(hip, path):
    """bitnet_hip_sample_host under a grammar == apply(walk(start, the list)), then the plain sample_host; the device words are left alone"""
    kw, miro = PATHS[path]
    V = 4097
    desc, _ = automaton(V, 33)
    g = hip.grammar(*desc)
    A, B = hip.sampler(V, seed=9, **kw), hip.sampler(V, seed=9, **kw)
    for s in (A, B):
        if miro:
            s.set_mirostat(*miro)
    A.set_grammar(g, 1)
    gen = []
    for i in range(STEPS):
        x = tcg.rows(V)[i % 3]
        s, taken = gr.walk(desc, 1, gen)
        assert g.walk(1, gen) == (s, taken)
        a = A.sample_host(x, gen)
        b = B.sample_host(gr.apply(x, desc, s), gen)
        assert a == b and A.draws() == B.draws() and A.mirostat_state() == B.mirostat_state(), (path, i, a, b)
        gen = gen + [a]
        if i == 7:
            gen = gen + [V + 3]  # a token outside the vocabulary: the walk stops in front of it, and the state stays there
    assert A.grammar_state() == (1, 0, 0)  # the state word and the counters are the device path's
    A.close()
    B.close()
    g.close()


def test_destroy_order(hip, torch_):
    """destroy the handle while bound, launch, unbind, launch with the grammar off; and a handle bound to two samplers outlives the first"""
    V = 1000
    desc, single = automaton(V, 33)
    S = desc[1].shape[0]
    x = tcg.rows(V)[0]
    g = hip.grammar(*desc)
    A = Lane(torch_, hip, V, dict(temperature=0.0), None, [1])
    B = Lane(torch_, hip, V, dict(temperature=0.0), None, [1])
    A.smp.set_grammar(g, S - 2)
    B.smp.set_grammar(g, S - 2)
    g.close()  # bound twice: takes effect when the last sampler lets go
    A.step(x)
    assert int(A.tok.item()) == single
    A.smp.set_grammar(None)
    A.step(x)
    assert int(A.tok.item()) == amax(x) and A.smp.grammar_state() == (-1, 0, 0)
    B.step(x)  # still bound through B
    assert int(B.tok.item()) == single
    B.close()  # the sampler's destruction is the last unbinding
    A.step(x)
    assert int(A.tok.item()) == amax(x)
    A.close()
    assert g.walk(S - 2, [single])[1] == 1  # the descriptor outlives the handle


def test_refusals_that_need_the_vocabulary_change_nothing(hip, pkg, torch_):
    V = 1000
    desc, single = automaton(V, 33)
    S = desc[1].shape[0]
    x = tcg.rows(V)[0]
    g = hip.grammar(*desc)
    other = hip.grammar(*automaton(4097, 33)[0])
    A = Lane(torch_, hip, V, dict(temperature=0.0), None, [1])
    A.smp.set_grammar(g, S - 2)
    for bad in (lambda: A.smp.set_grammar(other, 0), lambda: A.smp.set_grammar(g, S), lambda: A.smp.set_grammar(g, -1),
                lambda: A.smp.set_grammar_state(S), lambda: A.smp.set_grammar_state(-1)):
        with pytest.raises(pkg.BitNetHipError) as e:
            bad()
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT
        assert A.smp.grammar_state() == (S - 2, 0, 0)
    A.step(x)
    assert int(A.tok.item()) == single  # the grammar in force is still the first one, at its state
    P = Lane(torch_, hip, V, dict(temperature=0.0), None, [1])
    with pytest.raises(pkg.BitNetHipError, match="no grammar is bound"):
        P.smp.set_grammar_state(0)
    for l in (A, P):
        l.close()
    g.close()
    other.close()


def masked_cases():
    return [(v, name) for v in gc.MASKED_VOCABS for name in gc.MASKED_CFGS]


@pytest.mark.parametrize("vocab,name", masked_cases())
def test_masked_rows_on_path_f(hip, torch_, vocab, name):
    """rows that are -inf everywhere but k survivors: A (grammar, raw row) equals B (edited row) bit for bit, and B alone is judged by the chain's
    acceptance rule against the numpy ChainRef; undecided draws stay under the caps of tests/test_sampler_chain_gpu.py (the CPU file shows the
    restatement needs none)"""
    cfg, ex = gc.MASKED_CFGS[name]
    kw = dict(temperature=cfg[0], top_k=cfg[1], top_p=cfg[2], repetition_penalty=cfg[3], **ex)
    calls = undecided = 0
    for k in gc.MASKED_K:
        x, ids = gc.masked_row(vocab, k)
        desc = gc.masked_desc(vocab, ids)
        y = gr.apply(x, desc, 0)
        g = hip.grammar(*desc)
        A, B = Lane(torch_, hip, vocab, kw, None, [], seed=11), Lane(torch_, hip, vocab, kw, None, [], seed=11)
        A.smp.set_grammar(g, 0)
        ref = cref.ChainRef(*cfg, seed=11, **ex)
        hist = []
        for step in range(gc.MASKED_STEPS):
            A.step(x)
            B.step(y)
            assert_same(A, B, (name, vocab, k, step))
            got = int(B.tok.item())
            want = ref.sample(y, hist)
            ok, reason = ca.accepts(ref, got)
            print(f"masked {name} V={vocab} k={k} step={step}: want {want} got {got} undecided {ref.last['undecided']}")
            assert ok, (name, vocab, k, step, reason)
            calls += 1
            undecided += bool(ref.last["undecided"])
            hist = hist + [got]
        assert A.smp.grammar_state() == (0, gc.MASKED_STEPS, 0) and B.smp.draws() == ref.rng.draws
        A.close()
        B.close()
        g.close()
    cap = UNDECIDED_CAP_TYP if "typical" in name else UNDECIDED_CAP_MINP
    print(f"masked {name} V={vocab}: calls {calls} undecided {undecided} cap {cap * calls}")
    assert undecided <= cap * calls
