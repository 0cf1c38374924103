"""CPU, no GPU: the restatement of the GRAMMAR stage (tests/grammar_ref.py) against a brute-force loop, the byte-level compiler
(bitnet-rs_amd/grammar.py) against walking every token's bytes from every state one by one, and the masked rows of the GPU file
(tests/grammar_cases.py) through the chain's acceptance analysis: the restatement reports every one of their draws decided."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grammar_cases as gc  # noqa: E402
import grammar_ref as gr  # noqa: E402
import sampler_chain_accept as ca  # noqa: E402
import sampler_chain_ref as cr  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def G():
    return importlib.import_module("bitnet-rs_amd.grammar")


def test_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(1)
    for case in range(40):
        S, C, V = int(rng.integers(3, 9)), int(rng.integers(1, 40)), int(rng.integers(1, 200))
        desc, single = gr.random_automaton(rng, S, C, V, float(rng.random()))
        tc, nx = desc
        assert tc.dtype == np.uint16 and nx.dtype == np.int32 and nx.shape == (S, C) and tc.max() < C and nx.min() >= -1 and nx.max() < S - 1
        x = rng.standard_normal(V).astype(F)
        x[int(rng.integers(0, V))] = np.inf
        for s in list(range(S)) + [-1, S, 1 << 20]:
            ok = [0 <= s < S and nx[s][tc[t]] >= 0 for t in range(V)]
            assert gr.allowed(desc, s).tolist() == ok
            y = gr.apply(x, desc, s)
            assert y.dtype == F and all((y[t] == x[t]) if ok[t] else (y[t] == -np.inf) for t in range(V))
        assert not gr.allowed(desc, S - 1).any()  # the empty state
        if C >= 2 and V >= 2:
            assert np.flatnonzero(gr.allowed(desc, S - 2)).tolist() == [single]  # the state that allows one token
        toks = rng.integers(-2, V + 2, size=12).tolist()
        for s0 in range(S):
            s, k = s0, 0
            for t in toks:  # brute force
                if not 0 <= t < V or nx[s][tc[t]] < 0:
                    break
                s, k = int(nx[s][tc[t]]), k + 1
            assert gr.walk(desc, s0, toks) == (s, k)


def toy_vocab(rng):
    """all 256 single bytes, about 40 multi-byte tokens (pieces of the choices among them), one empty token, and an EOS (no bytes either)"""
    multi = [b"ye", b"yes", b"es", b"no", b"may", b"maybe", b"be", b"ayb", b"yesno", b"n", b"nom", b"ma", b"ybe", b"\xc3\xa9", b"s\x00", b"noo"]
    while len(multi) < 40:
        multi.append(bytes(rng.integers(97, 123, size=int(rng.integers(2, 5))).astype(np.uint8)))
    vocab = [bytes([b]) for b in range(256)] + multi + [b""]
    eos = len(vocab)
    return vocab + [b""], eos


def test_token_automaton_against_walking_every_token_from_every_state(G):
    rng = np.random.default_rng(2)
    vocab, eos = toy_vocab(rng)
    dfa = G.ByteDFA.from_choices([b"yes", b"no", b"maybe", b"yesno"])
    tc, nx, start = G.token_automaton(dfa, vocab, eos)
    assert tc.dtype == np.uint16 and nx.dtype == np.int32 and tc.shape == (len(vocab),) and nx.shape[0] == dfa.n + 1 and start == dfa.start
    assert nx.shape[1] == len({tuple(nx[:, c]) for c in range(nx.shape[1])})  # equal columns share a class
    end = dfa.n
    for t, b in enumerate(vocab):
        for s in range(dfa.n + 1):
            if t == eos:
                want = end if (s in dfa.accepting or s == end) else -1
            elif len(b) == 0 or s == end:
                want = -1
            else:
                want = s
                for byte in b:  # one byte at a time
                    want = int(dfa.next[want, byte])
                    if want < 0:
                        break
            assert int(nx[s, tc[t]]) == want, (t, b, s)


def test_from_choices_accepts_exactly_the_choices(G):
    rng = np.random.default_rng(3)
    choices = [b"yes", b"no", b"maybe"]
    pieces = [b"y", b"e", b"s", b"n", b"o", b"m", b"a", b"b", b"ye", b"es", b"yes", b"no", b"may", b"be", b"maybe", b"x", b"yesno", b""]
    eos = len(pieces)
    vocab = pieces + [b""]
    dfa = G.ByteDFA.from_choices(choices)
    desc = G.token_automaton(dfa, vocab, eos)[:2]
    end = dfa.n
    texts = set()
    for n in range(1, 5):
        for seq in itertools.product(range(len(vocab)), repeat=n):
            if seq[-1] != eos or eos in seq[:-1]:
                continue
            s, k = gr.walk(desc, dfa.start, seq)
            if k == n:
                assert s == end
                texts.add(b"".join(vocab[t] for t in seq[:-1]))
    assert texts == set(choices)
    assert dfa.run(dfa.start, b"maybe") in dfa.accepting and dfa.run(dfa.start, b"mayb") not in dfa.accepting and dfa.run(dfa.start, b"yess") == -1
    del rng


def test_limit_errors(G):
    with pytest.raises(ValueError, match="no choices"):
        G.ByteDFA.from_choices([])
    with pytest.raises(ValueError, match=r"\[n, 256\]"):
        G.ByteDFA(np.zeros((2, 255), np.int32), 0, [])
    with pytest.raises(ValueError, match="next entry"):
        G.ByteDFA(np.full((2, 256), 2, np.int32), 0, [])
    with pytest.raises(ValueError, match="start"):
        G.ByteDFA(np.full((2, 256), -1, np.int32), 2, [])
    with pytest.raises(ValueError, match="accepting"):
        G.ByteDFA(np.full((2, 256), -1, np.int32), 0, [5])
    small = G.ByteDFA.from_choices([b"a"])
    with pytest.raises(ValueError, match="eos_id"):
        G.token_automaton(small, [b"a", b""], 2)
    with pytest.raises(ValueError, match="vocabulary"):
        G.token_automaton(small, [], None)
    # states: a chain of 65536 states and the end state exceed BITNET_HIP_GRAMMAR_MAX_STATES
    n = G.MAX_STATES
    chain = np.full((n, 256), -1, np.int32)
    chain[np.arange(n - 1), 97] = np.arange(1, n)
    with pytest.raises(ValueError, match="states"):
        G.token_automaton(G.ByteDFA(chain, 0, [n - 1]), [b"a", b""], 1)
    # classes: 16385 two-byte tokens with pairwise different columns -- from state 0 the token (hi, lo) leads to state 2 + lo, from state 1 to 2 + hi
    t = np.full((2 + 256 + 512, 256), -1, np.int32)
    t[0, :] = 2 + 256 + np.arange(256)        # 0 --hi--> A[hi]
    t[1, :] = 2 + 512 + np.arange(256)        # 1 --hi--> B[hi]
    t[2 + 256:2 + 512, :] = 2 + np.arange(256)[None, :]  # A[hi] --lo--> 2 + lo
    t[2 + 512:, :] = 2 + np.arange(256)[:, None]         # B[hi] --lo--> 2 + hi
    dfa = G.ByteDFA(t, 0, [2])
    vocab = [bytes([i >> 8, i & 255]) for i in range(G.MAX_CLASSES + 1)]
    with pytest.raises(ValueError, match="classes"):
        G.token_automaton(dfa, vocab, None)
    tc, nx, _ = G.token_automaton(dfa, vocab[:300], None)
    assert nx.shape == (t.shape[0] + 1, 300) and sorted(tc.tolist()) == list(range(300))
    # table entries: 65536 states * 257 classes (the 256 bytes, each with a column of its own, and the empty token) exceed 2^24
    n = G.MAX_STATES - 1
    fan = np.full((n, 256), -1, np.int32)
    fan[0, :] = 1 + np.arange(256)
    with pytest.raises(ValueError, match="table entries"):
        G.token_automaton(G.ByteDFA(fan, 0, [1]), [bytes([b]) for b in range(256)] + [b""], None)


def masked_cases():
    return [(v, k, name) for v in gc.MASKED_VOCABS for k in gc.MASKED_K for name in gc.MASKED_CFGS]


@pytest.mark.parametrize("vocab,k,name", masked_cases())
def test_the_masked_rows_are_decided_by_the_chain_analysis(vocab, k, name):
    """every draw of every masked row of tests/test_grammar_gpu.py: the restatement's own token is accepted and the analysis calls the draw
    decided, so the cap on undecided draws there is one the restatement meets with zero"""
    cfg, ex = gc.MASKED_CFGS[name]
    x, ids = gc.masked_row(vocab, k)
    y = gr.apply(x, gc.masked_desc(vocab, ids), 0)
    assert np.count_nonzero(y > -np.inf) == k
    surv = np.sort(y[ids])
    assert k == 1 or np.min(np.diff(surv)) >= 0.25
    ref = cr.ChainRef(*cfg, seed=11, **ex)
    hist = []
    for step in range(gc.MASKED_STEPS):
        want = ref.sample(y, hist)
        assert ref.last_path == "F"
        ok, reason = ca.accepts(ref, want)
        assert ok and not ref.last["undecided"], (vocab, k, name, step, reason)
        an = ca.analyse(ref)
        assert not an["undecided"], (vocab, k, name, step)
        assert want in ids
        hist = hist + [want]
