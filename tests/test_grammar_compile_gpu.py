"""GPU: bitnet_hip_grammar_compile (csrc/kernels_gramc.hip) against the numpy compiler, bitnet-rs_amd/grammar.py token_automaton, by equality: the
same class count and the same expanded function (state, token) -> next[state][token_class[token]], classes numbered by their smallest token id.
The state tile is 32 states wide and the automaton has n_states + 1 states, so n_states 31 / 32 / 33 / 65 sit on both sides of a tile boundary."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_constraint_gpu import Lane  # noqa: E402

pytestmark = pytest.mark.gpu
G = importlib.import_module("bitnet-rs_amd.grammar")
ALPHABET = b"abcd"


def random_dfa(rng, n, density=0.5):
    """transitions on four bytes only, half of them missing: most longer tokens die somewhere, many columns are all -1"""
    nx = np.full((n, 256), -1, np.int32)
    for b in ALPHABET:
        nx[:, b] = np.where(rng.random(n) < density, rng.integers(0, n, n), -1)
    return G.ByteDFA(nx, int(rng.integers(0, n)), np.flatnonzero(rng.random(n) < 0.3))


def random_vocab(rng, V):
    toks = [bytes(rng.choice(list(ALPHABET), int(rng.integers(0, 10))).tolist()) for _ in range(V)]
    if V >= 3:
        toks[1], toks[2] = bytes(rng.choice(list(ALPHABET), 300).tolist()), b""
    return toks


def compile_both(hip, dfa, toks, eos, vh=None):
    """compiles on the device, holds the result to numpy's and returns (grammar, token_class, next) of the device"""
    tc_np, nx_np, _ = G.token_automaton(dfa, toks, eos)
    g, start = G.compile_on_device(hip, dfa, vh or hip.vocab(toks), eos)
    tc, nx = g.tables()
    assert start == dfa.start and g.info() == (len(toks), dfa.n + 1, nx_np.shape[1]) and nx.shape == nx_np.shape
    assert np.array_equal(nx[:, tc], nx_np[:, tc_np])
    classes, first = np.unique(tc, return_index=True)
    assert np.array_equal(classes, np.arange(nx.shape[1])) and np.all(np.diff(first) > 0)  # numbered by smallest token id
    return g, tc, nx


@pytest.mark.parametrize("eos", [False, True])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 200])
def test_random_dfas(hip, n, V, eos):
    rng = np.random.default_rng(1000 * n + V)
    compile_both(hip, random_dfa(rng, n), random_vocab(rng, V), V // 2 if eos else None)


def test_tries_with_duplicates_and_prefixes(hip):
    dfa = G.ByteDFA.from_choices([b"yes", b"no", b"maybe", b"yesterday"])
    toks = [b"y", b"ye", b"yes", b"ye", b"s", b"terday", b"n", b"o", b"no", b"may", b"be", b"maybe", b"x", b"", b"<eos>", b"yes"]
    _, tc, _ = compile_both(hip, dfa, toks, 14)
    assert tc[1] == tc[3] and tc[2] == tc[15] and tc[1] != tc[2] and tc[12] == tc[13]  # duplicates share; a prefix does not; dead == empty


def test_planted_partitions(hip):
    """columns that differ in one state only, at either end of the state range: refinement has to look at every tile"""
    n = 70  # 71 states: tiles [0, 32), [32, 64), [64, 71)
    rng = np.random.default_rng(5)
    nx = np.full((n, 256), -1, np.int32)
    for pair, odd_state in ((b"ab", n - 1), (b"cd", 0)):
        nx[:, pair[0]] = nx[:, pair[1]] = rng.integers(0, n, n)
        nx[odd_state, pair[1]] = (nx[odd_state, pair[0]] + 1) % n
    toks = [b"a", b"b", b"c", b"d", b"zz", b"<eos>"]
    _, tc, nxt = compile_both(hip, G.ByteDFA(nx, 0, []), toks, 5)
    assert len(set(tc.tolist())) == 6 and tc[0] != tc[1] and tc[2] != tc[3]
    assert np.flatnonzero(nxt[:, tc[4]] != nxt[:, tc[5]]).tolist() == [n]  # nothing accepts: EOS and a dead token differ in the end state alone
    # 63 DFA states: the end state is the last state of the last full tile
    _, tc, _ = compile_both(hip, G.ByteDFA(nx[:63].clip(max=62), 0, []), toks, 5)
    assert tc[4] != tc[5]
    _, tc, _ = compile_both(hip, G.ByteDFA(nx, 0, [3]), [b"a"] * 50, 7)
    assert sorted(set(tc.tolist())) == [0, 1] and tc[7] == 1


def pair_dfa():
    """root --a--> P[a] --b--> Q[b] and X --a--> Y[a] --b--> Y[a], a in 0..127, b in 128..255: the column of the token (a, b) shows b at the root and
    a at X, so two-byte tokens have pairwise distinct columns; (0, 0) dies everywhere"""
    nx = np.full((2 + 3 * 128, 256), -1, np.int32)
    a, b = np.arange(128), np.arange(128, 256)
    nx[0, a], nx[1, a] = 2 + a, 258 + a
    nx[2:130, b] = 130 + np.arange(128)
    nx[258 + a[:, None], b[None, :]] = (258 + a)[:, None]
    return G.ByteDFA(nx, 0, [])


def test_pairwise_distinct_columns(hip):
    toks = [bytes([i % 128, 128 + i // 128]) for i in range(499)] + [b"\0\0"]
    _, tc, _ = compile_both(hip, pair_dfa(), toks, None)
    assert np.array_equal(tc, np.arange(500))


def test_too_many_classes_is_refused_and_the_vocab_handle_lives_on(hip, pkg):
    toks = [bytes([i % 128, 128 + i // 128]) for i in range(16384)] + [b"\0\0"]
    vh = hip.vocab(toks)
    with pytest.raises(pkg.BitNetHipError, match="16385 token classes") as e:
        hip.grammar_compile(vh, pair_dfa(), None)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.BitNetHipError, match="eos_id 16385 is outside"):
        hip.grammar_compile(vh, G.ByteDFA.from_choices([b"\1"]), len(toks))
    g, tc, _ = compile_both(hip, G.ByteDFA.from_choices([bytes([5, 128])]), toks, 0, vh)
    assert g.info()[2] == 3  # EOS, the one token the trie spells, everything else


def test_read_returns_what_create_was_given(hip):
    rng = np.random.default_rng(9)
    tc, nx = rng.integers(0, 37, 500).astype(np.uint16), rng.integers(-1, 11, (11, 37)).astype(np.int32)
    g = hip.grammar(tc, nx)
    got = g.tables()
    assert g.info() == (500, 11, 37) and np.array_equal(got[0], tc) and np.array_equal(got[1], nx)


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.0)], ids=["greedy", "seeded"])
def test_sampler_on_the_compiled_handle_follows_the_numpy_one(hip, kw):
    import torch

    rng = np.random.default_rng(12)
    dfa = G.ByteDFA.from_choices([b"abca", b"abd", b"cab", b"dd"])
    toks = [b"<eos>"] + [bytes(rng.choice(list(ALPHABET), int(rng.integers(1, 3))).tolist()) for _ in range(299)]
    tc_np, nx_np, start = G.token_automaton(dfa, toks, 0)
    a, _ = G.compile_on_device(hip, dfa, hip.vocab(toks), 0)
    b = hip.grammar(tc_np, nx_np)
    A, B = Lane(torch, hip, 300, kw, None, [1]), Lane(torch, hip, 300, kw, None, [1])
    A.smp.set_grammar(a, start)
    B.smp.set_grammar(b, start)
    picked = []
    for i in range(12):
        x = rng.standard_normal(300).astype(np.float32)
        x[0] -= 4.0  # EOS late: the text usually runs to the end of a choice first
        A.step(x)
        B.step(x)
        picked.append(int(A.tok.item()))
        assert picked[-1] == int(B.tok.item()) and A.smp.grammar_state() == B.smp.grammar_state(), i
    state, steps, viol = A.smp.grammar_state()
    assert (state, steps, viol) == (dfa.n, 12, 0) and a.walk(start, picked) == (dfa.n, 12)  # reached the end state; walk reads the device's tables
