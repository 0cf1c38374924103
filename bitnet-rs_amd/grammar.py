"""Byte-level automata compiled to the token automaton the sampler's GRAMMAR stage takes (include/bitnet_hip.h, bitnet_hip_grammar_desc).
Pure numpy, no GPU.

    dfa = ByteDFA.from_choices([b"yes", b"no", b"maybe"])
    token_class, next_table, start = token_automaton(dfa, vocab_bytes, eos_id)
    g = lib.grammar(token_class, next_table); sampler.set_grammar(g, start)

A ByteDFA is a deterministic automaton over bytes: next[n, 256] int32 (-1: no transition), a start state, a set of accepting states.
token_automaton lifts it to tokens: a token's column says where its bytes lead from every state, equal columns share a class.  A
regular-expression or JSON-schema front end would produce a ByteDFA and plug in here; none is part of this file.
"""
from __future__ import annotations

import numpy as np

MAX_STATES, MAX_CLASSES, MAX_CELLS, MAX_VOCAB = 65536, 16384, 1 << 24, 1 << 20  # the limits of bitnet_hip_grammar_create


class ByteDFA:
    """next[n, 256] int32 with -1 for "no transition", start in [0, n), accepting: the states in which the text may end."""

    def __init__(self, next, start: int, accepting):  # noqa: A002 -- the table's name in the C descriptor
        nx = np.ascontiguousarray(next, dtype=np.int32)
        if nx.ndim != 2 or nx.shape[1] != 256 or nx.shape[0] < 1:
            raise ValueError(f"ByteDFA: next must be [n, 256] with n >= 1, got shape {nx.shape}")
        n = nx.shape[0]
        if nx.min() < -1 or nx.max() >= n:
            raise ValueError(f"ByteDFA: a next entry is outside [-1, {n})")
        if not 0 <= int(start) < n:
            raise ValueError(f"ByteDFA: start {start} is outside [0, {n})")
        acc = sorted({int(s) for s in accepting})
        if acc and (acc[0] < 0 or acc[-1] >= n):
            raise ValueError(f"ByteDFA: an accepting state is outside [0, {n})")
        self.next, self.start, self.accepting, self.n = nx, int(start), frozenset(acc), n

    @classmethod
    def from_choices(cls, choices) -> "ByteDFA":
        """The trie of a list of byte strings: accepts exactly the choices."""
        choices = [bytes(c) for c in choices]
        if not choices:
            raise ValueError("ByteDFA.from_choices: no choices")
        rows, accepting = [np.full(256, -1, np.int32)], set()
        for c in choices:
            s = 0
            for b in c:
                if rows[s][b] < 0:
                    rows[s][b] = len(rows)
                    rows.append(np.full(256, -1, np.int32))
                s = int(rows[s][b])
            accepting.add(s)
        return cls(np.stack(rows), 0, accepting)

    def run(self, state: int, data: bytes) -> int:
        """the state after `data` from `state`, or -1"""
        for b in data:
            if state < 0:
                break
            state = int(self.next[state, b])
        return state


def token_automaton(dfa: ByteDFA, vocab_bytes, eos_id: int | None):
    """(token_class [vocab] uint16, next [dfa.n + 1, n_classes] int32, start) for bitnet_hip_grammar_desc.

    vocab_bytes[t] is the byte string of token t.  A token's column is where its bytes lead from every state of the DFA, or -1; a token with no
    bytes is never allowed.  eos_id (None: the vocabulary has none) is allowed exactly in accepting states and leads to an added end state,
    dfa.n, in which only it is allowed (and which it keeps).  Equal columns share a class.  ValueError when a limit of the library is exceeded.

    Cost: a dense [vocab, n_states] int32 array and one row sort of it (np.unique).  That suits tries and small DFAs -- 128 K tokens by 100
    states is 50 MB -- and not the library's limit of 65536 states; a front end with thousands of states should group tokens as it goes."""
    V, n = len(vocab_bytes), dfa.n
    if not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"token_automaton: the vocabulary must have 1..{MAX_VOCAB} tokens, got {V}")
    if eos_id is not None and not 0 <= int(eos_id) < V:
        raise ValueError(f"token_automaton: eos_id {eos_id} is outside [0, {V})")
    S = n + 1
    if S > MAX_STATES:
        raise ValueError(f"token_automaton: {S} states (the DFA's and the end state), the limit is {MAX_STATES}")
    # columns[t, s]: all tokens advance one byte at a time, vectorised over (token, state); -1 is absorbing
    cols = np.full((V, S), -1, np.int32)
    lens = np.array([len(b) for b in vocab_bytes], dtype=np.int64)
    live = np.flatnonzero(lens > 0)
    cur = np.tile(np.arange(n, dtype=np.int32), (live.size, 1))
    maxlen = int(lens.max()) if V else 0
    padded = np.zeros((live.size, maxlen), np.uint8)
    for r, t in enumerate(live):
        padded[r, :lens[t]] = np.frombuffer(bytes(vocab_bytes[t]), np.uint8)
    for k in range(maxlen):
        on = lens[live] > k
        step = dfa.next[np.maximum(cur, 0), padded[:, k][:, None]]
        step = np.where(cur >= 0, step, -1)
        cur = np.where(on[:, None], step, cur)
    cols[live, :n] = cur
    if eos_id is not None:
        e = int(eos_id)
        cols[e, :] = -1
        cols[e, sorted(dfa.accepting)] = n
        cols[e, n] = n
    uniq, inverse = np.unique(cols, axis=0, return_inverse=True)
    if uniq.shape[0] > MAX_CLASSES:
        raise ValueError(f"token_automaton: {uniq.shape[0]} token classes, the limit is {MAX_CLASSES}")
    if S * uniq.shape[0] > MAX_CELLS:
        raise ValueError(f"token_automaton: {S} states * {uniq.shape[0]} classes exceed {MAX_CELLS} table entries")
    return np.ascontiguousarray(inverse.reshape(-1), dtype=np.uint16), np.ascontiguousarray(uniq.T, dtype=np.int32), dfa.start
