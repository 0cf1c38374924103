"""numpy restatement of the sampler's GRAMMAR stage (include/bitnet_hip.h, bitnet_hip_grammar_*): a token automaton in class-compressed form.

    desc = (token_class [vocab] uint16, next [n_states, n_classes] int32)
    allowed(desc, s) -> bool [vocab]        token t is allowed in state s iff next[s][token_class[t]] >= 0; a state outside the table allows nothing
    apply(x, desc, s) -> float32 row        -inf at every id that is not allowed, the rest untouched
    walk(desc, s, tokens) -> (state, taken) takes tokens while they are allowed; stops in front of the first that is not, or is out of range

A sampler WITHOUT a grammar that is given apply(x, desc, s) must do exactly what a sampler WITH the grammar in state s does on x: that
equivalence is what the GPU tests hold, bit for bit."""
import numpy as np

F = np.float32
NEG_INF = F(-np.inf)


def allowed(desc, s):
    tc, nx = desc
    if not 0 <= int(s) < nx.shape[0]:
        return np.zeros(tc.size, bool)
    return nx[int(s)][tc.astype(np.int64)] >= 0


def apply(x, desc, s):
    y = np.array(x, dtype=F, copy=True)
    y[~allowed(desc, s)] = NEG_INF
    return y


def step(desc, s, t):
    """the next state, or -1"""
    tc, nx = desc
    t = int(t)
    if not 0 <= t < tc.size or not 0 <= int(s) < nx.shape[0]:
        return -1
    return int(nx[int(s), int(tc[t])])


def walk(desc, s, tokens):
    s, k = int(s), 0
    for t in tokens:
        n = step(desc, s, t)
        if n < 0:
            break
        s, k = n, k + 1
    return s, k


def random_automaton(rng, S, C, vocab, p_ban, pinned=()):
    """A random automaton with S >= 3 states, C classes and `vocab` tokens; each (state, class) is banned with probability p_ban.  State S - 1
    allows nothing; state S - 2 allows exactly one token (which has a class of its own when C >= 2 and vocab >= 2, else the state allows one
    class); no transition leads into S - 1, so only a caller's start state or set_grammar_state puts a sampler there.  `pinned`: token ids that
    get classes of their own first (the edge ids of a launch's slices), as far as the classes go.  Returns (desc, the single token's id)."""
    assert S >= 3 and C >= 1 and vocab >= 1
    tc = rng.integers(0, C, size=vocab).astype(np.uint16)
    k = 0
    for t in pinned:
        if k < C - 1 and 0 <= t < vocab:
            tc[t] = k
            k += 1
    single = int(rng.integers(0, vocab))
    if C >= 2 and vocab >= 2:
        tc[tc == C - 1] = max(0, C - 2)  # class C - 1 belongs to the single token alone
        tc[single] = C - 1
    # every class keeps at least one token where the vocabulary is large enough: the class bitmap's last word gets used
    if vocab >= 2 * C:
        taken = set(pinned) | {single}
        free = np.array([t for t in range(vocab) if t not in taken][:C - 1], dtype=np.int64)
        tc[free] = np.arange(free.size, dtype=np.uint16)
    nx = rng.integers(0, S - 1, size=(S, C)).astype(np.int32)  # targets: any state but the empty one
    nx[rng.random((S, C)) < p_ban] = -1
    nx[S - 1, :] = -1
    nx[S - 2, :] = -1
    nx[S - 2, int(tc[single])] = int(rng.integers(0, S - 1))
    return (tc, nx), single
