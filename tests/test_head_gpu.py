"""GPU: the decode head -- final LayerNorm, f16 tied-embedding matvec, greedy pick, history and position update -- through
bitnet_hip_logits_f16_dev and bitnet_hip_logits_f16_batch_dev, against tests/head_ref.py (float64), at one hidden size per kernel instance of
launch_logits_f16 / launch_logits_f16_batch plus the extremes of the guarded instances:

    hidden   512     1024    1536          2048    2560              3584          4096    4608           8192
    batch-1  <1,4>   <2,4>   <8,2,guard>   <4,4>   <5,3> (<5,2>,     <8,2,guard>   <8,2>   <16,1,guard>   <16,1,guard>
    batched  <1,4>   <2,4>   <8,2,guard>   <4,4>   <5,4>  <5,4> by   <8,2,guard>   <8,2>   <16,1,guard>   <16,1,guard>
                                                          the switch)

a. integer inputs: every product and partial sum is an integer below 2^24, so the f32 result is exact in ANY order and is compared by value, at
   vocabularies that end inside a wave's R rows, inside a workgroup's 4 R rows, at one row, and below the grid's first sweep.
b. float inputs through the fused norm, against float64 within a derived bound (below).
c. the pick's rules on logits placed by hand, and the history / position rule.
d. the batched entry: each slot's bits against batch-1 on the same inputs (every instance; 8 x 2560 and 8 x 4608 take the raised-LDS launch), and
   against the exact integers.
e. the rows-per-wave switch (BITNET_HIP_LOGIT_ROWS = 2, 4; read once per process, hence one child process each).

The float bound, per logit v, with u = 2^-24, n = hidden, M_v = sum_k |xn_k E_vk| (xn the float64 norm):

    |got_v - want_v| <= (n / 64 + 16) * 2 u * M_v

Derivation (first order in u; block256_sum_f = xor butterfly in each wave, then (w0 + w1) + (w2 + w3)):
  mean     a thread adds n / 256 values (the first onto 0: n / 256 - 1 roundings), 6 butterfly steps, 2 across the waves, 1 division:
           |mean_f - mean| <= (n / 256 + 8) u mean|x|.  This moves every xs_k by the SAME amount dm / sigma * gamma_k: not an error relative to the
           products, so it is evaluated on the test's own inputs (head_ref.mean_shift_term: dm / sigma * |sum_k gamma_k E_vk|) rather than folded
           into a constant.  It is small beside the rest because the table's signs do not follow gamma's: the sum is O(sqrt(n)), M_v is O(n).
           Its effect on the variance is second order (the deviations sum to 0).
  xs_k     sigma^2: the squared deviations carry 2 (each deviation rounded once), the chain of n / 256 fused multiply-adds, the 8 steps of the block
           sum, the division, + eps: n / 256 + 12; sqrtf halves that and rounds once: n / 512 + 7 for the denominator.  xs_k itself: the deviation
           (1), / denom (1), * gamma_k (1): n / 512 + 10, taken as n / 512 + 11.
  dot      lane l's chain is n / 64 fused multiply-adds (each rounds once), then the 6 butterfly additions: n / 64 + 6.
  total    (n / 64 + 6 + n / 512 + 11) u M_v + the mean term.  head_ref.relative_units is the bracket; the asserted constant (n / 32 + 32) leaves
           (7 n / 512 + 15) u M_v for the mean term, and every case below asserts, on its own inputs, that the derived sum fits inside the asserted
           bound.  tests/test_head_ref.py shows that the bound still catches a dropped lane, a misread chunk and a missing mean subtraction tenfold.
A constant row normalises to exactly 0 (head_ref.float_case), M_v = 0, and the bound asks for logits equal to 0."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

HIDDENS = [512, 1024, 1536, 2048, 2560, 3584, 4096, 4608, 8192]
EPS = 1e-5
VOCAB = 1031        # prime: no multiple of any R or 4 R
SENT = -12345.0     # behind the logits: rows past the end are never stored
N_SENT = 64


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=2)
def int_inputs(hidden):
    return H.int_case(hidden, VOCAB)


def i32(torch_, v):
    return torch_.tensor(v, dtype=torch_.int32, device="cuda")


def run_head(hip, torch_, table_d, x_d, gamma_d, hidden, vocab, n_wg, pos=None, history=None, n_forced=None, want_token=True):
    """one batch-1 call on fresh buffers -> dict(logits [vocab], tail [N_SENT], token, pos, history)"""
    logits = torch_.full((vocab + N_SENT,), SENT, device="cuda")
    scratch = torch_.full((2 * n_wg,), 3e38, device="cuda")  # a partial that a workgroup failed to write would win the pick
    tok = i32(torch_, [-1]) if want_token else None
    pos_d = None if pos is None else i32(torch_, [pos])
    hist_d = None if history is None else i32(torch_, history)
    nf_d = None if n_forced is None else i32(torch_, [n_forced])
    hip.logits_f16_dev(table_d, x_d, gamma_d, EPS, hidden, vocab, logits, scratch, n_wg, token=tok, pos=pos_d, history=hist_d, n_forced=nf_d)
    torch_.cuda.synchronize()
    lg = logits.cpu().numpy()
    return dict(logits=lg[:vocab], tail=lg[vocab:], token=None if tok is None else int(tok.item()), pos=None if pos_d is None else int(pos_d.item()),
                history=None if hist_d is None else hist_d.cpu().numpy())


# ---------------------------------------------------------------- a. exact indexing
@pytest.mark.parametrize("hidden", HIDDENS)
def test_integer_head_is_exact_at_every_tail(hip, torch_, hidden):
    x, table, want = int_inputs(hidden)
    td, xd = dev(torch_, table), dev(torch_, x)
    # 1: one row; 37: inside the first wave sweep of 40 workgroups (most own no row), ends inside a wave's R rows; 1000 / 1031: no multiple of 4 R / of R
    for vocab in (1, 37, 1000, VOCAB):
        for n_wg in (1, 40, 300):  # 300 partials: k_argmax_final's 256 threads take a second stride
            got = run_head(hip, torch_, td, xd, None, hidden, vocab, n_wg)
            tag = (hidden, vocab, n_wg)
            assert np.array_equal(got["logits"], want[:vocab]), (tag, np.flatnonzero(got["logits"] != want[:vocab])[:8])
            assert np.all(got["tail"] == SENT), tag
            assert got["token"] == H.pick(want[:vocab]), tag
    # a distinctive last row that holds the maximum: rows past the end re-read it, and must neither be stored nor be picked
    top = (4.0 * np.sign(x)).astype(np.float16)
    for vocab in (37, VOCAB):
        td2 = td.clone()
        td2[vocab - 1] = dev(torch_, top)
        want2 = want[:vocab].copy()
        want2[vocab - 1] = 4.0 * np.abs(x).sum()
        assert np.all(want2[:vocab - 1] < want2[vocab - 1])
        for n_wg in (1, 40, 300):
            got = run_head(hip, torch_, td2, xd, None, hidden, vocab, n_wg)
            assert np.array_equal(got["logits"], want2) and np.all(got["tail"] == SENT) and got["token"] == vocab - 1, (hidden, vocab, n_wg, got["token"])


# ---------------------------------------------------------------- b. float path, fused norm
@pytest.mark.parametrize("case", H.FLOAT_CASES)
@pytest.mark.parametrize("hidden", HIDDENS)
def test_float_head_vs_f64_within_the_derived_bound(hip, torch_, hidden, case):
    vocab, n_wg = 601, 40
    x, gamma, table = H.float_case(case, hidden, vocab)
    want, mag = H.logits(x, gamma, EPS, table)
    bound = H.bound(hidden, mag)
    derived = H.relative_units(hidden) * 2.0 ** -24 * mag + H.mean_shift_term(x, gamma, EPS, table)
    assert np.all(derived <= bound)  # the derivation's two terms fit inside the asserted constant on these inputs
    got = run_head(hip, torch_, dev(torch_, table), dev(torch_, x), dev(torch_, gamma), hidden, vocab, n_wg)
    err = np.abs(got["logits"].astype(np.float64) - want)
    print(f"head {hidden} {case}: max err {err.max():.3e}, max err / bound {np.max(err / np.where(bound > 0, bound, np.inf)):.3f}, "
          f"max err / derived {np.max(err / np.where(derived > 0, derived, np.inf)):.3f}, token {got['token']} (f64 {H.pick(want)})")
    assert np.all(err <= bound), (hidden, case, int(np.argmax(err - bound)), err.max())
    assert np.all(got["tail"] == SENT)
    tok = got["token"]
    assert tok == H.pick(got["logits"])                                   # the pick is the head's own maximum, lowest index
    best = H.pick(want)
    assert want[tok] >= want[best] - (bound[tok] + bound[best])           # ... which float64 cannot tell from its own
    if case == "const":
        assert not got["logits"].any() and tok == 0                       # LN of a constant row is 0: all logits tie at 0


# ---------------------------------------------------------------- c. pick semantics, history and position
def column_case(name, vocab):
    """column 0 of the table (x is the unit vector e_0 and there is no norm: logits[v] = E[v, 0]) -> f16 [vocab]"""
    col = (-1.0 - (np.arange(vocab) % 7)).astype(np.float16)
    kind, rows = name
    if kind == "tie":
        col[list(rows)] = 5.0
    elif kind == "zeros":      # -0.0 against 0.0 is a tie: the lower index wins whichever sign it carries
        col[rows[0]], col[rows[1]] = -0.0, 0.0
    elif kind == "inf":
        col[[5, 6, 900]] = 60000.0
        col[rows[0]] = np.inf
    elif kind == "neginf":
        col[:] = -np.inf
    return col


# workgroup w, wave s of a 40-workgroup grid starts at row (4 w + s) R: the R rows of one wave, two waves, two workgroups, a second sweep of the grid,
# and pairs whose LOWER index is met later in launch order
PICK_CASES = [("tie", (2, 3)), ("tie", (1, 5)), ("tie", (3, 17)), ("tie", (1030, 40)), ("tie", (700, 20, 21)), ("tie", (1029, 1030)), ("tie", (0, 1030)),
              ("zeros", (4, 10)), ("zeros", (10, 4)), ("inf", (777,)), ("inf", (1030,)), ("neginf", ())]


@pytest.mark.parametrize("hidden", [512, 1536, 2560, 4608])  # R = 4, 2 (guarded), 3, 1 (guarded)
def test_pick_rules_on_placed_logits(hip, torch_, hidden):
    vocab, n_wg = VOCAB, 40
    x = np.zeros(hidden, np.float32)
    x[0] = 1.0
    xd = dev(torch_, x)
    td = torch_.zeros((vocab, hidden), dtype=torch_.float16, device="cuda")
    for name in PICK_CASES:
        col = column_case(name, vocab)
        td[:, 0] = dev(torch_, col)
        got = run_head(hip, torch_, td, xd, None, hidden, vocab, n_wg)
        want = col.astype(np.float32)
        assert np.array_equal(got["logits"], want), (hidden, name, got["logits"][:8])
        assert got["token"] == H.pick(want), (hidden, name, got["token"])
        if name[0] == "tie":
            assert got["token"] == min(name[1])
        if name[0] == "inf":
            assert got["token"] == name[1][0]
    # a NaN in the row: every logit NaN, NaN counts as -inf, nothing is above -inf -> token 0
    td[:, 0] = dev(torch_, column_case(("tie", (9,)), vocab))
    xn = x.copy()
    xn[hidden - 3] = np.nan
    for gamma in (None, dev(torch_, np.ones(hidden, np.float32))):
        got = run_head(hip, torch_, td, dev(torch_, xn), gamma, hidden, vocab, n_wg)
        assert np.isnan(got["logits"]).all() and got["token"] == 0 and np.all(got["tail"] == SENT), hidden


def test_token_history_and_position_rule(hip, torch_):
    hidden, vocab, n_wg = 512, 37, 40
    x, table, want = H.int_case(hidden, vocab, seed=1)
    td, xd = dev(torch_, table), dev(torch_, x)
    tok = H.pick(want)
    hist = [-7] * 8
    run = lambda **kw: run_head(hip, torch_, td, xd, None, hidden, vocab, n_wg, **kw)
    got = run(history=hist)                                   # a token and no position: the token is written, nothing advances
    assert got["token"] == tok and list(got["history"]) == hist
    got = run(pos=3, want_token=False)                        # a position alone: it advances, nothing else is written
    assert got["pos"] == 4 and got["token"] is None
    got = run(pos=3, history=hist)                            # greedy: history[p + 1] = token
    assert (got["pos"], list(got["history"])) == (4, list(H.advance(3, tok, hist)[1])) and got["history"][4] == tok
    got = run(pos=3, history=hist, want_token=False)          # the history is written without a token pointer too
    assert got["pos"] == 4 and got["history"][4] == tok
    for n_forced in (6, 5, 4, 3, 0):                          # 5: p + 1 == n_forced - 1 keeps the history; 4: p + 1 == n_forced writes it
        got = run(pos=3, history=hist, n_forced=n_forced)
        p, h = H.advance(3, tok, hist, n_forced=n_forced)
        assert got["pos"] == p == 4 and list(got["history"]) == list(h) and got["token"] == tok, n_forced
        assert (got["history"][4] == tok) == (n_forced <= 4)


# ---------------------------------------------------------------- d. batched entry
def ptr_table(torch_, tensors):
    return torch_.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch_.int64, device="cuda")


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint8)


def batch_vs_one(hip, torch_, td, xs, gamma_d, hidden, vocab, n_wg, roles):
    """roles[b]: "greedy" (token, position, history), "forced" (the same at a forced position), "logits" (no token, no position), "idle" (no logits
    pointer).  Runs the batched entry and batch-1 per slot on private buffers -> (batched, batch-1) buffer dicts; asserts what an idle slot keeps."""
    n_seq, max_pos = len(roles), 16
    p0 = [3 + b for b in range(n_seq)]
    forced = [p0[b] + 3 if roles[b] == "forced" else 0 for b in range(n_seq)]
    mk = lambda: dict(pos=[i32(torch_, [p]) for p in p0], hist=[i32(torch_, [-7] * max_pos) for _ in range(n_seq)], nf=[i32(torch_, [f]) for f in forced],
                      tok=[i32(torch_, [-1]) for _ in range(n_seq)], logits=[torch_.full((vocab + N_SENT,), SENT, device="cuda") for _ in range(n_seq)])
    one, bat = mk(), mk()
    x = dev(torch_, xs)
    for b, role in enumerate(roles):
        if role == "idle":
            continue
        kw = {} if role == "logits" else dict(token=one["tok"][b], pos=one["pos"][b], history=one["hist"][b], n_forced=one["nf"][b])
        hip.logits_f16_dev(td, x[b].clone(), gamma_d, EPS, hidden, vocab, one["logits"][b], torch_.full((2 * n_wg,), 3e38, device="cuda"), n_wg, **kw)
    picks = lambda key: ptr_table(torch_, [bat[key][b] if roles[b] in ("greedy", "forced") else None for b in range(n_seq)])
    lt = ptr_table(torch_, [None if roles[b] == "idle" else bat["logits"][b] for b in range(n_seq)])
    hip.logits_f16_batch_dev(td, x, gamma_d, EPS, hidden, vocab, n_seq, lt, torch_.full((2 * n_wg * n_seq,), 3e38, device="cuda"), n_wg, token_ptrs=picks("tok"),
                             pos_ptrs=picks("pos"), history_ptrs=picks("hist"), n_forced_ptrs=picks("nf"))
    torch_.cuda.synchronize()
    for b, role in enumerate(roles):
        for key in ("logits", "tok", "pos", "hist"):
            assert np.array_equal(bits(bat[key][b]), bits(one[key][b])), (hidden, n_seq, b, role, key)
        lg = bat["logits"][b].cpu().numpy()
        assert np.all(lg[vocab:] == SENT)
        p, t, h = int(bat["pos"][b].item()), int(bat["tok"][b].item()), bat["hist"][b].cpu().numpy()
        if role in ("idle", "logits"):
            assert p == p0[b] and t == -1 and np.all(h == -7), (b, role)
            assert np.all(lg[:vocab] == SENT) == (role == "idle")
        else:
            assert p == p0[b] + 1 and t == H.pick(lg[:vocab]) and (h[p] == t) == (role == "greedy") and np.sum(h != -7) == (role == "greedy"), (b, role)
    return bat, one


def batch_sizes(hidden):
    return [1, 8] if 8 * hidden * 4 <= 152 * 1024 else [1, 4]  # 8 slots up to hidden 4608 (144 KiB); 4 at 8192 (128 KiB)


ROLES8 = ["greedy", "greedy", "forced", "logits", "greedy", "idle", "greedy", "greedy"]


@pytest.mark.parametrize("hidden", HIDDENS)
def test_batched_head_bits_equal_batch1_and_the_exact_integers(hip, torch_, hidden):
    vocab, n_wg = VOCAB, 40
    _, table, _ = int_inputs(hidden)
    td = dev(torch_, table)
    rng = np.random.default_rng(hidden)
    for n_seq in batch_sizes(hidden):  # above 64 KiB of vectors (8 x 2560 ... 8 x 4608, 4 x 8192) the launch raises the kernel's LDS limit
        roles = ROLES8[:n_seq] if n_seq == 8 else ["greedy"] * n_seq
        xs = rng.integers(-3, 4, (n_seq, hidden)).astype(np.float32)
        bat, _ = batch_vs_one(hip, torch_, td, xs, None, hidden, vocab, n_wg, roles)
        for b, role in enumerate(roles):
            if role != "idle":
                want = H.int_logits(xs[b], table)
                assert np.array_equal(bat["logits"][b].cpu().numpy()[:vocab], want), (hidden, n_seq, b)
                if role != "logits":
                    assert int(bat["tok"][b].item()) == H.pick(want)


@pytest.mark.parametrize("hidden", HIDDENS)
def test_batched_head_bits_equal_batch1_through_the_norm(hip, torch_, hidden):
    """float vectors and a gamma: the batched kernel restates the compiled batch-1 arithmetic (a fused variance sum, a fused dot chain, the guarded
    instances' padding), so the bits must agree at every instance; slots differ on purpose (zeros and signed zeros in the products, a large scale,
    an offset mean, a NaN)."""
    vocab, n_wg = 601, 40
    n_seq = batch_sizes(hidden)[-1]
    rng = np.random.default_rng(hidden + 1)
    table = rng.normal(0, 1, (vocab, hidden)).astype(np.float16)
    table[rng.random((vocab, hidden)) < 0.05] = 0.0
    table[rng.random((vocab, hidden)) < 0.05] = -0.0
    table[7] = 0.0
    table[8] = -0.0
    table[9, 3], table[10, 5] = np.inf, -np.inf   # in chunk 0, which the guarded instances' padding must not read a second time
    gamma = rng.uniform(0.5, 1.5, hidden).astype(np.float32)
    xs = rng.normal(0.1, 1.0, (n_seq, hidden)).astype(np.float32)
    xs[1] *= rng.choice([0.0, 1.0, 30.0], hidden).astype(np.float32)
    xs[2] = rng.normal(3.0, 0.5, hidden)
    xs[3] *= 1e4
    if n_seq == 8:
        xs[4, hidden - 9] = np.nan
        xs[6] = 1.5
        xs[7] = -np.abs(xs[7])
    roles = ROLES8[:n_seq] if n_seq == 8 else ["greedy", "forced", "logits", "greedy"]
    for g in (dev(torch_, gamma), None):
        bat, _ = batch_vs_one(hip, torch_, dev(torch_, table), xs, g, hidden, vocab, n_wg, roles)
        lg0 = bat["logits"][0].cpu().numpy()[:vocab]
        assert np.isinf(lg0[9]) and np.isinf(lg0[10]) and np.isfinite(np.delete(lg0, [9, 10])).all(), hidden


# ---------------------------------------------------------------- e. the rows-per-wave switch
_CHILD = r"""
import importlib, json, sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
import head_ref as H
import test_head_gpu as T
x, table, want = H.int_case(2560, T.VOCAB)
got = T.run_head(hip, torch, T.dev(torch, table), T.dev(torch, x), None, 2560, T.VOCAB, 40)
print("GOT", json.dumps([bool(np.array_equal(got["logits"], want)), bool(np.all(got["tail"] == T.SENT)), got["token"], H.pick(want)]))
"""


@pytest.mark.parametrize("rows", ["2", "4"])
def test_rows_per_wave_switch_gives_the_exact_integers(rows):
    """BITNET_HIP_LOGIT_ROWS selects k_logits_f16<5, 2> / <5, 4> at hidden 2560 (1031 rows: no multiple of 2, 4, 8 or 16)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=root)], env=dict(os.environ, BITNET_HIP_LOGIT_ROWS=rows), capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    equal, tail_kept, token, want_token = json.loads([l for l in p.stdout.splitlines() if l.startswith("GOT ")][0][4:])
    assert equal and tail_kept and token == want_token, (rows, equal, tail_kept, token, want_token)
