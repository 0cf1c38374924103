"""GPU: Mirostat v2 on the device (bitnet_hip_sampler_set_mirostat, csrc/kernels_sample.hip mirostat_finish) against the numpy restatement
(tests/mirostat_ref.py), call by call through the rule of tests/mirostat_accept.py, over the seeded inputs of tests/mirostat_cases.py.

Every call is judged from the mu the device held before it, read back, and from the sampler's word counter before and after: no draw is left
out of the rule, and state cannot drift between the two sides.  Per case at most 1/8 of the draws may be loose (ambiguous mass above 1e-4 of
the kept mass).  The fallback's token (the highest index of the maximum), its unchanged word counter, the edge rows, a forced position, reset,
switching off, a captured graph across set_mirostat and bitnet_hip_sample_host are held here too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirostat_accept as ma  # noqa: E402
import mirostat_cases as mc  # noqa: E402
import mirostat_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def make(hip, case):
    """a device sampler and its restatement for a case, Mirostat on"""
    smp = hip.sampler(case["vocab"], case["temperature"], 0, 1.0, case["repetition_penalty"], seed=case["seed"],
                      frequency_penalty=case["frequency_penalty"], presence_penalty=case["presence_penalty"])
    smp.set_mirostat(case["tau"], case["eta"])
    return smp, mr.MirostatRef(**mc.ref_kwargs(case))


class Judged:
    """one device sampler against its restatement: `call(x, run)` reads the state, lets `run()` make one device call (-> token), reads the
    state again and judges the call from the device's own mu_before and word counter"""

    def __init__(self, smp, ref, tag):
        self.smp, self.ref, self.tag = smp, ref, tag
        self.hist, self.calls, self.draws, self.loose, self.fallbacks = [], 0, 0, 0, 0

    def call(self, x, run, generated=None):
        mu_b, fb_b = self.smp.mirostat_state()
        d_b = self.smp.draws()
        tok = int(run())
        mu_a, fb_a = self.smp.mirostat_state()
        d_a = self.smp.draws()
        self.ref.rng.draws = d_b
        self.ref.sample(x, self.hist if generated is None else generated, mu=F(mu_b))
        rec = self.ref.last
        v = ma.judge(rec, ma.u_of(self.ref.rng, d_b), tok, F(mu_a), d_a - d_b)
        print(f"  {self.tag} call {self.calls}: token {tok} (restatement {rec['token']}) mu {mu_b!r} -> {mu_a!r} words {d_a - d_b}: {v['reason']}")
        assert v["ok"], (self.tag, self.calls, v["reason"])
        assert fb_a - fb_b == (1 if v["mode"] == "fallback" else 0), (self.tag, self.calls, fb_b, fb_a)
        self.calls += 1
        self.draws += v["mode"] == "draw"
        self.fallbacks += v["mode"] == "fallback"
        self.loose += bool(v["loose"])
        self.hist = self.hist + [tok]
        return tok, v

    def cap(self):
        assert self.loose <= mc.LOOSE_CAP * max(self.draws, 1), (self.tag, self.loose, self.draws)


def dev_runner(torch, smp, xd, tok):
    def run():
        smp.sample_dev(xd, tok)
        torch.cuda.synchronize()
        return tok.item()

    return run


@pytest.mark.parametrize("case", mc.CASES, ids=[c["id"] for c in mc.CASES])
def test_32_chained_calls_pass_the_rule(hip, torch_, case):
    torch = torch_
    x = mc.row(case)
    smp, ref = make(hip, case)
    xd = torch.from_numpy(x).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    j = Judged(smp, ref, case["id"])
    assert smp.mirostat_state() == (float(F(2) * F(case["tau"])), 0)
    for _ in range(case["steps"]):
        j.call(x, dev_runner(torch, smp, xd, tok))
    j.cap()
    print(f"{case['id']}: {j.draws} draws ({j.loose} loose), {j.fallbacks} fallbacks")
    if case["vocab"] >= 257 and case["tau"] == 0.5 or case["vocab"] >= 32000 and case["tau"] == 3.0:
        assert j.fallbacks == case["steps"] and smp.draws() == 0 and smp.mirostat_state()[1] == case["steps"]
    if case["vocab"] >= 257 and case["tau"] == 0.5:
        assert smp.mirostat_state()[0] < 0  # mu runs negative
    smp.close()


TIES = [("different-slices-and-the-last-chunk", 4099, [10, 900, 2500, 4098], 4098), ("the-last-of-three-slices", 4099, [10, 900, 2500], 2500),
        ("inside-one-slice", 4099, [3, 400, 801], 801), ("one-chunk", 257, [0, 128, 255], 255)]


@pytest.mark.parametrize("name,vocab,where,want", TIES, ids=[t[0] for t in TIES])
def test_the_fallback_takes_the_highest_index_and_draws_no_word(hip, torch_, name, vocab, where, want):
    torch = torch_
    case = dict(vocab=vocab, tau=0.5, eta=0.1, temperature=1.0, seed=11, **mc.PEN_OFF)
    x = mc.tie_row(vocab, where)
    smp, ref = make(hip, case)
    xd = torch.from_numpy(x).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    j = Judged(smp, ref, name)
    for _ in range(4):
        got, v = j.call(x, dev_runner(torch, smp, xd, tok))
        assert got == want and v["mode"] == "fallback" and v["decided"]
    assert smp.draws() == 0 and smp.mirostat_state()[1] == 4
    smp.close()


EDGES = mc.edge_rows()


@pytest.mark.parametrize("name,x,temperature", EDGES, ids=[e[0] for e in EDGES])
def test_edge_rows(hip, torch_, name, x, temperature):
    """all -inf, all NaN, +inf entries, a single finite entry, a temperature small enough to overflow x / T: first with mu high (a draw), then
    with mu low (the fallback: the highest index of the maximum)"""
    torch = torch_
    vocab = x.size
    xd = torch.from_numpy(x).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    for tau, mode in ((5.0, "draw"), (2.0, "fallback")):
        case = dict(vocab=vocab, tau=tau, eta=0.1, temperature=temperature, seed=21, **mc.PEN_OFF)
        smp, ref = make(hip, case)
        j = Judged(smp, ref, f"{name}-tau{tau}")
        for i in range(4):
            got, v = j.call(x, dev_runner(torch, smp, xd, tok))
            assert v["decided"]
            if name == "single-finite":
                assert got == 1234 and v["mode"] == "draw"  # surprise 0 <= mu at either tau; mu' = mu + eta * tau bit for bit (the rule)
            elif i == 0:
                assert v["mode"] == mode, (name, tau, v["mode"])  # ln 2500 = 7.8 against mu = 10, then against mu = 4
            if v["mode"] == "fallback" and name in ("all-neg-inf", "all-nan"):
                assert got == vocab - 1
            if v["mode"] == "fallback" and name == "pos-inf":
                assert got == vocab - 300
        smp.close()


def test_a_forced_position_moves_nothing(hip, torch_):
    torch = torch_
    case = dict(vocab=1025, tau=5.0, eta=0.1, temperature=0.7, seed=31, **mc.PEN_ON)
    smp, _ = make(hip, case)
    xd = torch.from_numpy(mc.row(dict(case, sigma=2.0))).cuda()
    tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = torch.tensor([7, 8, 9, 10, -1, -1, -1, -1], dtype=torch.int32, device="cuda")
    nf = torch.tensor([4], dtype=torch.int32, device="cuda")
    before = smp.mirostat_state()
    for want in (8, 9, 10):
        smp.sample_dev(xd, tok, pos, hist, nf)
        torch.cuda.synchronize()
        assert tok.item() == want and smp.mirostat_state() == before and smp.draws() == 0
    smp.sample_dev(xd, tok, pos, hist, nf)  # position 4 is free: this one samples
    torch.cuda.synchronize()
    assert pos.item() == 4 and hist[4].item() == tok.item() and smp.mirostat_state() != before and smp.draws() == 1
    smp.close()


def test_refusals_leave_the_state_unchanged(hip, pkg, torch_):
    torch = torch_
    smp = hip.sampler(1000, 0.8, 40, 1.0, 1.0, seed=1)
    for kw in (dict(top_k=40), dict(top_p=0.9), dict(min_p=0.05), dict(typical_p=0.9), dict(temperature=0.0)):
        cfg = dict(temperature=0.8, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0)
        cfg.update(kw)
        smp.configure(cfg["temperature"], cfg["top_k"], cfg["top_p"], 1.0, 1, min_p=cfg["min_p"], typical_p=cfg["typical_p"])
        with pytest.raises(pkg.BitNetHipError, match="Mirostat needs") as e:
            smp.set_mirostat(5.0, 0.1)
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT and smp.mirostat_state() == (0.0, 0)
    smp.configure(0.8, 0, 1.0, 1.0, 1)
    smp.set_mirostat(5.0, 0.1)
    xd = torch.from_numpy(mc.row(dict(vocab=1000, sigma=2.0, seed=4))).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    smp.sample_dev(xd, tok)
    torch.cuda.synchronize()
    state = smp.mirostat_state()
    assert state[0] != 10.0
    for bad in ((float("nan"), 0.1), (0.0, 0.1), (5.0, -1.0), (float("inf"), 0.1), (5.0, float("inf"))):
        with pytest.raises(pkg.BitNetHipError):
            smp.set_mirostat(*bad)
        assert smp.mirostat_state() == state
    for kw in (dict(top_k=40), dict(top_p=0.9), dict(min_p=0.05), dict(typical_p=0.9), dict(temperature=0.0)):  # configure, while it is on
        cfg = dict(temperature=0.8, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0)
        cfg.update(kw)
        with pytest.raises(pkg.BitNetHipError, match="Mirostat needs"):
            smp.configure(cfg["temperature"], cfg["top_k"], cfg["top_p"], 1.0, 1, min_p=cfg["min_p"], typical_p=cfg["typical_p"])
        assert smp.mirostat_state() == state and smp.draws() == 1  # nothing was copied: the word counter is where it was
    smp.configure(0.7, 0, 1.0, 1.2, 9, frequency_penalty=0.1)  # a config it takes leaves mu alone
    assert smp.mirostat_state() == state and smp.draws() == 0
    smp.reset()
    assert smp.mirostat_state() == (10.0, 0)
    smp.close()


@pytest.mark.parametrize("top_k", [0, 40])
def test_switched_on_and_off_again_is_a_sampler_that_never_was(hip, torch_, top_k):
    torch = torch_
    vocab = 4099
    x = mc.row(dict(vocab=vocab, sigma=2.0, seed=8))
    xd = torch.from_numpy(x).cuda()
    a, b = hip.sampler(vocab, 0.8, 0, 1.0, 1.1, seed=5), hip.sampler(vocab, 0.8, top_k, 1.0, 1.1, seed=5)
    ta, tb = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    a.set_mirostat(5.0, 0.1)
    for _ in range(3):
        a.sample_dev(xd, ta)
    torch.cuda.synchronize()
    assert a.mirostat_state()[0] != 10.0
    a.reset()
    assert a.mirostat_state() == (10.0, 0) and a.draws() == 0  # reset restores mu
    a.set_mirostat(None)
    assert a.mirostat_state() == (0.0, 0)
    a.configure(0.8, top_k, 1.0, 1.1, 5)  # with Mirostat off the truncation stages are free again
    for i in range(16):
        a.sample_dev(xd, ta)
        b.sample_dev(xd, tb)
        torch.cuda.synchronize()
        assert ta.item() == tb.item(), (top_k, i)
    assert a.draws() == b.draws() == 16 and a.mirostat_state() == b.mirostat_state() == (0.0, 0)
    a.close()
    b.close()


def test_a_captured_chain_follows_set_mirostat(hip, torch_):
    """16 launches captured once and replayed: the tokens, the final mu, the fallback count and the word counter are those of an eager twin
    whose 16 calls each pass the rule (the kernel is deterministic: the same bits).  set_mirostat with another tau, then a second replay of the
    same graph: it follows without re-capture."""
    torch = torch_
    case = dict(vocab=4099, tau=5.0, eta=0.1, temperature=0.7, seed=41, sigma=2.0, **mc.PEN_ON)
    x = mc.row(case)
    xd = torch.from_numpy(x).cuda()
    g_smp, _ = make(hip, case)
    t_smp, ref = make(hip, case)
    n = 16
    lanes = [dict(tok=torch.full((1,), -1, dtype=torch.int32, device="cuda"), pos=torch.zeros(1, dtype=torch.int32, device="cuda"),
                  hist=torch.full((64,), -1, dtype=torch.int32, device="cuda"), nf=torch.zeros(1, dtype=torch.int32, device="cuda")) for _ in range(2)]
    G, T = lanes
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    twin = Judged(t_smp, ref, "twin")

    def twin_call():
        def run():
            t_smp.sample_dev(xd, T["tok"], T["pos"], T["hist"], T["nf"])
            torch.cuda.synchronize()
            return T["tok"].item()

        return twin.call(x, run)

    with torch.cuda.stream(stream):
        g_smp.sample_dev(xd, G["tok"], G["pos"], G["hist"], G["nf"], stream=stream.cuda_stream)  # warm-up: one real call
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(n):
                g_smp.sample_dev(xd, G["tok"], G["pos"], G["hist"], G["nf"], stream=stream.cuda_stream)
    twin_call()
    assert torch.equal(G["hist"], T["hist"]) and g_smp.mirostat_state() == t_smp.mirostat_state()
    for tau in (None, 0.5):
        if tau is not None:  # another tau before the second replay: the graph reads the mode from device memory
            for s in (g_smp, t_smp):
                s.set_mirostat(tau, 0.2)
            ref.tau, ref.eta = F(tau), F(0.2)
        graph.replay()
        torch.cuda.synchronize()
        for _ in range(n):
            twin_call()
        assert torch.equal(G["hist"], T["hist"]) and G["pos"].item() == T["pos"].item()
        mg, mt = g_smp.mirostat_state(), t_smp.mirostat_state()
        assert F(mg[0]).tobytes() == F(mt[0]).tobytes() and mg[1] == mt[1] and g_smp.draws() == t_smp.draws()
    twin.cap()
    assert twin.fallbacks > 0 and twin.draws > 0  # tau 0.5 (mu = 1) falls back at this vocabulary, tau 5 draws
    g_smp.close()
    t_smp.close()


def test_sample_host_runs_the_same_path(hip, torch_):
    """the host-pointer drop-in: the whole generated list on every call, its own list-derived counts; mu and the stream are the sampler's"""
    case = dict(vocab=1025, tau=5.0, eta=0.1, temperature=0.7, seed=51, sigma=2.0, **mc.PEN_ON)
    x = mc.row(case)
    smp, ref = make(hip, case)
    j = Judged(smp, ref, "host")
    gen = [3, 3, 900]
    for _ in range(12):
        got, _ = j.call(x, lambda: smp.sample_host(x, gen), generated=gen)
        gen = gen + [got]
    j.cap()
    assert j.draws > 0
    # sample_dev afterwards goes on from the same mu and word counter
    torch = torch_
    xd = torch.from_numpy(x).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    d0, mu0 = smp.draws(), smp.mirostat_state()[0]
    smp.sample_dev(xd, tok)
    torch.cuda.synchronize()
    assert smp.draws() - d0 in (0, 1) and smp.mirostat_state()[0] != mu0
    smp.close()
