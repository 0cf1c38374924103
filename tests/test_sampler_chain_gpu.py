"""GPU: the sampler chain on the device (bitnet_hip_sampler_create_ex / _configure_ex, csrc/kernels_sample.hip) -- additive penalties,
min-p and typical-p around the CLI sampler's stages -- against the numpy restatement (tests/sampler_chain_ref.py), draw by draw through the
acceptance rule of tests/sampler_chain_accept.py, over the case lists of tests/sampler_chain_cases.py (which
tests/test_sampler_chain_accept.py walks on the CPU).

Path G is bit-exact; path S is equal or within 2^-20 of a flip; path F (min-p, typical-p) passes the interval rule, and the share of
undecided draws stays under the caps.  Exact rows hold the comparisons themselves (`<` at the min-p
threshold, `>=` at the typical-p cut, ascending ids among tied deviations).  k_sample_batch, a captured graph across configure_ex, the
decoder and a batch member are held to k_sample / their own twins bit for bit."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
import sampler_chain_accept as ca  # noqa: E402
import sampler_chain_cases as cc  # noqa: E402
import sampler_chain_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

UNDECIDED_CAP_MINP = 0.02
UNDECIDED_CAP_TYP = 0.10


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


class Pool:
    """one device sampler per vocabulary, made on first use"""

    def __init__(self, hip):
        self.hip, self.by_vocab = hip, {}

    def get(self, vocab):
        if vocab not in self.by_vocab:
            self.by_vocab[vocab] = self.hip.sampler(vocab, 1.0, 0, 1.0, 1.0, seed=0)
        return self.by_vocab[vocab]

    def close(self):
        for s in self.by_vocab.values():
            s.close()


def run_case(smp, torch, case, mode, stats):
    """host: sample_host with the growing list (the case's own list first).  dev: sample_dev counts the tokens it chose itself, so the
    case's list is left out and the restatement is fed the device's tokens."""
    x = sc.row(case)
    smp.configure(*case["cfg"], case["seed"], **case["ex"])
    smp.reset()
    ref = cr.ChainRef(*case["cfg"], seed=case["seed"], **case["ex"])
    hist = sc.gen(case) if mode == "host" else []
    if mode == "dev":
        xd = torch.from_numpy(x).cuda()
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    toks = []
    for step in range(case["steps"]):
        if mode == "host":
            got = smp.sample_host(x, hist)
        else:
            smp.sample_dev(xd, tok)
            torch.cuda.synchronize()
            got = int(tok.item())
        want = ref.sample(x, hist)
        ok, reason = ca.accepts(ref, got)
        if got != want:
            print(f"  mismatch {mode} {case['id']} step {step}: want {want} got {got}: {reason}")
        assert ok, (mode, case["id"], step, reason)
        stats["calls"] += 1
        stats["equal"] += got == want
        stats["undecided"] += bool(ref.last["undecided"])
        hist = hist + [got]
        toks.append(got)
    assert smp.draws() == ref.rng.draws, case["id"]
    return toks


def run_list(hip, torch, cases, mode):
    pool, stats = Pool(hip), dict(calls=0, equal=0, undecided=0)
    toks = {c["id"]: run_case(pool.get(c["vocab"]), torch, c, mode, stats) for c in cases}
    pool.close()
    print(f"\n{mode}: {stats}")
    assert stats["calls"] == sum(c["steps"] for c in cases)
    return toks, stats


@pytest.mark.parametrize("mode", ["dev", "host"])
def test_path_g_with_additive_penalties_is_bit_exact(hip, torch_, mode):
    toks, stats = run_list(hip, torch_, cc.GREEDY, mode)
    assert stats["equal"] == stats["calls"]  # and run_case held draws() at 0: no word is consumed
    assert len(set(toks["chain-G-v1000-two_top"])) > 1  # the penalties moved the favourite


@pytest.mark.parametrize("mode", ["dev", "host"])
def test_path_s_runs_the_stages_in_the_reference_order(hip, torch_, mode):
    toks, stats = run_list(hip, torch_, cc.SMALL, mode)
    assert stats["calls"] - stats["equal"] <= max(1, 0.01 * stats["calls"]), stats  # the S allowance of tests/test_sampling_gpu.py
    # typical_p 0.5 over 64 equal survivors keeps ids 0..31: `>=`, and tied deviations by ascending id
    assert all(t < 32 for c in cc.SMALL if "equal-typ" in c["id"] for t in toks[c["id"]])
    # min_p 1 keeps the entries tied at the maximum: the even ids
    assert all(t % 2 == 0 for c in cc.SMALL if "interleaved-minp1" in c["id"] for t in toks[c["id"]])


@pytest.mark.parametrize("mode", ["dev", "host"])
def test_path_f_min_p_passes_the_rule_draw_by_draw(hip, torch_, mode):
    _, stats = run_list(hip, torch_, cc.FULL, mode)
    assert stats["undecided"] <= UNDECIDED_CAP_MINP * stats["calls"], stats


@pytest.mark.parametrize("mode", ["dev", "host"])
def test_path_f_typical_p_passes_the_rule_draw_by_draw(hip, torch_, mode):
    _, stats = run_list(hip, torch_, cc.FULL_TYP, mode)
    assert stats["undecided"] <= UNDECIDED_CAP_TYP * stats["calls"], stats


def test_exact_rows(hip, torch_):
    toks, _ = run_list(hip, torch_, cc.EXACT_F, "dev")
    for c in cc.EXACT_F:
        x = sc.row(c)
        if c["row"][0] == "equal_one":  # exp(-2.5) < 0.5: only the large entry survives min-p
            assert toks[c["id"]] == [int(np.argmax(x))], c["id"]
        if c["row"][0] == "two_interleaved":
            assert toks[c["id"]][0] % 2 == 0, c["id"]
        if "v64-equal-typ" in c["id"]:
            assert toks[c["id"]][0] < 32, c["id"]
        if "v2049-equal-typ" in c["id"]:  # typical_p 0.25 of 2049 equal entries: the first 513 ids
            assert toks[c["id"]][0] < 513, c["id"]
    # 64 seeds over 64 equal survivors, typical_p 0.5, on path F (vocab 64, top_k 0) and on path S (top_k 64 of 1000): all deviations tie
    # and the sums are exact, so the kept set is ids 0..31 -- `>=` at the cut, ascending ids among the ties
    for vocab, k in ((64, 0), (1000, 64)):
        smp = hip.sampler(vocab, 0.8, k, 1.0, 1.0, seed=0, typical_p=0.5)
        xd = torch_.full((vocab,), 0.5, dtype=torch_.float32, device="cuda")
        tok = torch_.zeros(1, dtype=torch_.int32, device="cuda")
        seen = set()
        for seed in range(64):
            smp.configure(0.8, k, 1.0, 1.0, seed, typical_p=0.5)
            smp.sample_dev(xd, tok)
            seen.add(int(tok.item()))
        smp.close()
        assert max(seen) < 32 and len(seen) > 16, (vocab, k, sorted(seen))


# ---- k_sample_batch: per slot what sample_dev alone leaves ---------------------------------------------------------------------------
BATCH = [((1.0, 0, 1.0, 1.1), {}), ((0.0, 0, 1.0, 1.1), dict(frequency_penalty=0.5, presence_penalty=0.3)),
         ((0.8, 40, 0.95, 1.1), {}), ((0.8, 40, 0.95, 1.1), dict(min_p=0.05, typical_p=0.9)),
         ((0.8, 0, 0.95, 1.1), {}), ((0.8, 0, 0.95, 1.1), dict(min_p=0.05, typical_p=0.9, frequency_penalty=0.2, presence_penalty=0.1))]


def test_batch_slots_equal_sample_dev_alone(hip, torch_):
    torch = torch_
    vocab, n_slots, hist_n = 1000, 8, 16
    rng = np.random.default_rng(99)

    def lane(i):
        cfg, ex = BATCH[i]
        return dict(smp=hip.sampler(vocab, *cfg, seed=300 + i, **ex), tok=torch.full((1,), -1, dtype=torch.int32, device="cuda"),
                    pos=torch.zeros(1, dtype=torch.int32, device="cuda"), hist=torch.full((hist_n,), -1, dtype=torch.int32, device="cuda"),
                    nf=torch.zeros(1, dtype=torch.int32, device="cuda"), logits=torch.zeros(vocab, dtype=torch.float32, device="cuda"))

    members, twins = [lane(i) for i in range(len(BATCH))], [lane(i) for i in range(len(BATCH))]
    table = hip.sample_batch(vocab, n_slots)
    for b, m in enumerate(members):  # slots 6 and 7 stay empty
        table.set(b, m["smp"], m["logits"], m["tok"], m["pos"], m["hist"], m["nf"])
    for call in range(8):
        for m, t in zip(members, twins):
            x = torch.from_numpy((4.0 * rng.standard_normal(vocab)).astype(np.float32))
            m["logits"].copy_(x)
            t["logits"].copy_(x)
        table.launch()
        for t in twins:
            t["smp"].sample_dev(t["logits"], t["tok"], t["pos"], t["hist"], t["nf"])
        torch.cuda.synchronize()
        for b, (m, t) in enumerate(zip(members, twins)):
            for key in ("tok", "pos", "hist"):
                assert torch.equal(m[key], t[key]), (call, b, key, m[key], t[key])
            assert int(m["pos"].item()) == call + 1
    for b, (m, t) in enumerate(zip(members, twins)):
        assert m["smp"].draws() == t["smp"].draws() == (0 if b < 2 else 8), b
    # the hand-over was re-armed and the counts are the twin's: one more call alone on either side gives the same token
    for m, t in zip(members, twins):
        table.set(members.index(m), None)
        for l in (m, t):
            l["smp"].sample_dev(l["logits"], l["tok"], l["pos"], l["hist"], l["nf"])
        torch.cuda.synchronize()
        assert torch.equal(m["tok"], t["tok"]) and torch.equal(m["hist"], t["hist"])
    table.close()
    for l in members + twins:
        l["smp"].close()


# ---- configure_ex under a captured graph ---------------------------------------------------------------------------------------------
def test_a_captured_graph_follows_configure_ex_and_the_counts_stay(hip, torch_):
    torch = torch_
    vocab = 1000
    x = (4.0 * np.random.default_rng(3).standard_normal(vocab)).astype(np.float32)
    x[:2] = [30.0, 29.0]
    xd = torch.from_numpy(x).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    neutral, chain = (0.0, 0, 1.0, 1.0), dict(frequency_penalty=0.6, presence_penalty=0.5)
    smp = hip.sampler(vocab, *neutral, seed=1)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        smp.sample_dev(xd, tok, stream=stream.cuda_stream)  # warm-up: counts token 0 once
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            smp.sample_dev(xd, tok, stream=stream.cuda_stream)
    ref = cr.ChainRef(*neutral, seed=1)
    hist = [ref.sample(x, [])]
    assert int(tok.item()) == 0

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        return int(tok.item())

    got = replay()
    assert got == ref.sample(x, hist) == 0  # neutral: the argmax, whatever was counted
    hist.append(got)
    smp.configure(*neutral, 1, **chain)  # no re-capture
    counts = ref.counts
    ref = cr.ChainRef(*neutral, seed=1, **chain)
    ref.counts = counts
    for _ in range(3):
        got = replay()
        assert got == ref.sample(x, hist), hist  # two occurrences counted before the configure: 30 - 1.2 - 0.5 < 29
        hist.append(got)
    assert hist[2] == 1 and smp.draws() == 0
    smp.reset()
    assert replay() == 0  # the counts are gone
    smp.close()


# ---- decoder level -------------------------------------------------------------------------------------------------------------------
DEC_F = dict(top_k=0, top_p=0.95, min_p=0.05, typical_p=0.9, frequency_penalty=0.2, presence_penalty=0.1)
DEC_S = dict(top_k=40, top_p=0.95, min_p=0.05, typical_p=0.9, frequency_penalty=0.2, presence_penalty=0.1)


@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
def test_decoder_runs_the_chain_inside_its_graphs(hip, pkg, fmt):
    tg = importlib.import_module("test_sampling_gpu")
    synth = importlib.import_module("bitnet-rs_amd.synth")
    cfg, dec = tg.make_decoder(pkg, synth, tg.SMALL, fmt)
    prompt = synth.prompt(5, cfg.vocab)
    for kw, seed in ((DEC_F, 42), (DEC_S, 43)):
        dec.set_sampling(0.8, seed=seed, **kw)
        ref = cr.ChainRef(0.8, kw["top_k"], kw["top_p"], 1.0, seed=seed, **{k: v for k, v in kw.items() if k not in ("top_k", "top_p")})
        dec.reset()
        dec.feed(prompt)
        dec.run(len(prompt) - 1, with_logits=False, use_graph=True)
        gen = []
        for i in range(16):
            dec.run(1, with_logits=True, use_graph=True)
            got = int(dec.history(len(prompt) + i + 1)[-1])
            want = ref.sample(dec.last_logits(), gen)
            ok, reason = ca.accepts(ref, got)
            assert ok, (fmt, kw, i, reason)
            gen.append(got)
        assert dec.sampling_draws() == 16 and len(set(gen)) > 1
    with pytest.raises(pkg.BitNetHipError, match="min_p"):
        dec.set_sampling(0.8, min_p=float("nan"), seed=1)
    dec.close()


def test_a_batch_member_with_the_chain_gets_the_tokens_of_its_own_run(hip, pkg, worlds_):
    tb = importlib.import_module("test_batch_sampling_gpu")
    W = worlds_
    c = tb.Cast(pkg, W, 2)

    def join(b, length, offset, kw, seed, member=None):
        m, t = member or c.owner.shared(), W.twin(pkg)
        for d in (m, t):
            if kw:
                d.set_sampling(0.8, seed=seed, **kw)
            tb.start(d, W, length, offset)
        c.batch.set_slot(b, m)
        c.members[b], c.twins[b] = m, t
        c.all += [x for x in (m, t) if x is not c.owner]

    join(0, 20, 0, DEC_F, 51, member=c.owner)
    join(1, 22, 5, None, 0)  # stays greedy
    c.steps(8, "chain member beside a greedy one")
    assert c.members[0].sampling_draws() >= 8 and c.members[1].sampling_draws() == 0
    c.members[0].set_sampling(0.8, seed=52, **DEC_S)  # a new config on an existing sampler: no re-capture
    c.twins[0].set_sampling(0.8, seed=52, **DEC_S)
    c.steps(4, "the member switched to the one-lane stages")
    assert c.batch.captures() == 1
    c.close()


@pytest.fixture(scope="module")
def worlds_(pkg):
    tb = importlib.import_module("test_batch_sampling_gpu")
    return tb.World(importlib.import_module("bitnet-rs_amd.synth"), "qk256")
