"""The device sampler (bitnet_hip_sampler_* / bitnet_hip_sample_*, csrc/kernels_sample.hip) against the numpy restatement of the
reference's Sampler (tests/sampler_ref.py), at the kernel level and behind the decoder's captured graphs.

Agreement rules.  The greedy shortcut and top_k = 1 must match on every case (only comparisons decide them).  Every other result
that differs from the restatement's token is judged on its own by `sampler_accept.accepts` (its docstring derives the rule): on
the S path (top_k <= SMALL_K, the reference's summation order) the restatement's deciding comparison must have lain within 2^-20
of flipping; on the F path (parallel sums over the vocabulary) the device's token must belong to the largest kept set the
reference's own rounding admits, and u must lie within the case's tolerance -- the reference's measured f32 drift on that row
plus the derived allowance for the device's arithmetic -- of that token's float64 interval.  So a mismatch is checked for where
it landed: a neighbour in cumulative mass passes, a token from another chunk, a filtered entry or a stray last index does not.

On the rows of the original grid (peaked: sigma 1, 4, 12) two older conditions hold in addition, unchanged: a differing case must
also have had its deciding comparison within 2^-20 (S) or 2^-12 (F) of flipping, and the mismatches per path are capped: at most
1 % of the S cases and F_RATE of the F cases.  The case lists of tests/sampler_cases.py (vocabulary sweep, adversarial rows,
penalty edges, ends of the draw) are judged by `accepts` alone: on a flat row the reference's f32 total drifts by up to 1e-3, a
device that sums exactly lands a hundred entries away and legitimately differs on most draws, so neither the 2^-12 margin nor a
mismatch rate says anything there.  tests/test_sampler_accept.py holds the rule itself to account on the CPU, over the same lists."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_accept as sa  # noqa: E402
import sampler_cases as sc  # noqa: E402
import sampler_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_K = 64
MARGIN = {"S": 2.0 ** -20, "F": 2.0 ** -12}
F_RATE = 0.03  # F-path mismatches allowed per F case (every one of them near a boundary); measured rates: EXPERIMENTS.md section 9


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module("bitnet-rs_amd.synth")


def planted_logits(rng, vocab, sigma, k):
    x = (sigma * rng.standard_normal(vocab)).astype(np.float32)
    idx = rng.choice(vocab, 12, replace=False)
    x[idx[0]] = np.nan
    x[idx[1]] = -np.inf
    x[idx[2]] = 0.0
    x[idx[3]] = -0.0
    x[idx[4:6]] = x[idx[6]]  # plain duplicates
    if 0 < k < vocab:  # duplicates of the k-th value: the stable tie rule decides which survive
        kth = np.sort(np.where(np.isnan(x), -np.inf, x))[::-1][k - 1]
        x[idx[7:10]] = kth
    return x


class Tally:
    """grid=True (the original grid's rows): the margin rule and the rate caps, and `accepts` on every mismatch in addition.
    grid=False (the lists of sampler_cases.py): `accepts` alone."""

    def __init__(self, grid=True):
        self.grid = grid
        self.cases, self.flagged, self.mismatch = {"G": 0, "S": 0, "F": 0}, {"S": 0, "F": 0}, []
        self.exact = {"G": 0, "S": 0, "F": 0}
        self.worst, self.far = (0.0, None), (0, None)  # largest dist / T and largest index distance among the accepted mismatches

    def check(self, ref: sr.RefSampler, got: int, want: int, what):
        path = ref.last_path
        self.cases[path] += 1
        self.exact[path] += got == want
        if path == "G" or ref.k == 1:
            assert got == want, (what, path, got, want)
            return
        near = ref.last_margin < MARGIN[path]
        self.flagged[path] += near
        if got != want:
            if self.grid:
                assert near, (what, path, got, want, ref.last_margin)
            ok, reason = sa.accepts(ref, got)
            print(f"  mismatch {what} want {want} got {got}: {reason}")
            assert ok, (what, path, reason)
            self.mismatch.append((path,) + tuple(what))
            v = ref.last["verdict"]
            if v["T"] > 0 and v["dist"] / v["T"] > self.worst[0]:
                self.worst = (v["dist"] / v["T"], what)
            if v["idx"] > self.far[0]:
                self.far = (v["idx"], what)

    def report(self, name=""):
        per = {p: sum(1 for m in self.mismatch if m[0] == p) for p in ("S", "F")}
        msg = (f"{name}: cases {self.cases}, exact {self.exact}, accepted mismatches {per}, near-boundary {self.flagged}, "
               f"worst dist/T {self.worst[0]:.3f} {self.worst[1]}, largest index distance {self.far[0]} {self.far[1]}")
        print(msg)
        if self.grid:
            # each path on its own count: S sums in the reference's order (only expf can differ); F's parallel sums differ from
            # the reference's sequential f32 sum by its own drift, which moves a high-entropy draw to a neighbour now and then
            assert per["S"] <= max(1, 0.01 * self.cases["S"]), msg
            assert per["F"] <= max(1, F_RATE * self.cases["F"]), msg
        return msg


GRID = [(t, k, p, rp) for t in (0.0, 0.7, 1.0, 1.3) for k in (0, 1, 50, SMALL_K, SMALL_K + 1, 5000) for p in (1.0, 0.95, 0.5, 0.0, -0.5) for rp in (1.0, 1.1)]


@pytest.mark.parametrize("vocab", [1000, 128256])
def test_sample_host_grid_matches_the_restatement(hip, vocab):
    rng = np.random.default_rng(vocab)
    tally = Tally()
    smp = hip.sampler(vocab, 1.0, 0, 1.0, 1.0, seed=0)
    for ci, (t, k, p, rp) in enumerate(GRID):
        sigma = (1.0, 4.0, 12.0)[ci % 3]
        n_gen = (0, 1, 37)[(ci // 3) % 3]
        x = planted_logits(rng, vocab, sigma, k)
        if ci % 37 == 5:
            x[:] = -np.inf
        gen = [int(g) for g in rng.integers(0, vocab, n_gen)]
        if n_gen > 1:
            gen[1:6] = [gen[0]] * 5  # repeats
            gen[6] = int(np.nanargmax(x))  # the favourite is penalised
        seed = 1000 + ci
        ref = sr.RefSampler(t, k, p, rp, seed=seed)
        smp.configure(t, k, p, rp, seed)
        smp.reset()
        want = ref.sample(x, gen)
        got = smp.sample_host(x, gen)
        tally.check(ref, got, want, ("host", vocab, t, k, p, rp, sigma, n_gen))
        assert smp.draws() == (0 if ref.last_path == "G" else 1)
    tally.report("grid")
    smp.close()


@pytest.mark.parametrize("vocab", [1000, 128256])
def test_sample_dev_sequences_match_the_restatement(hip, torch_, vocab):
    """sample_dev counts the tokens it chose itself: 4 calls per config, the restatement fed the growing list of the device's tokens."""
    torch = torch_
    rng = np.random.default_rng(vocab + 1)
    tally = Tally()
    smp = hip.sampler(vocab, 1.0, 0, 1.0, 1.0, seed=0)
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    for ci, (t, k, p, rp) in enumerate(GRID):
        seed = 7 * ci + 3
        smp.configure(t, k, p, rp, seed)
        smp.reset()
        ref = sr.RefSampler(t, k, p, rp, seed=seed)
        gen: list[int] = []
        base = planted_logits(rng, vocab, (1.0, 4.0, 12.0)[ci % 3], k)
        for step in range(4):
            x = base.copy()
            if step == 3 and ci % 29 == 0:
                x[:] = -np.inf
            xd = torch.from_numpy(x).cuda()
            smp.sample_dev(xd, tok)
            torch.cuda.synchronize()
            got = int(tok.item())
            want = ref.sample(x, gen)
            tally.check(ref, got, want, ("dev", vocab, t, k, p, rp, step))
            gen.append(got)  # the device's own choice is what it counts next
        assert smp.draws() == ref.rng.draws
    tally.report("grid")
    smp.close()


def test_sample_dev_writes_history_and_skips_forced_positions(hip, torch_):
    torch = torch_
    vocab = 1000
    smp = hip.sampler(vocab, 0.8, 0, 0.9, 1.1, seed=5)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(vocab).astype(np.float32)).cuda()
    pos = torch.tensor([3], dtype=torch.int32, device="cuda")
    hist = torch.full((16,), -1, dtype=torch.int32, device="cuda")
    hist[4] = 77
    nf = torch.tensor([5], dtype=torch.int32, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    smp.sample_dev(x, tok, pos, hist, nf)  # p + 1 = 4 < 5: a prompt token sits there
    torch.cuda.synchronize()
    assert int(pos.item()) == 4 and int(hist[4].item()) == 77 and int(tok.item()) == 77 and smp.draws() == 0
    smp.sample_dev(x, tok, pos, hist, nf)
    torch.cuda.synchronize()
    assert int(pos.item()) == 5 and int(hist[5].item()) == int(tok.item()) and smp.draws() == 1


# ---- the case lists of tests/sampler_cases.py: judged by sampler_accept.accepts alone ---------------------------------------
LISTS = {"sweep": sc.SWEEP, "adversarial": sc.ADVERSARIAL, "penalty": sc.PENALTY, "ends": sc.ENDS}


class Samplers:
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


def run_case(smp, torch, case, mode, tally):
    """host: every call passes the growing list (the case's own list first) to sample_host.  dev: sample_dev counts the tokens it
    chose itself, so the case's list is left out and the restatement is fed the device's tokens."""
    x = sc.row(case)
    smp.configure(*case["cfg"], case["seed"])
    smp.reset()
    ref = sr.RefSampler(*case["cfg"], seed=case["seed"])
    hist = sc.gen(case) if mode == "host" else []
    if mode == "dev":
        xd = torch.from_numpy(x).cuda()
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    for step in range(case["steps"]):
        if mode == "host":
            got = smp.sample_host(x, hist)
        else:
            smp.sample_dev(xd, tok)
            torch.cuda.synchronize()
            got = int(tok.item())
        want = ref.sample(x, hist)
        tally.check(ref, got, want, (mode, case["id"], step))
        hist = hist + [got]
    assert smp.draws() == ref.rng.draws, case["id"]


@pytest.mark.parametrize("mode", ["host", "dev"])
@pytest.mark.parametrize("name", list(LISTS))
def test_case_lists_are_defensible_draw_by_draw(hip, torch_, name, mode):
    tally = Tally(grid=False)
    pool = Samplers(hip)
    for case in LISTS[name]:
        run_case(pool.get(case["vocab"]), torch_, case, mode, tally)
    pool.close()
    tally.report(f"{name}/{mode}")
    assert sum(tally.cases.values()) == sum(c["steps"] for c in LISTS[name])


def test_ends_of_the_draw_seeds():
    lo, hi = sr.ChaCha20Rng(sc.SEED_U_LOW).random_f32(), sr.ChaCha20Rng(sc.SEED_U_HIGH).random_f32()
    assert 0 <= lo < 2.0 ** -16 and 1 - 2.0 ** -16 <= hi < 1


def test_sample_dev_512_calls_with_a_compounding_penalty(hip, torch_):
    """512 calls at vocab 128256 with rp 1.3: the exponents reach the hundreds of thousands, powi(1.3, e) is inf from e = 339 on, so
    positive favourites go to +0, negative ones to -inf, and the draw moves on to fresh tokens.  The restatement is fed the
    device's own tokens."""
    torch = torch_
    vocab, cfg, seed = 128256, (0.7, 0, 0.95, 1.3), 77
    base = (4.0 * np.random.default_rng(5).standard_normal(vocab)).astype(np.float32)
    smp = hip.sampler(vocab, *cfg, seed=seed)
    ref = sr.RefSampler(*cfg, seed=seed)
    tally = Tally(grid=False)
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    bd = torch.from_numpy(base).cuda()
    hist: list[int] = []
    for step in range(512):
        sh = (step * 9973) % vocab
        smp.sample_dev(torch.roll(bd, sh), tok)
        torch.cuda.synchronize()
        got = int(tok.item())
        want = ref.sample(np.roll(base, sh), hist)
        tally.check(ref, got, want, ("dev512", step))
        hist.append(got)
    assert smp.draws() == ref.rng.draws == 512
    tally.report("dev 512 calls")
    smp.close()


def test_configure_mid_sequence_keeps_the_counts(hip, torch_):
    """A new config and seed without reset(): the stream restarts, the counts stay (what a new reference Sampler would not do, so
    the restatement's counts are carried over by hand)."""
    torch = torch_
    vocab = 128256
    x = (12.0 * np.random.default_rng(11).standard_normal(vocab)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    tally = Tally(grid=False)
    a, b = (0.7, 0, 0.9, 1.5), (1.0, 0, 1.0, 1.5)  # F, then the penalised argmax, then S
    smp = hip.sampler(vocab, *a, seed=1)
    ref = sr.RefSampler(*a, seed=1)
    hist: list[int] = []
    for ci, cfg in enumerate([a, b, (0.9, 40, 0.95, 1.5)]):
        if ci:
            smp.configure(*cfg, 100 + ci)
            counts = ref.counts
            ref = sr.RefSampler(*cfg, seed=100 + ci)
            ref.counts = counts
        for step in range(4):
            smp.sample_dev(xd, tok)
            torch.cuda.synchronize()
            got = int(tok.item())
            want = ref.sample(x, hist)
            tally.check(ref, got, want, ("configure", ci, step))
            hist.append(got)
        assert smp.draws() == ref.rng.draws
    assert len(set(hist)) > 1  # the penalty moved the favourite: the counts mattered
    tally.report("configure mid-sequence")
    smp.close()


def test_two_samplers_of_different_vocabulary_alternate_on_one_stream(hip, torch_):
    """2^20 first, then 1000: the kernel's dynamic-LDS attribute only ever grows, so the later, smaller sampler leaves it alone."""
    torch = torch_
    tally = Tally(grid=False)
    big, small = 1 << 20, 1000
    cb, cs = (0.7, 0, 0.9, 1.1), (1.3, 0, 0.5, 1.1)
    sb = hip.sampler(big, *cb, seed=3)
    ss = hip.sampler(small, *cs, seed=4)
    rb, rs = sr.RefSampler(*cb, seed=3), sr.RefSampler(*cs, seed=4)
    xb = (4.0 * np.random.default_rng(1).standard_normal(big)).astype(np.float32)
    xs = np.random.default_rng(2).standard_normal(small).astype(np.float32)
    xbd, xsd = torch.from_numpy(xb).cuda(), torch.from_numpy(xs).cuda()
    tb = torch.zeros(1, dtype=torch.int32, device="cuda")
    ts = torch.zeros(1, dtype=torch.int32, device="cuda")
    hb, hs = [], []
    for step in range(4):
        sb.sample_dev(xbd, tb)
        ss.sample_dev(xsd, ts)
        torch.cuda.synchronize()
        gb, gs = int(tb.item()), int(ts.item())
        tally.check(rb, gb, rb.sample(xb, hb), ("alternate", big, step))
        tally.check(rs, gs, rs.sample(xs, hs), ("alternate", small, step))
        hb.append(gb)
        hs.append(gs)
    assert sb.draws() == 4 and ss.draws() == 4
    tally.report("two samplers")
    sb.close()
    ss.close()


def test_greedy_then_full_then_greedy_on_one_sampler(hip):
    vocab = 128256
    x = (4.0 * np.random.default_rng(21).standard_normal(vocab)).astype(np.float32)
    tally = Tally(grid=False)
    smp = hip.sampler(vocab, 1.0, 0, 1.0, 1.1, seed=8)
    for ci, cfg in enumerate([(1.0, 0, 1.0, 1.1), (0.7, 0, 0.95, 1.1), (0.0, 50, 0.5, 1.1)]):
        smp.configure(*cfg, 8)
        ref = sr.RefSampler(*cfg, seed=8)
        got = smp.sample_host(x, [int(np.argmax(x))] * 3)
        tally.check(ref, got, ref.sample(x, [int(np.argmax(x))] * 3), ("G-F-G", ci))
        assert ref.last_path == "GFG"[ci] and smp.draws() == ref.rng.draws == (1 if ci == 1 else 0)
    smp.close()


def test_sampler_refuses_vocabularies_it_was_not_made_for(hip, pkg, torch_):
    for vocab in (0, (1 << 20) + 1):
        with pytest.raises(pkg.BitNetHipError, match=r"sampler_create: vocab must be in 1\.\.1048576"):
            hip.sampler(vocab, 1.0, 0, 1.0, 1.0, seed=0)
    smp = hip.sampler(1000, 0.7, 0, 0.9, 1.0, seed=0)
    tok = torch_.zeros(1, dtype=torch_.int32, device="cuda")
    with pytest.raises(pkg.BitNetHipError, match="sample_dev: vocab 999, the sampler was made for 1000"):
        smp.sample_dev(torch_.zeros(999, device="cuda"), tok)
    with pytest.raises(pkg.BitNetHipError, match="sample_host: vocab 1001, the sampler was made for 1000"):
        smp.sample_host(np.zeros(1001, np.float32), [])
    assert smp.draws() == 0
    smp.close()


# ---- decoder level ---------------------------------------------------------------------------------------------------------
SMALL = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=80, eps=1e-5, rope_theta=10000.0)
BIGV = dict(SMALL, vocab=128256)


def make_decoder(pkg, synth, cfgd, fmt="qk256"):
    cfg = synth.ModelConfig(**cfgd)
    dec = pkg.HostDecoder(cfg)
    for l in range(cfg.n_layers):
        w = synth.make_layer(cfg, l, fmt=fmt)
        if fmt == "qk256":
            dec.set_layer_qk256(l, w)
        else:
            dec.set_layer_i2s(l, w, 32)
    dec.set_globals(synth.make_globals(cfg))
    return cfg, dec


def sampled_run(dec, prompt, n, use_graph=True, ref=None, tally=None):
    """prompt forced, then n sampled steps one at a time; with `ref`, every step is held against the restatement fed the
    decoder's own logits and its growing list of generated tokens."""
    dec.reset()
    dec.feed(prompt)
    dec.run(len(prompt) - 1, with_logits=False, use_graph=use_graph)
    gen = []
    for i in range(n):
        dec.run(1, with_logits=True, use_graph=use_graph)
        got = int(dec.history(len(prompt) + i + 1)[-1])
        if ref is not None:
            want = ref.sample(dec.last_logits(), gen)
            tally.check(ref, got, want, ("decoder", i))
        gen.append(got)
    return gen


@pytest.mark.parametrize("cfgd,fmt", [(SMALL, "qk256"), (SMALL, "i2s"), (BIGV, "qk256")])
def test_decoder_sampling_matches_the_restatement(hip, pkg, synth, cfgd, fmt):
    cfg, dec = make_decoder(pkg, synth, cfgd, fmt)
    prompt = synth.prompt(5, cfg.vocab)
    tally = Tally()
    dec.set_sampling(0.7, 0, 0.95, 1.1, seed=42)
    ref = sr.RefSampler(0.7, 0, 0.95, 1.1, seed=42)
    toks = sampled_run(dec, prompt, 48, True, ref, tally)
    assert dec.sampling_draws() == 48
    # the greedy-with-penalty config is bit-exact for 64 steps
    dec.set_sampling(1.0, 0, 1.0, 1.1, seed=1)
    ref = sr.RefSampler(1.0, 0, 1.0, 1.1, seed=1)
    sampled_run(dec, prompt, 64, True, ref, tally)
    assert dec.sampling_draws() == 0
    # top-k 40 (S path) behind the graphs, eager too
    for use_graph in (True, False):
        dec.set_sampling(0.8, 40, 0.9, 1.1, seed=9)
        ref = sr.RefSampler(0.8, 40, 0.9, 1.1, seed=9)
        sampled_run(dec, prompt, 24, use_graph, ref, tally)
    tally.report("grid")
    assert len(set(toks)) > 1
    dec.close()


def test_decoder_sampling_switches_seeds_and_resets(hip, pkg, synth):
    cfg, dec = make_decoder(pkg, synth, SMALL)
    prompt = synth.prompt(5, cfg.vocab)
    greedy = sampled_run(dec, prompt, 32)
    cfg2, fresh = make_decoder(pkg, synth, SMALL)
    assert sampled_run(fresh, prompt, 32) == greedy
    fresh.close()
    # high-entropy logits: temperature 1.5 over the full vocabulary
    dec.set_sampling(1.5, 0, 1.0, 1.0, seed=123)
    a = sampled_run(dec, prompt, 32)
    b = sampled_run(dec, prompt, 32)  # reset() restarts the counts and the stream
    assert a == b and dec.sampling_draws() == 32
    dec.set_sampling(1.5, 0, 1.0, 1.0, seed=124)
    c = sampled_run(dec, prompt, 32)
    assert c != a
    dec.set_sampling(1.5, 0, 1.0, 1.0, seed=123)  # a new config keeps the graphs: the same seed, the same tokens
    assert sampled_run(dec, prompt, 32) == a
    # 48 per-token graphs replayed back to back give the tokens of the step-by-step run
    dec.set_sampling(0.7, 0, 0.95, 1.1, seed=42)
    steps = sampled_run(dec, prompt, 48)
    dec.reset()
    dec.feed(prompt)
    dec.run(len(prompt) - 1, with_logits=False, use_graph=True)
    dec.run(48, with_logits=True, use_graph=True)
    assert [int(t) for t in dec.history(len(prompt) + 48)[len(prompt):]] == steps and dec.sampling_draws() == 48
    dec.set_sampling(None)
    assert sampled_run(dec, prompt, 32) == greedy
    assert sampled_run(dec, prompt, 32, use_graph=False) == greedy
    dec.close()


def test_first_token_after_prefill_is_sampled(hip, pkg, synth):
    cfg, dec = make_decoder(pkg, synth, dict(SMALL, max_pos=160))
    prompt = synth.prompt(64, cfg.vocab)
    dec.set_sampling(0.7, 0, 0.95, 1.1, seed=42)
    dec.reset()
    dec.feed(prompt)
    dec.prefill(64, with_logits=True, digits=4)
    assert dec.sampling_draws() == 1 and dec.position() == 64
    ref = sr.RefSampler(0.7, 0, 0.95, 1.1, seed=42)
    want = ref.sample(dec.last_logits(), [])
    got = int(dec.history(65)[64])
    assert got == want or ref.last_margin < MARGIN["F"]
    assert sa.accepts(ref, got)[0], sa.accepts(ref, got)[1]
    with pytest.raises(pkg.BitNetHipError, match="sampling"):
        dec.reset()
        dec.feed(prompt)
        dec.prefill_sharded(128, 0, 1, None, with_logits=True)
    dec.close()
