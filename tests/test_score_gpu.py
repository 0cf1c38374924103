"""Teacher-forced scoring on the device (bitnet_hip_score_f16_dev, csrc/kernels_score.hip; Decoder::score / HostDecoder.score;
tools/score.py) against tests/score_ref.py, the CPU oracle and the decoder's own step path.

  1. kernel: the head against score_ref on the same f16-rounded LN(x) * gamma; ragged vocabularies and rows, targets -1 / >= vocab,
     logits_rows 0 / 5 / all; non-finite table rows and x rows; two calls bitwise equal.
  2. decoder, the bench's widths with 2 layers (tests/test_bench_prefill_instance.py WIDE): the state after score(n) is that of prefill(n);
     every position against OracleModel stepped with logits (one pass over the 2600-token prompt per format serves every n and both
     KV modes: its logits at position r depend only on the prefix).
  3. an f16 hand-over that saturates: score repeats the prompt at 4 digits as prefill does.
  4. full depth (30 layers, vocabulary 128256, 4096 tokens): score against the decoder's own step path teacher-forced.
  5. tools/score.py end to end.
Bounds: nll moves by at most twice the worst logit error, so the oracle bound is twice test_full_depth_parity's 1e-2-of-max logits bound."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = dict(hidden=2560, n_layers=2, n_heads=20, n_kv_heads=5, head_dim=128, ffn=6912, vocab=4096, max_pos=4224, eps=1e-5, rope_theta=500000.0)
T_WIDE = 2600
ORACLE_REL = 2e-2  # |dnll_r| <= ORACLE_REL * max_v |l_r,v|
BENCH_PATH = {"qk256": 0, "i2s": 1}  # last_prefill_path() of bench.py's prompt timings (digits 2, default switches)


def host_threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module("bitnet-rs_amd.synth")


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def run_kernel(hip, torch_, table16, x, gamma, targets, logits_rows, eps=1e-5):
    n, h = x.shape
    v = table16.shape[0]
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    t, xd, gd, td = dev(table16.view(np.int16)), dev(x), dev(gamma) if gamma is not None else None, dev(targets.astype(np.int32))
    nll = torch_.zeros(n, dtype=torch_.float32, device="cuda")
    am = torch_.zeros(n, dtype=torch_.int32, device="cuda")
    lg = torch_.zeros(max(logits_rows, 1) * v, dtype=torch_.float32, device="cuda")
    wsb = hip.score_workspace_bytes(n, h, v)
    ws = torch_.zeros(wsb, dtype=torch_.uint8, device="cuda")
    hip.score_f16_dev(t, xd, gd, eps, h, v, n, td, nll, am, lg if logits_rows else None, logits_rows, ws, wsb)
    torch_.cuda.synchronize()
    return nll.cpu().numpy(), am.cpu().numpy(), lg.cpu().numpy()[:logits_rows * v].reshape(logits_rows, v)


def ref_logits(table16, x, gamma, rows, eps=1e-5):
    a = sr.head_rows(x[rows], gamma, eps)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a @ table16.astype(np.float32).T).astype(np.float32)


def check_rows(got_nll, got_am, ref_l, targets, what):
    worst = 0.0
    for i in range(ref_l.shape[0]):
        l = ref_l[i]
        fin = l[np.isfinite(l)]
        scale = float(np.max(np.abs(fin))) if fin.size else 0.0
        bound = 5e-5 * scale + 1e-4
        want = sr.row_nll(l, int(targets[i]))
        if math.isnan(want) or math.isinf(want):
            assert (math.isnan(want) and math.isnan(got_nll[i])) or want == got_nll[i], (what, i, want, got_nll[i])
        else:
            worst = max(worst, abs(float(got_nll[i]) - want) / bound)
            assert abs(float(got_nll[i]) - want) <= bound, (what, i, want, got_nll[i], bound)
        if got_am is None:
            continue
        la = np.where(np.isnan(l), -np.inf, l)
        top2 = np.sort(la)[-2:]
        if la.size < 2 or top2[1] - top2[0] > bound:
            assert int(got_am[i]) == sr.argmax(l), (what, i)
    return worst


@pytest.mark.parametrize("n,h,v", [(1, 512, 1000), (37, 2560, 4099), (130, 2560, 128256), (4096, 2560, 128256)])
def test_kernel_matches_the_restatement(hip, torch_, n, h, v):
    rng = np.random.default_rng(n + v)
    table = rng.standard_normal((v, h), dtype=np.float32).astype(np.float16)
    x = (3.0 * rng.standard_normal((n, h), dtype=np.float32) + 0.5).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, h).astype(np.float32)
    targets = rng.integers(0, v, n).astype(np.int32)
    if n > 3:
        targets[1], targets[2], targets[3] = -1, v, v + 7
    rows = np.arange(n) if n <= 130 else np.sort(rng.choice(n, 64, replace=False))
    ref = ref_logits(table, x, gamma, rows)
    for lr in sorted({0, min(5, n), n if n <= 130 else 0}):
        nll, am, lg = run_kernel(hip, torch_, table, x, gamma, targets, lr)
        worst = check_rows(nll[rows], am[rows], ref, targets[rows], (n, h, v, lr))
        if lr:
            sel = rows < lr
            d = np.abs(lg[rows[sel]] - ref[sel])
            assert np.all(d <= 5e-5 * np.max(np.abs(ref[sel]), axis=1, keepdims=True) + 1e-4), (n, h, v, lr, float(d.max()))
        print(f"\n[kernel {n}x{h}x{v} logits_rows {lr}] worst |dnll| / bound {worst:.3f}")
    nll2, am2, _ = run_kernel(hip, torch_, table, x, gamma, targets, 0)
    assert nll.tobytes() == nll2.tobytes() and am.tobytes() == am2.tobytes()  # deterministic


def test_kernel_non_finite_inputs(hip, torch_):
    n, h, v = 40, 512, 1000
    rng = np.random.default_rng(7)
    table = rng.standard_normal((v, h), dtype=np.float32).astype(np.float16)
    table[123] = np.inf  # column 123 of every row becomes non-finite (inf, or NaN where inf meets 0 / both signs)
    x = rng.standard_normal((n, h), dtype=np.float32)
    x[5] = np.nan
    gamma = rng.uniform(0.5, 1.5, h).astype(np.float32)
    targets = rng.integers(0, v, n).astype(np.int32)
    targets[targets == 123] = 0
    targets[9] = 123
    nll, am, lg = run_kernel(hip, torch_, table, x, gamma, targets, n)
    assert nll[9] == np.inf
    assert math.isnan(nll[5])
    assert not np.isfinite(lg[:, 123]).any()
    ref = ref_logits(table, x, gamma, np.arange(n))
    keep = np.array([i for i in range(n) if i not in (5, 9)])
    ref_m = ref[keep].copy()
    ref_m[:, 123] = -np.inf  # the column as score.rs sees it
    check_rows(nll[keep], None, ref_m, targets[keep], "inf column")
    for i in range(n):  # argmax counts +inf as the largest value, NaN as -inf: the device's own logits row decides, with the kernel's rule
        assert int(am[i]) == sr.argmax(lg[i]), i


# ---------------------------------------------------------------------------------------------------------------- 2. decoder, small models
def make_decoder(pkg, synth, cfgd, fmt, layers=None, glob=None):
    cfg = synth.ModelConfig(**cfgd)
    dec = pkg.HostDecoder(cfg)
    layers = layers or [synth.make_layer(cfg, l, fmt=fmt, block=32) for l in range(cfg.n_layers)]
    for l, w in enumerate(layers):
        if fmt == "qk256":
            dec.set_layer_qk256(l, w)
        else:
            dec.set_layer_i2s(l, w, 32)
    dec.set_globals(glob if glob is not None else synth.make_globals(cfg))
    return cfg, dec, layers


@pytest.fixture(scope="module", params=["qk256", "i2s"])
def wide(request, pkg, hip, oracle, synth):
    fmt = request.param
    cfg, dec, layers = make_decoder(pkg, synth, WIDE, fmt)
    glob = synth.make_globals(cfg)
    prompt = synth.prompt(T_WIDE, cfg.vocab)
    om = oracle.OracleModel(cfg, [dict(w, ternary=32) if fmt == "i2s" else w for w in layers], glob, n_threads=host_threads())
    olog = np.stack([om.step(int(t), want_logits=True)[1] for t in prompt])
    om.close()
    yield fmt, cfg, dec, prompt, olog
    dec.close()


def against_oracle(res, olog, prompt, n, label):
    worst_nll, worst_cos, agree, checked = 0.0, 1.0, 0, 0
    for r in range(n - 1):
        o = olog[r]
        scale = float(np.max(np.abs(o)))
        d = abs(float(res.nll[r]) - sr.row_nll(o, int(prompt[r + 1])))
        worst_nll = max(worst_nll, d / scale)
        assert d <= ORACLE_REL * scale, (label, r, d, scale)
    for r in range(n):
        o = olog[r]
        top2 = np.sort(o)[-2:]
        if top2[1] - top2[0] > ORACLE_REL * np.max(np.abs(o)):
            checked += 1
            agree += int(res.argmax[r]) == sr.argmax(o)
            assert int(res.argmax[r]) == sr.argmax(o), (label, r)
        if res.logits is not None:
            c = cosine(res.logits[r], o)
            worst_cos = min(worst_cos, c)
            assert c >= 0.999, (label, r, c)
    print(f"\n[{label}] worst |dnll|/max|l| {worst_nll:.2e}, worst logits cosine {worst_cos:.6f}, argmax checked on {checked}/{n} rows")


@pytest.mark.parametrize("kv16", [False, True])
def test_decoder_score_small_models(wide, kv16):
    fmt, cfg, dec, prompt, olog = wide
    for n in (2, 77, T_WIDE):
        dec.reset()
        dec.set_kv_f16(kv16)
        dec.feed(prompt)
        res = dec.score(n, digits=2, logits_rows=n)
        assert res.nll.shape == (n - 1,) and res.argmax.shape == (n,) and res.logits.shape == (n, cfg.vocab) and res.ms > 0
        state = (dec.last_logits().tobytes(), dec.position(), dec.history(n + 1).tobytes(), dec.last_prefill_path())
        last = dec.last_logits()
        dec.reset()
        dec.set_kv_f16(kv16)
        dec.feed(prompt)
        dec.prefill(n, with_logits=True, digits=2)
        assert state == (dec.last_logits().tobytes(), dec.position(), dec.history(n + 1).tobytes(), dec.last_prefill_path()), (fmt, kv16, n)
        assert float(np.max(np.abs(res.logits[n - 1] - last))) <= 1e-3 * float(np.max(np.abs(last))), (fmt, kv16, n)
        against_oracle(res, olog, prompt, n, f"{fmt} kv16={kv16} n={n} path {dec.last_prefill_path()}")
    # the decoder goes on from where score left it
    dec.reset()
    dec.set_kv_f16(kv16)
    dec.feed(prompt[:77])
    dec.score(77)
    dec.run(1, with_logits=True)
    assert dec.position() == 78


def test_decoder_score_refusals(pkg, hip, synth):
    cfg, dec, _ = make_decoder(pkg, synth, dict(WIDE, n_layers=1, max_pos=64), "qk256")
    prompt = synth.prompt(10, cfg.vocab)
    dec.reset()
    dec.feed(prompt)
    with pytest.raises(pkg.BitNetHipError, match="n must be >= 2"):
        dec.score(1)
    with pytest.raises(pkg.BitNetHipError, match="feed"):
        dec.score(11)
    with pytest.raises(pkg.BitNetHipError, match="logits_rows"):
        dec.score(10, logits_rows=11)
    assert dec.position() == 0  # nothing ran
    dec.feed(synth.prompt(54, cfg.vocab))  # 64 fed = max_pos: n = 64 passes the fed check and meets the cache bound
    with pytest.raises(pkg.BitNetHipError, match="KV cache overflow"):
        dec.score(64)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 3. saturation
def test_score_after_an_f16_saturation(pkg, hip, oracle, synth):
    cfgd = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=1024, vocab=2048, max_pos=320, eps=1e-5, rope_theta=10000.0)
    cfg = synth.ModelConfig(**cfgd)
    glob = synth.make_globals(cfg)
    layers = [synth.make_layer(cfg, l, fmt="i2s", block=32) for l in range(cfg.n_layers)]
    layers[-1]["ffn_norm"] = layers[-1]["ffn_norm"].copy()
    layers[-1]["ffn_norm"][33] = 2e5
    om = oracle.OracleModel(cfg, [dict(w, ternary=32) for w in layers], glob, n_threads=8)
    T = 256
    prompt = synth.prompt(T, cfg.vocab)
    olog = np.stack([om.step(int(t), want_logits=True)[1] for t in prompt])
    om.close()
    _, dec, _ = make_decoder(pkg, synth, cfgd, "i2s", layers, glob)
    dec.reset()
    dec.feed(prompt)
    res = dec.score(T, digits=2, logits_rows=T)
    assert dec.saturation_fallbacks() == 1 and dec.last_prefill_path() == 0
    against_oracle(res, olog, prompt, T, "saturation")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 4. full depth
@pytest.mark.parametrize("fmt", ["qk256", "i2s"])
def test_full_depth_score_against_the_step_path(pkg, hip, synth, fmt):
    n = 4096
    cfg, dec, _ = make_decoder(pkg, synth, dict(synth.BITNET_2B_4T, max_pos=4160), fmt)
    prompt = synth.prompt(n, cfg.vocab)
    dec.reset()
    dec.feed(prompt)
    res = dec.score(n, digits=2, logits_rows=0)
    assert dec.last_prefill_path() == BENCH_PATH[fmt]
    dec.reset()
    dec.feed(prompt)
    worst, agree, checked, mism = 0.0, 0, 0, 0
    for r in range(n):
        dec.run(1, with_logits=True, use_graph=True)
        l = dec.last_logits()
        scale = float(np.max(np.abs(l)))
        if r < n - 1:
            d = abs(float(res.nll[r]) - sr.row_nll(l, int(prompt[r + 1])))
            worst = max(worst, d / scale)
            assert d <= ORACLE_REL * scale, (fmt, r, d, scale)
        want = sr.argmax(l)
        agree += int(res.argmax[r]) == want
        top2 = np.partition(l, -2)[-2:]
        if abs(float(top2[1] - top2[0])) > ORACLE_REL * scale:
            checked += 1
            mism += int(res.argmax[r]) != want
    print(f"\n[full depth {fmt}] worst |dnll|/max|l| {worst:.2e}, argmax agreement {agree}/{n}, mismatches beyond the gap bound {mism}/{checked}, "
          f"mean nll {float(np.mean(res.nll.astype(np.float64))):.4f}, score {res.ms:.1f} ms")
    assert mism == 0 and agree >= 0.99 * n
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the tool
def test_score_tool(pkg, hip, synth, tmp_path):
    over = dict(n_layers=2, vocab=4096, max_pos=512)
    ids = [list(synth.prompt(300, 4096)), [int(t) for t in (7 + 13 * np.arange(120)) % 4096]]
    f = tmp_path / "ids.txt"
    f.write_text("\n".join(" ".join(str(int(t)) for t in s) for s in ids) + "\n")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "score.py"), "--synthetic", "qk256", "--layers", "2", "--vocab", "4096", "--max-pos", "512",
           "--ids", str(f), "--dump-logit-steps", "3", "--logits-topk", "4"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout)
    for k in ("type", "tokens", "mean_nll", "ppl", "std_nll", "latency"):
        assert k in out
    assert out["type"] == "score" and out["tokens"] == 299 + 119 and "total_ms" in out["latency"]
    assert math.isclose(out["ppl"], math.exp(out["mean_nll"]), rel_tol=1e-12)
    assert len(out["logits_dump"]) == 3 and len(out["logits_dump"][0]["topk"]) == 4 and out["logits_dump"][1]["chosen_id"] == int(ids[0][2])
    cfg, dec, _ = make_decoder(pkg, synth, dict(synth.BITNET_2B_4T, **over), "qk256")
    v = []
    for s in ids:
        dec.reset()
        dec.feed(np.asarray(s, np.int32))
        v.append(dec.score(len(s)).nll)
    dec.close()
    t = sr.totals(np.concatenate(v))
    assert math.isclose(out["mean_nll"], t["mean_nll"], rel_tol=1e-12) and math.isclose(out["ppl"], t["ppl"], rel_tol=1e-12)
    p = subprocess.run(cmd + ["--max-tokens", "50"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout)["tokens"] == 50
