"""The screened greedy head on the device, through the C ABI: bitnet_hip_head_screen_build_dev + bitnet_hip_logits_screen_dev against
bitnet_hip_logits_f16_dev (token, history, position: equal; rescored rows: the full head's logits as bits) and against the float64 model of
tests/head_screen_ref.py (ub per row, the largest lb).

Shapes: hidden 512 / 1024 / 2560 (4, 4 and 3 row pairs per wave; 2560 is the benchmark's instance), vocab 1 / 5 / 257 / 4099 -- no multiple
of the rows per wave or per workgroup, an odd count (the image pads a row), counts below the grid.

The tolerance on ub (and on the largest lb), with u = 2^-24, K = hidden / 32 + 16, y the activations, E_v the row, w_v = c_v r the half width:
  a_v      the device's s_v * (q_v . y) differs from the exact one by at most (2 g(d) + u)(|E_v| + rho_v)|y| < K u |E_v| |y| (kernels_head.hip, (3));
  w_v      the device's c_v and r are f32 evaluations of the model's formulas, each within 2^-15 of them: 2^-14 w_v;
  rounding t = a + w, its outward step and the store: 3 roundings of a value of size |ub|: 2^-22 |ub|.
  underflow squares of activations below 2^-63 vanish from the device's f32 norm (their roots total < sqrt(hidden) 2^-63: the 2^-55 in r is there
           for them), and roundings in the subnormal range add < 2^-100: c_v sqrt(hidden) 2^-63 + 2^-99;
tol_v = K u |E_v| |y| + 2^-14 w_v + 2^-22 |ub_v| + the underflow term, and the model's own float64 evaluation is exact to 2^-50 of that.  gamma = None there, so that y
is the input itself; the token checks run with and without the norm."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_screen_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5
HIDDENS = [512, 1024, 2560]
VOCABS = [1, 5, 257, 4099]
FILL = 0x7FC0DEAD
N_WG = 40  # 160 waves: vocab 1, 5 and 257 leave most of the grid without a row; 4099 gives every wave several sweeps


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(torch_, v):
    return torch_.tensor(v, dtype=torch_.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def inputs(hidden, vocab):
    return ref.cases(hidden, vocab)


def ws_views(ws, hidden, vocab, n_wg):
    """the workspace layout of include/bitnet_hip.h -> dict of numpy views"""
    v4, n4 = (vocab + 3) // 4 * 4, (n_wg + 3) // 4 * 4
    a = ws.cpu().numpy()
    o = v4 + n4 + hidden
    return dict(ub=a[:vocab], lb_max=a[v4:v4 + n_wg], x=a[v4 + n4:o], count=a[o:o + 3].view(np.uint32), rescored=a[o + 4:o + 4 + vocab])


def build_image(hip, torch_, table_d, hidden, vocab):
    n = hip.head_screen_bytes(hidden, vocab)
    assert n >= vocab * hidden + 8 * vocab
    image = torch_.full((n + 64,), 0x5A, dtype=torch_.uint8, device="cuda")
    hip.head_screen_build_dev(table_d, hidden, vocab, image)
    torch_.cuda.synchronize()
    assert bool((image[n:] == 0x5A).all())  # nothing past the stated size
    return image


def run_both(hip, torch_, table_d, image, x, gamma, hidden, vocab, n_wg=N_WG, pos=None, history=None, n_forced=None):
    """the full head and the screened head on the same inputs, fresh buffers each -> (full dict, screened dict)"""
    out = []
    nws = hip.head_screen_ws_bytes(hidden, vocab, n_wg) // 4
    for screened in (False, True):
        x_d = dev(torch_, x)
        g_d = None if gamma is None else dev(torch_, gamma)
        scratch = torch_.full((2 * n_wg,), 3e38, device="cuda")
        tok = i32(torch_, [-1])
        pos_d = None if pos is None else i32(torch_, [pos])
        hist_d = None if history is None else i32(torch_, history)
        nf_d = None if n_forced is None else i32(torch_, [n_forced])
        kw = dict(token=tok, pos=pos_d, history=hist_d, n_forced=nf_d)
        if screened:
            wsi = torch_.full((nws + 16,), FILL, dtype=torch_.int32, device="cuda")  # a NaN no kernel produces: what is still FILL was never written
            off = (vocab + 3) // 4 * 4 + (n_wg + 3) // 4 * 4 + hidden
            wsi[off:off + 4] = 0  # the counter words start at zero
            ws = wsi.view(torch_.float32)
            hip.logits_screen_dev(table_d, x_d, g_d, EPS, hidden, vocab, image, ws, scratch, n_wg, **kw)
            torch_.cuda.synchronize()
            assert bool((wsi[nws:] == FILL).all())  # nothing past the stated size
            d = ws_views(ws[:nws], hidden, vocab, n_wg)
        else:
            logits = torch_.zeros(vocab, device="cuda")
            hip.logits_f16_dev(table_d, x_d, g_d, EPS, hidden, vocab, logits, scratch, n_wg, **kw)
            torch_.cuda.synchronize()
            d = dict(logits=logits.cpu().numpy())
        d.update(token=int(tok.item()), pos=None if pos_d is None else int(pos_d.item()), history=None if hist_d is None else hist_d.cpu().numpy())
        out.append(d)
    return out


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("hidden", HIDDENS)
def test_screened_head_is_the_full_head(hip, torch_, hidden, vocab):
    """every input of the model's list: same token; ub and the largest lb within the derived tolerance of the float64 model; every rescored
    row carries the full head's bits, every row the model keeps is among them, every other entry of the rescored vector is untouched"""
    images = {}
    k = hidden / 32 + 16
    for tn, yn, table, y in inputs(hidden, vocab):
        if tn not in images:
            td = dev(torch_, table)
            images[tn] = (td, build_image(hip, torch_, td, hidden, vocab), ref.build(table))
        td, image, (q, s, c, rho, norm) = images[tn]
        full, scr = run_both(hip, torch_, td, image, y, None, hidden, vocab)
        tag = (hidden, vocab, tn, yn)
        assert scr["token"] == full["token"], tag
        assert np.array_equal(scr["x"].view(np.uint32), y.view(np.uint32)), tag
        # the rescored rows: the full head's bits, and as many as the counter says
        done = scr["rescored"].view(np.uint32) != FILL
        assert np.array_equal(scr["rescored"].view(np.uint32)[done], full["logits"].view(np.uint32)[done]), tag
        assert int(scr["count"][0]) == int(done.sum()) >= 1 and int(scr["count"][1]) == 1 and int(scr["count"][2]) == int(scr["count"][0]), tag
        lb, ub = ref.interval(y, q, s, c)
        kept, L = ref.keep(lb, ub)
        finite_case = yn in ("normal", "range40", "zero", "tiny") and tn != "nonfinite"
        if finite_case:
            # ub, lb against the model
            y64 = y.astype(np.float64)
            ny = np.sqrt((y64 * y64).sum())
            w = c * (ny * ref.UP10 + 2.0 ** -55)
            under = c * np.sqrt(hidden) * 2.0 ** -63 + 2.0 ** -99  # squares the f32 norm loses to underflow, subnormal roundings
            tol = k * 2.0 ** -24 * norm * ny + 2.0 ** -14 * w + 2.0 ** -22 * np.abs(ub) + under
            assert np.all(np.abs(scr["ub"].astype(np.float64) - ub) <= tol), (tag, np.abs(scr["ub"] - ub).max(), tol.min())
            i = int(np.argmax(lb))
            tol_l = k * 2.0 ** -24 * norm[i] * ny + 2.0 ** -14 * w[i] + 2.0 ** -22 * abs(L) + under[i]
            assert abs(float(scr["lb_max"].max()) - L) <= tol_l, tag
            # a row the model keeps by more than the tolerance must have been rescored; one it drops by more than it must not
            sure_in = ub - tol > L + tol_l
            sure_out = ub + tol < L - tol_l
            assert done[sure_in].all() and not done[sure_out].any(), tag
        elif tn == "nonfinite" and yn == "normal":
            assert done[[0, vocab // 2, vocab - 1][:vocab]].all() if vocab > 2 else done.all(), tag  # the rows with a non-finite entry
        else:
            assert done.all(), tag  # non-finite or out-of-range activations: every row is rescored
        if tn == "identical":
            assert int(scr["count"][0]) == vocab, tag


@pytest.mark.parametrize("hidden", HIDDENS)
def test_screen_screens(hip, torch_, hidden):
    """so that a screen that keeps everything cannot pass: seeded normal rows, 4099 of them; the model keeps at most vocab / 16, the device at
    most vocab / 8.  With the final norm and a gamma, as the decoder calls it."""
    vocab = 4099
    table = ref.tables(hidden, vocab)["normal"]
    td = dev(torch_, table)
    image = build_image(hip, torch_, td, hidden, vocab)
    q, s, c, _, _ = ref.build(table)
    rng = np.random.default_rng([13, hidden])
    gamma = rng.uniform(0.5, 1.5, hidden).astype(np.float32)
    for seed in (0, 1):
        x = ref.activations(hidden, seed)["normal"]
        x64 = x.astype(np.float64)
        d = x64 - x64.mean()
        y = (d / np.sqrt((d * d).mean() + EPS) * gamma).astype(np.float32)  # the model's view of LN(x) * gamma, to f32 rounding
        n_model = int(ref.keep(*ref.interval(y, q, s, c))[0].sum())
        assert n_model <= vocab // 16, (hidden, seed, n_model)
        full, scr = run_both(hip, torch_, td, image, x, gamma, hidden, vocab)
        assert scr["token"] == full["token"]
        n_dev = int(scr["count"][0])
        print(f"hidden {hidden} seed {seed}: model keeps {n_model}, device keeps {n_dev} of {vocab}")
        assert 1 <= n_dev <= vocab // 8, (hidden, seed, n_dev)
        done = scr["rescored"].view(np.uint32) != FILL
        assert done.sum() == n_dev and np.array_equal(scr["rescored"].view(np.uint32)[done], full["logits"].view(np.uint32)[done])


@pytest.mark.parametrize("hidden", HIDDENS)
def test_history_position_and_forced_tokens(hip, torch_, hidden):
    vocab = 257
    table = ref.tables(hidden, vocab)["normal"]
    td = dev(torch_, table)
    image = build_image(hip, torch_, td, hidden, vocab)
    x = ref.activations(hidden)["normal"]
    gamma = np.ones(hidden, np.float32)
    hist = [9, 8, 7, 6, 5, 4, 3, 2]
    for n_wg in (1, 40, 300):  # 300: more screening workgroups than the rescoring grid of 128
        for pos, n_forced in ((2, None), (2, 0), (2, 3), (2, 4), (2, 9)):  # p + 1 = 3: free, free, free (3 >= 3), forced, forced
            full, scr = run_both(hip, torch_, td, image, x, gamma, hidden, vocab, n_wg=n_wg, pos=pos, history=hist, n_forced=n_forced)
            tag = (hidden, n_wg, pos, n_forced)
            assert scr["token"] == full["token"] and scr["pos"] == full["pos"] == pos + 1, tag
            assert np.array_equal(scr["history"], full["history"]), tag
            forced = n_forced is not None and pos + 1 < n_forced
            assert scr["history"][pos + 1] == (hist[pos + 1] if forced else full["token"]), tag
    # a token without a position: nothing but the token moves
    full, scr = run_both(hip, torch_, td, image, x, gamma, hidden, vocab)
    assert scr["token"] == full["token"] and scr["pos"] is None


def test_ties_go_to_the_lowest_index(hip, torch_):
    """duplicated rows that hold the maximum: the first of them, as the full head picks"""
    hidden, vocab = 512, 257
    table = ref.tables(hidden, vocab)["normal"].copy()
    x = ref.activations(hidden)["normal"]
    top = (3.0 * np.sign(x)).astype(np.float16)
    for rows in ((200, 31, 77), (256, 255), (0, 256)):
        t = table.copy()
        t[list(rows)] = top
        td = dev(torch_, t)
        image = build_image(hip, torch_, td, hidden, vocab)
        full, scr = run_both(hip, torch_, td, image, x, None, hidden, vocab)
        assert full["token"] == min(rows) and scr["token"] == min(rows), rows


def test_sizes_and_refusals(hip, pkg):
    assert hip.head_screen_bytes(2560, 128256) == 128256 * 2560 + 8 * 128256
    assert hip.head_screen_bytes(512, 5) == 6 * 512 + 8 * 6  # an odd vocabulary is padded by one row
    for hidden in (0, 256, 1536, 3072, 8192):  # no instance: the decoder keeps the full head there
        assert hip.head_screen_bytes(hidden, 100) == 0 and hip.head_screen_ws_bytes(hidden, 100, 8) == 0
    assert hip.head_screen_ws_bytes(512, 100, 0) == 0
    with pytest.raises(pkg.BitNetHipError, match="no instance"):
        hip._check(hip.c.bitnet_hip_head_screen_build_dev(1, 1536, 100, 1, None))
    with pytest.raises(pkg.BitNetHipError, match="Null pointer"):
        hip._check(hip.c.bitnet_hip_logits_screen_dev(None, None, None, 1e-5, 512, 100, None, None, None, 8, None, None, None, None, None))
