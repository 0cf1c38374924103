"""The tiled matmul's host rules, pinned on both sides of every boundary (kernels_gemm.hip: gemm_token_tiles, gemm_five_tiles, the f16h split,
the fp6w form, the scale modes, the route between the int8 planes, the f16 matrix cores and the fp6 x fp4 form).

Each row of CASES is one small launch through the C ABI; it asserts what the launcher reports of its choice -- bitnet_hip_matmul_last_tile,
_last_wave_rows, _last_resident_fp4 -- and a clean return (or, for the one refusal, the error code and wording).  The other tests pin the
benchmark's instances only (2560 .. 13824 rows x 4096 tokens); the boundaries of the rules are pinned here.

The expected values are NOT derived from the rules: they were recorded on an MI355X from the library built at commit 08affb8 (the parent of
the launch-layer refactor that added this file), so that a change of the host code which moves a launch to another kernel, tile or row form
shows up as a difference against what that commit ran.  K = 256 throughout (many tokens on a tiny K are cheap); outputs are not compared here --
the parity files do that."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SILU, INT8, FP6, FP6_EXPAND, YH_QB32 = 1, 8, 16, 32, 64
K = 256


def T(digits, wave_tokens, waves, scale_mode, wave_rows=64, resident=False):
    return {"tile": {"digits": digits, "wave_tokens": wave_tokens, "waves": waves, "scale_mode": scale_mode}, "wave_rows": wave_rows, "resident": resident}


# id -> (entry, matrix, rows, m, digits, flags, expected).  entry: fused = bitnet_hip_matmul_fused_dev, f16 = _matmul_f16_dev, qb32 = _matmul_qb32_dev;
# matrix: qk256 (unscaled), i2s256 / i2s32 (f32 block scales), i2s32h (32-block scales that are f16 values); a "+pair" matrix is two of `rows / 2`
# rows interleaved for silu * up.
CASES = {
    # ---- int8 planes, 2 digits, unscaled, 512 rows = 2 row blocks (cover: 384 tiles)
    "i8_m2048": ("fused", "qk256", 512, 2048, 2, 0, T(2, 16, 4, 0)),
    "i8_m6400": ("fused", "qk256", 512, 6400, 2, 0, T(2, 32, 4, 0)),
    "i8_m12288": ("fused", "qk256", 512, 12288, 2, 0, T(2, 64, 4, 0)),   # 384 tiles: one round
    "i8_m16640": ("fused", "qk256", 512, 16640, 2, 0, T(2, 32, 4, 0)),   # 520 tiles: the tail rule
    "i8_flag_m12288": ("fused", "qk256", 512, 12288, 2, INT8, T(2, 64, 4, 0)),
    "i8_3dig": ("fused", "qk256", 512, 2048, 3, 0, T(3, 32, 4, 0)),
    "i8_4dig": ("fused", "qk256", 512, 2048, 4, 0, T(4, 32, 4, 0)),
    "i8_block256": ("fused", "i2s256", 512, 2048, 2, 0, T(2, 32, 8, 1)),
    "i8_block32_f32": ("fused", "i2s32", 512, 2048, 2, 0, T(2, 32, 8, 2)),
    "i8_block32_f16_3dig": ("fused", "i2s32h", 512, 2048, 3, 0, T(3, 32, 4, 3)),
    "i8_block32_f16_4dig": ("fused", "i2s32h", 512, 2048, 4, 0, T(4, 16, 4, 3)),
    "i8_block32_f16_int8_flag": ("fused", "i2s32h", 512, 2048, 2, INT8, T(2, 32, 4, 3)),
    # ---- 2 digits on f16 32-block scales: the f16 matrix cores behind the f16 row quantiser
    "f16q_m2048": ("fused", "i2s32h", 512, 2048, 2, 0, T(2, 16, 4, 4)),
    "f16q_m8192": ("fused", "i2s32h", 512, 8192, 2, 0, T(2, 64, 4, 4)),
    # ---- the f16 chain, 1280 rows = 5 row blocks of 256 or 4 of 320
    "chain_m1024": ("f16", "qk256", 1280, 1024, 2, 0, T(2, 16, 4, 5)),
    "chain_m2048": ("f16", "qk256", 1280, 2048, 2, 0, T(2, 32, 4, 5)),
    "chain_m4096": ("f16", "qk256", 1280, 4096, 2, 0, T(2, 64, 4, 5)),
    "chain_m8192": ("f16", "qk256", 1280, 8192, 2, 0, T(2, 64, 4, 5, 80)),   # 512 workgroups of 320 rows: one round against two
    "chain_m8192_silu": ("f16", "qk256+pair", 1280, 8192, 2, SILU, T(2, 64, 4, 5)),  # paired rows: no 320-row form
    "chain_scaled_m4096": ("f16", "i2s32h", 1280, 4096, 2, 0, T(2, 64, 4, 4)),
    "chain_scaled_m8192": ("f16", "i2s32h", 1280, 8192, 2, 0, T(2, 64, 4, 4, 80)),
    "chain_qb32_m4096": ("f16", "qk256", 1280, 4096, 2, YH_QB32, T(2, 64, 4, 5)),
    "chain_qb32_m8192": ("f16", "qk256", 1280, 8192, 2, YH_QB32, T(2, 64, 4, 5, 80)),
    "chain_qb32_m1024": ("f16", "qk256", 1280, 1024, 2, YH_QB32,
                         {"error": (-1, "FUSE_YH_QB32: this launch does not run 64-token tiles (too few rows for the QB32 hand-over)")}),
    # ---- the f16h split of the chain's wide launches
    "f16h_split": ("f16", "qk256", 6144, 4096, 2, 0, T(2, 128, 4, 5)),    # 24 row blocks, 16 on the 128-token kernel
    "f16h_whole": ("f16", "qk256", 3840, 4096, 2, 0, T(2, 128, 4, 5)),    # 15 x 32 = 480 workgroups: one round, all on f16h
    "f16h_whole_scaled": ("f16", "i2s32h", 3840, 4096, 2, 0, T(2, 128, 4, 4)),
    # ---- the fp6 x fp4 form
    "fp6_resident_m16384": ("fused", "qk256", 512, 16384, 2, FP6, T(2, 64, 4, 6, 128, True)),   # fp6w
    "fp6_expand_m16384": ("fused", "qk256", 512, 16384, 2, FP6 | FP6_EXPAND, T(2, 64, 4, 6, 64, False)),
    "fp6_rows1280_m8192": ("fused", "qk256", 1280, 8192, 2, FP6, T(2, 64, 4, 6, 80, True)),
    "fp6_rows1280_m8192_expand": ("fused", "qk256", 1280, 8192, 2, FP6 | FP6_EXPAND, T(2, 64, 4, 6, 80, False)),
    "fp6_m8192": ("fused", "qk256", 512, 8192, 2, FP6, T(2, 32, 4, 6, 64, True)),
    "fp6_m2048": ("fused", "qk256", 512, 2048, 2, FP6, T(2, 16, 4, 6, 64, True)),
    "fp6_m2048_expand": ("fused", "qk256", 512, 2048, 2, FP6 | FP6_EXPAND, T(2, 16, 4, 6, 64, False)),
    "fp6_m1000": ("fused", "qk256", 512, 1000, 2, FP6, T(2, 16, 4, 6, 64, True)),   # under 2048 rows: the workgroup-per-row quantiser
    # ---- the QB32 consumer
    "qb32_m16384": ("qb32", "qk256", 512, 16384, 2, 0, T(2, 64, 4, 8, 64, True)),
    "qb32_m8192": ("qb32", "qk256", 512, 8192, 2, 0, T(2, 32, 4, 8, 64, True)),
    "qb32_m8192_silu": ("qb32", "qk256+pair", 512, 8192, 2, SILU, T(2, 32, 4, 8, 64, True)),
}
# the f16h split again with the switch off: the whole launch on the 64-token kernel (read once per process: a child process)
ENV_CASES = {"f16h_split": ({"BITNET_HIP_GEMM_F16H": "0"}, T(2, 64, 4, 5))}


def make_matrix(hip, rng, kind, rows):
    if kind == "qk256":
        return hip.weights_upload_qk256(rng.integers(0, 256, rows * (K // 4), dtype=np.uint8), rows, K, K // 4)
    block = 256 if kind == "i2s256" else 32
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(rows, K), p=[0.5, 0.25, 0.25])
    packed = (codes[:, 0::4] | codes[:, 1::4] << 2 | codes[:, 2::4] << 4 | codes[:, 3::4] << 6).astype(np.uint8)
    scales = (1.0 / ((np.arange(rows * (K // block)) % 100) + 1)).astype(np.float32)
    if kind == "i2s32h":
        scales = scales.astype(np.float16).astype(np.float32)
    return hip.weights_upload_i2s(packed.reshape(-1), scales, rows, K, block)


def run_case(hip, torch, name):
    """-> (what the launcher reported, or {"error": (code, message)}; the output tensor or None)"""
    entry, kind, rows, m, digits, flags, _ = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    handles = []
    if kind.endswith("+pair"):
        handles = [make_matrix(hip, rng, kind[:-5], rows // 2) for _ in range(2)]
        h = hip.weights_concat(handles, interleave16=True)
    else:
        h = make_matrix(hip, rng, kind, rows)
    handles.append(h)
    out_rows = rows // 2 if flags & SILU else rows
    mp = -(-m // 64) * 64
    x = torch.from_numpy(rng.normal(0.0, 1.0, (m, K)).astype(np.float32)).cuda()
    y = torch.full((m, out_rows), float("nan"), device="cuda")
    try:
        if entry == "fused":
            wsb = hip.matmul_workspace_bytes(m, K, digits)
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            hip.matmul_fused_dev(h, x, y, m, ws, wsb, flags=flags, digits=digits)
        elif entry == "f16":
            xh = torch.zeros(mp, K, dtype=torch.float16, device="cuda")
            hip.rows_to_f16_dev(x, None, m, K, xh, None)
            yh = torch.zeros(hip.qb32_bytes(m, rows), dtype=torch.uint8, device="cuda") if flags & YH_QB32 else None
            hip.matmul_f16_dev(h, xh, m, y=y, flags=flags, yh=yh)
        else:
            qb = torch.zeros(hip.qb32_bytes(m, K), dtype=torch.uint8, device="cuda")
            hip.rows_to_qb32_dev(x, None, m, K, qb, None)
            hip.matmul_qb32_dev(h, qb, m, y=y, flags=flags)
        torch.cuda.synchronize()
        got = {"tile": dict(hip.matmul_last_tile()), "wave_rows": hip.matmul_last_wave_rows(), "resident": hip.matmul_last_resident_fp4()}
    except Exception as e:  # the C ABI's refusals arrive as BitNetHipError(code, message)
        if not hasattr(e, "code"):
            raise
        got, y = {"error": (e.code, str(e))}, None
    for hh in handles:
        hip.weights_free(hh)
    return got, y


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


@pytest.mark.parametrize("name", list(CASES))
def test_launcher_choice_is_what_the_parent_commit_ran(hip, torch_, name):
    got, y = run_case(hip, torch_, name)
    want = CASES[name][-1]
    print(name, json.dumps(got))
    if "error" in want:
        assert got.get("error") == want["error"], got
        return
    assert got == want, (name, got, want)
    assert bool(torch_.isfinite(y).all())  # a clean return: every output element was written


_CHILD = r"""
import importlib, json, sys
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
pkg = importlib.import_module("bitnet-rs_amd")
hip = pkg.load(); hip.init(0)
import test_gemm_dispatch_gpu as D
got, y = D.run_case(hip, torch, {name!r})
print("GOT", json.dumps([got, bool(torch.isfinite(y).all())]))
"""


@pytest.mark.parametrize("name", list(ENV_CASES))
def test_launcher_choice_under_an_environment_switch(name):
    env, want = ENV_CASES[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=root, name=name)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    got, finite = json.loads([l for l in p.stdout.splitlines() if l.startswith("GOT ")][0][4:])
    print(name, env, json.dumps(got))
    assert got == want and finite, (name, got, want)
