"""CPU checks around the continuation attention (bitnet_hip_attention_extend_dev): the numpy restatement tests/extend_ref.py
against itself (a prompt continued in pieces IS the one-shot causal prompt; the cache layouts round-trip), and the loaded
library's refusals, which all happen before any device work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitnet-rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FAKE = 4096  # a non-null "device pointer": every refusal below happens before anything is dereferenced
D = 128


def tables(max_pos, rng):
    th = rng.uniform(0, 2 * np.pi, (max_pos, D // 2))
    return np.sin(th), np.cos(th)


@pytest.mark.parametrize("seed", range(6))
def test_pieces_equal_the_one_shot_prompt(seed):
    rng = np.random.default_rng(seed)
    n_kv = int(rng.choice([1, 2, 4]))
    n_heads = n_kv * int(rng.choice([1, 2, 4]))
    T = int(rng.integers(2, 150))
    sin, cos = tables(T, rng)
    qkv = rng.normal(0, 1.3, (T, (n_heads + 2 * n_kv) * D))
    want, k_all, v_all = er.causal_f64(qkv, n_heads, n_kv, sin, cos)
    cuts = np.unique(np.concatenate([[0, T], rng.integers(1, T, int(rng.integers(1, 5)))]))
    k_past, v_past = np.zeros((0, n_kv, D)), np.zeros((0, n_kv, D))
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, k_past, v_past = er.extend_f64(qkv[a:b], k_past, v_past, n_heads, n_kv, sin, cos)
        outs.append(o)
    got = np.concatenate(outs)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-12
    assert np.array_equal(k_past, k_all) and np.array_equal(v_past, v_all)


def test_first_row_sees_exactly_the_past_and_itself():
    rng = np.random.default_rng(11)
    n_heads, n_kv, past = 2, 1, 5
    sin, cos = tables(16, rng)
    qkv = rng.normal(0, 1, (past + 3, (n_heads + 2 * n_kv) * D))
    _, k_all, v_all = er.causal_f64(qkv[:past], n_heads, n_kv, sin, cos)
    out, _, _ = er.extend_f64(qkv[past:], k_all, v_all, n_heads, n_kv, sin, cos)
    changed = qkv.copy()
    changed[past + 1:] += 10.0  # later rows are invisible to the first new row
    out2, _, _ = er.extend_f64(changed[past:], k_all, v_all, n_heads, n_kv, sin, cos)
    assert np.array_equal(out[0], out2[0]) and not np.array_equal(out[1], out2[1])


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("max_pos,T,n_kv", [(64, 64, 1), (160, 37, 2), (100, 100, 5), (4096, 130, 2)])
def test_cache_layouts_round_trip(f16, max_pos, T, n_kv):
    rng = np.random.default_rng(T)
    k = rng.normal(0, 1, (T, n_kv, D)).astype(np.float16 if f16 else np.float32)
    v = rng.normal(0, 1, (T, n_kv, D)).astype(np.float16 if f16 else np.float32)
    C = er.chunks(max_pos)
    kf, vf = er.encode_k(k, max_pos, f16), er.encode_v(v, max_pos, f16)
    assert kf.size == vf.size == n_kv * C * 64 * D
    kd, vd = er.decode_k(kf, n_kv, max_pos, f16), er.decode_v(vf, n_kv, max_pos, f16)
    assert np.array_equal(kd[:T], k) and np.array_equal(vd[:T], v)
    assert not kd[T:].any() and not vd[T:].any()
    head = n_kv - 1
    for d, pos in ((0, 0), (1, T - 1), (127, T // 2), (64, min(T - 1, 63))):  # the index formula of the header, element by element
        assert kf[head * C * 64 * D + er.k_index(d, pos, f16)] == k[pos, head, d]
        assert vf[head * C * 64 * D + pos * D + d] == v[pos, head, d]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def test_symbols_are_exported_and_declared(pkg, lib):
    names = {"bitnet_hip_attention_extend_workspace_bytes", "bitnet_hip_attention_extend_dev"}
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    assert names <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert names <= set(pkg.declared_symbols())
    host = subprocess.check_output(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], text=True)
    assert {"bitnet_host_extend", "bitnet_host_rewind"} <= {line.split()[-1] for line in host.splitlines() if " T " in line}
    assert lib.c.bitnet_hip_attention_extend_dev.argtypes is not None and len(lib.c.bitnet_hip_attention_extend_dev.argtypes) == 16


def test_workspace_is_zero_for_refused_sizes_and_monotone(lib):
    ws = lib.attention_extend_workspace_bytes
    assert ws(4, 2, 0, 0) == 0          # seq_len >= 1
    assert ws(4, 0, 10, 10) == 0        # no KV heads
    assert ws(0, 2, 10, 10) == 0
    assert ws(5, 2, 10, 10) == 0        # heads not a multiple of KV heads
    assert ws(4, 2, 1 << 40, 1) == 0 and ws(4, 2, 1, 1 << 40) == 0 and ws(4, 2, (1 << 30) - 1, 1) == 0
    assert ws(4, 2, 0, 1) > 0
    for heads, kv in ((4, 2), (20, 5), (8, 8), (3, 3)):
        lens = [0, 1, 63, 64, 65, 200, 1000, 1023, 1024, 1025, 2047, 2048, 3264, 3265, 4000, 4096, 8192, 20000]
        grid = np.array([[ws(heads, kv, p, max(n, 1)) for n in lens] for p in lens], np.float64)
        assert (grid > 0).all()
        assert (np.diff(grid, axis=0) >= 0).all(), (heads, kv)  # in past_len
        assert (np.diff(grid, axis=1) >= 0).all(), (heads, kv)  # in seq_len
        # it holds the two f16 images of all past + seq keys
        assert ws(heads, kv, 1000, 24) >= 2 * kv * 1024 * D * 2


def call(lib, **kw):
    a = dict(qkv=FAKE, rope_sin=FAKE, rope_cos=FAKE, kcache=FAKE, vcache=FAKE, n_heads=4, n_kv=2, head_dim=128, max_pos=256, past_len=100,
             seq_len=27, workspace=FAKE, workspace_bytes=1 << 40, out=FAKE, flags=0)
    a.update(kw)
    lib.attention_extend_dev(a["qkv"], a["rope_sin"], a["rope_cos"], a["kcache"], a["vcache"], a["n_heads"], a["n_kv"], a["head_dim"], a["max_pos"],
                             a["past_len"], a["seq_len"], a["workspace"], a["workspace_bytes"], a["out"], a["flags"])


@pytest.mark.parametrize("kw,msg", [
    (dict(qkv=None), "Null pointer"),
    (dict(rope_sin=None), "Null pointer"),
    (dict(rope_cos=None), "Null pointer"),
    (dict(kcache=None), "Null pointer"),
    (dict(vcache=None), "Null pointer"),
    (dict(workspace=None), "Null pointer"),
    (dict(out=None), "Null pointer"),
    (dict(past_len=230), "KV cache overflow"),            # 230 + 27 > 256
    (dict(past_len=256, seq_len=1), "KV cache overflow"),
    (dict(past_len=1 << 62, seq_len=1), "KV cache overflow"),
    (dict(past_len=0, seq_len=257), "KV cache overflow"),
    (dict(seq_len=0), "seq_len"),
    (dict(head_dim=64), "head_dim 64 unsupported"),
    (dict(n_heads=5), "divisible"),
    (dict(flags=4), "unknown flag bits"),
    (dict(workspace_bytes=1000), "workspace too small"),
])
def test_refusals_before_device_work(pkg, lib, kw, msg):
    with pytest.raises(pkg.BitNetHipError, match=msg):
        call(lib, **kw)


def test_prep_kernel_compiles_without_scratch(tmp_path):
    """k_extend_prep for gfx950: no scratch, no spill, and the attention kernels beside it keep theirs at zero."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "kernels_prefill_attn.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{CSRC}", "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "kernels_prefill_attn.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = [k for k in usage if "k_extend_prep" in k]
    assert len(names) == 1, usage.keys()
    u = usage[names[0]]
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, u
    assert u["LDS Size [bytes/block]"] == 64 * 132 * 4, u
    body = open(out).read()
    start = body.index(names[0] + ":")
    body = body[start:body.index(".Lfunc_end", start)]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body  # the 16-byte accesses
    assert "scratch_" not in body
