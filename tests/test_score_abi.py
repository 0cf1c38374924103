"""CPU-side checks of the scoring entries (include/bitnet_hip.h bitnet_hip_score_*, host/decoder.hpp Decoder::score): they are exported,
refuse bad arguments before any device work, a dead decoder refuses score, and the head kernel compiles for gfx950 to the f16 matrix
instruction with no scratch.  No GPU compute here (n < 2 / n > fed need a live decoder: tests/test_score_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitnet-rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FAKE = 4096  # a non-null "device pointer": every refusal below happens before anything is dereferenced


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


def test_symbols_are_exported(pkg, lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"bitnet_hip_score_workspace_bytes", "bitnet_hip_score_f16_dev"} <= exported
    assert {"bitnet_hip_score_workspace_bytes", "bitnet_hip_score_f16_dev"} <= set(pkg.declared_symbols())
    host = subprocess.check_output(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], text=True)
    assert any(line.split()[-1] == "bitnet_host_score" for line in host.splitlines() if " T " in line)


def test_workspace_bytes(lib):
    # f16 rows padded to 128 | 4-byte target logits | 16-byte partial per (row, 128-entry vocabulary block)
    assert lib.score_workspace_bytes(4096, 2560, 128256) == 4096 * 2560 * 2 + 4096 * 4 + 4096 * 1002 * 16
    assert lib.score_workspace_bytes(1, 512, 1000) == 128 * 512 * 2 + 512 + 128 * 8 * 16
    assert lib.score_workspace_bytes(0, 512, 1000) == 0
    assert lib.score_workspace_bytes(1, 512, 0) == 0
    assert lib.score_workspace_bytes(1 << 62, 2560, 128256) == 0


def call(lib, **kw):
    a = dict(table=FAKE, x=FAKE, gamma=FAKE, eps=1e-5, hidden=512, vocab=1000, n_rows=4, targets=FAKE, nll=FAKE, argmax=None, logits=None,
             logits_rows=0, workspace=FAKE, workspace_bytes=1 << 40)
    a.update(kw)
    lib.score_f16_dev(a.pop("table"), a.pop("x"), a.pop("gamma"), a.pop("eps"), a.pop("hidden"), a.pop("vocab"), a.pop("n_rows"), a.pop("targets"),
                      a.pop("nll"), **a)


@pytest.mark.parametrize("kw,msg", [
    (dict(table=None), "Null pointer"),
    (dict(x=None), "Null pointer"),
    (dict(targets=None), "Null pointer"),
    (dict(nll=None), "Null pointer"),
    (dict(workspace=None), "Null pointer"),
    (dict(logits_rows=2, logits=None), "Null pointer"),
    (dict(hidden=100), "multiple of 64"),
    (dict(hidden=0), "multiple of 64"),
    (dict(vocab=0), "must be > 0"),
    (dict(n_rows=0), "must be > 0"),
    (dict(logits_rows=5, logits=FAKE), "logits_rows 5 > n_rows 4"),
    (dict(n_rows=1 << 40), "too large"),
    (dict(vocab=1 << 40), "too large"),
    (dict(hidden=1 << 40), "too large"),
    (dict(logits_rows=1 << 62, n_rows=1 << 62, logits=FAKE), "too large"),
    (dict(workspace_bytes=1000), "workspace too small: 147968 bytes needed, 1000 given"),
])
def test_refusals_before_device_work(pkg, lib, kw, msg):
    with pytest.raises(pkg.BitNetHipError, match=msg) as e:
        call(lib, **kw)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT


def test_dead_decoder_refuses_score(pkg):
    c = C.CDLL(pkg.HOST_LIB_PATH)
    c.bitnet_host_create.restype = C.c_void_p
    c.bitnet_host_create.argtypes = [C.POINTER(pkg.HostConfig)]
    c.bitnet_host_destroy.argtypes = [C.c_void_p]
    c.bitnet_host_score.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    hc = pkg.HostConfig(hidden=100, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=128, ffn=256, vocab=64, max_pos=32, eps=1e-5, rope_theta=1e4)
    d = c.bitnet_host_create(C.byref(hc))
    assert d
    nll = (C.c_float * 64)()
    try:
        assert c.bitnet_host_score(d, 4, 2, nll, None, None, 0, None) != 0
        assert c.bitnet_host_score(None, 4, 2, nll, None, None, 0, None) != 0
    finally:
        c.bitnet_host_destroy(d)


def test_head_uses_the_f16_matrix_instruction_without_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "kernels_score.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{CSRC}", "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "kernels_score.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = {k for k in usage if re.search(r"k_score_(rows_f16|head|combine)", k)}
    assert len(names) == 3, usage.keys()
    for k in names:
        assert usage[k]["ScratchSize [bytes/lane]"] == 0 and usage[k]["VGPRs Spill"] == 0, (k, usage[k])
    lines = open(out).read().split("\n")
    head = next(k for k in names if "k_score_head" in k)
    start = next(i for i, l in enumerate(lines) if l.startswith(head + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = "\n".join(lines[start:end])
    assert body.count("v_mfma_f32_16x16x32_f16") >= 32
    assert "global_load_lds_dwordx4" in body
    assert "scratch_" not in body and "buffer_store" not in body
