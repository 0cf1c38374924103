"""csrc/wave.hpp stands on its own (CPU only: hipcc cross-compiles gfx950 without a GPU).

wave.hpp is the one home of the lane helpers under every kernel; qact.hpp builds on it, and gemvq_stages.hpp holds the stages the QAct GEMV
and its batched form share.  Three translation units, each including ONLY one of the three, each hold one kernel that calls every reduction of
wave.hpp once on a value loaded from memory and stores the results; qact.hpp's also calls its three format helpers, gemvq_stages.hpp's every
stage.  All must compile device-only for gfx950 with -Wall -Werror, and the compiler's resource report must show no scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitnet-rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

REDUCTIONS_F = ("row16_sum_f", "row16_max_abs", "wave64_sum_f_xor", "wave64_max_f_xor", "wave64_sum_f_rows_readlane", "wave64_max_f_rows_readlane",
                "wave64_max_f_rows_xor", "wave64_max_bits_rows_bcast")
REDUCTIONS_D = ("row16_sum_d", "wave64_sum_d_rows_readlane", "wave64_sum_d_rows_permlane", "wave64_sum_d_xor")
REDUCTIONS_BLOCK = ("block256_sum_f", "block256_max_f")

KERNEL = """#include "%s"
using namespace bitnet_hip;
__global__ __launch_bounds__(256) void k_all(const float *x, float *yf, double *yd) {
    __shared__ float slot[4];
    const int t = threadIdx.x;
    const float v = x[t];
    const double d = (double)x[256 + t];
    float *of = yf + %d * t;
    double *od = yd + %d * t;
%s}
"""


QACT_FORMAT = ("qact_scales", "qact_digits", "qact_scale_slot")
STAGES = ("ring_block", "gemvq_block_value", "sum_kgroups", "ln_from_sums", "ln_row_stats")
# what a header has beyond wave.hpp, every function of it called once: lines of the kernel body (results stored through of / od), extra slots
EXTRA = {
    "qact.hpp": ("""    float sc, as;
    qact_scales(__float_as_uint(row16_max_abs(v)), sc, as);
    of[NF] = (float)qact_digits(v, sc);
    *qact_scale_slot(reinterpret_cast<uint8_t *>(yd), t >> 4) = as;
""", 1, 0),
    "gemvq_stages.hpp": ("""    of[NF] = (float)ring_block(t, 7, 3);
    of[NF + 1] = gemvq_block_value(v4i{t, 2 * t, 3 * t, 5 * t}, float4{v, 2.0f * v, 3.0f * v, 5.0f * v}, t & 1);
    of[NF + 2] = sum_kgroups(v);
    ln_from_sums(d, d * d, 0.5, 1e-5f, &od[ND], &od[ND + 1]);
    ln_row_stats(reinterpret_cast<const uint8_t *>(x), 32, t & 63, 0.5, 1e-5f, od[ND + 2], od[ND + 3]);
""", 3, 4),
}


def source(header):
    f = REDUCTIONS_F + REDUCTIONS_BLOCK
    body = "".join(f"    of[{i}] = {n}(v{', slot' if n in REDUCTIONS_BLOCK else ''});\n" for i, n in enumerate(f))
    body += "".join(f"    od[{i}] = {n}(d);\n" for i, n in enumerate(REDUCTIONS_D))
    extra, nf, nd = EXTRA.get(header, ("", 0, 0))
    body += extra.replace("NF", str(len(f))).replace("ND", str(len(REDUCTIONS_D)))
    return KERNEL % (header, len(f) + nf, len(REDUCTIONS_D) + nd, body)


@pytest.mark.parametrize("header, names", [("qact.hpp", QACT_FORMAT), ("gemvq_stages.hpp", STAGES)])
def test_every_helper_of_the_header_is_called(header, names):
    """a format helper added to qact.hpp, or a stage added to gemvq_stages.hpp, has to be listed above and called in EXTRA"""
    text = open(os.path.join(CSRC, header)).read()
    defined = set(re.findall(r"^__device__ __forceinline__ [\w ]+?[ *](\w+)\(", text, re.M)) - {"qact_emit"}
    assert defined == set(names)
    assert all(n + "(" in EXTRA[header][0] for n in names)


def test_every_reduction_of_the_header_is_listed():
    """a reduction added to wave.hpp has to be added above too"""
    text = open(os.path.join(CSRC, "wave.hpp")).read()
    defined = set(re.findall(r"^__device__ __forceinline__ \w+ ((?:row16|wave64|block256)_\w+)\(", text, re.M))
    assert defined == set(REDUCTIONS_F + REDUCTIONS_D + REDUCTIONS_BLOCK)


@pytest.mark.parametrize("header", ["wave.hpp", "qact.hpp", "gemvq_stages.hpp"])
def test_header_alone_compiles_for_gfx950_without_scratch(header, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src = tmp_path / "tu.hip"
    src.write_text(source(header))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-command-line-argument", f"-I{CSRC}", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / "tu.s")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "Function Name: _Z5k_allPKfPfPd" in p.stderr, p.stderr[-3000:]
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)
    assert scratch == ["0"], p.stderr[-3000:]
    asm = (tmp_path / "tu.s").read_text()
    assert "v_permlane16_swap" in asm and "row_bcast:15" in asm and "ds_bpermute" in asm  # the variants are all there, none folded into another
