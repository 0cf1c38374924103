"""host/dev_buffer.hpp, the one owner of device memory in the host layer, on the CPU.

(1) tests/host/dev_buffer_check.cpp -- a stand-alone program with a fake HIP runtime (malloc / free with counters) -- is built by the host
    compiler under the address and undefined-behaviour sanitizers and run: exit 0, no sanitizer report.  It asserts the life cycle of a
    buffer (alloc over a held block, move, borrow, alloc(0), a failed alloc, a group that grows) with the live-byte and live-block counts
    after every step.  The host library itself is never loaded under a sanitizer.
(2) the sources: outside dev_buffer.hpp nothing under host/ allocates or frees device memory, and the two decoder classes keep no raw
    pointer to device data as a member."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bitnet-rs_amd", "host")
HIP_INCLUDE = "/opt/rocm/include"


def test_dev_buffer_check_under_sanitizers(tmp_path):
    cxx = "g++"  # the compiler build.py builds the host library with
    exe = str(tmp_path / "dev_buffer_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-result", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-D__HIP_PLATFORM_AMD__", f"-I{HOST}", f"-I{HIP_INCLUDE}", os.path.join(ROOT, "tests", "host", "dev_buffer_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "dev_buffer_check: ok" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]


def _code(path):
    """the file without its comments"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_only_dev_buffer_allocates_and_frees():
    for name in sorted(os.listdir(HOST)):
        if name == "dev_buffer.hpp" or not name.endswith((".cpp", ".hpp")):
            continue
        calls = re.findall(r"\bhip(?:Malloc|Free)\w*\s*\(", _code(os.path.join(HOST, name)))
        assert not calls, (name, calls)


# the raw pointers the classes may keep: streams, events, graphs, and references to host objects
HANDLES = {"stream_", "comm_stream_", "sp_ev_pack_", "sp_ev_gather_", "batch_", "graph_", "graph_exec_", "bound_"}


@pytest.mark.parametrize("header", ["decoder.hpp", "batch_decoder.hpp"])
def test_no_raw_device_pointer_member(header):
    code = _code(os.path.join(HOST, header))
    code = code[code.index("namespace bitnet_host"):code.index('extern "C"', code.index("namespace bitnet_host"))]
    raw = []
    # member declarations `type *a_ = ..., *b_ = ...;` of a data type, or of void (an untyped buffer, or a handle)
    for m in re.finditer(r"^\s*(?:const\s+)?(float|double|void|u?int\d+_t|bitnet_hip_logprob_\w+)\s*(\*[^;()]*);", code, flags=re.M):
        for name in re.findall(r"\*+\s*(\w+_)\b", m.group(2)):
            if m.group(1) != "void" or name not in HANDLES:
                raw.append((m.group(1), name))
    assert not raw, raw
    assert "DevBuf<" in code
