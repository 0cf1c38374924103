#!/usr/bin/env python3
"""Prints the Rust `extern "C"` declaration of every entry point include/bitnet_hip.h declares (one line each), or with --missing only those
INTEGRATION.md section 2 does not spell out yet.  A mechanical map of the C prototypes (size_t -> usize, const T * -> *const T, ...); the
by-value / by-pointer structs and the opaque sampler are referred to by the names INTEGRATION.md gives them.   python tools/gen_rust_extern.py [--missing]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitnet-rs_amd"))
import cproto  # noqa: E402 -- the one header parser (the ctypes bindings derive from it too)

BASE = {"size_t": "usize", "int": "c_int", "float": "c_float", "double": "f64", "void": "c_void", "char": "c_char", "uint8_t": "u8", "int8_t": "i8",
        "uint16_t": "u16", "uint32_t": "u32", "int32_t": "i32", "uint64_t": "u64", "int64_t": "i64", "unsigned long long": "u64", "unsigned": "u32",
        "bitnet_hip_weights_t": "Weights", "bitnet_hip_device_info": "DeviceInfo", "bitnet_hip_gemv_item": "GemvItem", "_Float16": "u16",
        "bitnet_hip_sampling_config": "SamplingConfig", "bitnet_hip_sampling_config_ex": "SamplingConfigEx", "bitnet_hip_sampler": "Sampler", "bitnet_hip_sample_batch": "SampleBatch", "bitnet_hip_logprob_args": "LogprobArgs",
        "bitnet_hip_gemv_q_geometry_t": "GemvQGeometry", "bitnet_hip_gemv_geometry_t": "GemvGeometry", "bitnet_hip_mirostat_config": "MirostatConfig", "bitnet_hip_stop_config": "StopConfig", "bitnet_hip_stop_state": "StopState", "bitnet_hip_stop": "Stop",
        "bitnet_hip_stop_batch": "StopBatch", "bitnet_hip_constraints": "Constraints", "bitnet_hip_grammar_desc": "GrammarDesc", "bitnet_hip_grammar": "Grammar"}


def rust_type(c: str) -> str:
    c = c.strip()
    stars = c.count("*")
    c = c.replace("*", " ").replace("struct ", " ")
    const = bool(re.search(r"\bconst\b", c))
    base = re.sub(r"\bconst\b", " ", c).strip()
    base = re.sub(r"\s+", " ", base)
    t = BASE[base]
    for i in range(stars):
        t = ("*const " if const and i == 0 else "*mut ") + t
    return t


def prototypes(header: str):
    for name, ret, params in cproto.prototypes(header, "bitnet_hip_"):
        r = "" if ret == "void" else " -> " + rust_type(ret)
        yield name, "pub fn %s(%s)%s;" % (name, ", ".join(f"{n}: {rust_type(t)}" for t, n in params), r)


def main():
    header = open(os.path.join(ROOT, "include", "bitnet_hip.h")).read() + open(os.path.join(ROOT, "include", "bitnet_hip_grammar.h")).read()
    header += open(os.path.join(ROOT, "include", "bitnet_hip_kvsnap.h")).read() + open(os.path.join(ROOT, "include", "bitnet_hip_widetail.h")).read()
    have = set(re.findall(r"pub fn (bitnet_hip_[a-z0-9_]+)", open(os.path.join(ROOT, "INTEGRATION.md")).read())) if "--missing" in sys.argv else set()
    for name, line in prototypes(header):
        if name not in have:
            print("    " + line)


if __name__ == "__main__":
    main()
