"""CPU checks of the sampler restatement (tests/sampler_ref.py) and of the sampler entry points' argument checks.

The restatement is what the device sampler (bitnet-rs_amd/csrc/kernels_sample.hip) is held against in test_sampling_gpu.py, so it
is pinned here: the ChaCha20 keystream against a published vector (and openssl, when present), the reference's own unit tests
(crates/bitnet-cli/src/sampling.rs:219-285) replayed, and the closed form of the count exponent the device uses."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as sr  # noqa: E402

ZERO_KEY_BLOCK0 = bytes.fromhex(
    "76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
    "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586")


def _bytes(words):
    return b"".join(w.to_bytes(4, "little") for w in words)


def test_chacha20_zero_key_block():
    """ChaCha20Rng::from_seed([0; 32]) block 0 (not seed_from_u64(0))."""
    assert _bytes(sr.chacha20_block([0] * 8, 0)) == ZERO_KEY_BLOCK0


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on PATH")
def test_chacha20_random_key_against_openssl():
    key = [int(x) for x in np.random.default_rng(7).integers(0, 2**32, 8, dtype=np.uint64)]
    kb = _bytes(key)
    # IETF form: the first 4 IV bytes are the (32-bit) block counter, the rest the nonce; counter 0..3 = the 64-bit form's
    out = subprocess.run(["openssl", "enc", "-chacha20", "-K", kb.hex(), "-iv", "00" * 16], input=b"\0" * 256, capture_output=True,
                         check=True).stdout
    assert out == b"".join(_bytes(sr.chacha20_block(key, b)) for b in range(4))


def test_rng_words_and_f32():
    r = sr.ChaCha20Rng(seed=42)
    words = [r.next_u32() for _ in range(20)]  # crosses a block boundary
    assert words[:16] == sr.chacha20_block(sr.pcg32_key(42), 0) and words[16:] == sr.chacha20_block(sr.pcg32_key(42), 1)[:4]
    r2 = sr.ChaCha20Rng(seed=42)
    u = r2.random_f32()
    assert u.dtype == np.float32 and u == np.float32(words[0] >> 8) * np.float32(2.0 ** -24) and 0 <= u < 1


def test_pcg32_seed_expansion_shape():
    k0, k1 = sr.pcg32_key(0), sr.pcg32_key(1)
    assert len(k0) == 8 and all(0 <= w < 2**32 for w in k0) and k0 != k1
    # first output by hand: state = 0 * MUL + INC
    s = 11634580027462260723
    xs = (((s >> 18) ^ s) >> 27) & 0xFFFFFFFF
    rot = s >> 59
    assert k0[0] == ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF


def test_powi_is_the_square_and_multiply_loop():
    assert sr.powi(np.float32(1.1), 0) == 1
    assert sr.powi(np.float32(1.1), 1) == np.float32(1.1)
    a = np.float32(1.1)
    # b = 5: r = a; a = a^2; a = a^4; r = a * a^4 -- one rounding per step
    a2 = np.float32(a * a)
    a4 = np.float32(a2 * a2)
    assert sr.powi(a, 5) == np.float32(a * a4)


# ---- the reference's own unit tests (sampling.rs:219-285) -----------------------------------------------------------------

def test_reference_argmax_and_tie():
    assert sr.argmax(np.array([1.0, 3.0, 2.0], np.float32)) == 1
    assert sr.argmax(np.array([1.0, 2.0, 2.0, 1.5], np.float32)) == 1
    assert sr.argmax(np.full(5, -np.inf, np.float32)) == 0
    assert sr.argmax(np.array([-0.0, 0.0], np.float32)) == 0


def test_reference_softmax():
    p = sr.softmax(np.array([1.0, 2.0, 3.0], np.float32))
    assert abs(float(p.sum()) - 1) < 1e-6 and p[2] > p[1] > p[0]


def test_reference_greedy_sampling():
    s = sr.RefSampler(0.0, 0, 1.0, 1.0, seed=42)
    assert s.sample(np.array([1.0, 3.0, 2.0], np.float32), []) == 1 and s.rng.draws == 0


def _top_k_filter(x, k):
    x = np.asarray(x, np.float32)
    order = sr.stable_desc(np.where(np.isnan(x), -np.inf, x))
    f = np.full_like(x, -np.inf)
    f[order[:k]] = x[order[:k]]
    return f


def test_reference_top_k_filter():
    f = _top_k_filter([1.0, 3.0, 2.0, 0.5], 2)
    assert f[3] == -np.inf and f[1] == 3.0 and f[2] == 2.0
    assert list(_top_k_filter([1.0, np.nan, 3.0], 2)) == [1.0, -np.inf, 3.0]


def test_top_k_boundary_tie_merges_the_zeros():
    """partial_cmp: -0.0 == +0.0, so the stable sort keeps the lower index of the two at the boundary."""
    f = _top_k_filter([1.0, -0.0, 0.0, -1.0], 2)
    assert f[1] == 0 and np.signbit(f[1]) and f[2] == -np.inf


def test_reference_top_p_filter_with_nan_and_sample_with_nan_logits():
    # top_p 0.9 over [1, NaN, 3]: softmax of [1, -inf, 3] = [0.119, 0, 0.881]; cumsum over [3, 1, -inf] passes 0.9 at index 1
    s = sr.RefSampler(1.0, 0, 0.9, 1.0, seed=42)
    s.sample(np.array([1.0, np.nan, 3.0], np.float32), [])
    assert s.last_path == "F" and s.rng.draws == 1
    s = sr.RefSampler(1.0, 0, 1.0, 1.0, seed=42)
    assert s.is_greedy()
    assert s.sample(np.array([np.nan, 0.0, 1.0], np.float32), []) != 0


def test_all_neg_inf_row_falls_through_to_the_last_index():
    s = sr.RefSampler(0.7, 0, 0.95, 1.0, seed=1)
    assert s.sample(np.full(10, -np.inf, np.float32), []) == 9 and s.rng.draws == 1


def test_count_exponent_closed_form_matches_the_literal_replay():
    rng = np.random.default_rng(3)
    gen = [int(t) for t in rng.integers(0, 6, 40)]
    counts: dict[int, int] = {}
    for c in range(len(gen) + 1):
        for g in gen[:c]:  # sampling.rs:38-40, the caller passing the whole list each call
            counts[g] = counts.get(g, 0) + 1
        for t in range(6):
            assert counts.get(t, 0) == sr.count_exponent(gen[:c], t)


def test_penalty_divides_positive_and_multiplies_the_rest():
    s = sr.RefSampler(0.0, 0, 1.0, 1.1, seed=0)
    s.counts = {0: 2, 1: 1, 3: 1}
    x = s.penalise(np.array([2.0, -2.0, 5.0, 0.0], np.float32))
    p2 = sr.powi(np.float32(1.1), 2)
    assert x[0] == np.float32(np.float32(2.0) / p2) and x[1] == np.float32(np.float32(-2.0) * np.float32(1.1)) and x[2] == 5 and x[3] == 0


# ---- the entry points, without a GPU --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(pkg):
    # build.py loaded by path, as pkg.build() does: another test module may have imported bitnet-rs_amd.build as a submodule,
    # whose attribute then shadows the package's build() function
    pkg._load_build_module().build()
    return pkg.load()


def test_sampler_entry_points_validate_arguments_without_a_gpu(pkg, lib):
    c = C.CDLL(lib.path)
    c.bitnet_hip_get_last_error.restype = C.c_char_p
    c.bitnet_hip_sampler_create.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    h = C.c_void_p()
    cases = [((float("nan"), 0, 1.0, 1.0), b"temperature"), ((-0.5, 0, 1.0, 1.0), b"temperature"), ((1.0, 0, float("nan"), 1.0), b"top_p"),
             ((1.0, 0, 1.0, 0.0), b"repetition_penalty"), ((1.0, 0, 1.0, -1.1), b"repetition_penalty"), ((1.0, -3, 1.0, 1.0), b"top_k")]
    for cfg, word in cases:
        assert c.bitnet_hip_sampler_create(1000, C.byref(pkg.SamplingConfig(*cfg, 0)), C.byref(h)) == pkg.ERR_INVALID_ARGUMENT
        assert word in c.bitnet_hip_get_last_error() and not h.value
    assert c.bitnet_hip_sampler_create(0, C.byref(pkg.SamplingConfig(1.0, 0, 1.0, 1.0, 0)), C.byref(h)) == pkg.ERR_INVALID_ARGUMENT
    assert b"vocab" in c.bitnet_hip_get_last_error()
    assert c.bitnet_hip_sampler_create(1000, None, C.byref(h)) == pkg.ERR_INVALID_ARGUMENT
    for name, args in (("bitnet_hip_sampler_configure", [None, None]), ("bitnet_hip_sampler_reset", [None]), ("bitnet_hip_sampler_draws", [None, None]),
                       ("bitnet_hip_sample_dev", [None, None, 10, None, None, None, None, None]), ("bitnet_hip_sample_host", [None, None, 10, None, 0, None])):
        f = getattr(c, name)
        f.argtypes = [C.c_size_t if isinstance(a, int) else C.c_void_p for a in args]
        assert f(*args) == pkg.ERR_INVALID_ARGUMENT, name
        assert b"Null" in c.bitnet_hip_get_last_error(), name
    c.bitnet_hip_sampler_destroy.argtypes = [C.c_void_p]
    c.bitnet_hip_sampler_destroy(None)  # a no-op


def test_python_binding_binds_the_sampler_at_load(lib):
    L = lib.c
    assert L.bitnet_hip_sample_dev.argtypes is not None and L.bitnet_hip_sample_host.argtypes is not None
    assert L.bitnet_hip_sampler_create.argtypes is not None and L.bitnet_hip_sampler_destroy.restype is None


# ---- the emitted ISA of the sampler (hipcc cross-compiles gfx950 without a GPU) ---------------------------------------------

@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="no hipcc")
def test_sampler_isa_writes_memory_only_through_vector_instructions(tmp_path):
    """The ticket, the counts and the token go through vector stores / vector atomics; no scalar-unit write to memory and no
    scalar-cache write-back or discard (the pattern is assembled so that this file does not spell those mnemonics)."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "bitnet-rs_amd", "csrc")
    out = str(tmp_path / "kernels_sample.s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{root}/include",
           f"-I{csrc}", "-S", "--cuda-device-only", os.path.join(csrc, "kernels_sample.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    text = open(out).read()
    s_ = "s" + "_"
    banned = re.compile(r"^\s*" + s_ + "(" + "|".join(["st" + "ore", "buffer_" + "st" + "ore", "scr" + "atch_" + "st" + "ore", "at" + "omic",
                                                      "buffer_" + "at" + "omic", "dc" + "ache_" + "wb", "dc" + "ache_" + "dis" + "card"]) + r")", re.M | re.I)
    body = text[text.index("k_sample"):]
    assert "global_atomic_add" in body  # the ticket
    assert not banned.search(text)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", text)  # no scratch
