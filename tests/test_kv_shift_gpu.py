"""GPU: bitnet_hip_kv_shift_dev (include/bitnet_hip.h) on raw buffers, no decoder: in place, slot j of every layer's K and V takes slot j + discard
for j in [keep, n - discard), V bit for bit, K re-rotated between RoPE table rows j + discard and j; every other byte keeps its value.

The caches are written directly through tests/extend_ref.py's encode_k / encode_v -- every slot, the padding of the last chunk included, holds
normal-range random data with exact zeros and -0.0 planted -- into ONE device arena with 256-byte guard gaps in front of, between and behind them.
The expected bytes are tests/shift_ref.py's shift_f32 (numpy float32, operation by operation) encoded the same way, and the comparison is over the
WHOLE arena: moved slots, untouched slots, padding and guards in one equality.  There is no tolerance anywhere.

max_pos 300 (5 chunks, the last partial) with n_kv in {1, 2, 5}, 1 and 3 layers, both cache types, and the (keep, discard, n) list below: one
position, whole chunks, shifts one short of / one past a chunk, the disjoint edge moved == discard and one past it (where the ranges start to
overlap and one workgroup walks a segment), and two calls that move nothing.  Then max_pos 1024 (16 chunks): the smallest size at which a
chunk-parallel decomposition that reads a slot after another workgroup overwrote it is likely to show."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402
import shift_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

D = er.D
GUARD = 64  # 32-bit words between two caches of an arena (256 bytes: every cache stays 16-byte aligned)
THETA = 5e5
SMALL = [(0, 1, 2), (0, 64, 128), (3, 1, 299), (4, 63, 297), (4, 65, 297), (64, 64, 299), (5, 147, 299), (5, 146, 299), (0, 299, 299), (100, 199, 299)]
CACHE_F16, OUT_F16 = 1, 2  # bitnet_hip_attention_extend_dev's flags


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


class Caches:
    """K and V of n_layers layers ([slots, kv, D] each, slots = whole chunks) in ONE device arena: K of layer l is cache l, V cache n_layers + l"""

    def __init__(self, torch, rng, n_layers, n_kv, max_pos, f16):
        self.torch, self.n_layers, self.n_kv, self.max_pos, self.f16 = torch, n_layers, n_kv, max_pos, f16
        self.slots = er.chunks(max_pos) * 64
        dt = np.float16 if f16 else np.float32
        self.words = n_kv * self.slots * D // (2 if f16 else 1)
        self.host = rng.integers(0, 1 << 32, size=GUARD + 2 * n_layers * (self.words + GUARD), dtype=np.uint32)
        self.k, self.v = [], []
        for l in range(n_layers):
            k, v = (rng.standard_normal((self.slots, n_kv, D)).astype(dt) for _ in range(2))
            for a in (k, v):  # exact zeros and -0.0, in moved slots and elsewhere
                at = rng.integers(0, a.size, a.size // 50)
                a.reshape(-1)[at[::2]] = 0.0
                a.reshape(-1)[at[1::2]] = -0.0
            self.k.append(k), self.v.append(v)
            self.view(self.host, l)[:] = er.encode_k(k, max_pos, f16).view(np.uint32)
            self.view(self.host, n_layers + l)[:] = er.encode_v(v, max_pos, f16).view(np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        table = lambda ptrs: torch.tensor(ptrs, dtype=torch.int64, device="cuda")
        self.k_ptrs = table([self.ptr(l) for l in range(n_layers)])
        self.v_ptrs = table([self.ptr(n_layers + l) for l in range(n_layers)])
        sin, cos = sr.rope_tables(max_pos, THETA)
        self.sin, self.cos = sin, cos
        self.sin_d, self.cos_d = torch.from_numpy(sin).cuda(), torch.from_numpy(cos).cuda()

    def offset(self, i):
        return GUARD + i * (self.words + GUARD)

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.offset(i)

    def view(self, host, i):
        return host[self.offset(i):self.offset(i) + self.words]

    def restore(self):
        self.dev.copy_(self.torch.from_numpy(self.host.view(np.int32)))

    def read(self):
        return self.dev.cpu().numpy().view(np.uint32)

    def shift(self, hip, keep, discard, n):
        hip.kv_shift_dev(self.k_ptrs, self.v_ptrs, self.sin_d, self.cos_d, self.n_layers, self.n_kv, D, self.max_pos, keep, discard, n, kv_f16=self.f16)
        self.torch.cuda.synchronize()

    def expected(self, steps):
        """the arena after the (keep, discard, n) calls of `steps`, and the final per-layer (k, v)"""
        want = self.host.copy()
        out = []
        for l in range(self.n_layers):
            k, v = self.k[l], self.v[l]
            for keep, discard, n in steps:
                k, v = sr.shift_f32(k, v, self.sin, self.cos, keep, discard, n)
            self.view(want, l)[:] = er.encode_k(k, self.max_pos, self.f16).view(np.uint32)
            self.view(want, self.n_layers + l)[:] = er.encode_v(v, self.max_pos, self.f16).view(np.uint32)
            out.append((k, v))
        return want, out

    def check(self, steps, what):
        want, out = self.expected(steps)
        got = self.read()
        bad = np.flatnonzero(got != want)
        if bad.size:
            w = int(bad[0])
            cache = (w - GUARD) // (self.words + GUARD)
            inside = w - self.offset(cache)
            where = "a guard word" if not 0 <= inside < self.words else f"{'V' if cache >= self.n_layers else 'K'} of layer {cache % self.n_layers}, word {inside}"
            pytest.fail(f"{what}: {bad.size} words differ, first at arena word {w} ({where}): got {got[w]:#010x}, want {want[w]:#010x}")
        return out


def test_the_test_encodes_what_it_decodes():
    """CPU-side sanity of the arena's expected bytes: encode(decode(x)) is the identity on bits, -0.0 included"""
    rng = np.random.default_rng(0)
    for f16 in (False, True):
        k = rng.standard_normal((320, 2, D)).astype(np.float16 if f16 else np.float32)
        k[3, 1, 5] = -0.0
        flat = er.encode_k(k, 300, f16)
        assert np.array_equal(er.decode_k(flat, 2, 300, f16).view(np.uint8), k.view(np.uint8))
        flat = er.encode_v(k, 300, f16)
        assert np.array_equal(er.decode_v(flat, 2, 300, f16).view(np.uint8), k.view(np.uint8))


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("n_kv", [1, 2, 5])
def test_shift_moves_the_slots_and_nothing_else(hip, torch_, n_kv, n_layers, f16):
    rng = np.random.default_rng(100 * n_kv + 10 * n_layers + int(f16))
    c = Caches(torch_, rng, n_layers, n_kv, 300, f16)
    for keep, discard, n in SMALL:
        c.restore()
        c.shift(hip, keep, discard, n)
        c.check([(keep, discard, n)], f"keep={keep} discard={discard} n={n}")


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
def test_sixteen_chunks_overlapped_and_disjoint(hip, torch_, f16):
    rng = np.random.default_rng(1024 + int(f16))
    c = Caches(torch_, rng, 2, 5, 1024, f16)
    for discard in (1, 63, 64, 65, 509, 510):  # 509: moved 510 > discard, one workgroup per segment; 510: moved 509, split over parts
        c.restore()
        c.shift(hip, 4, discard, 1023)
        c.check([(4, discard, 1023)], f"max_pos 1024 keep=4 discard={discard} n=1023")


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
def test_two_shifts_in_a_row(hip, torch_, f16):
    rng = np.random.default_rng(77 + int(f16))
    c = Caches(torch_, rng, 2, 2, 300, f16)
    c.shift(hip, 4, 100, 299)
    c.shift(hip, 4, 30, 199)
    c.check([(4, 100, 299), (4, 30, 199)], "shift(4, 100) at 299, then shift(4, 30) at 199")


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
def test_the_continuation_attention_reads_a_shifted_cache(hip, torch_, f16):
    """bitnet_hip_attention_extend_dev, 3 new tokens at past = n - discard over the shifted cache of one layer, against extend_ref.extend_f64 fed
    the restated K and V (tests/test_extend_gpu.py's gates: max|diff| <= 6e-3, cosine >= 0.999995)"""
    torch = torch_
    n_heads, n_kv, max_pos, keep, discard, n, new = 4, 2, 300, 4, 147, 299, 3
    rng = np.random.default_rng(5 + int(f16))
    c = Caches(torch, rng, 1, n_kv, max_pos, f16)
    c.shift(hip, keep, discard, n)
    (k, v), = c.check([(keep, discard, n)], "the shift in front of the attention")
    past = n - discard
    qkv = rng.normal(0, 1.3, (new, (n_heads + 2 * n_kv) * D)).astype(np.float32)
    sin64, cos64 = c.sin.astype(np.float64), c.cos.astype(np.float64)
    want, _, _ = er.extend_f64(qkv, k[:past].astype(np.float64), v[:past].astype(np.float64), n_heads, n_kv, sin64, cos64)
    wsb = hip.attention_extend_workspace_bytes(n_heads, n_kv, past, new)
    assert wsb > 0
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((new, n_heads * D), float("nan"), dtype=torch.float32, device="cuda")
    hip.attention_extend_dev(torch.from_numpy(qkv).cuda(), c.sin_d, c.cos_d, c.ptr(0), c.ptr(1), n_heads, n_kv, D, max_pos, past, new, ws, wsb, out,
                             CACHE_F16 if f16 else 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(new, n_heads, D)
    assert not np.isnan(got).any()
    err, cs = float(np.max(np.abs(got - want))), cosine(got, want)
    print(f"extend over a shifted cache f16={f16}: max|diff| {err:.3e} cosine {cs:.8f}")
    assert err <= 6e-3 and cs >= 0.999995
