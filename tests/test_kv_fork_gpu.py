"""GPU: bitnet_hip_kv_fork_dev (include/bitnet_hip.h) on raw buffers, no decoder: cache slots [0, n) of every layer's K and V of one source become
the destinations', bit for bit, and every other byte of every destination keeps its value.

The expected bytes are a numpy statement over the private layouts (tests/extend_ref.py: k_index for K, [kv][C * 64][D] for V); the comparison is
over the WHOLE destination arena -- copied slots, untouched slots and 256-byte guard gaps between the caches in one equality -- so there is no
tolerance anywhere.  The source holds random 32-bit patterns with NaN payloads, infinities and denormals planted in copied slots (it is a bit copy);
the destinations hold another random pattern.

3 layers x 2 KV heads x D = 128 (12 segments: K and V of every layer and head, several workgroups each); max_pos 64 (one chunk), 100 (a padded last
chunk), 640; n in {0, 1, 63, 64, 65, 130, max_pos}: nothing, one word per row of a partial chunk, a full partial chunk, exactly one whole chunk, a
whole chunk + a partial one, two + a partial one, the whole cache.  No stream-capture case: the suite has no capture helper; the entry point and its
launcher allocate nothing, synchronise nothing and copy nothing (csrc/abi.hip, csrc/kernels_kvfork.hip: argument checks, one kernel launch)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

N_LAYERS, N_KV, D = 3, 2, er.D
GUARD = 64  # 32-bit words between two caches of an arena (256 bytes: every cache stays 16-byte aligned)
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000, 0xFFFFFFFF, 0x7BFF7E01, 0x0001FC00],
                    np.uint32)  # quiet / signalling NaNs with payloads, infinities, denormals, -0 -- as f32 words and as f16 pairs


def cache_words(max_pos, f16):
    return N_KV * er.chunks(max_pos) * 64 * D // (2 if f16 else 1)


class Arena:
    """`count` caches of `words` 32-bit words each in ONE device tensor, GUARD words in front of, between and behind them"""

    def __init__(self, torch, rng, count, words):
        self.words, self.count = words, count
        self.host = rng.integers(0, 1 << 32, size=GUARD + count * (words + GUARD), dtype=np.uint32)
        self.torch = torch
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()

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


def copied_words(max_pos, n, f16):
    """-> (K, V): flat 32-bit word indices inside ONE cache that the first n positions occupy"""
    elem = np.uint16 if f16 else np.uint32
    head = er.chunks(max_pos) * 64 * D  # elements per KV head
    d, pos = np.meshgrid(np.arange(D), np.arange(n), indexing="ij")
    k_head = er.k_index(d.reshape(-1), pos.reshape(-1), f16)  # elements of one head
    v_head = (pos.reshape(-1) * D + d.reshape(-1))            # [C * 64][D]
    per_word = 4 // np.dtype(elem).itemsize
    out = []
    for idx in (k_head, v_head):
        full = (np.arange(N_KV)[:, None] * head + idx[None, :]).reshape(-1)
        out.append(np.unique(full // per_word))
        assert out[-1].size * per_word == full.size  # whole words only: an f16 word is a (d even, d odd) pair / two neighbouring dims of ONE position
    return out


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


@pytest.mark.parametrize("n_dst", [1, 3, 8])
@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("max_pos", [64, 100, 640])
def test_fork_copies_the_prefix_and_nothing_else(hip, torch_, max_pos, f16, n_dst):
    torch = torch_
    rng = np.random.default_rng(1000 * max_pos + 10 * n_dst + int(f16))
    words = cache_words(max_pos, f16)
    # caches of an arena: source [K | V][layer]; destinations [K | V][dst][layer]
    src = Arena(torch, rng, 2 * N_LAYERS, words)
    dst = Arena(torch, rng, 2 * n_dst * N_LAYERS, words)
    sk = lambda l: l
    sv = lambda l: N_LAYERS + l
    dk = lambda d, l: d * N_LAYERS + l
    dv = lambda d, l: (n_dst + d) * N_LAYERS + l
    # NaN payloads, infinities and denormals inside the slots every n >= 1 copies (position 0) and further on
    for l in range(N_LAYERS):
        for i in (sk(l), sv(l)):
            v = src.view(src.host, i)
            at = rng.choice(words, size=4 * SPECIALS.size, replace=False)
            v[at] = np.tile(SPECIALS, 4)
            v[:SPECIALS.size] = SPECIALS                    # V: position 0; K: row 0, positions 0 .. 10
            v[np.arange(SPECIALS.size) * 64] = SPECIALS     # K: position 0 of rows 0 .. 10
    src.restore()
    table = lambda ptrs: torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    src_k, src_v = table([src.ptr(sk(l)) for l in range(N_LAYERS)]), table([src.ptr(sv(l)) for l in range(N_LAYERS)])
    dst_k = table([dst.ptr(dk(d, l)) for d in range(n_dst) for l in range(N_LAYERS)])
    dst_v = table([dst.ptr(dv(d, l)) for d in range(n_dst) for l in range(N_LAYERS)])
    for n in [n for n in (0, 1, 63, 64, 65, 130, max_pos) if n <= max_pos]:
        dst.restore()
        hip.kv_fork_dev(src_k, src_v, dst_k, dst_v, N_LAYERS, n_dst, N_KV, D, max_pos, n, kv_f16=f16)
        torch.cuda.synchronize()
        want = dst.host.copy()
        kw, vw = copied_words(max_pos, n, f16)
        for l in range(N_LAYERS):
            for d in range(n_dst):
                dst.view(want, dk(d, l))[kw] = src.view(src.host, sk(l))[kw]
                dst.view(want, dv(d, l))[vw] = src.view(src.host, sv(l))[vw]
        got = dst.read()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"n={n}", f"{bad.size} words differ, first at arena word {bad[0]}", f"copied K words {kw.size}, V words {vw.size} per cache")
        assert np.array_equal(src.read(), src.host), f"n={n}: the source changed"
        if n:
            assert kw.size == vw.size == N_KV * n * D // (2 if f16 else 1)
