"""GPU: bitnet_hip_kv_save_dev / bitnet_hip_kv_restore_dev (include/bitnet_hip_kvsnap.h) on raw buffers, no decoder.

save: cache slots [0, n) of every layer's K and V of one sequence become a position-major snapshot K [layers][kv][n][128] then V the same, bit for
bit.  The expected snapshot is the private layouts decoded by tests/extend_ref.py (decode_k / decode_v), slots [0, n); 64 guard words in front of and
behind the snapshot keep their values.
restore: positions [0, m) of a snapshot of S positions (m == S and m < S) go into 1, 3 and 8 destinations.  The yardstick is bitnet_hip_kv_fork_dev
from the ORIGINAL caches into an identical arena of sentinel-filled destinations: the two arenas -- copied slots, untouched slots, padding slots of
the last chunk and the guard gaps between the caches -- are compared whole, on the device, so there is no tolerance anywhere.  Sources and snapshot
are unchanged afterwards.  Once more inside a captured graph.

The caches hold random 32-bit patterns with NaN payloads, infinities and denormals planted in the copied slots (it is a bit copy).  3 layers; 1, 2
and 5 KV heads; max_pos 64 (one chunk), 100 (a padded last chunk), 640; f32 and f16 caches; n in {1, 63, 64, 65, 130, max_pos}: one word per row
of a partial chunk, a full partial chunk, exactly one whole chunk, a whole chunk + a partial one, two + a partial one, the whole cache."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

N_LAYERS, D = 3, er.D
GUARD = 64  # 32-bit words (256 bytes: everything stays 16-byte aligned)
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000, 0xFFFFFFFF, 0x7BFF7E01, 0x0001FC00],
                    np.uint32)  # quiet / signalling NaNs with payloads, infinities, denormals, -0 -- as f32 words and as f16 pairs
NS = (1, 63, 64, 65, 130)


def cache_words(n_kv, max_pos, f16):
    return n_kv * er.chunks(max_pos) * 64 * D // (2 if f16 else 1)


def snapshot_words(n_kv, n, f16):
    return 2 * N_LAYERS * n_kv * n * D // (2 if f16 else 1)


class Arena:
    """`count` buffers of `words` 32-bit words each in ONE device tensor, GUARD words in front of, between and behind them; `master` keeps the
    initial bytes on the device"""

    def __init__(self, torch, host, count, words):
        assert host.size == GUARD + count * (words + GUARD)
        self.words, self.count, self.host = words, count, host
        self.master = torch.from_numpy(host.view(np.int32).copy()).cuda()
        self.dev = self.master.clone()

    @staticmethod
    def size(count, words):
        return GUARD + count * (words + GUARD)

    def offset(self, i):
        return GUARD + i * (self.words + GUARD)

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.offset(i)

    def view(self, host, i):
        return host[self.offset(i):self.offset(i) + self.words]

    def reset(self):
        self.dev.copy_(self.master)

    def unchanged(self, torch):
        return bool(torch.equal(self.dev, self.master))


def expected_snapshot(src, n_kv, max_pos, n, f16):
    """the snapshot of the first n positions, as uint32 words, from the source arena's host bytes (caches [K | V][layer])"""
    ft = np.float16 if f16 else np.float32
    ut = np.uint16 if f16 else np.uint32
    parts = []
    for decode, first in ((er.decode_k, 0), (er.decode_v, N_LAYERS)):
        for l in range(N_LAYERS):
            flat = src.view(src.host, first + l).view(ft)                   # a view: no value conversion anywhere
            full = decode(flat, n_kv, max_pos, f16).view(ut)                # [C * 64, kv, D]
            parts.append(np.ascontiguousarray(full[:n].transpose(1, 0, 2)))  # [kv, n, D]
    return np.concatenate([p.reshape(-1) for p in parts]).view(np.uint32)


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def make_source(torch, rng, n_kv, max_pos, f16):
    words = cache_words(n_kv, max_pos, f16)
    host = rng.integers(0, 1 << 32, size=Arena.size(2 * N_LAYERS, words), dtype=np.uint32)
    src = Arena(torch, host, 2 * N_LAYERS, words)
    for i in range(2 * N_LAYERS):
        v = src.view(host, i)
        at = rng.choice(words, size=4 * SPECIALS.size, replace=False)
        v[at] = np.tile(SPECIALS, 4)
        v[:SPECIALS.size] = SPECIALS                 # V: position 0; K: row 0, positions 0 .. 10
        v[np.arange(SPECIALS.size) * 64] = SPECIALS  # K: position 0 of rows 0 .. 10
    src.master = torch.from_numpy(host.view(np.int32).copy()).cuda()
    src.reset()
    return src


@pytest.mark.parametrize("f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("max_pos", [64, 100, 640])
@pytest.mark.parametrize("n_kv", [1, 2, 5])
def test_save_then_restore_equals_fork(hip, torch_, n_kv, max_pos, f16):
    torch = torch_
    rng = np.random.default_rng(10000 * n_kv + 10 * max_pos + int(f16))
    words = cache_words(n_kv, max_pos, f16)
    src = make_source(torch, rng, n_kv, max_pos, f16)
    table = lambda ptrs: torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    src_k, src_v = table([src.ptr(l) for l in range(N_LAYERS)]), table([src.ptr(N_LAYERS + l) for l in range(N_LAYERS)])
    # two identical arenas of 8 sentinel-filled destinations, caches [K | V][dst][layer]: one for restore, one for fork
    M = 8
    sentinel = rng.integers(0, 1 << 32, size=Arena.size(2 * M * N_LAYERS, words), dtype=np.uint32)
    got, want = Arena(torch, sentinel, 2 * M * N_LAYERS, words), Arena(torch, sentinel, 2 * M * N_LAYERS, words)
    tables = {}
    for a in (got, want):
        tables[a] = (table([a.ptr(d * N_LAYERS + l) for d in range(M) for l in range(N_LAYERS)]),
                     table([a.ptr((M + d) * N_LAYERS + l) for d in range(M) for l in range(N_LAYERS)]))
    for n in sorted({n for n in NS + (max_pos,) if n <= max_pos}):
        sw = snapshot_words(n_kv, n, f16)
        assert hip.kv_snapshot_bytes(N_LAYERS, n_kv, D, n, kv_f16=f16) == 4 * sw
        snap_host = rng.integers(0, 1 << 32, size=Arena.size(1, sw), dtype=np.uint32)
        snap = Arena(torch, snap_host, 1, sw)
        hip.kv_save_dev(src_k, src_v, N_LAYERS, n_kv, D, max_pos, n, snap.ptr(0), kv_f16=f16)
        torch.cuda.synchronize()
        out = snap.dev.cpu().numpy().view(np.uint32)
        exp = snap_host.copy()
        snap.view(exp, 0)[:] = expected_snapshot(src, n_kv, max_pos, n, f16)
        bad = np.flatnonzero(out != exp)
        assert bad.size == 0, (f"save n={n}", f"{bad.size} words differ, first at word {bad[0] - GUARD} of the snapshot ({sw} words)")
        assert src.unchanged(torch), f"save n={n}: the source changed"
        saved = snap.dev.clone()
        for m in (n, 2 * n // 3):  # the whole snapshot, and fewer positions than it holds
            for n_dst in (1, 3, 8):
                got.reset(), want.reset()
                hip.kv_restore_dev(snap.ptr(0), n, *tables[got], N_LAYERS, n_dst, n_kv, D, max_pos, m, kv_f16=f16)
                hip.kv_fork_dev(src_k, src_v, *tables[want], N_LAYERS, n_dst, n_kv, D, max_pos, m, kv_f16=f16)
                torch.cuda.synchronize()
                if not torch.equal(got.dev, want.dev):
                    bad = torch.nonzero(got.dev != want.dev).flatten()
                    pytest.fail(f"restore S={n} m={m} n_dst={n_dst}: {bad.numel()} arena words differ from fork's, first at {int(bad[0])} "
                                f"(cache {(int(bad[0]) - GUARD) // (words + GUARD)}, word {(int(bad[0]) - GUARD) % (words + GUARD)} of {words})")
                if m == 0 or n_dst < M:
                    assert torch.equal(got.dev[got.offset(2 * M * N_LAYERS - 1):], got.master[got.offset(2 * M * N_LAYERS - 1):])  # an unnamed destination
                assert src.unchanged(torch) and torch.equal(snap.dev, saved), f"restore S={n} m={m}: the source or the snapshot changed"


def test_save_and_restore_inside_a_captured_graph(hip, torch_):
    """both launches captured once (no allocation, no synchronisation, no workspace), replayed on fresh contents: the eager results"""
    torch = torch_
    n_kv, max_pos, f16, n, m, n_dst = 2, 100, False, 70, 65, 3
    rng = np.random.default_rng(77)
    words = cache_words(n_kv, max_pos, f16)
    src = make_source(torch, rng, n_kv, max_pos, f16)
    table = lambda ptrs: torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    src_k, src_v = table([src.ptr(l) for l in range(N_LAYERS)]), table([src.ptr(N_LAYERS + l) for l in range(N_LAYERS)])
    sentinel = rng.integers(0, 1 << 32, size=Arena.size(2 * n_dst * N_LAYERS, words), dtype=np.uint32)
    got, want = Arena(torch, sentinel, 2 * n_dst * N_LAYERS, words), Arena(torch, sentinel, 2 * n_dst * N_LAYERS, words)
    tabs = lambda a: (table([a.ptr(d * N_LAYERS + l) for d in range(n_dst) for l in range(N_LAYERS)]),
                      table([a.ptr((n_dst + d) * N_LAYERS + l) for d in range(n_dst) for l in range(N_LAYERS)]))
    got_t, want_t = tabs(got), tabs(want)
    sw = snapshot_words(n_kv, n, f16)
    snap = Arena(torch, rng.integers(0, 1 << 32, size=Arena.size(1, sw), dtype=np.uint32), 1, sw)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def both(s):
        hip.kv_save_dev(src_k, src_v, N_LAYERS, n_kv, D, max_pos, n, snap.ptr(0), kv_f16=f16, stream=s)
        hip.kv_restore_dev(snap.ptr(0), n, *got_t, N_LAYERS, n_dst, n_kv, D, max_pos, m, kv_f16=f16, stream=s)

    with torch.cuda.stream(stream):
        both(stream.cuda_stream)  # warm-up: one real call
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            both(stream.cuda_stream)
    # fresh contents everywhere, then the replay alone
    got.reset(), snap.reset()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    hip.kv_fork_dev(src_k, src_v, *want_t, N_LAYERS, n_dst, n_kv, D, max_pos, m, kv_f16=f16)
    torch.cuda.synchronize()
    assert torch.equal(got.dev, want.dev)
    exp = snap.host.copy()
    snap.view(exp, 0)[:] = expected_snapshot(src, n_kv, max_pos, n, f16)
    assert np.array_equal(snap.dev.cpu().numpy().view(np.uint32), exp)
    assert src.unchanged(torch)
