"""GPU: the movers of the paged KV cache (bitnet_hip_kv_page_in_dev / _page_out_dev / _page_copy_dev, csrc/kernels_kvpaged.hip) on raw buffers, bit
for bit, and the paged attention on paged-in caches against bitnet_hip_attention_decode_rows_dev on the contiguous ones."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_decode_ref as dr  # noqa: E402
import extend_ref as er  # noqa: E402
import test_attn_paged_gpu as ap  # noqa: E402

pytestmark = pytest.mark.gpu

D, N_KV, N_LAYERS, MAX_POS, N_PAGES = 128, 2, 3, 300, 16
C = er.chunks(MAX_POS)


def ptrs(t, tensors):
    return t.tensor([x.data_ptr() for x in tensors], dtype=t.int64, device="cuda")


def random_words(t, rng, n):
    return t.from_numpy(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 200))
@pytest.mark.parametrize("f16", (False, True), ids=("kv32", "kv16"))
def test_page_in_then_out_is_bit_equal_and_touches_nothing_else(hip, f16, n):
    import torch as t

    rng = np.random.default_rng(100 * n + f16)
    R = 64 if f16 else 128
    cache_words, pool_words = N_KV * C * 64 * R, N_PAGES * N_KV * 64 * R
    assert hip.kv_pool_bytes(N_PAGES, N_KV, D, kv_f16=f16) == 4 * pool_words
    src = [[random_words(t, rng, cache_words) for _ in range(N_LAYERS)] for _ in range(2)]
    back = [[random_words(t, rng, cache_words) for _ in range(N_LAYERS)] for _ in range(2)]
    pools = [[random_words(t, rng, pool_words) for _ in range(N_LAYERS)] for _ in range(2)]
    back0, pools0 = [[x.clone() for x in kv] for kv in back], [[x.clone() for x in kv] for kv in pools]
    table = rng.permutation(N_PAGES)[:C].astype(np.uint32)  # scrambled, non-monotone
    table_d = t.from_numpy(table.view(np.int32)).cuda()
    n_chunks = (n + 63) // 64
    hip.kv_page_in_dev(ptrs(t, src[0]), ptrs(t, src[1]), ptrs(t, pools[0]), ptrs(t, pools[1]), table_d, N_PAGES, N_LAYERS, N_KV, D, MAX_POS, n, kv_f16=f16)
    hip.kv_page_out_dev(ptrs(t, pools[0]), ptrs(t, pools[1]), table_d, N_PAGES, ptrs(t, back[0]), ptrs(t, back[1]), N_LAYERS, N_KV, D, MAX_POS, n, kv_f16=f16)
    t.cuda.synchronize()
    live_k = np.broadcast_to((np.arange(C)[:, None, None] * 64 + np.arange(64)[None, None, :]) < n, (N_KV, C, R, 64)).copy()  # words of positions [0, n)
    live_v = np.zeros((N_KV, C * 64, R), bool)
    live_v[:, :n] = True
    for is_v, live in ((0, live_k.reshape(-1)), (1, live_v.reshape(-1))):
        for layer in range(N_LAYERS):
            got, want, before = (x[is_v][layer].cpu().numpy() for x in (back, src, back0))
            assert np.array_equal(got[live], want[live]), (is_v, layer, "the live region is not bit-equal")
            assert np.array_equal(got[~live], before[~live]), (is_v, layer, "a destination word outside [0, n) changed")
            # the pool: only the named pages of the walked chunks changed, and of a partial page only its live positions
            pool, pool_before = (x[is_v][layer].cpu().numpy().reshape(N_PAGES, N_KV, 64 * R) for x in (pools, pools0))
            tile, mask = want.reshape(N_KV, C, 64 * R), live.reshape(N_KV, C, 64 * R)
            untouched = np.ones(N_PAGES, bool)
            for c in range(n_chunks):
                pg = int(table[c])
                untouched[pg] = False
                assert np.array_equal(pool[pg][mask[:, c]], tile[:, c][mask[:, c]]), (is_v, layer, c)
                assert np.array_equal(pool[pg][~mask[:, c]], pool_before[pg][~mask[:, c]]), (is_v, layer, c, "dead slots of a partial page changed")
            assert np.array_equal(pool[untouched], pool_before[untouched]), (is_v, layer, "a page no walked chunk names changed")


@pytest.mark.parametrize("f16", (False, True), ids=("kv32", "kv16"))
def test_page_copy_of_several_pairs(hip, f16):
    import torch as t

    rng = np.random.default_rng(7 + f16)
    R = 64 if f16 else 128
    pools = [[random_words(t, rng, N_PAGES * N_KV * 64 * R) for _ in range(N_LAYERS)] for _ in range(2)]
    before = [[x.cpu().numpy().reshape(N_PAGES, -1) for x in kv] for kv in pools]
    pairs = [(3, 9), (3, 0), (15, 7), (1, 14)]  # a source shared by two pairs, the pool's first and last page
    hip.kv_page_copy_dev(ptrs(t, pools[0]), ptrs(t, pools[1]), N_PAGES, pairs, N_LAYERS, N_KV, D, kv_f16=f16)
    t.cuda.synchronize()
    want_from = np.arange(N_PAGES)
    for s, d in pairs:
        want_from[d] = s
    for is_v in range(2):
        for layer in range(N_LAYERS):
            assert np.array_equal(pools[is_v][layer].cpu().numpy().reshape(N_PAGES, -1), before[is_v][layer][want_from]), (is_v, layer)


@pytest.mark.parametrize("f16", (False, True), ids=("kv32", "kv16"))
def test_paged_attention_on_paged_in_caches_agrees_with_the_rows_form(hip, oracle, f16):
    """one sequence at pos 200 (a partial fourth page), 8 heads over 2 KV heads, the model's step from test_attn_paged_gpu.py's Rig.  Both forms
    are held to float64, each within its own tolerance; they sum in different orders, so their difference is bounded by the sum of the two"""
    import torch as t

    rig, pos, H, n_splits, MP = ap.Rig(hip, oracle, t), 200, 8, 2, ap.MAX_POS
    ref, Cp, R = rig.ref(f16, H, "gauss", pos, 0), er.chunks(ap.MAX_POS), 64 if f16 else 128
    kc, vc = (rig.dev(enc(ref[x].transpose(1, 0, 2)[:pos], MP, f16)) for enc, x in ((er.encode_k, "kp"), (er.encode_v, "vp")))
    kpool, vpool = (t.zeros(N_PAGES * N_KV * 64 * R, dtype=t.int32, device="cuda") for _ in range(2))
    table_d = rig.dev(np.random.default_rng(8).permutation(N_PAGES)[:Cp].astype(np.uint32).view(np.int32))
    hip.kv_page_in_dev(ptrs(t, [kc]), ptrs(t, [vc]), ptrs(t, [kpool]), ptrs(t, [vpool]), table_d, N_PAGES, 1, N_KV, D, MP, pos, kv_f16=f16)
    pos_d, qkv_d = t.tensor([pos], dtype=t.int32, device="cuda"), rig.dev(ref["qkv"][None])
    out_p, out_r = (t.zeros((1, H * D), dtype=t.float32, device="cuda") for _ in range(2))
    scratch_p = t.zeros(hip.attention_paged_scratch_bytes(1, N_KV, n_splits) // 4, dtype=t.float32, device="cuda")
    hip.attention_decode_paged_dev(qkv_d, rig.sin_d, rig.cos_d, kpool, vpool, N_PAGES, ptrs(t, [table_d]), ptrs(t, [pos_d]), 1, H, N_KV, D, MP, pos + 1, n_splits,
                                   scratch_p, out_p, kv_f16=f16)
    scratch_r = t.zeros(int(hip.c.bitnet_hip_attention_scratch_bytes(N_KV, MP)) // 4, dtype=t.float32, device="cuda")
    hip.attention_decode_rows_dev(qkv_d, rig.sin_d, rig.cos_d, ptrs(t, [kc]), ptrs(t, [vc]), ptrs(t, [pos_d]), 1, H, N_KV, D, MP, pos + 1, scratch_r, out_r, kv_f16=f16)
    t.cuda.synchronize()
    tol_r = ref["tol"]
    tol_p = tol_r + 2.0 ** -23 * (pos // 64 + 1 + n_splits) * ref["pav"]
    got_p, got_r = (x.cpu().numpy().reshape(H, D).astype(np.float64) for x in (out_p, out_r))
    rp, rr, rd = dr.ratio(got_p, ref["out"], tol_p), dr.ratio(got_r, ref["out"], tol_r), dr.ratio(got_p, got_r, tol_p + tol_r)
    print(f"PAGED-vs-ROWS f16={f16}: paged err/tol {rp:.4f}, rows err/tol {rr:.4f}, difference / (sum of both) {rd:.4f}")
    assert rp <= 1.0 and rr <= 1.0 and rd <= 1.0
