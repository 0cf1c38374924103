"""GPU: the two elementwise operators of the unfused decode step (Decoder::run_reference; csrc/kernels_decode.hip: k_add, k_silu_mul), which other
tests use as the reference of the fused step: bitnet_hip_add_dev bit for bit against f32 numpy, bitnet_hip_silu_mul_dev against float64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 6912]  # one element, either side of one 256-thread workgroup, the headline ffn
SENT = -12345.0
N_SENT = 32


@pytest.fixture(scope="module")
def torch_():
    import torch

    return torch


def dev(torch_, a):
    return torch_.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", SIZES)
def test_add_is_numpy_f32_addition(hip, torch_, n):
    rng = np.random.default_rng(n)
    a = (rng.normal(0, 1, n) * rng.choice([1e-20, 1.0, 1e20], n)).astype(np.float32)
    b = (rng.normal(0, 1, n) * rng.choice([1e-20, 1.0, 1e20], n)).astype(np.float32)
    a[0], b[0] = np.float32(1.0), np.float32(2.0 ** -24)   # a tie: rounds to even
    if n > 2:
        a[1], b[1] = np.float32(np.inf), np.float32(-np.inf)  # NaN
        a[2], b[2] = np.float32(3e38), np.float32(3e38)       # overflow to +inf
    ad, bd = dev(torch_, a), dev(torch_, b)
    out = torch_.full((n + N_SENT,), SENT, device="cuda")
    hip.add_dev(ad, bd, out, n)
    torch_.cuda.synchronize()
    got = out.cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        want = a + b
    assert np.array_equal(got[:n], want, equal_nan=True)
    finite = ~np.isnan(want)
    assert np.array_equal(got[:n][finite].view(np.uint32), want[finite].view(np.uint32))   # the bits, signed zeros included
    assert np.all(got[n:] == SENT)
    assert np.array_equal(ad.cpu().numpy(), a, equal_nan=True) and np.array_equal(bd.cpu().numpy(), b, equal_nan=True)
    hip.add_dev(ad, bd, ad, n)   # in place on the first operand, as the residual add runs it
    torch_.cuda.synchronize()
    assert np.array_equal(ad.cpu().numpy(), want, equal_nan=True)


# with a tile the entry takes whole tiles only: 1, 255 and 257 are refused (asserted below), so the tiled walk is also run at one tile and at the
# whole tiles either side of a workgroup
@pytest.mark.parametrize("tile", [0, 16])
@pytest.mark.parametrize("n", SIZES + [16, 240, 272])
def test_silu_mul_vs_f64(hip, pkg, torch_, n, tile):
    """out[i] = silu(gate[j]) * up[j], j = i without a tile, else (i / tile) * 2 * tile + i % tile (gate and up rows interleaved tile by tile, each
    operand pointing at its own first tile).  Bound: one expf, the sum, the division and the product round once each and expf is good to a couple
    of ulp -- about 6 * 2^-24 = 3.6e-7 relative; 1e-6 relative (+ 1e-30 for the subnormal results) is a factor of three over that."""
    rng = np.random.default_rng(n * 2 + tile)
    span = n if not tile else (n - 1) // tile * 2 * tile + (n - 1) % tile + 1   # last index read + 1
    gate = (rng.normal(0, 3, span)).astype(np.float32)
    up = rng.normal(0, 2, span).astype(np.float32)
    j = np.arange(n) if not tile else (np.arange(n) // tile) * 2 * tile + np.arange(n) % tile
    edge = np.array([-100.0, -20.0, 0.0, 20.0, 100.0, -0.0, -88.0, 88.0], np.float32)   # expf(100) = +inf: -100 / inf * u = -+0, never NaN
    k = min(n, edge.size)
    gate[j[:k]] = edge[:k]
    if n == 1:
        gate[0] = -100.0
    out = torch_.full((n + N_SENT,), SENT, device="cuda")
    gd, ud = dev(torch_, gate), dev(torch_, up)
    if tile and n % tile:
        with pytest.raises(pkg.BitNetHipError, match=f"silu_mul: n {n} is not a multiple of the tile {tile}") as e:
            hip.silu_mul_dev(gd, ud, out, n, tile=tile)
        assert e.value.code == pkg.ERR_INVALID_ARGUMENT
        torch_.cuda.synchronize()
        assert np.all(out.cpu().numpy() == SENT)   # refused before the launch
        return
    hip.silu_mul_dev(gd, ud, out, n, tile=tile)
    torch_.cuda.synchronize()
    got = out.cpu().numpy()
    g64, u64 = gate[j].astype(np.float64), up[j].astype(np.float64)
    want = g64 / (1.0 + np.exp(-g64)) * u64
    err = np.abs(got[:n] - want)
    print(f"silu_mul n={n} tile={tile}: max err / (1e-6 |want| + 1e-30) = {np.max(err / (1e-6 * np.abs(want) + 1e-30)):.3f}")
    assert not np.isnan(got[:n]).any()
    assert np.all(err <= 1e-6 * np.abs(want) + 1e-30), (n, tile, int(np.argmax(err - 1e-6 * np.abs(want))))
    m100 = np.flatnonzero(gate[j] == np.float32(-100.0))
    assert m100.size and np.all(got[:n][m100] == 0.0)     # -100 / (1 + inf) = -0: a zero of either sign, not NaN
    assert np.all(got[n:] == SENT)
    assert np.array_equal(gd.cpu().numpy(), gate) and np.array_equal(ud.cpu().numpy(), up)
