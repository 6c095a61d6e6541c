"""K78 (xai_conv1x1_bwd_data_f32, csrc/conv/conv1x1_bwd_kernels.hip) at its edges.  It must return the BITS of K79, the one-wave-per-tile
kernel that reads its operands straight from global memory, for every walk -- both split memberships, both k groupings, both
adding orders, from the first partial sum or from +0, one and three partial sums (and 19 where K has the blocks) -- on both tile
heights and the library's choice, and write nothing outside gx.  Both kernels must also hold against the fp64 sum within the
forward-error bound of the walk,
    |computed - exact| <= (gamma(16 * max_s count_s + S - 1) + gamma64(K)) * sum_k |gy_k| |w_k|
(tests/conv_walk_restated.py derives it), and K79 must be the NumPy emulation of the walk bit for bit on the smallest shape.

Shapes (N, K, C, HW): HW = 49 and HW = 1; a column count that ends mid-tile (3 * 49 = 147 = 2 * 64 + 19); row counts that are no
multiple of either tile height (24, 40, 72: one, two and three 32-row tiles, the last one partial); five K-blocks over three partial
sums (K = 80); fewer K-blocks than partial sums (K = 16, 32); N = 1; and 20 blocks over 19 partial sums on more than one tile each
way."""
import itertools

import numpy as np
import pytest
import torch

import conv_walk_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(3, 80, 24, 49), (1, 16, 40, 49), (2, 32, 40, 1), (1, 80, 24, 1), (3, 320, 72, 49), (2, 32, 24, 49)]
GUARD = 256


def walks(K):
    out = [(1, 0, g, 0, z) for g in (0, 1) for z in (0, 1)]
    out += [(3, m, g, o, z) for m, g, o, z in itertools.product((0, 1), (0, 1), (0, 1), (0, 1))]
    if K // 16 >= 19:
        out += [(19, m, g, o, 0) for m, g, o in itertools.product((0, 1), (0, 1), (0, 1))]
    return out


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels, load_library
    load_library()
    return kernels


@pytest.fixture(scope="module")
def data():
    """per shape: gy, weight, the fp64 sum and sum |gy| |w|, computed once"""
    out = {}
    g = torch.Generator().manual_seed(11)
    for (N, Kc, Cc, HW) in SHAPES:
        H, W = (7, 7) if HW == 49 else (1, 1)
        gy = torch.randn(N, Kc, H, W, generator=g).to(DEV)
        w = (torch.randn(Kc, Cc, 1, 1, generator=g) * 0.05).to(DEV)
        g64, w64 = gy.double().view(N, Kc, HW), w.double().view(Kc, Cc)
        exact = torch.einsum("nkp,kc->ncp", g64, w64).view(N, Cc, H, W)
        abs_sum = torch.einsum("nkp,kc->ncp", g64.abs(), w64.abs()).view(N, Cc, H, W)
        out[(N, Kc, Cc, HW)] = (gy, w, exact, abs_sum)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_the_fast_kernel_is_the_simple_kernel_bit_for_bit_and_both_hold_against_fp64(K, data, shape):
    N, Kc, Cc, HW = shape
    gy, w, exact, abs_sum = data[shape]
    n = exact.numel()
    for walk in walks(Kc):
        want = K.conv1x1_bwd_data(gy, w, walk, simple=True)
        limit = torch.from_numpy(np.asarray(R.bound(Kc, walk[0], walk[1], walk[3], abs_sum.cpu().numpy()))).to(DEV)
        err = (want.double() - exact).abs()
        print(shape, walk, "max |K79 - fp64| / bound", float((err / limit).max()))
        assert bool((err <= limit).all()), (shape, walk)
        for tile in (0, 32, 64):
            buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
            got = K.conv1x1_bwd_data(gy, w, walk, tile_rows=tile, out=buf[GUARD:GUARD + n])
            assert bits(got, want), (shape, walk, tile)
            assert bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + n:].isnan().all()) and not bool(got.isnan().any())


def test_the_walks_are_different_sums_and_the_simple_kernel_is_their_emulation(K, data):
    """on (3, 80, 24, 49): K79 returns tests/conv_walk_restated.emulate's bits for every walk, and the walks do not all agree --
    a kernel that ignored its walk would pass the comparison above"""
    shape = SHAPES[0]
    gy, w, _, _ = data[shape]
    N, Kc, Cc, HW = shape
    seen = set()
    for walk in walks(Kc):
        got = K.conv1x1_bwd_data(gy, w, walk, simple=True).cpu().numpy()
        for n in range(N):
            want = R.emulate(gy[n].view(Kc, HW).cpu().numpy(), w.view(Kc, Cc).cpu().numpy(), walk)
            assert (got[n].reshape(Cc, HW).view(np.int32) == want.view(np.int32)).all(), (walk, n)
        seen.add(got.tobytes())
    assert len(seen) >= 8


def test_the_wrapper_refuses_what_the_kernel_cannot_take(K):
    gy = torch.zeros(1, 24, 7, 7, device=DEV)
    with pytest.raises(Exception, match="xai_conv1x1_bwd_data_f32 failed"):
        K.conv1x1_bwd_data(gy, torch.zeros(24, 8, device=DEV), (1, 0, 0, 0, 0))              # K % 16 != 0
    with pytest.raises(ValueError):
        K.conv1x1_bwd_data(gy, torch.zeros(32, 8, device=DEV), (1, 0, 0, 0, 0))              # weight of another K
    with pytest.raises(Exception, match="lives on"):
        K.conv1x1_bwd_data(gy.cpu(), torch.zeros(24, 8), (1, 0, 0, 0, 0))
