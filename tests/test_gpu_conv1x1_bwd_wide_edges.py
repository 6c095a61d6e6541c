"""K80 (xai_convw_bwd_data_f32, csrc/conv/conv1x1_bwd_wide_kernels.hip) at its edges.  It must return the BITS of the plain kernels
for every walk it accepts -- K79's for the two k groupings without a stagger, from the first partial sum or from +0, and K81's for
the staggered starts (loop depth 16 | 32 | 64, tiles of 32 | 64 along hw, SU 2 | 32, strides of one and of two iterations) -- in
both regimes (one chunk of rows streaming K; several chunks over gy slabs held in LDS, or one workgroup per chunk where K is too
long to hold), on 16-byte loads and on the dword path, and write nothing outside gx.  K81 without a stagger must be K79, and with one
the NumPy emulation of tests/conv_stagger_restated.py on the smallest shapes.  All kernels must hold against the fp64 sum within
the forward-error bound of one partial sum of K terms,
    |computed - exact| <= (gamma(K) + gamma64(K)) * sum_k |gy_k| |w_k|
(tests/conv_walk_restated.py derives it; the start of the loop only moves roundings around inside the chain).

Shapes (N, K, C, HW): the columns end mid-tile (196 = 3 * 64 + 4); a long sum onto 64 rows, 100 = 64 + 36 columns; 272 rows = two
chunks of 128 and one of 16 over slabs held in LDS, 36 columns; one K-block and one partial tile; K = 80 straddles a 64-wide loop
iteration; 256 rows on 784 columns; HW % 4 != 0 (the dword path); 384 rows under K = 192, which is too long to hold (a workgroup
per chunk); and every shape once more with gx starting 4 bytes off a 16-byte boundary."""
import numpy as np
import pytest
import torch

import conv_stagger_restated as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(2, 64, 64, 196), (3, 256, 64, 100), (2, 128, 272, 36), (1, 16, 16, 4), (1, 80, 48, 64), (1, 64, 256, 784), (2, 32, 40, 49),
          (1, 192, 384, 100)]
GUARD = 256


def staggers(K):
    """(grouping, from_zero, depth, tile, axis, stagger, stride) with a start that differs from tile to tile, where K has the iterations"""
    out = []
    for depth, tile, su, stride in ((16, 32, 32, 64), (16, 64, 2, 64), (32, 64, 32, 256), (64, 32, 32, 256), (16, 32, 32, 128)):
        p = S.plan(K, depth, tile, 0, su, stride)
        if p is not None and p[4] != 0:
            out.append((len(out) % 2, 0, depth, tile, 0, su, stride))
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
    g = torch.Generator().manual_seed(12)
    for (N, Kc, Cc, HW) in SHAPES:
        gy = torch.randn(N, Kc, HW, 1, generator=g).to(DEV)
        w = (torch.randn(Kc, Cc, 1, 1, generator=g) * 0.05).to(DEV)
        g64, w64 = gy.double().view(N, Kc, HW), w.double().view(Kc, Cc)
        exact = torch.einsum("nkp,kc->ncp", g64, w64).view(N, Cc, HW, 1)
        abs_sum = torch.einsum("nkp,kc->ncp", g64.abs(), w64.abs()).view(N, Cc, HW, 1)
        out[(N, Kc, Cc, HW)] = (gy, w, exact, abs_sum)
    return out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_fast_kernel_is_the_plain_kernels_bit_for_bit_and_all_hold_against_fp64(K, data, shape, offset):
    N, Kc, Cc, HW = shape
    gy, w, exact, abs_sum = data[shape]
    n = exact.numel()
    limit = torch.from_numpy(np.asarray(S.bound(Kc, abs_sum.cpu().numpy()))).to(DEV)
    plain = [(g, z, 16, 64, 0, 0, 0) for g in (0, 1) for z in (0, 1)]
    for walk in plain + staggers(Kc):
        want = K.conv1x1_bwd_data_wide(gy, w, walk, simple=True)
        if walk[5] == 0:                                  # no stagger: K81 is K79 on the walk of one partial sum
            assert bits(want, K.conv1x1_bwd_data(gy, w, (1, 0, walk[0], 0, walk[1]), simple=True)), (shape, walk)
        err = (want.double() - exact).abs()
        print(shape, walk, "max |K81 - fp64| / bound", float((err / limit).max()))
        assert bool((err <= limit).all()), (shape, walk)
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
        got = K.conv1x1_bwd_data_wide(gy, w, walk, out=buf[GUARD + offset:GUARD + offset + n])
        assert got.data_ptr() % 16 == 4 * offset
        assert bits(got, want), (shape, walk)
        assert bool(buf[:GUARD + offset].isnan().all()) and bool(buf[GUARD + offset + n:].isnan().all()) and not bool(got.isnan().any())


def test_an_input_off_the_16_byte_boundary_takes_the_dword_path_to_the_same_bits(K, data):
    shape = SHAPES[0]
    gy, w, _, _ = data[shape]
    walk = (0, 0, 16, 32, 0, 32, 64)
    want = K.conv1x1_bwd_data_wide(gy, w, walk, simple=True)
    shifted = torch.empty(gy.numel() + 1, device=DEV)[1:].view(gy.shape).copy_(gy)
    assert shifted.data_ptr() % 16 == 4 and bits(K.conv1x1_bwd_data_wide(shifted, w, walk), want)


def test_the_starts_are_different_sums_and_the_plain_kernel_is_their_emulation(K, data):
    """on (1, 80, 48, 64) and (2, 64, 64, 196): K81 returns tests/conv_stagger_restated.emulate's bits along both axes, and the
    staggered sums differ from the plain one -- a kernel that ignored its stagger would pass the comparison above"""
    for shape in (SHAPES[4], SHAPES[0]):
        gy, w, _, _ = data[shape]
        N, Kc, Cc, HW = shape
        seen = set()
        for walk in [(0, 0, 16, 64, 0, 0, 0), (1, 1, 16, 16, 0, 4, 64), (0, 0, 16, 32, 0, 32, 64), (0, 0, 16, 16, 1, 2, 64), (1, 0, 16, 32, 1, 32, 128)]:
            p = S.plan(Kc, *walk[2:])
            got = K.conv1x1_bwd_data_wide(gy, w, walk, simple=True).cpu().numpy()
            for n in range(N):
                want = S.emulate(gy[n].view(Kc, HW).cpu().numpy(), w.view(Kc, Cc).cpu().numpy(), walk[0], walk[1], p)
                assert (got[n].reshape(Cc, HW).view(np.int32) == want.view(np.int32)).all(), (shape, walk, n)
            seen.add(got.tobytes())
        assert len(seen) == 5


def test_the_wrapper_refuses_what_the_kernel_cannot_take(K):
    gy = torch.zeros(1, 64, 8, 8, device=DEV)
    w = torch.zeros(64, 8, device=DEV)
    with pytest.raises(Exception, match="xai_convw_bwd_data_f32 failed"):
        K.conv1x1_bwd_data_wide(torch.zeros(1, 24, 8, 8, device=DEV), torch.zeros(24, 8, device=DEV), (0, 0, 16, 64, 0, 0, 0))   # K % 16 != 0
    with pytest.raises(Exception, match="xai_convw_bwd_data_f32 failed"):
        K.conv1x1_bwd_data_wide(gy, w, (0, 0, 48, 64, 0, 0, 0))                              # K % depth != 0
    with pytest.raises(Exception, match="xai_convw_bwd_data_f32 failed"):
        K.conv1x1_bwd_data_wide(gy, w, (0, 0, 16, 64, 1, 4, 64))                             # a stagger along c: K81 only
    with pytest.raises(Exception, match="xai_convw_bwd_data_f32 failed"):
        K.conv1x1_bwd_data_wide(gy, w, (0, 0, 16, 16, 0, 4, 64))                             # tiles of 16 columns: K81 only
    K.conv1x1_bwd_data_wide(gy, w, (0, 0, 16, 16, 0, 4, 64), simple=True)
    with pytest.raises(ValueError):
        K.conv1x1_bwd_data_wide(gy, torch.zeros(32, 8, device=DEV), (0, 0, 16, 64, 0, 0, 0))  # weight of another K
    with pytest.raises(Exception, match="lives on"):
        K.conv1x1_bwd_data_wide(gy.cpu(), w.cpu(), (0, 0, 16, 64, 0, 0, 0))
