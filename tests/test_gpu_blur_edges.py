"""K7 (csrc/blur_kernels.hip: blur_sep_kernel<16 | 32, 31 | 0> and the blur_1d_kernel pair) on the MI355X against
tests/blur_restated.py at the edges of its tiles.

Per cell of the matrix (klen x image shape, 2 images x 2 channels): integer data on which any order of fp32 arithmetic is exact
must come back element for element; single impulses at corners, tile seams and inside must come back as the rounded tap
products on the clipped footprint and +0.0 elsewhere, bit for bit; the fused kernel must equal the two 1-D passes bit for bit
(the promise of the file's header); and both must lie inside the derived per-pixel bound around the fp64 restatement.  All tap
vectors are asymmetric, so a reversed tap order or passes along the wrong axes show.  The 32-row instantiations, which only
batches reach, get their own cases with the kernel that ran read from a profiler trace."""
import math

import numpy as np
import pytest
import torch

import blur_restated as R
from conftest import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGAINST = "fp64 restatement"
CELLS = [pytest.param(k, s, id=f"{k}-{s[0]}x{s[1]}") for k, s in R.cells()]


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def two_pass(K, x, k):
    """xai_blur_1d_f32 along W, then along H, through a scratch tensor."""
    B, C, H, W = x.shape
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    K._call("xai_blur_1d_f32", x.device, x.data_ptr(), k.data_ptr(), k.numel(), 1, B, C, H, W, tmp.data_ptr())
    K._call("xai_blur_1d_f32", x.device, tmp.data_ptr(), k.data_ptr(), k.numel(), 0, B, C, H, W, out.data_ptr())
    return out


def same_bits(got, want, what):
    np.testing.assert_array_equal(np.asarray(got).view(np.int32), np.asarray(want, np.float32).view(np.int32), err_msg=str(what))


@pytest.mark.parametrize("klen,shape", CELLS)
def test_integer_data_comes_back_exactly(K, klen, shape):
    """Every partial sum is an integer below 2^24: no rounding anywhere, so nothing but the int64 correlation is right --
    from K.blur_sep (fused up to 63 taps, two passes above) and from the two 1-D passes called directly."""
    x, k, want = R.exact_case(klen, R.PLANES + shape, 2)
    xd, kd = dev(x), dev(k)
    np.testing.assert_array_equal(K.blur_sep(xd, kd).cpu().numpy().astype(np.int64), want)
    np.testing.assert_array_equal(two_pass(K, xd, kd).cpu().numpy().astype(np.int64), want)
    np.testing.assert_array_equal(xd.cpu().numpy(), x, err_msg="x is read only")


@pytest.mark.parametrize("klen,shape", CELLS)
def test_impulses_come_back_as_rounded_tap_products(K, klen, shape):
    """One 1.0 per plane, at the corners, at both sides of the tile seams and inside: out == fp32(k[i]) * fp32(k[j]) on the
    clipped klen x klen footprint and +0.0 everywhere else, through int32 views; then one NaN, whose footprint must be exactly
    that square (every tap is non-zero) with +0.0 around it."""
    H, W = shape
    k = R.taps(klen, 4)
    kd = dev(k)
    at = R.impulse_positions(H, W)
    n = math.prod(R.PLANES)
    for lo in range(0, len(at), n):
        group = [at[(lo + i) % len(at)] for i in range(n)]
        x = np.zeros((n, H, W), np.float32)
        for p, (py, px) in enumerate(group):
            x[p, py, px] = 1.0
        want = np.stack([R.impulse_response(k, H, W, py, px)[0] for py, px in group])
        xd = dev(x.reshape(R.PLANES + shape))
        same_bits(K.blur_sep(xd, kd).cpu().numpy().reshape(n, H, W), want, (klen, shape, group))
        same_bits(two_pass(K, xd, kd).cpu().numpy().reshape(n, H, W), want, (klen, shape, group, "two passes"))
    py, px = (16, 64) if H > 16 and W > 64 else (H - 1, W - 1)          # the far side of the first seam where there is one
    x = np.zeros(R.PLANES + shape, np.float32)
    x[1, 0, py, px] = np.nan
    got = K.blur_sep(dev(x), kd).cpu().numpy()
    foot = R.impulse_response(k, H, W, py, px)[1]
    np.testing.assert_array_equal(np.isnan(got[1, 0]), foot, err_msg=str((klen, shape, py, px)))
    got[1, 0][foot] = 0.0
    same_bits(got, np.zeros_like(got), (klen, shape, "around the NaN footprint"))


@pytest.mark.parametrize("klen,shape", CELLS)
def test_fused_equals_two_passes_bitwise_and_both_are_inside_the_bound(K, klen, shape):
    """N(0, 1) data, random asymmetric taps.  The ratio |got - blur64| / bound(x, k) goes to the ledger per form
    (profiles/blur_edges_parity.json, tied by tests/test_cpu_blur.py); 1.0 is the derived condition, not a measured slack."""
    x, k = R.normal_case(klen, R.PLANES + shape, 1)
    xd, kd = dev(x), dev(k)
    sep, two = K.blur_sep(xd, kd).cpu().numpy(), two_pass(K, xd, kd).cpu().numpy()
    same_bits(sep, two, (klen, shape))
    want, b = R.blur64(x, k, k), R.bound(x, k)
    for form, got in zip(R.FORMS, (sep, two)):
        ratio = float((np.abs(got.astype(np.float64) - want) / b).max())
        print(f"{R.ledger_name(klen, shape, form)}: {ratio:.4f}")
        check(R.ledger_name(klen, shape, form), ratio, 0, 1.0, against=AGAINST, absolute=True)


def test_63_taps_and_65_taps_with_zero_ends_give_the_same_bits(K):
    """The hand-over of K.blur_sep: 63 taps run fused, the same taps between two exact zeros run as two blur_1d_kernel passes --
    the two extra products are zeros of finite data added to a chain, which changes no bit."""
    for shape in R.LONG_SHAPES:
        x, k63 = R.normal_case(63, R.PLANES + shape, 9)
        k65 = np.concatenate([[0], k63, [0]]).astype(np.float32)
        xd = dev(x)
        same_bits(K.blur_sep(xd, dev(k65)).cpu().numpy(), K.blur_sep(xd, dev(k63)).cpu().numpy(), shape)


# ---- the 32-row instantiations: batches only ---------------------------------------------------------------------------------

def kernels_of(fn):
    """Names of the device kernels `fn` launched, spaces removed."""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if getattr(e, "self_device_time_total", getattr(e, "self_cuda_time_total", 0)) > 0]
    return out, [n.replace(" ", "") for n in names]


def ran(names, th, klen_arg):
    """blur_sep_kernel<th, klen_arg> is among the kernels (demangled, or in the Itanium mangling) and no other instantiation is."""
    mine = [n for n in names if "blur_sep_kernel" in n]
    ok = [n for n in mine if f"blur_sep_kernel<{th},{klen_arg}>" in n or f"blur_sep_kernelILi{th}ELi{klen_arg}EE" in n]
    return len(mine) == 1 and ok == mine


@pytest.mark.parametrize("shape", [(33, 65), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("klen,th,klen_arg", [(31, 32, 31), (11, 32, 0), (57, 32, 0), (59, 16, 0)])
def test_batches_run_the_32_row_tiles_and_small_calls_the_16_row_ones(K, klen, th, klen_arg, shape):
    """xai_blur_sep_f32 takes 32-row tiles once the call has 8 workgroups of 16 rows per CU and the 32-row tile fits 64 KiB of
    LDS (klen <= 57); klen 31 has its own form at either height.  With just enough planes for that threshold: the kernel that
    ran carries the expected template arguments, the same shape with 2 x 2 planes runs <16, ...>, integer data comes back
    exactly over the whole batch and N(0, 1) data equals the two 1-D passes bit for bit."""
    H, W = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    planes = math.ceil(8 * cus / (math.ceil(W / 64) * math.ceil(H / 16)))
    assert planes <= 65535
    x, k, want = R.exact_case(klen, (planes, 1) + shape, 3)
    xd, kd = dev(x), dev(k)
    got, names = kernels_of(lambda: K.blur_sep(xd, kd))
    assert ran(names, th, klen_arg), names
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want)
    few = xd[:4].view(R.PLANES + shape)
    _, names = kernels_of(lambda: (K.blur_sep(few, kd), two_pass(K, few, kd)))
    assert ran(names, 16, klen_arg) and any("blur_1d_kernel" in n for n in names), names
    x, k = R.normal_case(klen, (planes, 1) + shape, 3)
    xd, kd = dev(x), dev(k)
    same_bits(K.blur_sep(xd, kd).cpu().numpy(), two_pass(K, xd, kd).cpu().numpy(), (klen, shape, planes))


def test_one_plane_short_of_the_threshold_still_runs_16_row_tiles(K):
    """tiles16 >= 8 x CU count is the rule: one plane fewer at one tile per plane stays on <16, 31>."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x, k = R.normal_case(31, (8 * cus - 1, 1, 16, 64), 3)
    xd, kd = dev(x), dev(k)
    got, names = kernels_of(lambda: K.blur_sep(xd, kd))
    assert ran(names, 16, 31), names
    same_bits(got.cpu().numpy(), two_pass(K, xd, kd).cpu().numpy(), "8 CU - 1 planes")


# ---- GaussianBlur ------------------------------------------------------------------------------------------------------------

def test_gaussian_blur_accepts_host_strided_and_double_inputs(K):
    """xai_engine.blur.GaussianBlur moves, converts and packs its input before K7 sees it: a CPU tensor, a non-contiguous device
    view and a float64 tensor (of fp32 values) give the bits of the contiguous fp32 device tensor."""
    from xai_engine.blur import GaussianBlur
    blur = GaussianBlur(31, 31, DEV)
    x = torch.from_numpy(R.normal_case(31, (2, 3, 33, 65), 11)[0])
    want = blur(x.to(DEV)).cpu().numpy()
    same_bits(want, K.blur_sep(x.to(DEV), blur.k1d).cpu().numpy(), "GaussianBlur is K.blur_sep")
    same_bits(blur(x).cpu().numpy(), want, "CPU input")
    wide = torch.randn(2, 3, 33, 130, device=DEV)
    wide[..., ::2] = x.to(DEV)
    strided = wide[..., ::2]
    assert not strided.is_contiguous() and torch.equal(strided, x.to(DEV))
    same_bits(blur(strided).cpu().numpy(), want, "non-contiguous input")
    transposed = x.to(DEV).transpose(2, 3).contiguous().transpose(2, 3)
    assert not transposed.is_contiguous()
    same_bits(blur(transposed).cpu().numpy(), want, "transposed input")
    same_bits(blur(x.double()).cpu().numpy(), want, "float64 host input")
    same_bits(blur(x.double().to(DEV)).cpu().numpy(), want, "float64 device input")
