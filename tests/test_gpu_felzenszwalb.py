"""Device Felzenszwalb segmentation on the MI355X: K69-K74 (include/xai_hip_felz.h) and xai_engine/felzenszwalb.py against
scikit-image 0.18.3's binary (tests/golden/felzenszwalb.npz) and the NumPy restatement of the header's contract
(tests/felzenszwalb_restated.py), which tests/test_cpu_felzenszwalb.py and the fixture's generator hold to that binary.

Everything is exact: the contract fixes the order of every operation, so the smoothed image and the costs are compared as bits and the
order, labels and counts as integers.  The fixture's cases have pairwise distinct costs (asserted by its generator), so there the
labels are skimage's; the block image has equal costs and is held to the restatement's stable order."""
import functools
import warnings

import numpy as np
import pytest
import torch

import felzenszwalb_restated as R
from conftest import load_golden
from helpers import tiny_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMALL = ["a", "b", "c", "d", "e", "d23", "d17", "d71", "d11"]
XRAI_SCALES = [50, 100, 150, 250, 500, 1200]


@pytest.fixture(scope="module")
def F():
    from xai_engine import felzenszwalb
    return felzenszwalb


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("felzenszwalb.npz")


def smoothed(seed, H, W, blur, C=3):
    """tests/golden/make_golden_felzenszwalb.py's image generator (C = 3 there)"""
    img = np.random.RandomState(seed).rand(H, W, C)
    for _ in range(blur):
        p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
        img = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    lo, hi = img.min(), img.max()
    if hi > lo:
        img = (img - lo) / (hi - lo) * 2.0 - 1.0
    return img.astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(tag):
    g = golden()
    sigma, min_size = g[f"{tag}_params"]
    return g[f"{tag}_image"].astype(np.float64), float(sigma), int(min_size), g[f"{tag}_scales"], g[f"{tag}_weights"]


@functools.lru_cache(maxsize=None)
def _want(tag):
    """the restatement of a fixture case, fed the stored weights; computed once, never modified"""
    image, sigma, min_size, scales, weights = _case(tag)
    return R.felzenszwalb(image, scales, sigma, min_size, weights=weights)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ the stages against the fixture
@pytest.mark.parametrize("tag", SMALL)
def test_smoothed_bits_key_bits_and_order_given_the_stored_weights(F, tag):
    image, sigma, min_size, scales, weights = _case(tag)
    sm, keys, order, _, stats, _, _, status = F._stages(_dev(image[None]), scales, sigma, min_size, weights)
    assert int(status[0]) == 0
    g, want = golden(), _want(tag)
    assert np.array_equal(_bits(sm[0].cpu().numpy()), _bits(g[f"{tag}_smoothed"]))          # SciPy's gaussian_filter, bit for bit
    E = len(want.costs)                                                          # 0 for the 1 x 1 image
    assert np.array_equal(keys[0, :E].cpu().numpy(), _bits(want.costs[want.order]))
    assert np.array_equal(order[0, :E].cpu().numpy(), want.order)
    assert np.array_equal(stats[0].cpu().numpy(), np.stack([want.tested, want.merged], 1))


@pytest.mark.parametrize("tag", SMALL)
def test_labels_and_counts_equal_skimage_for_every_scale(F, tag):
    image, sigma, min_size, scales, weights = _case(tag)
    out = F._stages(_dev(image[None]), scales, sigma, min_size, weights)
    want = golden()[f"{tag}_labels"]
    assert int(out[7][0]) == 0 and out[5].dtype == torch.int32 and out[6].dtype == torch.int32
    assert np.array_equal(out[5][0].cpu().numpy(), want)
    assert np.array_equal(out[6][0].cpu().numpy(), want.reshape(len(scales), -1).max(1) + 1)


def test_the_big_case_once(F):
    g = golden()
    image = smoothed(3, 224, 224, 2)
    labels, counts = F.felzenszwalb_batch(image[None], g["big_scales"], 0.8, 150)
    assert labels.is_cuda and tuple(labels.shape) == (1, 6, 224, 224)
    assert np.array_equal(labels[0].cpu().numpy(), g["big_labels"])
    assert np.array_equal(counts[0].cpu().numpy(), g["big_labels"].reshape(6, -1).max(1) + 1)


def test_a_batch_of_three_different_images_equals_the_three_single_calls(F):
    images = np.stack([smoothed(seed, 37, 29, 2) for seed in (21, 22, 23)])
    labels, counts = F.felzenszwalb_batch(images, [30, 300], 0.8, 10)
    assert tuple(labels.shape) == (3, 2, 37, 29) and tuple(counts.shape) == (3, 2)
    for b in range(3):
        one, cnt = F.felzenszwalb_batch(images[b:b + 1], [30, 300], 0.8, 10)
        assert torch.equal(one[0], labels[b]) and torch.equal(cnt[0], counts[b])
        assert np.array_equal(one[0].cpu().numpy(), R.felzenszwalb(images[b], [30, 300], 0.8, 10).labels)
    assert len({labels[b].cpu().numpy().tobytes() for b in range(3)}) == 3


# ------------------------------------------------------------------------------------------------ against the restatement
def test_equal_costs_follow_the_stable_rule(F):
    """constant 8 x 8 blocks: about half of the 8930 costs are repeated"""
    blocks = np.random.RandomState(5).rand(6, 6, 3).round(1)
    image = np.kron(blocks, np.ones((8, 8, 1)))
    want = R.felzenszwalb(image, XRAI_SCALES + [1], 0.8, 20)
    assert len(np.unique(want.costs)) < len(want.costs) // 2 + 500 and len(want.costs) == 8930
    out = F._stages(_dev(image[None]), XRAI_SCALES + [1], 0.8, 20, None)
    assert np.array_equal(out[2][0].cpu().numpy(), want.order)
    assert np.array_equal(out[5][0].cpu().numpy(), want.labels) and np.array_equal(out[6][0].cpu().numpy(), want.counts)


@pytest.mark.parametrize("kw", [dict(sigma=0), dict(min_size=0), dict(min_size=1000), dict(scale=0), dict(scale=1e9)],
                         ids=["sigma0", "min0", "min1000", "scale0", "scale1e9"])
def test_the_ends_of_every_parameter(F, kw):
    image = smoothed(31, 12, 10, 1).astype(np.float64)
    p = dict(dict(scale=30, sigma=0.8, min_size=3), **kw)
    want = R.felzenszwalb(image, [p["scale"]], p["sigma"], p["min_size"])
    got = F.felzenszwalb(image, **p)
    assert got.dtype == np.int64 and np.array_equal(got, want.labels[0])
    if kw == dict(min_size=1000) or kw == dict(scale=1e9):
        assert got.max() == 0
    if kw == dict(sigma=0):
        sm = F._stages(_dev(image[None]), [30], 0, 3, None)[0]
        assert np.array_equal(sm[0].cpu().numpy(), image)                        # no launch for a skipped axis: the image itself


def test_one_and_four_channels_uint8_and_float32(F):
    grey = smoothed(41, 40, 40, 2, C=1)[..., 0].astype(np.float64)              # a 2-D image
    assert np.array_equal(F.felzenszwalb(grey, 100, 0.8, 20), R.felzenszwalb(grey, [100], 0.8, 20).labels[0])
    f32 = smoothed(42, 40, 40, 2)
    assert f32.dtype == np.float32 and np.array_equal(F.felzenszwalb(f32, 100, 0.8, 20), R.felzenszwalb(f32, [100], 0.8, 20).labels[0])
    four = smoothed(43, 20, 20, 1, C=4).astype(np.float64)
    with pytest.warns(RuntimeWarning, match="third dimension of 4"):
        got = F.felzenszwalb(four, 50, 0.8, 5)
    assert np.array_equal(got, R.felzenszwalb(four, [50], 0.8, 5).labels[0])
    u8 = np.round((smoothed(44, 20, 20, 2) + 1) * 127.5).astype(np.uint8)
    want = R.felzenszwalb(u8, [50], 0.8, 5)
    assert np.array_equal(F.felzenszwalb(u8, 50, 0.8, 5), want.labels[0]) and want.counts[0] > 1
    wide = smoothed(45, 3, 4, 0).astype(np.float64)                              # sigma 2: the kernel's radius 8 is wider than the image
    assert np.array_equal(F.felzenszwalb(wide, 100, 2.0, 0), R.felzenszwalb(wide, [100], 2.0, 0).labels[0])


def test_a_nan_image_raises(F):
    from xai_engine import XaiHipError
    image = smoothed(51, 9, 9, 1).astype(np.float64)
    image[4, 4, 1] = np.nan
    with pytest.raises(XaiHipError, match="NaN or an infinite pixel"):            # the status word K70 set
        F.felzenszwalb_batch(_dev(image[None]), [50])
    with pytest.raises(XaiHipError, match="NaN or an infinite pixel"):
        F.felzenszwalb(image, 50)
    image[4, 4, 1] = np.inf
    with pytest.raises(XaiHipError, match="NaN or an infinite pixel"):
        F.felzenszwalb_batch(_dev(image[None]), [50])


@pytest.mark.parametrize("tag", ["a", "d17"])
def test_the_skimage_signature_returns_skimages_int64_labels(F, tag):
    image, sigma, min_size, scales, weights = _case(tag)
    if not np.array_equal(F.gaussian_weights(sigma), weights):
        pytest.fail("gaussian_weights differs from the stored weights under this NumPy: the bit-for-bit claim needs weights=")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = F.felzenszwalb(image, scale=scales[0], sigma=sigma, min_size=min_size)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, golden()[f"{tag}_labels"][0])


# ------------------------------------------------------------------------------------------------ XRAI
def test_xrai_getmask_with_device_segments(F):
    import xrai_restated as XR
    from xai_engine import xrai
    x = smoothed(61, 32, 32, 2)                                                    # (H, W, C) float32
    attr = np.random.RandomState(62).randn(32, 32, 3).astype(np.float32)
    maps = xrai.device_felzenszwalb_label_maps(x, device=DEV)
    assert maps.is_cuda and maps.dtype == torch.int32 and tuple(maps.shape) == (6, 32, 32)
    norm = xrai._normalize_image(x).numpy().astype(np.float64)
    want = R.felzenszwalb(norm, XRAI_SCALES, 0.8, 150)
    assert np.array_equal(maps.cpu().numpy(), want.labels) and want.counts.max() > 1
    both = xrai.device_felzenszwalb_label_maps(np.stack([x, x[::-1].copy()]), device=DEV)
    assert tuple(both.shape) == (2, 6, 32, 32) and torch.equal(both[0], maps)
    masks = XR.dilate(XR.unpack(maps.cpu().numpy()), 5)
    got = xrai.XRAI().GetMask(x, segments="device", base_attribution=attr)
    np.testing.assert_array_equal(got, xrai.XRAI().GetMask(x, segments=masks, base_attribution=attr))
    with pytest.raises(ValueError, match="'device'"):
        xrai.XRAI().GetMask(x, segments="gpu", base_attribution=attr)


def test_the_xrai_sweep_row_with_the_device_segmenter(F):
    from xai_engine import xrai
    from xai_engine.sweep import get_CNN_attr
    model = tiny_from(load_golden("ig_small.npz"), DEV)
    x = torch.from_numpy(smoothed(71, 224, 224, 3).transpose(2, 0, 1)[None].copy())
    with torch.no_grad():
        t = model(x.to(DEV)).argmax(1)[0]
    td = {"models": [model], "img_hw": 224, "batch_size": 25, "device": DEV, "attr_func": "xrai"}
    got = get_CNN_attr(x, None, t, dict(td, xrai_felzenszwalb="device"))
    maps = xrai.device_felzenszwalb_label_maps(x[0].permute(1, 2, 0), device=DEV)
    assert int(maps.amax()) > 0
    want = get_CNN_attr(x, None, t, dict(td, xrai_label_maps=lambda x_hwc: maps))
    assert got.shape == (224, 224) and np.array_equal(got, want)
    # an explicit xrai_label_maps wins over the key
    np.testing.assert_array_equal(get_CNN_attr(x, None, t, dict(td, xrai_felzenszwalb="device", xrai_label_maps=lambda x_hwc: maps)), want)
    with pytest.raises(ValueError, match="xrai_felzenszwalb"):
        get_CNN_attr(x, None, t, dict(td, xrai_felzenszwalb="opencv"))
