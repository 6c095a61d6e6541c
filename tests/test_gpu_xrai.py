"""XRAI on the MI355X: K29 bit for bit against scipy's dilation and a host bit-pack, K30 against the reference's recorded runs
(tests/golden/xrai.npz) and the fp64 restatement (tests/xrai_restated.py), the reference interface and the harness row.

What is exact and what is not.  K29 is integer work: every word equal.  K30's counts, selection keys, pixel_iter and ranks are
integers and must be equal; a gain is float32(fp64 sum / count) where the reference takes a float32 pairwise mean, so `out` is
held to conftest.BAR.  The selections can only be compared where they do not hinge on that rounding: every case here, stored or
seeded, is asserted (never skipped) to keep a margin between the winner and the best candidate with a different pixel set of at
least 100 times the largest float32-vs-fp64 gain difference (xrai_restated.conditioned)."""
import functools

import numpy as np
import pytest
import torch

import xrai_restated as R
from conftest import BAR, check, load_golden
from helpers import tiny_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN_CASES = "abcdef"


@pytest.fixture(scope="module")
def X():
    from xai_engine import xrai
    return xrai


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_attr(attr3):
    """(H, W, C) host attribution -> (1, C, H, W) on the device."""
    return torch.from_numpy(np.ascontiguousarray(attr3)).permute(2, 0, 1)[None].to(DEV)


# ------------------------------------------------------------------------------------------------------------- K29
@functools.lru_cache(maxsize=None)
def _pack_case(H, W):
    """Two label maps: Voronoi cells relabelled -3, -1, 1, ... (gaps: every second label is absent; a negative label_min) and a
    coarser one from 0; the cells tile the image, so masks touch all four borders."""
    rng = np.random.default_rng(H * 1000 + W)
    a = R.voronoi_labels(H, W, 9, rng).astype(np.int32) * 2 - 3
    b = R.voronoi_labels(H, W, 4, rng).astype(np.int32)
    maps = np.stack([a, b])
    masks = R.unpack(maps)
    assert any(not m.any() for m in masks) and a.min() == -3
    for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert any(m[edge].any() for m in masks)
    return maps, masks


@pytest.mark.parametrize("radius", [0, 2, 5])
@pytest.mark.parametrize("shape", [(40, 36), (65, 63), (7, 300)])
def test_k29_packs_and_dilates_bit_for_bit(X, shape, radius):
    """(65, 63) has 4095 pixels: one dead tail bit; (7, 300): H is smaller than the footprint of radius 5."""
    H, W = shape
    maps, masks = _pack_case(H, W)
    want = R.pack_bits(R.dilate(masks, radius), shape)
    packed = X.pack_segments(maps, dilation_rad=radius, device=DEV)
    assert packed.counts == [len(masks)] and packed.mask_first.tolist() == [0, len(masks)] and (packed.H, packed.W) == shape
    got = _u64(packed.bits)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(packed.span.cpu().numpy(), R.spans(want))
    tail = (H * W) % 64
    if tail:
        assert not (got[:, -1] >> np.uint64(tail)).any()
    # the uint8-mask path equals the label path; boolean masks and a list of (H, W) masks are the same input
    as_u8 = X.pack_segments(np.stack(masks).astype(np.uint8), dilation_rad=radius, device=DEV)
    np.testing.assert_array_equal(_u64(as_u8.bits), want)
    np.testing.assert_array_equal(as_u8.span.cpu().numpy(), R.spans(want))
    as_list = X.pack_segments([torch.from_numpy(m) for m in masks], dilation_rad=radius, device=DEV)
    np.testing.assert_array_equal(_u64(as_list.bits), want)


def test_k29_ignores_labels_outside_the_stated_range(X):
    """The raw entry: a label below label_min or above label_max belongs to no mask, and writes nothing outside the planes."""
    from xai_engine import kernels as K
    lab = torch.tensor([[[0, 1, 2, 3], [4, 5, -7, 99]]], dtype=torch.int32, device=DEV)
    lo, hi = torch.tensor([1], dtype=torch.int32, device=DEV), torch.tensor([4], dtype=torch.int32, device=DEV)
    bits, span = K.xrai_pack(2, 4, 0, 4, labels=lab, label_min=lo, label_max=hi)
    assert _u64(bits)[:, 0].tolist() == [1 << 1, 1 << 2, 1 << 3, 1 << 4] and span.tolist() == [[0, 0]] * 4


# ------------------------------------------------------------------------------------------------------------- K30
def _run(X, attr3, segments, th=1.0, mpd=50, fast=False):
    out, rk = X.xrai_batch(_dev_attr(attr3), segments, area_threshold=th, min_pixel_diff=mpd, algorithm="fast" if fast else "full",
                           want_segments=True)
    return out, rk


def _compare(name, out, rk, i, want, against):
    """image i of a K30 result against a restated / recorded run: integers equal, `out` within BAR"""
    assert rk.n_sel[i] == len(want["keys"]) and rk.n_uncomputed[i] == want["n_uncomputed"], (name, rk.n_sel[i], rk.n_uncomputed[i])
    np.testing.assert_array_equal(rk.sel_key[i].cpu().numpy(), want["keys"], err_msg=name)
    np.testing.assert_array_equal(rk.pixel_iter[i].cpu().numpy(), want["pixel_iter"], err_msg=name)
    check(f"xrai/{name}/gains", rk.sel_gain[i].cpu().numpy(), want["gains"], BAR, against=against)
    check(f"xrai/{name}/out", out[i].cpu().numpy(), want["out"], BAR, against=against)


@functools.lru_cache(maxsize=None)
def _golden(tag):
    g = load_golden("xrai.npz")
    i, radius, mpd, th, fast = g[f"{tag}_params"].tolist()
    maps, attr3 = g[f"in{int(i)}_maps"], g[f"in{int(i)}_attr"]
    masks = R.dilate(R.unpack(maps), int(radius))
    attr = attr3.max(-1)
    r32 = R.xrai_fast(attr, masks, int(mpd), np.float32) if fast else R.xrai(attr, masks, float(th), int(mpd), np.float32)
    assert np.array_equal(r32["keys"], g[f"{tag}_keys"]) and np.array_equal(r32["ranks"], g[f"{tag}_ranks"])
    margin, gain_err = g[f"{tag}_cond"].tolist()
    assert margin >= 100 * gain_err
    want = dict(r32, out=g[f"{tag}_out"], gains=g[f"{tag}_gains"])
    return maps, attr3, int(radius), int(mpd), float(th), bool(fast), want, g[f"{tag}_ranks"]


@pytest.mark.parametrize("tag", GOLDEN_CASES)
def test_k30_against_the_reference_runs(X, tag):
    """a, b: coverage equal to 1 (min_pixel_diff 50 and 1); c: coverage below 1; d: area_threshold 0.3; e, f: algorithm "fast"."""
    maps, attr3, radius, mpd, th, fast, want, ranks = _golden(tag)
    out, rk = _run(X, attr3, X.pack_segments(maps, dilation_rad=radius, device=DEV), th, mpd, fast)
    _compare(f"golden/{tag}", out, rk, 0, want, "reference XRAI")
    np.testing.assert_array_equal(X.ranked_segments(rk.pixel_iter[0].cpu().numpy(), rk.sel_gain[0].cpu().numpy()), ranks)


@functools.lru_cache(maxsize=None)
def _seeded(kind):
    """-> maps (or None), masks, attr3, mpd, th, fast, the fp64 restatement's result.  Every case is asserted well conditioned."""
    th, mpd, fast, maps = 1.0, 50, False, None
    if kind in ("big", "big_fast", "big_threshold"):
        maps, attr3 = R.seeded_case(130, 126, (40, 15, 5), 1)
        masks = R.dilate(R.unpack(maps), 5)
        fast, th = kind == "big_fast", 0.3 if kind == "big_threshold" else 1.0
    elif kind == "twins":
        one, attr3 = R.seeded_case(40, 36, (12,), 3)
        maps = np.concatenate([one, one])
        masks, mpd = R.dilate(R.unpack(maps), 2), 1
    elif kind == "gaps":
        maps, attr3 = R.seeded_case(65, 63, (30, 12), 4)
        maps = maps * 3 - 5                                           # two of three labels absent, label_min -5
        masks = R.dilate(R.unpack(maps), 5)
    elif kind == "cells150":
        maps, attr3 = R.seeded_case(65, 63, (150,), 5)
        masks, mpd = R.unpack(maps), 1
        assert len(masks) >= 120                                      # more candidates than waves in the workgroup
    elif kind == "negative":
        maps, attr3 = R.seeded_case(65, 63, (30, 12, 4), 6)
        attr3 = attr3 - (attr3.max() + 1.0)
        masks = R.dilate(R.unpack(maps), 5)
    else:
        raise KeyError(kind)
    attr = attr3.max(-1)
    want = R.xrai_fast(attr, masks, mpd, np.float64) if fast else R.xrai(attr, masks, th, mpd, np.float64)
    assert R.conditioned(want), (kind, want["margin"], want["gain_err"])
    return maps, masks, attr3, mpd, th, fast, want


@pytest.mark.parametrize("kind", ["big", "big_fast", "big_threshold", "twins", "gaps", "cells150", "negative"])
def test_k30_against_the_restatement(X, kind):
    """130 x 126 (full, fast, area_threshold 0.3); the same label map twice; absent labels; 150 one-cell masks; attr all negative."""
    maps, masks, attr3, mpd, th, fast, want = _seeded(kind)
    radius = {"twins": 2, "cells150": 0}.get(kind, 5)
    out, rk = _run(X, attr3, X.pack_segments(maps, dilation_rad=radius, device=DEV), th, mpd, fast)
    _compare(f"restated/{kind}", out, rk, 0, want, "restatement, fp64 sums")
    if kind == "twins":
        # every candidate ties with its twin: the lower index wins, the twin adds nothing afterwards and is dropped
        n = len(masks) // 2
        assert len(want["keys"]) == n and (want["keys"] < n).all()
    if kind == "gaps":
        assert sum(not m.any() for m in masks) > len(masks) // 2
    if kind == "negative":
        assert (out < 0).all()
    if kind == "big_threshold":
        assert 0 < rk.n_uncomputed[0] < 0.7 * 130 * 126


def test_k30_without_masks_and_a_batch_of_images_with_different_mask_counts(X):
    """M = 0: nothing is selected and every pixel gets the mean attribution.  A batch of three images, the middle one without a
    mask, gives what the three images give alone."""
    a, b = _golden("a"), _golden("b")
    attr3 = a[1]
    out, rk = _run(X, attr3, [[]])
    assert rk.n_sel == [0] and rk.n_uncomputed == [40 * 36] and (rk.pixel_iter == -1).all() and rk.sel_key[0].numel() == 0
    mean = np.float32(attr3.max(-1).astype(np.float64).sum() / (40 * 36))
    check("xrai/no_masks/out", out[0].cpu().numpy(), np.full((40, 36), mean), BAR, against="fp64 mean")
    assert len(np.unique(out.cpu().numpy())) == 1

    # per-image parameters are shared in one launch: both stored cases with b's min_pixel_diff
    batch = torch.cat([_dev_attr(a[1]), _dev_attr(attr3), _dev_attr(b[1])])
    segs = X.pack_segments([R.dilate(R.unpack(a[0]), 2), [], np.stack(R.dilate(R.unpack(b[0]), 5))], dilation_rad=0, device=DEV)
    assert segs.counts == [19, 0, 18] and segs.mask_first.tolist() == [0, 19, 19, 37]
    outs, rks = X.xrai_batch(batch, segs, min_pixel_diff=1, want_segments=True)
    singles = [_run(X, a[1], X.pack_segments(a[0], 2, device=DEV), mpd=1), (out, rk), _run(X, b[1], X.pack_segments(b[0], 5, device=DEV), mpd=1)]
    for i, (o1, r1) in enumerate(singles):
        assert torch.equal(outs[i], o1[0]) and torch.equal(rks.pixel_iter[i], r1.pixel_iter[0])
        assert torch.equal(rks.sel_key[i], r1.sel_key[0]) and torch.equal(rks.sel_gain[i], r1.sel_gain[0])
        assert rks.n_sel[i] == r1.n_sel[0] and rks.n_uncomputed[i] == r1.n_uncomputed[0]
    _compare("batch/b", outs, rks, 2, b[6], "reference XRAI")


def test_k30_two_runs_give_the_same_bits(X):
    maps, masks, attr3, mpd, th, fast, want = _seeded("big")
    segs = X.pack_segments(maps, dilation_rad=5, device=DEV)
    (o1, r1), (o2, r2) = _run(X, attr3, segs), _run(X, attr3, segs)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(r1.pixel_iter, r2.pixel_iter)
    assert torch.equal(r1.sel_key[0], r2.sel_key[0]) and torch.equal(r1.sel_gain[0].view(torch.int32), r2.sel_gain[0].view(torch.int32))


def test_k30_stops_where_the_reference_crashes_on_a_nan_patch(X):
    """Disjoint cells, a patch of NaN: the cells without NaN are selected, then masks remain and none has a gain above -inf --
    the reference's KeyError (remaining_masks[None]), a ValueError here."""
    maps, attr3 = R.seeded_case(40, 36, (12,), 7)
    attr3 = attr3.copy()
    attr3[10:14, 8:13] = np.nan
    with pytest.raises(KeyError):
        R.xrai(attr3.max(-1), R.unpack(maps), 1.0, 1, np.float64)
    segs = X.pack_segments(maps, dilation_rad=0, device=DEV)
    with pytest.raises(ValueError, match="reference crashes"):
        _run(X, attr3, segs, mpd=1)
    with pytest.raises(ValueError, match="sort"):
        _run(X, attr3, segs, mpd=1, fast=True)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_getmask_matches_the_reference_interface_run(X):
    """XRAI().GetMask / GetMaskWithDetails(x, segments=..., base_attribution=...) against the reference's own call on case c."""
    from util.attribution_methods import XRAIBuilder
    g = load_golden("xrai.npz")
    maps, attr3, radius = _golden("c")[:3]
    masks = R.dilate(R.unpack(maps), radius)
    x = np.zeros_like(attr3)
    mask = XRAIBuilder.XRAI().GetMask(x, segments=masks, base_attribution=attr3)
    assert isinstance(mask, np.ndarray) and mask.dtype == np.float64 and mask.shape == attr3.shape[:2]
    assert np.array_equal(mask, mask.astype(np.float32))              # float64 holding float32 gains, as the reference's
    check("xrai/api/GetMask", mask, g["api_mask"], BAR, against="reference XRAI")
    p = XRAIBuilder.XRAIParameters(return_xrai_segments=True, return_ig_attributions=True)
    res = XRAIBuilder.XRAI().GetMaskWithDetails(x, segments=masks, base_attribution=torch.from_numpy(attr3).to(DEV), extra_parameters=p)
    assert isinstance(res, XRAIBuilder.XRAIOutput) and res.baselines is None and res.ig_attribution is not None
    np.testing.assert_array_equal(res.attribution_mask, mask)
    np.testing.assert_array_equal(res.segments, g["api_segments"])
    p.flatten_xrai_segments = False
    res = XRAIBuilder.XRAI().GetMaskWithDetails(x, segments=masks, base_attribution=attr3, extra_parameters=p)
    assert len(res.segments) == int(g["api_mask_count"]) and res.segments[0].dtype == bool
    np.testing.assert_array_equal(np.packbits(np.stack(res.segments), axis=None), g["api_mask_list"])


SWEEP_SEED = 2


def _stub_label_maps(x_hwc):
    """about 100 masks at 224 x 224 in place of Felzenszwalb's segmentation"""
    assert tuple(x_hwc.shape) == (224, 224, 3) and not x_hwc.is_cuda
    rng = np.random.default_rng(SWEEP_SEED)
    return np.stack([R.voronoi_labels(224, 224, n, rng) for n in (60, 30, 10)])


def test_the_xrai_harness_row_on_a_tiny_classifier(X):
    """evaluatePerturbation.py:142-146 on TinyNet at 224 x 224: the engine's IG, max over the channels, the segmenter's label maps
    dilated by 5, the greedy loop, |.| -- against the restatement fed with the same IG."""
    from xai_engine.ig import IG
    from xai_engine.sweep import get_CNN_attr
    model = tiny_from(load_golden("ig_small.npz"), DEV)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((1, 3, 224, 224)).astype(np.float32))
    with torch.no_grad():
        t = model(x.to(DEV)).argmax(1)[0]
    td = {"models": [model], "img_hw": 224, "batch_size": 25, "device": DEV, "attr_func": "xrai", "xrai_label_maps": _stub_label_maps}
    host = get_CNN_attr(x, None, t, td)
    devm = get_CNN_attr(x, None, t, dict(td, device_maps=True))
    assert isinstance(host, np.ndarray) and host.shape == (224, 224) and host.dtype == np.float32 and devm.is_cuda
    np.testing.assert_array_equal(host, devm.cpu().numpy())
    ig = IG(x, model, 50, 25, 1, 0, DEV, t).detach().cpu().numpy()
    masks = R.dilate(R.unpack(_stub_label_maps(x[0].permute(1, 2, 0))), 5)
    assert 90 <= len(masks) <= 110
    want = R.xrai(ig.max(0), masks, 1.0, 50, np.float64)
    assert R.conditioned(want), (want["margin"], want["gain_err"])
    check("xrai/harness_row", host, np.abs(want["out"]), BAR, against="restatement, fp64 sums")
    with pytest.raises(ImportError, match="segments="):
        get_CNN_attr(x, None, t, dict(td, xrai_label_maps=None))
