"""Device quickshift on the MI355X: K53-K55 (include/xai_hip_ext5.h) against the NumPy restatement of scikit-image 0.18.3
(tests/quickshift_restated.py) on the same features and the same noise.

What is exact and what is bounded.  The squared distances, every comparison, `closest`, `dist`, `parent`, the tree, the labels and D
are integers or correctly rounded fp64 operations in a stated order: compared bit for bit.  The densities add exp terms, and the
device's exp and NumPy's may differ in the last place: compared within the per-case bound of quickshift_restated.margin,
n_terms * (2^-52 + ulp(max density)).  A parent can only be compared where no density comparison hinges on that difference: every
case is asserted (never skipped) to keep all compared densities at least 100 bounds apart."""
import functools

import numpy as np
import pytest
import torch

import quickshift_restated as R
from conftest import load_golden
from helpers import tiny_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device(K, f, noise, ks, md):
    """One image through K53-K55 -> the dict of R.quickshift_from, as host arrays"""
    fd, nd = _dev(f)[None], _dev(noise)[None]
    dens = K.quickshift_density(fd, nd, ks)
    parent, closest, dist, tree = K.quickshift_parent(fd, dens, ks, md, want_tree=True)
    labels, D = K.quickshift_labels(parent)
    torch.cuda.synchronize()
    host = lambda t: t[0].cpu().numpy()  # noqa: E731
    return dict(dens=host(dens), parent=host(parent), tree=host(tree), closest=host(closest), dist=host(dist), labels=host(labels),
                D=int(D[0]))


def _same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def _hold(name, got, want, f, ks):
    """The margin condition, then: densities within the bound, everything else exactly."""
    bound, gap = R.margin(f, want["dens"], ks)
    nan = np.isnan(want["dens"])
    err = float(np.abs(got["dens"][~nan] - want["dens"][~nan]).max())
    print(f"{name}: bound {bound:.3e} gap {gap:.3e} max |dens - restated| {err:.3e} D {want['D']}")
    assert gap >= 100 * bound, (name, gap, bound)
    assert np.array_equal(np.isnan(got["dens"]), nan) and err <= bound, (name, err, bound)
    assert np.array_equal(got["tree"], want["tree"]) and np.array_equal(got["parent"], want["parent"]), name
    assert _same_bits(got["closest"], want["closest"]) and _same_bits(got["dist"], want["dist"]), name
    assert np.array_equal(got["labels"], want["labels"]) and got["D"] == want["D"], name


# ------------------------------------------------------------------------------------------------ skimage's recorded runs
@pytest.mark.parametrize("tag", ["lime", "cut", "roots"])
def test_fixture_cases_equal_skimage(K, tag):
    g = load_golden("quickshift.npz")
    ratio, ks, md, seed = g[f"{tag}_params"].tolist()
    f = g[f"{tag}_features"]
    noise = np.random.RandomState(int(seed)).normal(scale=0.00001, size=f.shape[:2])
    got = _device(K, f, noise, ks, md)
    _hold(tag, got, R.quickshift_from(f, noise, ks, md), f, ks)
    assert np.array_equal(got["labels"], g[f"{tag}_labels"]) and np.array_equal(got["tree"], g[f"{tag}_parent"])
    assert _same_bits(got["dist"], g[f"{tag}_dist"])


def test_quickshift_with_skimages_signature_equals_skimage():
    """the whole front: this engine's own Lab features (within 1e-12 of skimage's) and draw, the kernels, the host arrays"""
    from xai_engine import quickshift as Q
    g = load_golden("quickshift.npz")
    for tag in ("cut", "lime"):
        ratio, ks, md, seed = g[f"{tag}_params"].tolist()
        labels, parent, dist = Q.quickshift(g[f"{tag}_image"], ratio=ratio, kernel_size=ks, max_dist=md, return_tree=True, random_seed=int(seed),
                                            device=DEV)
        assert labels.dtype == parent.dtype == np.int64 and dist.dtype == np.float64
        assert np.array_equal(labels, g[f"{tag}_labels"]) and np.array_equal(parent, g[f"{tag}_parent"])
        assert np.abs(dist - g[f"{tag}_dist"]).max() <= 1e-11             # features within 1e-12: distances of order 10 move by as much
        assert np.array_equal(Q.quickshift(g[f"{tag}_image"], ratio=ratio, kernel_size=ks, max_dist=md, random_seed=int(seed), device=DEV), labels)


# ------------------------------------------------------------------------------------------------ shapes
@functools.lru_cache(maxsize=None)
def _seeded(H, W, C, ks, md, seed):
    """Lab-like features (a smooth field plus texture, scaled so that max_dist cuts some parents) and skimage's noise -> (f, noise, want)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.stack([3.0 * np.sin(0.37 * yy + c) * np.cos(0.23 * xx - c) + rng.random((H, W)) for c in range(C)], -1)
    noise = np.random.RandomState(seed).normal(scale=0.00001, size=(H, W))
    return f, noise, R.quickshift_from(f, noise, ks, md)


SHAPES = [(5, 7, 3, 4.0), (33, 47, 3, 4.0), (1, 40, 3, 1.0), (40, 1, 3, 1.0), (33, 47, 1, 1.5), (20, 23, 3, 1.0), (17, 16, 1, 1.5)]


@pytest.mark.parametrize("H, W, C, ks", SHAPES)
def test_shapes_against_the_restatement(K, H, W, C, ks):
    """5 x 7 at kw = 12: smaller than the window in both axes; 33 x 47: no multiple of the tile, 3 x 3 workgroups; one row, one
    column; C = 1 and C = 3; kernel_size 1 (kw 3), 1.5 (kw = ceil(4.5) = 5) and 4 (kw 12)"""
    f, noise, want = _seeded(H, W, C, ks, 2.5, 1000 + H)
    _hold(f"{H}x{W}x{C} ks {ks}", _device(K, f, noise, ks, 2.5), want, f, ks)


def test_c1_without_lab_through_the_front():
    from xai_engine import quickshift as Q
    rng = np.random.default_rng(8)
    img = rng.random((14, 19))
    f = Q.quickshift_features(img, 2.0, convert2lab=False)
    want = R.quickshift_from(f, np.random.RandomState(3).normal(scale=0.00001, size=(14, 19)), 1.5, 1.0)
    assert R.margin(f, want["dens"], 1.5)[1] >= 100 * R.margin(f, want["dens"], 1.5)[0]
    labels, parent, dist = Q.quickshift(img, ratio=2.0, kernel_size=1.5, max_dist=1.0, return_tree=True, convert2lab=False, random_seed=3, device=DEV)
    assert np.array_equal(labels, want["labels"]) and np.array_equal(parent, want["tree"]) and _same_bits(dist, want["dist"])


# ------------------------------------------------------------------------------------------------ ties, chains, the cut, NaN
def test_constant_image_first_in_scan_order_wins_exact_ties(K):
    """every colour distance is 0, so many neighbours tie exactly at d = 1, 2, 4, ...: the strict < keeps the first in scan order"""
    f = np.full((12, 14, 3), 0.25)
    noise = np.random.RandomState(5).normal(scale=0.00001, size=(12, 14))
    want = R.quickshift_from(f, noise, 1.0, 10.0)
    got = _device(K, f, noise, 1.0, 10.0)
    _hold("constant", got, want, f, 1.0)
    real = want["closest"] < R.DBL_MAX
    assert set(np.unique(want["closest"][real])) <= {1.0, 2.0, 4.0, 5.0, 8.0, 9.0, 10.0, 13.0, 18.0}      # sums of two squares <= 3^2 + 3^2
    # a pixel whose two nearest denser neighbours tie: the earlier one in scan order is the parent
    dens, tied = want["dens"], 0
    for r in range(1, 11):
        for c in range(1, 13):
            if want["closest"][r, c] == 1.0:
                denser = [(r_, c_) for r_, c_ in ((r - 1, c), (r, c - 1), (r, c + 1), (r + 1, c)) if dens[r_, c_] > dens[r, c]]
                tied += len(denser) > 1
                assert got["tree"][r, c] == denser[0][0] * 14 + denser[0][1]
    assert tied > 5


def test_monotone_ramp_gives_chains_far_longer_than_the_window(K):
    """a constant 4 x 200 image with a crafted noise ramp: every pixel's parent lies towards larger columns, so the chains to the root
    are about 200 links at a window of 7: K55's walk, not a fixed number of doublings"""
    H, W = 4, 200
    f = np.zeros((H, W, 1))
    noise = 10.0 * np.arange(W)[None, :] + 0.01 * np.arange(H)[:, None]
    want = R.quickshift_from(f, noise, 1.0, 1e6)
    depth, at = 0, np.arange(H * W)
    while (want["parent"].ravel()[at] != at).any():
        at, depth = want["parent"].ravel()[at], depth + 1
    assert depth >= W - 10 and want["D"] <= H
    _hold("ramp", _device(K, f, noise, 1.0, 1e6), want, f, 1.0)


def test_closest_on_both_sides_of_max_dist(K):
    """on a constant image every parent is at d = 1, 2, ... exactly: max_dist = 1 keeps the parents at dist 1 (1 > 1 is false), the
    next double below 1 cuts every one of them, sqrt(2) keeps the diagonal ones too"""
    f = np.full((9, 11, 1), 0.5)
    noise = np.random.RandomState(2).normal(scale=0.00001, size=(9, 11))
    base = R.quickshift_from(f, noise, 1.0, 1e6)
    assert (base["closest"] == 1.0).sum() > 20 and (base["closest"] == 2.0).sum() > 0
    for md in (1.0, float(np.nextafter(1.0, 0.0)), float(np.sqrt(2.0)), float(np.nextafter(np.sqrt(2.0), 0.0))):
        want = R.quickshift_from(f, noise, 1.0, md)
        got = _device(K, f, noise, 1.0, md)
        _hold(f"max_dist {md!r}", got, want, f, 1.0)
        idx = np.arange(99).reshape(9, 11)
        kept = got["parent"] != idx
        assert np.array_equal(kept, (base["closest"] < R.DBL_MAX) & ~(np.sqrt(base["closest"]) > md))
    assert R.quickshift_from(f, noise, 1.0, float(np.nextafter(1.0, 0.0)))["D"] == 99


def test_one_nan_feature(K):
    """exp(NaN) makes the density of every pixel whose window holds the NaN pixel NaN; NaN > x and x > NaN are false: those pixels
    are roots and nobody's parent"""
    f, noise, _ = _seeded(20, 23, 3, 1.0, 2.5, 77)
    f = f.copy()
    f[10, 11, 1] = np.nan
    want = R.quickshift_from(f, noise, 1.0, 2.5)
    nan = np.isnan(want["dens"])
    assert nan.sum() == 49 and nan[7:14, 8:15].all()
    got = _device(K, f, noise, 1.0, 2.5)
    _hold("nan", got, want, f, 1.0)
    idx = np.arange(20 * 23).reshape(20, 23)
    assert (got["parent"][nan] == idx[nan]).all() and not np.isin(got["tree"][~nan], idx[nan]).any()


# ------------------------------------------------------------------------------------------------ batches, graphs
def test_a_batch_equals_its_images_one_by_one(K):
    from xai_engine import quickshift as Q
    f, _, _ = _seeded(33, 47, 3, 4.0, 2.5, 1033)
    fs = np.stack([f, f[::-1].copy(), f])
    noises = np.stack([np.random.RandomState(s).normal(scale=scale, size=(33, 47)) for s, scale in ((1, 0.00001), (2, 0.00001), (3, 1.0))])
    labels, D, tree, dist = Q.quickshift_batch(_dev(fs), _dev(noises), 4.0, 2.5, return_tree=True)
    assert labels.shape == (3, 33, 47) and labels.dtype == torch.int32 and D.shape == (3,) and D.dtype == torch.int32
    for b in range(3):
        one = Q.quickshift_batch(_dev(fs[b:b + 1]), _dev(noises[b:b + 1]), 4.0, 2.5, return_tree=True)
        for got, want in zip((labels, D, tree, dist), one):
            assert torch.equal(got[b:b + 1].view(torch.int64 if got.dtype == torch.float64 else got.dtype),
                               want.view(torch.int64 if want.dtype == torch.float64 else want.dtype))
    assert not torch.equal(labels[0], labels[2])                                    # the same image, a noise that reorders the densities


def test_a_captured_graph_replays_the_eager_launches(K):
    from xai_engine import quickshift as Q
    f, noise, _ = _seeded(33, 47, 3, 4.0, 2.5, 1033)
    fd, nd = _dev(f)[None].clone(), _dev(noise)[None].clone()
    eager = Q.quickshift_batch(fd, nd, 4.0, 2.5, return_tree=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = Q.quickshift_batch(fd, nd, 4.0, 2.5, return_tree=True)
    f2, noise2, _ = _seeded(33, 47, 3, 4.0, 2.5, 2033)
    for ff, nn, want in ((f, noise, eager), (f2, noise2, None), (f, noise, eager)):
        fd.copy_(_dev(ff)[None]); nd.copy_(_dev(nn)[None])
        graph.replay()
        torch.cuda.synchronize()
        want = want or Q.quickshift_batch(fd, nd, 4.0, 2.5, return_tree=True)
        for g, w in zip(out, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ LIME end to end
def test_lime_batch_with_the_device_segmenter_equals_lime_batch_fed_the_restated_labels():
    """two 32 x 40 images on the small test classifier: bit for bit the run whose segments come from the restatement with the same
    drawn seeds, and the RandomState is left in the same state"""
    from xai_engine import lime
    model = tiny_from(load_golden("ig_small.npz"), DEV)
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:32, 0:40]
    imgs = np.stack([np.stack([0.5 + 0.45 * np.sin(0.3 * yy * (b + 1) + c) * np.cos(0.2 * xx + b) for c in range(3)]) for b in range(2)])
    x = torch.from_numpy((imgs + 0.04 * rng.random(imgs.shape)).clip(0, 1).astype(np.float32)).to(DEV)
    seen = []

    def restated(image, seed):
        r = R.quickshift(image, ratio=0.2, kernel_size=4, max_dist=200, random_seed=seed)
        f = R.features(image, 0.2)
        bound, gap = R.margin(f, r["dens"], 4)
        assert gap >= 100 * bound, (gap, bound)
        seen.append(r["D"])
        return r["labels"]
    kw = dict(num_samples=120, top_labels=3, hide_color=0, pass_size=60, want="details")
    rs_a, rs_b = np.random.RandomState(21), np.random.RandomState(21)
    out_a, det_a = lime.lime_batch(x, model, lime.device_quickshift_segments, random_state=rs_a, **kw)
    out_b, det_b = lime.lime_batch(x, model, restated, random_state=rs_b, **kw)
    print("superpixels per image:", seen)
    assert len(seen) == 2 and min(seen) >= 2
    assert rs_a.randint(0, 1 << 30) == rs_b.randint(0, 1 << 30)
    assert all(np.array_equal(a, b) for a, b in zip(det_a.data, det_b.data))
    assert out_a.cpu().numpy().tobytes() == out_b.cpu().numpy().tobytes()
    for name in ("labels", "distances", "weights", "coef", "intercept", "score", "local_pred", "order", "top_labels"):
        assert getattr(det_a, name).cpu().numpy().tobytes() == getattr(det_b, name).cpu().numpy().tobytes(), name
    # hide_color=None needs the labels on the host for the mean colours: still the same run
    kw["hide_color"] = None
    out_c = lime.lime_batch(x, model, lime.device_quickshift_segments, random_state=np.random.RandomState(21), **kw)[0]
    out_d = lime.lime_batch(x, model, restated, random_state=np.random.RandomState(21), **kw)[0]
    assert out_c.cpu().numpy().tobytes() == out_d.cpu().numpy().tobytes()
    # and the token as a plain function: the host labels of one image
    host = lime.device_quickshift_segments(x[0].cpu().numpy().transpose(1, 2, 0), 5)
    assert host.dtype == np.int64 and np.array_equal(host, R.quickshift(x[0].cpu().numpy().transpose(1, 2, 0), 0.2, 4, 200, random_seed=5)["labels"])


def test_harness_row_with_the_device_key():
    """get_CNN_attr(attr_func="lime") with testing_dict["lime_quickshift"] = "device" at 224 x 224: the map of lime_batch with the token
    and the same RandomState, no skimage and no `lime_segments`; another value of the key is refused"""
    from xai_engine import lime
    from xai_engine.sweep import get_CNN_attr
    model = tiny_from(load_golden("ig_small.npz"), DEV)
    yy, xx = np.mgrid[0:224, 0:224]
    rng = np.random.default_rng(60)
    img = np.stack([0.5 + 0.4 * np.sin(yy / 17.0 + c) * np.cos(xx / 23.0 - c) for c in range(3)]).astype(np.float32)
    trans = torch.from_numpy(np.clip(img + 0.1 * (rng.random(img.shape).astype(np.float32) - 0.5), 0, 1))
    td = dict(models=[model], batch_size=50, img_hw=224, device=DEV, attr_func="lime", lime_quickshift="device")
    got = get_CNN_attr(trans[None], trans, 0, dict(td, lime_random_state=np.random.RandomState(7)))
    want, det = lime.lime_batch(trans[None].to(DEV), model, lime.device_quickshift_segments, num_samples=1000, top_labels=5, hide_color=0,
                                random_state=np.random.RandomState(7), want="details")
    assert isinstance(got, np.ndarray) and got.shape == (224, 224) and np.array_equal(got, want[0].cpu().numpy())
    assert det.data[0].shape[1] >= 2 and set(np.unique(got).tolist()) <= {0.0, 3.0}
    with pytest.raises(ValueError, match="lime_quickshift"):
        get_CNN_attr(trans[None], trans, 0, dict(td, lime_quickshift="slic"))


def test_evaluate_perturbation_runs_the_lime_row_with_the_device_segmenter(tmp_path, monkeypatch):
    """a sweep of three synthetic images with --attr_func lime and testing_dict["lime_quickshift"] = "device" through the harness, on
    three streams, in an interpreter that may have no scikit-image: every image attributed, the CSV written"""
    import os
    from PIL import Image
    from xai_engine import harness, lime
    monkeypatch.setattr(lime, "quickshift_segments", lambda image, seed: (_ for _ in ()).throw(AssertionError("the host segmenter ran")))
    model = tiny_from(load_golden("ig_small.npz"), DEV)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:70, 0:76]
    names = []
    for i in range(3):
        name = f"ILSVRC2012_val_{i + 1:08d}.png"
        img = np.stack([0.5 + 0.4 * np.sin(yy / (5.0 + i) + c) * np.cos(xx / 7.0 - c) for c in range(3)], -1) + 0.1 * (rng.random((70, 76, 3)) - 0.5)
        Image.fromarray((img.clip(0, 1) * 255).astype(np.uint8)).save(tmp_path / name)
        names.append(name)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    monkeypatch.setattr(harness, "select_images", lambda td, cc, rank=0, world=1, lazy=False:
                        (names, harness.SelectedImages(str(tmp_path), names, 64, *norm), [0, 0, 0]))
    td = {"models": [model, model], "img_hw": 64, "batch_size": 25, "device": DEV, "attr_func": "lime", "normalize": norm,
          "imagenet_dataset": str(tmp_path), "model_name": "R50", "image_count": 3, "lime_quickshift": "device"}
    total, used, _ = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"), streams=3)
    assert used == 3 and all(np.isfinite(float(v)) for v in total.values())
    assert os.path.exists(tmp_path / "out" / "R50" / "lime_3_images.csv")
