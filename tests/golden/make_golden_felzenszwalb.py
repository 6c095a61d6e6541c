"""Regenerate tests/golden/felzenszwalb.npz from scikit-image's own Felzenszwalb segmentation.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_felzenszwalb.py        (an interpreter that has scikit-image and SciPy)

The stored fixture was made with scikit-image 0.18.3, the release whose algorithm K69-K74 restate, SciPy 1.7.1 and NumPy 1.26.4
(`version_skimage`, `version_scipy`, `version_numpy` in the file).  skimage.segmentation.felzenszwalb and
scipy.ndimage.gaussian_filter run unmodified on the host.

Cases (`names`); every image is `smoothed(seed, H, W)`: RandomState(seed).rand(H, W, 3), `blur` times 3 x 3 box-filtered, stretched
to [-1, 1] and rounded to float32 (stored so; the segmenters are fed its exact float64 conversion):
  <tag>_image      (H, W, 3) float32
  <tag>_params     [sigma, min_size]
  <tag>_scales     the scales, float64
  <tag>_weights    the Gaussian kernel SciPy used (its _gaussian_kernel1d under this NumPy), float64
  <tag>_smoothed   scipy.ndimage.gaussian_filter(image, [sigma, sigma, 0]), float64
  <tag>_labels     (S, H, W) int16: skimage.segmentation.felzenszwalb(image, scale, sigma, min_size) for every scale
    a 64 x 48 min_size 20, b 33 x 47 min_size 5, c 57 x 43 min_size 150, d 5 x 9 min_size 2, e 112 x 112 min_size 150: sigma 0.8,
      XRAI's six scales and 1
    d23 2 x 3 min_size 1, d17 1 x 7, d71 7 x 1, d11 1 x 1 min_size 2: sigma 0.8, scale 50
  big_labels, big_scales   224 x 224, seed 3, blur 2, XRAI's six scales, sigma 0.8, min_size 150: labels only, the image is regenerated
The generator asserts for every case that the restatement (tests/felzenszwalb_restated.py) equals skimage -- the labels exactly, the
smoothed image bit for bit -- and that the case's edge costs are pairwise distinct (skimage's order among equal costs is unpinned).
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import felzenszwalb_restated as R  # noqa: E402

try:
    import scipy
    import skimage
    from scipy import ndimage as ndi
    from scipy.ndimage.filters import _gaussian_kernel1d
    from skimage.segmentation import felzenszwalb
except ImportError:
    sys.exit("make_golden_felzenszwalb.py: needs scikit-image and SciPy (the fixture was made with 0.18.3 and 1.7.1)")

warnings.filterwarnings("ignore")
XRAI_SCALES = [50, 100, 150, 250, 500, 1200]
BIG = (3, 224, 224, 2)                              # seed, H, W, blur
# tag: (seed, H, W, blur, sigma, min_size, scales)
CASES = {
    "a": (1, 64, 48, 2, 0.8, 20, XRAI_SCALES + [1]),
    "b": (2, 33, 47, 2, 0.8, 5, XRAI_SCALES + [1]),
    "c": (4, 57, 43, 2, 0.8, 150, XRAI_SCALES + [1]),
    "d": (5, 5, 9, 1, 0.8, 2, XRAI_SCALES + [1]),
    "e": (6, 112, 112, 2, 0.8, 150, XRAI_SCALES + [1]),
    "d23": (7, 2, 3, 0, 0.8, 1, [50]),
    "d17": (8, 1, 7, 0, 0.8, 2, [50]),
    "d71": (9, 7, 1, 0, 0.8, 2, [50]),
    "d11": (10, 1, 1, 0, 0.8, 2, [50]),
}


def smoothed(seed, H, W, blur):
    """A random (H, W, 3) image, `blur` times 3 x 3 box-filtered (edges replicated), stretched to [-1, 1] and rounded to float32"""
    img = np.random.RandomState(seed).rand(H, W, 3)
    for _ in range(blur):
        p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
        img = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    lo, hi = img.min(), img.max()
    if hi > lo:
        img = (img - lo) / (hi - lo) * 2.0 - 1.0
    return img.astype(np.float32)


def one_case(image, sigma, min_size, scales):
    """-> (weights, smoothed, labels (S, H, W)) of skimage / SciPy, checked against the restatement"""
    image64 = image.astype(np.float64)
    weights = _gaussian_kernel1d(sigma, 0, int(4.0 * sigma + 0.5))[::-1]
    sm = ndi.gaussian_filter(image64, sigma=[sigma, sigma, 0])
    labels = np.stack([np.asarray(felzenszwalb(image64, scale=s, sigma=sigma, min_size=min_size)) for s in scales])
    got = R.felzenszwalb(image64, scales, sigma, min_size, weights=np.ascontiguousarray(weights))
    assert np.array_equal(got.smoothed.view(np.int64), sm.view(np.int64)), "the smoothed image differs in a bit"
    assert len(np.unique(got.costs)) == len(got.costs), "two edge costs are equal: skimage's order is unpinned on this image"
    assert np.array_equal(got.labels, labels), "the labels differ"
    assert np.array_equal(got.counts, labels.reshape(len(scales), -1).max(1) + 1)
    return np.ascontiguousarray(weights), sm, labels


def main():
    out = {"names": np.array(list(CASES)), "version_skimage": np.array(skimage.__version__),
           "version_scipy": np.array(scipy.__version__), "version_numpy": np.array(np.__version__)}
    for tag, (seed, H, W, blur, sigma, min_size, scales) in CASES.items():
        image = smoothed(seed, H, W, blur)
        weights, sm, labels = one_case(image, sigma, min_size, scales)
        out[f"{tag}_image"] = image
        out[f"{tag}_params"] = np.array([sigma, min_size], dtype=np.float64)
        out[f"{tag}_scales"] = np.array(scales, dtype=np.float64)
        out[f"{tag}_weights"] = weights
        out[f"{tag}_smoothed"] = sm
        out[f"{tag}_labels"] = labels.astype(np.int16)
        print(tag, image.shape, "segments per scale:", (labels.reshape(len(scales), -1).max(1) + 1).tolist())
    _, _, labels = one_case(smoothed(*BIG), 0.8, 150, XRAI_SCALES)
    out["big_labels"] = labels.astype(np.int16)
    out["big_scales"] = np.array(XRAI_SCALES, dtype=np.float64)
    print("big segments per scale:", (labels.reshape(6, -1).max(1) + 1).tolist())
    path = os.path.join(HERE, "felzenszwalb.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
