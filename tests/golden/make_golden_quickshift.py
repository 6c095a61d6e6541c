"""Regenerate tests/golden/quickshift.npz from scikit-image's own quickshift.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quickshift.py        (an interpreter that has scikit-image)

The stored fixture was made with scikit-image 0.18.3, the release whose algorithm K53-K55 restate (`version` in the file).
skimage.segmentation.quickshift(image, ..., return_tree=True) and skimage.color.rgb2lab run unmodified on the host.

Cases (`names`), per case <tag>:
  <tag>_image     (H, W, 3) float32 in [0, 1]; skimage is fed its exact fp64 conversion
  <tag>_params    [ratio, kernel_size, max_dist, random_seed]
  <tag>_features  skimage.color.rgb2lab(image) * ratio, fp64
  <tag>_labels, <tag>_parent (int32), <tag>_dist (fp64): skimage's three return values; parent is the tree BEFORE the max_dist cut,
                  dist is sqrt(DBL_MAX) at a pixel without a denser neighbour (0.18.3 starts `closest` at DBL_MAX)
  <tag>_margin    [bound, gap] of tests/quickshift_restated.margin on the restatement's densities
    lime   LIME's arguments (kernel_size 4, max_dist 200, ratio 0.2) on a smoothed random image, 56 x 64; at least 4 segments
    cut    kernel_size 2, max_dist 4, ratio 0.5 at 24 x 27: the cut binds for some pixels
    roots  kernel_size 1, max_dist 3, ratio 1 at 17 x 20 on an unsmoothed random image: every pixel is a root (340 segments)
The generator asserts for every case: gap >= 100 * bound (the decision margin: no comparison of two densities can be turned by one
differing `exp` per term), the restatement equals skimage (labels and parent exactly, dist bit for bit), the cut binds where stated.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import quickshift_restated as R  # noqa: E402

try:
    import skimage
    from skimage.color import rgb2lab
    from skimage.segmentation import quickshift
except ImportError:
    sys.exit("make_golden_quickshift.py: needs scikit-image (the fixture was made with 0.18.3)")


def smoothed(seed, H, W, passes):
    """A random (H, W, 3) image in [0, 1], `passes` times 3 x 3 box-filtered (edges replicated), stretched to the full range and
    rounded to float32"""
    img = np.random.RandomState(seed).uniform(size=(H, W, 3))
    for _ in range(passes):
        p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
        img = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    img = (img - img.min()) / (img.max() - img.min())
    return img.astype(np.float32)


CASES = [  # tag, image, ratio, kernel_size, max_dist, seed
    ("lime", smoothed(3, 56, 64, 1), 0.2, 4, 200, 531),
    ("cut", smoothed(4, 24, 27, 3), 0.5, 2, 4, 42),
    ("roots", smoothed(8, 17, 20, 0), 1.0, 1, 3, 7),
]


def main():
    out = {"version": np.array(skimage.__version__), "names": np.array([c[0] for c in CASES])}
    for tag, image, ratio, ks, md, seed in CASES:
        img64 = image.astype(np.float64)
        feats = np.ascontiguousarray(rgb2lab(img64) * ratio)
        labels, parent, dist = quickshift(img64, ratio=ratio, kernel_size=ks, max_dist=md, return_tree=True, random_seed=seed)
        labels, parent, dist = np.asarray(labels), np.asarray(parent), np.asarray(dist)
        D = int(labels.max()) + 1
        noise = np.random.RandomState(seed).normal(scale=0.00001, size=image.shape[:2])
        r = R.quickshift_from(feats, noise, ks, md)
        bound, gap = R.margin(feats, r["dens"], ks)
        cut = int(((dist > md) & (dist < np.sqrt(R.DBL_MAX))).sum())       # parents removed by max_dist, the pixels without one aside
        print(f"{tag}: {image.shape[:2]} D={D} cut={cut} bound={bound:.3e} gap={gap:.3e} "
              f"|features - restated|={np.abs(feats - R.features(img64, ratio)).max():.2e}")
        assert gap >= 100 * bound, (tag, gap, bound)
        assert (r["labels"] == labels).all() and r["D"] == D and (r["tree"] == parent).all(), tag
        assert r["dist"].tobytes() == dist.tobytes(), tag
        if tag == "lime":
            assert D >= 4, D
        if tag == "cut":
            assert 0 < cut < labels.size - D, (cut, D)                         # some parents are cut, some are kept
        if tag == "roots":
            assert D == labels.size
        out.update({f"{tag}_image": image, f"{tag}_params": np.array([ratio, ks, md, seed], np.float64), f"{tag}_features": feats,
                    f"{tag}_labels": labels.astype(np.int32), f"{tag}_parent": parent.astype(np.int32), f"{tag}_dist": dist,
                    f"{tag}_margin": np.array([bound, gap])})
    np.savez_compressed(os.path.join(HERE, "quickshift.npz"), **out)


if __name__ == "__main__":
    main()
