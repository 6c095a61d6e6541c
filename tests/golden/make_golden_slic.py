"""Regenerate tests/golden/slic.npz from scikit-image's own SLIC.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_slic.py        (an interpreter that has scikit-image)

The stored fixture was made with scikit-image 0.18.3, the release whose algorithm K65-K68 restate (`version` in the file).
skimage.segmentation.slic, skimage.color.rgb2lab and the two Cython functions of skimage.segmentation._slic run unmodified on the host.

Cases (`names`), each in float32 and float64 (`<tag>_f32_*`, `<tag>_f64_*`; the float64 run is fed the exact conversion of the image):
  <tag>_image             (H, W, 3) float32 in [0, 1]
  <tag>_params            [n_segments, compactness]
  <tag>_centroids, _step  _get_grid_centroids: (S, 2) int32 of (y, x), and max(steps)
  <tag>_sizes             [min_size, max_size] of the connectivity pass
  <tag>_<T>_features      skimage's `rgb2lab(image) * (1 / compactness)` in T
  <tag>_<T>_raw           slic(..., enforce_connectivity=False), int16
  <tag>_<T>_labels        slic(...), int16
  <tag>_<T>_centres       (S, 2 + C) T: `segments` after a direct `_slic_cython(features, None, segments, step, 10, ...)`, the z column
                          dropped: the centres after the tenth update
  <tag>_<T>_regular       whether every component of the raw labels has min_size <= size < max_size
    mda     112 x 112, 49 segments, compactness 10000: step 16, MDA's geometry at a quarter of the size
    ragged  57 x 43, 25 segments, compactness 10000: S = 24, no dimension a multiple of a tile or of 64
    colour  40 x 56, 12 segments, compactness 0.5: the colour term decides
    wide    33 x 47, 20 segments, compactness 0.02
    one     24 x 24, 1 segment, compactness 10: a single cluster whose window is the image
  conn<i>_raw, conn<i>_labels, conn<i>_sizes   irregular inputs of the connectivity pass alone (CONN below: float32 runs of smooth
              images at a low compactness; 8, 11 and 27 final labels), int16: the raw labels, skimage's final labels, [min_size, max_size]
  big_labels  slic(image, 196, 10000, start_label=0) of smoothed(BIG_SEED, 224, 224, 2) in float32, int16: the image is regenerated
  small_labels  the same for smoothed(SMALL_SEED, 32, 32, 1) with 16 segments (the tiny ViT of tests/test_gpu_mda.py): 16 labels
The generator asserts for every case that the restatement (tests/slic_restated.py) equals skimage: the raw labels and the labels
exactly and the centres bit for bit; the regular rule where the case is regular, and, where xai_engine is importable, the sequential
host pass (xai_engine.slic_host.enforce_connectivity_host) on every case and on the `conn` cases.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import slic_restated as R  # noqa: E402

try:
    import skimage
    from skimage.color import rgb2lab
    from skimage.segmentation import slic
    from skimage.segmentation import slic_superpixels as SP
    from skimage.segmentation._slic import _enforce_label_connectivity_cython, _slic_cython
except ImportError:
    sys.exit("make_golden_slic.py: needs scikit-image (the fixture was made with 0.18.3)")

try:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "image-classification-xai_amd"))
    from xai_engine.slic_host import enforce_connectivity_host
except ImportError:
    enforce_connectivity_host = None

warnings.filterwarnings("ignore")
BIG_SEED = 3
SMALL_SEED = 12
CONN = [(5, 96, 80, 12, 30, 5.0), (7, 64, 48, 10, 20, 10.0), (4, 60, 72, 12, 30, 20.0)]      # seed, H, W, passes, n_segments, compactness


def smoothed(seed, H, W, passes):
    """A random (H, W, 3) image in [0, 1], `passes` times 3 x 3 box-filtered (edges replicated), stretched to the full range and
    rounded to float32"""
    img = np.random.RandomState(seed).uniform(size=(H, W, 3))
    for _ in range(passes):
        p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
        img = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    img = (img - img.min()) / (img.max() - img.min())
    return img.astype(np.float32)


CASES = [  # tag, image, n_segments, compactness
    ("mda", smoothed(11, 112, 112, 2), 49, 10000.0),
    ("ragged", smoothed(8, 57, 43, 1), 25, 10000.0),
    ("colour", smoothed(1, 40, 56, 1), 12, 0.5),
    ("wide", smoothed(5, 33, 47, 1), 20, 0.02),
    ("one", smoothed(6, 24, 24, 1), 1, 10.0),
]


def main():
    out = {"version": np.array(skimage.__version__), "names": np.array([c[0] for c in CASES]), "big_seed": np.array(BIG_SEED)}
    for tag, image, n, comp in CASES:
        H, W = image.shape[:2]
        out[f"{tag}_image"] = image
        out[f"{tag}_params"] = np.array([n, comp], np.float64)
        for T, name in ((np.float32, "f32"), (np.float64, "f64")):
            img = image.astype(T)
            lab = rgb2lab(img[None])
            assert lab.dtype == T
            cent, steps = SP._get_grid_centroids(lab, n)
            step = max(steps)
            S = cent.shape[0]
            feat = np.ascontiguousarray(lab * (1.0 / comp), dtype=T)
            segs = np.ascontiguousarray(np.concatenate([cent, np.zeros((S, 3))], axis=-1), dtype=T)
            raw = slic(img, n_segments=n, compactness=comp, start_label=0, enforce_connectivity=False)
            labels = slic(img, n_segments=n, compactness=comp, start_label=0)
            direct = np.asarray(_slic_cython(feat, None, segs, step, 10, np.ones(3, dtype=T), False, ignore_color=False, start_label=0))[0]
            assert (direct == raw).all(), tag
            centres = np.ascontiguousarray(segs[:, 1:])
            mn, mx = int(0.5 * H * W / S), int(3 * H * W / S)
            conn = np.asarray(_enforce_label_connectivity_cython(np.ascontiguousarray(raw[None], dtype=np.intp), mn, mx, start_label=0))[0]
            assert (conn == labels).all(), tag
            # the restatement
            got_raw, trace, status = R.kmeans(feat[0], R.initial(cent[:, 1:], 3, T), step, 10)
            assert status == 0 and (got_raw == raw).all(), (tag, name, status)
            assert trace[-1].tobytes() == centres.tobytes(), (tag, name)
            compo, st, sweeps = R.components(got_raw, mn, mx)
            regular = st == 0
            if regular:
                got, count = R.number(compo, 0)
                assert (got == labels).all() and count == len(np.unique(labels)), (tag, name)
            if enforce_connectivity_host is not None:
                for start in (0, 1):
                    want = np.asarray(_enforce_label_connectivity_cython(np.ascontiguousarray(raw[None] + start, dtype=np.intp), mn, mx,
                                                                         start_label=start))[0]
                    assert (enforce_connectivity_host(raw + start, mn, mx, start) == want).all(), (tag, name, start)
            print(f"{tag} {name}: {H}x{W} S={S} step={step} sizes=({mn}, {mx}) raw labels={len(np.unique(raw))} "
                  f"final={len(np.unique(labels))} regular={regular} sweeps={sweeps} host pass checked={enforce_connectivity_host is not None}")
            if T is np.float32:
                out[f"{tag}_centroids"] = cent[:, 1:].astype(np.int32)
                out[f"{tag}_step"] = np.array(step, np.float64)
                out[f"{tag}_sizes"] = np.array([mn, mx], np.int32)
            out.update({f"{tag}_{name}_features": feat[0], f"{tag}_{name}_raw": raw.astype(np.int16),
                        f"{tag}_{name}_labels": labels.astype(np.int16), f"{tag}_{name}_centres": centres,
                        f"{tag}_{name}_regular": np.array(regular)})
    for i, (seed, H, W, passes, n, comp) in enumerate(CONN):
        img = smoothed(seed, H, W, passes)
        raw = slic(img, n_segments=n, compactness=comp, start_label=0, enforce_connectivity=False)
        S = SP._get_grid_centroids(img[None], n)[0].shape[0]
        mn, mx = int(0.5 * H * W / S), int(3 * H * W / S)
        for start in (0, 1):
            labels = slic(img, n_segments=n, compactness=comp, start_label=start)
            if enforce_connectivity_host is not None:
                assert (enforce_connectivity_host(raw + start, mn, mx, start) == labels).all(), (i, start)
        labels = slic(img, n_segments=n, compactness=comp, start_label=0)
        _, st, _ = R.components(raw.astype(np.int32), mn, mx)
        print(f"conn{i}: {H}x{W} raw labels={len(np.unique(raw))} final={len(np.unique(labels))} irregular={st != 0}")
        assert st == R.IRREGULAR and len(np.unique(labels)) > 1, i
        out.update({f"conn{i}_raw": raw.astype(np.int16), f"conn{i}_labels": labels.astype(np.int16),
                    f"conn{i}_sizes": np.array([mn, mx], np.int32)})
    out["conn_count"] = np.array(len(CONN))
    big = smoothed(BIG_SEED, 224, 224, 2)
    big_labels = slic(big, n_segments=196, compactness=10000, start_label=0)
    assert len(np.unique(big_labels)) == 196
    out["big_labels"] = big_labels.astype(np.int16)
    small_labels = slic(smoothed(SMALL_SEED, 32, 32, 1), n_segments=16, compactness=10000, start_label=0)
    assert len(np.unique(small_labels)) == 16
    out["small_labels"], out["small_seed"] = small_labels.astype(np.int16), np.array(SMALL_SEED)
    np.savez_compressed(os.path.join(HERE, "slic.npz"), **out)
    print("slic.npz:", os.path.getsize(os.path.join(HERE, "slic.npz")), "bytes")


if __name__ == "__main__":
    main()
