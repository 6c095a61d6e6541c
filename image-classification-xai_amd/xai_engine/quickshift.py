"""Quickshift superpixels on the HIP kernels K53 - K55 (include/xai_hip_ext5.h), defined by scikit-image 0.18.3
(skimage/segmentation/_quickshift.py and _quickshift_cy.pyx): fp64, in skimage's operation order.

What stays on the host, in NumPy fp64, is what skimage does once per image before its pixel loops: the Lab features
(`quickshift_features`, a restatement of skimage.color.rgb2lab) and the tie noise (`tie_noise`, the one RandomState draw).  The
pixel loops are the kernels: K53 the densities, K54 the nearest denser neighbour, K55 the roots and their numbering.
`quickshift_batch` runs them on device tensors of B images; `quickshift` has skimage's signature and returns a host array.

Parity ("Device quickshift"): given the same features and noise every distance, comparison, parent and label is skimage's
bit for bit; the densities differ by the device's `exp` (within 2 ulp per term) and so are bounded, and a segmentation equals
skimage's whenever no two compared densities are closer than that bound (tests/golden/quickshift.npz states the condition).
"""
import numpy as np
import torch

from . import kernels as K
from .ig import hip_device

# skimage/color/colorconv.py: xyz_from_rgb and the D65 / 2 degree white point (get_xyz_coords("D65", "2"))
XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423],
                         [0.212671, 0.715160, 0.072169],
                         [0.019334, 0.119193, 0.950227]])
D65_WHITE = np.array([0.95047, 1., 1.08883])
TIE_NOISE_SCALE = 0.00001          # _quickshift_cy.pyx: random_state.normal(scale=0.00001, size=(height, width))
TIE_NOISE_KINDS = ("RandomState", "generator")


def _as_float64(image):
    """skimage.util.img_as_float for what this engine serves: a floating image as it is (in fp64), uint8 divided by 255."""
    image = np.asarray(image)
    if image.dtype.kind == "f":
        return image.astype(np.float64)
    if image.dtype == np.uint8:
        return image.astype(np.float64) / 255.0
    raise TypeError(f"quickshift: the image must be floating point or uint8, got {image.dtype}")


def rgb2lab(rgb):
    """skimage.color.rgb2lab (colorconv.py: rgb2xyz, xyz2lab with D65 / 2 degrees) in its own sequence of NumPy operations.
    rgb: (..., 3) fp64 in [0, 1] -> (..., 3) fp64."""
    arr = np.array(rgb, dtype=np.float64)
    if arr.shape[-1] != 3:
        raise ValueError(f"Input array must have a shape == (..., 3)), got {arr.shape}")
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    arr = arr @ XYZ_FROM_RGB.T
    arr = arr / D65_WHITE
    mask = arr > 0.008856
    arr[mask] = np.cbrt(arr[mask])
    arr[~mask] = 7.787 * arr[~mask] + 16. / 116.
    x, y, z = arr[..., 0], arr[..., 1], arr[..., 2]
    L = (116. * y) - 16.
    a = 500.0 * (x - y)
    b = 200.0 * (y - z)
    return np.concatenate([v[..., np.newaxis] for v in [L, a, b]], axis=-1)


def quickshift_features(image, ratio, convert2lab=True):
    """_quickshift.py:59-69 without the smoothing: img_as_float(np.atleast_3d(image)), rgb2lab, `* ratio`, C-contiguous
    (H, W, C) fp64 on the host."""
    image = _as_float64(np.atleast_3d(image))
    if image.ndim != 3:
        raise ValueError(f"quickshift: the image must be (H, W) or (H, W, C), got {image.shape}")
    if convert2lab:
        image = rgb2lab(image)
    return np.ascontiguousarray(image * ratio)


def tie_noise(seed, H, W, kind="RandomState"):
    """The (H, W) fp64 tie-breaking noise.  "RandomState": np.random.RandomState(seed).normal(scale=0.00001, size=(H, W)), what
    skimage 0.18.3 draws.  "generator": np.random.default_rng(seed).normal(...), what later releases are believed to draw."""
    if kind == "RandomState":
        return np.random.RandomState(seed).normal(scale=TIE_NOISE_SCALE, size=(H, W))
    if kind == "generator":
        return np.random.default_rng(seed).normal(scale=TIE_NOISE_SCALE, size=(H, W))
    raise ValueError(f"tie_noise: kind must be one of {TIE_NOISE_KINDS}, got {kind!r}")


_draw_tie_noise = tie_noise         # `quickshift` has an argument of that name


def quickshift_batch(features_dev, noise_dev, kernel_size, max_dist, return_tree=False):
    """features_dev (B, H, W, C) fp64 and noise_dev (B, H, W) fp64 on a HIP device -> (labels (B, H, W) int32, D (B,) int32), both
    on the device; with `return_tree` also (parent (B, H, W) int32, dist (B, H, W) fp64) as skimage's return_tree gives them: the
    parent BEFORE the max_dist cut and sqrt(closest), sqrt(DBL_MAX) at a pixel without a denser neighbour.  Three entries, five
    launches, no read-back."""
    dens = K.quickshift_density(features_dev, noise_dev, kernel_size)
    parent, _, dist, tree = K.quickshift_parent(features_dev, dens, kernel_size, max_dist, want_tree=return_tree)
    labels, D = K.quickshift_labels(parent)
    return (labels, D, tree, dist) if return_tree else (labels, D)


def quickshift(image, ratio=1.0, kernel_size=5, max_dist=10, return_tree=False, sigma=0, convert2lab=True, random_seed=42,
               tie_noise="RandomState", device="cuda"):
    """skimage.segmentation.quickshift's signature (0.18.3) -> the (H, W) int64 label array on the host; with `return_tree`
    (labels, parent (H, W) int64, dist (H, W) fp64).  `sigma` must be 0: the reference never smooths.  Two arguments skimage does
    not have: `tie_noise`, the kind of draw (`tie_noise()` above), and `device`."""
    if sigma != 0:
        raise NotImplementedError("quickshift: sigma != 0 (Gaussian smoothing before the segmentation) is not served; the reference "
                                  "never smooths")
    if tie_noise not in TIE_NOISE_KINDS:
        raise ValueError(f"quickshift: tie_noise must be one of {TIE_NOISE_KINDS}, got {tie_noise!r}")
    if kernel_size < 1:
        raise ValueError("`kernel_size` should be >= 1.")
    feats = quickshift_features(image, ratio, convert2lab)
    H, W = feats.shape[:2]
    dev = hip_device(device)
    noise = _draw_tie_noise(random_seed, H, W, tie_noise)
    out = quickshift_batch(torch.from_numpy(feats)[None].to(dev), torch.from_numpy(noise)[None].to(dev), kernel_size, max_dist, return_tree)
    labels = out[0][0].cpu().numpy().astype(np.int64)
    if return_tree:
        return labels, out[2][0].cpu().numpy().astype(np.int64), out[3][0].cpu().numpy()
    return labels
