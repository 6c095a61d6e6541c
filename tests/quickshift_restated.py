"""Plain NumPy fp64 restatement of quickshift as scikit-image 0.18.3 computes it (skimage/segmentation/_quickshift.py and
_quickshift_cy.pyx), the arithmetic K53-K55 (include/xai_hip_ext5.h) are held to.

skimage walks pixel after pixel and, per pixel, the clipped window with r_ ascending and then c_ ascending.  Here the loop runs over
the window OFFSETS (dr ascending, then dc ascending) and every step is vectorised over the pixels for which that offset lies inside
the image, so each pixel still accumulates its terms in exactly skimage's sequential order.

  - d = the channel terms from +0 in ascending order, then (r - r_)^2, then (c - c_)^2; every product and sum rounded once
  - density = the terms exp(d * inv) added in scan order from +0, then + noise
  - parent = the first neighbour in scan order with the strictly smallest d among the strictly denser ones
  - the cut, skimage's own `while (old != parent).any(): parent = parent[parent]` and np.unique(..., return_inverse=True)[1]

np.exp and the C library's exp (and the device's) may differ in the last place; tests/golden/quickshift.npz states per case the bound
on what that does to a density and that every compared pair of densities is 100 bounds apart.
"""
import math

import numpy as np

# skimage/color/colorconv.py
XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
D65_WHITE = np.array([0.95047, 1., 1.08883])
DBL_MAX = float(np.finfo(np.float64).max)      # _quickshift_cy.pyx: closest = DBL_MAX, so a pixel without a denser neighbour has dist sqrt(DBL_MAX)


def rgb2lab(rgb):
    """skimage.color.rgb2lab, operation for operation (rgb2xyz, then xyz2lab with the D65 / 2 degree white point)"""
    arr = np.array(rgb, dtype=np.float64)
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    arr = arr @ XYZ_FROM_RGB.T
    arr = arr / D65_WHITE
    mask = arr > 0.008856
    arr[mask] = np.cbrt(arr[mask])
    arr[~mask] = 7.787 * arr[~mask] + 16. / 116.
    x, y, z = arr[..., 0], arr[..., 1], arr[..., 2]
    return np.stack([(116. * y) - 16., 500.0 * (x - y), 200.0 * (y - z)], axis=-1)


def features(image, ratio, convert2lab=True):
    image = np.atleast_3d(np.asarray(image, dtype=np.float64))
    return np.ascontiguousarray((rgb2lab(image) if convert2lab else image) * ratio)


def kernel_width(kernel_size):
    return int(math.ceil(3 * kernel_size))


def _offsets(f, kw):
    """Yields, in scan order, (dr, dc, own, other, d): the slices of the pixels whose neighbour at that offset is inside the image,
    the slices of those neighbours, and the squared distances d between them."""
    H, W, C = f.shape
    for dr in range(-kw, kw + 1):
        r0, r1 = max(0, -dr), min(H, H - dr)
        if r0 >= r1:
            continue
        for dc in range(-kw, kw + 1):
            c0, c1 = max(0, -dc), min(W, W - dc)
            if c0 >= c1:
                continue
            own = (slice(r0, r1), slice(c0, c1))
            other = (slice(r0 + dr, r1 + dr), slice(c0 + dc, c1 + dc))
            d = np.zeros((r1 - r0, c1 - c0))
            for ch in range(C):
                t = f[own + (ch,)] - f[other + (ch,)]
                d = d + t * t
            t = float(-dr)                    # r - r_
            d = d + t * t
            t = float(-dc)                    # c - c_
            d = d + t * t
            yield dr, dc, own, other, d


def density(f, noise, kernel_size):
    """K53: (H, W, C) features, (H, W) noise -> (H, W) densities"""
    inv = -0.5 / (kernel_size * kernel_size)
    dens = np.zeros(f.shape[:2])
    with np.errstate(invalid="ignore"):
        for _, _, own, _, d in _offsets(f, kernel_width(kernel_size)):
            dens[own] += np.exp(d * inv)
    return dens + noise


def parents(f, dens, kernel_size, max_dist):
    """K54: -> (parent with the cut, tree = the parent before the cut, closest, dist), flat pixel indices as (H, W) arrays"""
    H, W = dens.shape
    idx = np.arange(H * W).reshape(H, W)
    tree = idx.copy()
    closest = np.full((H, W), DBL_MAX)
    with np.errstate(invalid="ignore"):
        for _, _, own, other, d in _offsets(f, kernel_width(kernel_size)):
            better = (dens[other] > dens[own]) & (d < closest[own])
            closest[own] = np.where(better, d, closest[own])
            tree[own] = np.where(better, idx[other], tree[own])
        dist = np.sqrt(closest)
        too_far = dist > max_dist
    parent = np.where(too_far, idx, tree)
    return parent, tree, closest, dist


def labels_of(parent):
    """K55: skimage's own flattening loop and numbering -> ((H, W) labels, D)"""
    flat = np.asarray(parent).ravel().copy()
    old = np.zeros_like(flat)
    while (old != flat).any():
        old = flat
        flat = flat[flat]
    ids, inverse = np.unique(flat, return_inverse=True)
    return inverse.reshape(np.shape(parent)), int(ids.shape[0])


def quickshift_from(f, noise, kernel_size, max_dist):
    """Steps 3-5 on given features and noise -> dict(dens, parent, tree, closest, dist, labels, D)"""
    dens = density(f, noise, kernel_size)
    parent, tree, closest, dist = parents(f, dens, kernel_size, max_dist)
    labels, D = labels_of(parent)
    return dict(dens=dens, parent=parent, tree=tree, closest=closest, dist=dist, labels=labels, D=D)


def quickshift(image, ratio=1.0, kernel_size=5, max_dist=10, convert2lab=True, random_seed=42):
    """skimage.segmentation.quickshift(..., sigma=0) -> the dict of `quickshift_from`"""
    f = features(image, ratio, convert2lab)
    noise = np.random.RandomState(random_seed).normal(scale=0.00001, size=f.shape[:2])
    return quickshift_from(f, noise, kernel_size, max_dist)


def ulp(x):
    return float(np.spacing(np.abs(x)))


def margin(f, dens, kernel_size):
    """The decision margin of a case -> (bound, gap).
    bound = n_terms * (2^-52 + ulp(max density)): every one of the at most n_terms = (2 kw + 1)^2 accumulation steps can differ by
    one differing exp (<= 2 ulp of a value <= 1, i.e. <= 2^-52) plus one rounding of the running sum.
    gap = the smallest |dens[p] - dens[q]| over the pairs the parent pass compares (q in the window of p, q != p)."""
    kw = kernel_width(kernel_size)
    finite = dens[np.isfinite(dens)]
    bound = (2 * kw + 1) ** 2 * (2.0 ** -52 + ulp(finite.max()))
    gap = np.inf
    H, W = dens.shape
    for dr in range(-kw, kw + 1):
        r0, r1 = max(0, -dr), min(H, H - dr)
        for dc in range(-kw, kw + 1):
            c0, c1 = max(0, -dc), min(W, W - dc)
            if (dr, dc) == (0, 0) or r0 >= r1 or c0 >= c1:
                continue
            diff = np.abs(dens[r0:r1, c0:c1] - dens[r0 + dr:r1 + dr, c0 + dc:c1 + dc])
            diff = diff[np.isfinite(diff)]
            if diff.size:
                gap = min(gap, float(diff.min()))
    return bound, gap
