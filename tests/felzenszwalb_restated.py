"""scikit-image 0.18.3's Felzenszwalb segmentation (_felzenszwalb_cy.pyx with scipy.ndimage.gaussian_filter) restated in NumPy, step
by step, as include/xai_hip_felz.h states it: fp64, every operation rounded once, equal costs ordered by edge index.  The tests hold
the kernels to this file and this file to skimage's binary (tests/golden/felzenszwalb.npz, made by make_golden_felzenszwalb.py).
Not a test module: it is imported by tests/test_cpu_felzenszwalb.py, tests/test_gpu_felzenszwalb.py and the fixture's generator."""
import collections

import numpy as np

Restated = collections.namedtuple("Restated", "smoothed costs order labels counts tested merged")


def as_float64(image):
    """np.atleast_3d, then img_as_float64 of a float or uint8 image"""
    image = np.atleast_3d(np.asarray(image))
    if image.dtype == np.uint8:
        return image.astype(np.float64) / 255.0
    return image.astype(np.float64)


def weights_of(sigma):
    """_gaussian_kernel1d of order 0; None for a skipped axis"""
    if not sigma > 1e-15:
        return None
    r = int(4.0 * sigma + 0.5)
    w = np.exp(-0.5 / (sigma * sigma) * np.arange(-r, r + 1) ** 2)
    return w / w.sum()


def reflect(idx, n):
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def smooth_axis(x, w, axis):
    """correlate1d's symmetric branch along `axis` with mode reflect: t = x[l] w[r]; t += (x[l + ll] + x[l - ll]) w[ll + r]"""
    r = len(w) // 2
    n = x.shape[axis]
    l = np.arange(n)
    t = np.take(x, l, axis=axis) * w[r]
    for ll in range(-r, 0):
        t = t + (np.take(x, reflect(l + ll, n), axis=axis) + np.take(x, reflect(l - ll, n), axis=axis)) * w[ll + r]
    return t


def smooth(image, w):
    if w is None:
        return image
    return smooth_axis(smooth_axis(image, w, 0), w, 1)


def edge_pixels(H, W):
    """(a, b) flat pixel indices of every edge: right, down, down-right, up-right, each in raster order"""
    idx = np.arange(H * W).reshape(H, W)
    a = [idx[:, :-1], idx[:-1, :], idx[:-1, :-1], idx[:-1, 1:]]
    b = [idx[:, 1:], idx[1:, :], idx[1:, 1:], idx[1:, :-1]]
    return np.concatenate([v.ravel() for v in a]), np.concatenate([v.ravel() for v in b])


def edge_costs(image, a, b):
    flat = image.reshape(-1, image.shape[2])
    total = np.zeros(len(a))
    for c in range(image.shape[2]):                  # sequentially over the channels
        d = flat[b, c] - flat[a, c]
        total = total + d * d
    return np.sqrt(total)


def _find(parent, x):
    while parent[x] != x:
        x = parent[x]
    return x


def _find_halving(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def merge(a, b, costs, order, n, scale, min_size):
    """the two walks -> (root of every pixel, edges that reached the test of the thresholds, edges that merged)"""
    parent = list(range(n))
    size = [1] * n
    cint = [0.0] * n
    tested = merged = 0
    ea, eb, ec = a[order].tolist(), b[order].tolist(), costs[order].tolist()
    for p, q, cost in zip(ea, eb, ec):
        ra, rb = _find_halving(parent, p), _find_halving(parent, q)
        if ra == rb:
            continue
        tested += 1
        if cost < min(cint[ra] + scale / size[ra], cint[rb] + scale / size[rb]):
            merged += 1
            lo, hi = min(ra, rb), max(ra, rb)
            parent[hi] = lo
            size[lo] = size[ra] + size[rb]
            cint[lo] = cost
    for p, q in zip(ea, eb):
        ra, rb = _find_halving(parent, p), _find_halving(parent, q)
        if ra == rb:
            continue
        if size[ra] < min_size or size[rb] < min_size:
            lo, hi = min(ra, rb), max(ra, rb)
            parent[hi] = lo
            size[lo] = size[ra] + size[rb]
    return np.array([_find(parent, p) for p in range(n)]), tested, merged


def labels_of(roots):
    """the rank of every pixel's root among the roots in ascending pixel index, and their number"""
    is_root = roots == np.arange(len(roots))
    rank = np.cumsum(is_root) - 1
    return rank[roots], int(is_root.sum())


def felzenszwalb(image, scales, sigma=0.8, min_size=20, weights=None):
    """-> Restated for a sequence of scales: smoothed (H, W, C), costs (E,), order (E,) (stable), labels (S, H, W) int64,
    counts / tested / merged (S,)"""
    image = as_float64(image)
    H, W = image.shape[:2]
    sm = smooth(image, weights_of(sigma) if weights is None else weights)
    a, b = edge_pixels(H, W)
    costs = edge_costs(sm, a, b)
    order = np.argsort(costs, kind="stable")
    labels, counts, tested, merged = [], [], [], []
    for scale in np.atleast_1d(scales):
        roots, t, m = merge(a, b, costs, order, H * W, float(scale) / 255., min_size)
        lab, cnt = labels_of(roots)
        labels.append(lab.reshape(H, W))
        counts.append(cnt)
        tested.append(t)
        merged.append(m)
    return Restated(sm, costs, order, np.stack(labels), np.array(counts), np.array(tested), np.array(merged))
