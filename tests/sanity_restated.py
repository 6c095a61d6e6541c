"""The yardstick of the sanity-test kernels (K39-K43), on NumPy and scipy alone.

  normalize_image   evaluateSanity.py:68-79 (guard=True) and util/test_methods/sanityForMethods.py:60-72 (guard=False), verbatim
  ssim              skimage.metrics.structural_similarity(gaussian_weights=True, data_range=R) on one fp32 channel, restated on
                    scipy.ndimage.gaussian_filter itself: the filter is scipy's own, only skimage's arithmetic around it is rewritten
  spearman          scipy.stats.spearmanr itself
  hog               skimage.feature.hog(orientations=9, pixels_per_cell=cell, cells_per_block=(3, 3), block_norm='L2-Hys') on one
                    channel, restated in NumPy from its documented algorithm (include/xai_hip_ext2.h, K43)
  get_sanity        evaluateSanity.py:82-106 on the three above
"""
import warnings
from collections import Counter

import numpy as np
from scipy.ndimage import gaussian_filter
from scipy.stats import spearmanr

F32 = np.float32


def normalize_image(x, guard=True):
    x = np.array(x).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        if guard and (x.max() - x.min()) == 0:
            return x
        x[x == float("Inf")] = 0
        x[x == float("-Inf")] = 0
        return (x - x.min()) / (x.max() - x.min())


def ssim(im1, im2, data_range=2.0):
    """-> (mean SSIM as fp64, the full fp32 S map) of two (H, W) fp32 images; ValueError below 11 x 11 like skimage"""
    im1, im2 = np.asarray(im1), np.asarray(im2)
    assert im1.dtype == F32 and im2.dtype == F32 and im1.ndim == 2 and im1.shape == im2.shape
    win_size = 11                                           # r = int(3.5 * 1.5 + 0.5); 2 r + 1
    if min(im1.shape) < win_size:
        raise ValueError("win_size exceeds image extent")
    filt = lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")          # noqa: E731
    NP = win_size ** 2
    cov_norm = F32(NP / (NP - 1))                           # a Python float next to fp32 arrays: fp32 under NumPy 2
    C1, C2 = F32((0.01 * data_range) ** 2), F32((0.03 * data_range) ** 2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ux, uy = filt(im1), filt(im2)
        uxx, uyy, uxy = filt(im1 * im1), filt(im2 * im2), filt(im1 * im2)
        vx = cov_norm * (uxx - ux * ux)
        vy = cov_norm * (uyy - uy * uy)
        vxy = cov_norm * (uxy - ux * uy)
        A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
        S = (A1 * A2) / (B1 * B2)
    assert S.dtype == F32
    pad = (win_size - 1) // 2
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64), S


def spearman(a, b):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(spearmanr(np.asarray(a).ravel(), np.asarray(b).ravel())[0])


def hog_gradients(img):
    """-> (magnitude, orientation in [0, 180]) fp64 per pixel"""
    img = np.asarray(img)
    assert img.dtype == F32 and img.ndim == 2
    g_row = np.zeros(img.shape, F32)
    g_col = np.zeros(img.shape, F32)
    with np.errstate(invalid="ignore"):
        g_row[1:-1, :] = img[2:, :] - img[:-2, :]
        g_col[:, 1:-1] = img[:, 2:] - img[:, :-2]
        g_row, g_col = g_row.astype(np.float64), g_col.astype(np.float64)
        return np.hypot(g_col, g_row), np.rad2deg(np.arctan2(g_row, g_col)) % 180


def hog_length(H, W, cell=(16, 16)):
    return (H // cell[0] - 2) * (W // cell[1] - 2) * 81


def hog(img, cell=(16, 16)):
    """-> fp32 features, flattened [H // ch - 2][W // cw - 2][3][3][9]; ValueError with fewer than 3 cells on an axis"""
    H, W = np.asarray(img).shape
    ch, cw = cell
    n_r, n_c = H // ch, W // cw
    if n_r < 3 or n_c < 3:
        raise ValueError("fewer than 3 cells on an axis")
    mag, ori = hog_gradients(img)
    hist = np.zeros((n_r, n_c, 9), np.float64)
    for r in range(n_r):
        for c in range(n_c):
            m = mag[r * ch:(r + 1) * ch, c * cw:(c + 1) * cw].ravel()
            o = ori[r * ch:(r + 1) * ch, c * cw:(c + 1) * cw].ravel()
            for i in range(9):
                with np.errstate(invalid="ignore"):
                    inside = (o >= 20.0 * i) & (o < 20.0 * (i + 1))
                hist[r, c, i] = np.cumsum(np.where(inside, m, 0.0))[-1] / (ch * cw)      # a row-major chain
    out = np.zeros((n_r - 2, n_c - 2, 3, 3, 9), F32)
    eps = 1e-5
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(n_r - 2):
            for c in range(n_c - 2):
                b = hist[r:r + 3, c:c + 3, :]
                v = b / np.sqrt(np.sum(b ** 2) + eps ** 2)
                v = np.minimum(v, 0.2)
                out[r, c] = v / np.sqrt(np.sum(v ** 2) + eps ** 2)
    return out.ravel()


def get_sanity(normal_attr, random_layer_attr, data_range=2.0, guard=True, cell=(16, 16)):
    """evaluateSanity.py:82-106 for one-channel maps given as (H, W) or (H, W, 1)"""
    a = np.asarray(normal_attr).reshape(np.asarray(normal_attr).shape[:2])
    b = np.asarray(random_layer_attr).reshape(a.shape)
    an, bn = normalize_image(a, guard), normalize_image(b, guard)
    return Counter({"SSIM": ssim(an, bn, data_range)[0], "SPR": spearman(a, b), "HOG": spearman(hog(an, cell), hog(bn, cell))})
