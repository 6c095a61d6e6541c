"""Felzenszwalb-Huttenlocher segmentation on the HIP kernels K69 - K74 (include/xai_hip_felz.h), defined by scikit-image 0.18.3
(skimage/segmentation/_felzenszwalb_cy.pyx, with scipy.ndimage.gaussian_filter for its smoothing): fp64, in skimage's operation order.

What stays on the host, in NumPy, is what depends on no pixel: the Gaussian weights (`gaussian_weights`) and `scale / 255`.  The
pixel work is the kernels: K69 the smoothing (one launch per axis), K70 the edge costs, K71 / K72 their stable order, K73 the merge
and minimum-size walks (one wave per image and scale: the smoothing, the costs and the order are shared by every scale of a call),
K74 the labels.  `felzenszwalb_batch` runs them on B images with no read-back but the status word; `felzenszwalb` has skimage's
signature and returns a host array.  Neither needs scikit-image or SciPy.

Parity: given the weights, the smoothed image and the costs are SciPy's and skimage's bit for bit, and where no two
costs are equal so are the labels.  skimage orders equal costs with NumPy's default, unstable argsort, which pins nothing; the
kernels order them by edge index, and on such inputs they are held to the restatement with that rule (tests/felzenszwalb_restated.py).
NumPy's `exp` differs by an ulp between versions at some sigmas (not at XRAI's 0.8), so `weights=` takes the ones to equal.
"""
import warnings

import numpy as np
import torch

from . import kernels as K
from ._lib import XaiHipError
from .ig import hip_device

NONFINITE, INVARIANT = K.FELZ_NONFINITE, K.FELZ_INVARIANT
_NONFINITE_TEXT = "felzenszwalb: the image has a NaN or an infinite pixel (an edge cost is not finite); NumPy's NaN-last order is not imitated"


def gaussian_weights(sigma):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5)) in its own NumPy operations -> (2 r + 1,) float64;
    None where gaussian_filter skips the axis (sigma <= 1e-15)."""
    sigma = float(sigma)
    if sigma < 0:
        raise ValueError(f"felzenszwalb: sigma must be >= 0, got {sigma}")
    if not sigma > 1e-15:
        return None
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi_x / phi_x.sum()


def _as_float64(image):
    """skimage.util.img_as_float64 for what this engine serves: a float image as float64 (exact), uint8 / 255."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image.astype(np.float64) / 255.0
    if image.dtype in (np.float16, np.float32, np.float64):
        return image.astype(np.float64)
    raise TypeError(f"felzenszwalb: the image must be a float or uint8 array, got {image.dtype}")


def _scales(scales):
    scales = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    if scales.ndim != 1 or scales.size < 1 or not np.all(np.isfinite(scales)):
        raise ValueError(f"felzenszwalb: scales must be finite numbers, one or a 1-d sequence of them, got {scales!r}")
    return np.array([float(s) / 255. for s in scales], dtype=np.float64)


def _min_size(min_size):
    if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 0:
        raise ValueError(f"felzenszwalb: min_size must be an integer >= 0, got {min_size!r}")
    return int(min_size)


def _weights(sigma, weights):
    if weights is None:
        return gaussian_weights(sigma)
    if float(sigma) < 0:
        raise ValueError(f"felzenszwalb: sigma must be >= 0, got {sigma}")
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if weights.ndim != 1 or weights.size % 2 != 1 or not np.array_equal(weights, weights[::-1]):
        raise ValueError("felzenszwalb: weights must be a symmetric 1-d kernel of 2 r + 1 taps")
    return weights


def _stages(images, scales, sigma, min_size, weights):
    """-> (smoothed, keys, order, roots, stats, labels, counts, status): every stage of the device path, for the tests and the
    profile.  images: (B, H, W, C) float64 device tensor."""
    scaled = _scales(scales)
    min_size = _min_size(min_size)
    w = _weights(sigma, weights)
    B, H, W, C = K._felz_image(images, "images")           # the device last: every other refusal needs none
    dev = images.device
    cap = K.felz_limits()
    if scaled.size > cap[2]:
        raise ValueError(f"felzenszwalb: {scaled.size} scales are over THE LIMITS ({cap[2]} per call) (include/xai_hip_felz.h)")
    if w is not None and w.size // 2 > cap[3]:
        raise ValueError(f"felzenszwalb: the kernel radius {w.size // 2} (sigma {sigma}) is over THE LIMITS ({cap[3]}) (include/xai_hip_felz.h)")
    smoothed = images
    if w is not None:
        w_dev = torch.from_numpy(w).to(dev)
        smoothed = K.felz_smooth(K.felz_smooth(images, w_dev, 0), w_dev, 1)
    status = K.felz_clear(torch.empty(1, dtype=torch.int32, device=dev))
    ws = K.felz_workspace(dev, B, H, W, int(scaled.size))
    keys, order, _ = K.felz_costs(smoothed, status)
    K.felz_sort(keys, order, H, W, int(scaled.size), ws)
    roots, stats, _ = K.felz_merge(keys, order, torch.from_numpy(scaled).to(dev), H, W, min_size, status, ws)
    labels, counts, _ = K.felz_labels(roots, status)
    return smoothed, keys, order, roots, stats, labels, counts, status


def raise_for_status(status):
    """The one read-back of a call: the status word -> XaiHipError by name."""
    st = int(status[0])
    if st & NONFINITE:
        raise XaiHipError(_NONFINITE_TEXT)
    if st & INVARIANT:
        raise XaiHipError("felzenszwalb: K73 / K74 met a forest that is none (an edge index outside the image, a parent above its child "
                          "or a root walk over H * W hops): an error of the kernels, never of the input")


def felzenszwalb_batch(images, scales, sigma=0.8, min_size=20, *, weights=None, device=None):
    """images (B, H, W, C) on the host (array: float or uint8, as img_as_float64 reads it) or on a HIP device (float tensor), one
    `scale` or a sequence of S of them -> (labels (B, S, H, W) int32, counts (B, S) int32), on the device.  The smoothing, the costs
    and their order are computed once and shared by the scales.  weights: the symmetric smoothing kernel instead of
    `gaussian_weights(sigma)`.  Nothing is read back but the status word: a non-finite image raises XaiHipError."""
    if isinstance(images, torch.Tensor):
        if not images.is_floating_point():
            raise TypeError(f"felzenszwalb_batch: a device image must be a float tensor, got {images.dtype}")
        dev = images.device if images.is_cuda else hip_device(device or "cuda")
        t = images.to(dev, torch.float64).contiguous()
    else:
        dev = hip_device(device or "cuda")
        t = torch.from_numpy(np.ascontiguousarray(_as_float64(images))).to(dev)
    out = _stages(t, scales, sigma, min_size, weights)
    raise_for_status(out[7])
    return out[5], out[6]


def felzenszwalb(image, scale=1, sigma=0.8, min_size=20, multichannel=True, *, device=None):
    """skimage.segmentation.felzenszwalb's signature and defaults (0.18.3) -> the (H, W) int64 label array on the host.  One argument
    skimage does not have: `device`."""
    image = np.asarray(image)
    if not multichannel and image.ndim > 2:
        raise ValueError("This algorithm works only on single or "
                         "multi-channel 2d images. ")
    image = np.atleast_3d(image)
    if image.ndim != 3:
        raise ValueError(f"felzenszwalb: the image must be (H, W) or (H, W, C), got {image.shape}")
    if image.shape[2] > 3:
        warnings.warn(RuntimeWarning("Got image with third dimension of %s. This image will be interpreted as a multichannel 2d image, "
                                     "which may not be intended." % str(image.shape[2])), stacklevel=2)
    image = _as_float64(image)
    if float(sigma) < 0:
        raise ValueError(f"felzenszwalb: sigma must be >= 0, got {sigma}")
    if not np.all(np.isfinite(image)):
        raise XaiHipError(_NONFINITE_TEXT)
    labels, _ = felzenszwalb_batch(image[None], [scale], sigma, min_size, device=device)
    return labels[0, 0].cpu().numpy().astype(np.int64)
