"""SLIC superpixels on the HIP kernels K65 - K68 (include/xai_hip_slic.h), defined by scikit-image 0.18.3
(skimage/segmentation/slic_superpixels.py and _slic.pyx): in the image's own dtype, float32 or float64, in skimage's operation order.

What stays on the host, in NumPy, is what skimage does once per image before its pixel loops: the Lab features (`slic_features`, a
restatement of skimage.color.rgb2lab in the image's dtype) and the grid of initial centres (`grid_centroids`).  The pixel loops are
the kernels: K65 the assignment, K66 the update, K67 the connected components with their sizes, K68 their numbering.  `slic_batch`
runs them on device tensors of B images with no read-back; `slic` has skimage's signature and returns a host array.

Parity: given the same features every label, centre and count is skimage's bit for bit.  The connectivity pass is
computed on the device in the regular case (every 4-connected component of equal raw label has min_size <= size < max_size: MDA's
case, always); any other case is reported in the status word and `slic` finishes it on the host from the raw labels, with skimage's
own pass where it is importable and with `enforce_connectivity_host`, its sequential restatement, where it is not.  A pixel in no
window and a cluster without a pixel are states skimage leaves undefined: they raise.
"""
import numpy as np
import torch

from . import kernels as K
from ._lib import XaiHipError
from .ig import hip_device
from .quickshift import D65_WHITE, XYZ_FROM_RGB
from .slic_host import enforce_connectivity_host  # noqa: F401

UNCOVERED, EMPTY, IRREGULAR = K.SLIC_UNCOVERED, K.SLIC_EMPTY, K.SLIC_IRREGULAR


def _as_float(image):
    """skimage.util.img_as_float for what this engine serves: a float32 or float64 image as it is, uint8 / 255 in float64."""
    image = np.asarray(image)
    if image.dtype in (np.float32, np.float64):
        return image
    if image.dtype == np.uint8:
        return image.astype(np.float64) / 255.0
    raise TypeError(f"slic: the image must be float32, float64 or uint8, got {image.dtype}")


def rgb2lab32(rgb):
    """skimage.color.rgb2lab (colorconv.py: rgb2xyz, xyz2lab with D65 / 2 degrees) in its own sequence of NumPy operations and in
    the array's own dtype, which for MDA's float32 image is float32 (quickshift.rgb2lab is the float64 twin).
    rgb: (..., 3) float32 or float64 -> (..., 3) of the same dtype."""
    arr = np.array(_as_float(rgb))
    dtype = arr.dtype
    if arr.shape[-1] != 3:
        raise ValueError(f"Input array must have a shape == (..., 3)), got {arr.shape}")
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    arr = arr @ XYZ_FROM_RGB.T.astype(dtype)
    arr = arr / np.asarray(D65_WHITE, dtype=dtype)
    mask = arr > 0.008856
    arr[mask] = np.cbrt(arr[mask])
    arr[~mask] = 7.787 * arr[~mask] + 16. / 116.
    x, y, z = arr[..., 0], arr[..., 1], arr[..., 2]
    L = (116. * y) - 16.
    a = 500.0 * (x - y)
    b = 200.0 * (y - z)
    return np.concatenate([v[..., np.newaxis] for v in [L, a, b]], axis=-1)


def slic_features(image, compactness, convert2lab=None):
    """slic_superpixels.py:232-254 and :306-308 without the smoothing: img_as_float, rgb2lab of a three-channel image unless
    convert2lab is False, `image * (1 / compactness)`: C-contiguous (H, W, C) in the image's dtype, on the host."""
    image = _as_float(image)
    if image.ndim == 2:
        image = image[..., np.newaxis]
    if image.ndim != 3:
        raise NotImplementedError(f"slic: volumes are not served, the image must be (H, W) or (H, W, C), got {image.shape}")
    dtype = image.dtype
    if convert2lab or convert2lab is None:
        if image.shape[-1] != 3 and convert2lab:
            raise ValueError("Lab colorspace conversion requires a RGB image.")
        elif image.shape[-1] == 3:
            image = rgb2lab32(image)
    ratio = 1.0 / compactness
    return np.ascontiguousarray(image * ratio, dtype=dtype)


def _regular_grid(ar_shape, n_points):
    """skimage.util.regular_grid (0.18.3), its own sequence of operations -> (starts, steps), a step None where the slice has none"""
    ar_shape = np.asanyarray(ar_shape)
    ndim = len(ar_shape)
    unsort_dim_idxs = np.argsort(np.argsort(ar_shape))
    sorted_dims = np.sort(ar_shape)
    space_size = float(np.prod(ar_shape))
    if space_size <= n_points:
        return [0] * ndim, [None] * ndim
    stepsizes = np.full(ndim, (space_size / n_points) ** (1.0 / ndim), dtype='float64')
    if (sorted_dims < stepsizes).any():
        for dim in range(ndim):
            stepsizes[dim] = sorted_dims[dim]
            space_size = float(np.prod(sorted_dims[dim + 1:]))
            stepsizes[dim + 1:] = ((space_size / n_points) ** (1.0 / (ndim - dim - 1)))
            if (sorted_dims >= stepsizes).all():
                break
    starts = (stepsizes // 2).astype(int)
    stepsizes = np.round(stepsizes).astype(int)
    return [int(starts[i]) for i in unsort_dim_idxs], [int(stepsizes[i]) for i in unsort_dim_idxs]


def grid_centroids(H, W, n_segments):
    """_get_grid_centroids of an image of depth 1 (slic_superpixels.py:71-104) -> (centres (S, 2) int64 of (y, x) in raster order,
    step): step is `max(steps)`, an integer in value, 1.0 where no slice has a step.  S may differ from n_segments."""
    starts, steps = _regular_grid((1, int(H), int(W)), int(n_segments))
    ys = np.arange(H)[slice(starts[1], None, steps[1])]
    xs = np.arange(W)[slice(starts[2], None, steps[2])]
    centres = np.stack(np.meshgrid(ys, xs, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int64)
    return centres, max(float(s) if s is not None else 1.0 for s in steps)


def size_bounds(H, W, S, min_size_factor=0.5, max_size_factor=3):
    """slic_superpixels.py:324-326: (min_size, max_size) of the connectivity pass"""
    segment_size = np.prod((1, H, W)) / S
    return int(min_size_factor * segment_size), int(max_size_factor * segment_size)


def _finish_on_host(raw, min_size, max_size, start_label):
    """the connectivity pass of an irregular case, on raw labels that start at start_label as skimage's do: skimage's own where it is
    importable, else the restated one"""
    try:
        from skimage.segmentation._slic import _enforce_label_connectivity_cython
    except ImportError:
        return enforce_connectivity_host(raw, min_size, max_size, start_label)
    return np.asarray(_enforce_label_connectivity_cython(np.ascontiguousarray(raw[None], dtype=np.intp), min_size, max_size,
                                                         start_label=start_label))[0].astype(np.int64)


def initial_centres(centres, B, C, dtype, device):
    """(S, 2) host centres -> the (B, S, 2 + C) device tensor the kernels take: (y, x) and zero colour, as slic_superpixels.py:298-301"""
    centres = np.asarray(centres)
    if centres.ndim != 2 or centres.shape[1] != 2 or centres.shape[0] < 1:
        raise ValueError(f"centres must be (S, 2) with S >= 1, got {centres.shape}")
    full = np.zeros((B, centres.shape[0], 2 + C), dtype=np.float64)
    full[:, :, :2] = centres
    return torch.from_numpy(full).to(dtype).to(device)


def slic_batch(features_dev, centres, step, max_iter=10, enforce_connectivity=True, min_size_factor=0.5, max_size_factor=3,
               start_label=0):
    """features_dev (B, H, W, C) float32 or float64 on a HIP device, centres (S, 2) and step from `grid_centroids` (or a
    (B, S, 2 + C) device tensor of the features' dtype, which is updated in place) -> (labels (B, H, W) int32, label counts (B,)
    int32, status (B,) int32 of the bits UNCOVERED, EMPTY, IRREGULAR, the final centres (B, S, 2 + C)), all on the device, no
    read-back.  Without enforce_connectivity the labels are start_label + the raw ones (an uncovered pixel's -1 included: it is
    reported in status) and the counts are S.  Where status has IRREGULAR the
    labels are not skimage's: finish from the raw labels on the host (`slic` does)."""
    out = _slic_batch(features_dev, centres, step, max_iter, enforce_connectivity, min_size_factor, max_size_factor, start_label)
    return out[0], out[1], out[2], out[3]


def _slic_batch(features_dev, centres, step, max_iter, enforce_connectivity, min_size_factor, max_size_factor, start_label):
    if start_label not in (0, 1):
        raise ValueError("start_label should be 0 or 1.")
    if float(step) != int(step) or int(step) < 1:
        raise ValueError(f"step must be a positive integer in value, got {step!r}")
    B, H, W, C = K._slic_shape(features_dev)               # the device last: every other refusal needs none
    if not isinstance(centres, torch.Tensor):
        centres = initial_centres(centres, B, C, features_dev.dtype, features_dev.device)
    S = int(centres.shape[1]) if centres.dim() == 3 else 0
    raw, status = K.slic_iterate(features_dev, centres, int(step), max_iter)
    if not enforce_connectivity:                           # _slic_cython (slic_superpixels.py:316-318) returns start_label + k
        labels = raw + start_label if start_label else raw
        return labels, torch.full((B,), S, dtype=torch.int32, device=raw.device), status, centres, raw
    min_size, max_size = size_bounds(H, W, S, min_size_factor, max_size_factor)
    ws = K.slic_workspace(raw)
    comp = K.slic_components(raw, min_size, max_size, status, ws)
    labels, counts = K.slic_number(comp, start_label, ws)
    return labels, counts, status, centres, raw


def slic(image, n_segments=100, compactness=10., max_iter=10, sigma=0, spacing=None, multichannel=True, convert2lab=None,
         enforce_connectivity=True, min_size_factor=0.5, max_size_factor=3, slic_zero=False, start_label=None, mask=None,
         device="cuda"):
    """skimage.segmentation.slic's signature and defaults (0.18.3) -> the (H, W) int64 label array on the host.  One argument skimage
    does not have: `device`.  Not served, each a NotImplementedError: sigma != 0, spacing, mask, slic_zero, volumes."""
    if np.any(np.asarray(sigma) != 0):
        raise NotImplementedError("slic: sigma != 0 (Gaussian smoothing before the segmentation) is not served; the reference never smooths")
    if spacing is not None:
        raise NotImplementedError("slic: spacing is not served; the kernels take isotropic pixels")
    if mask is not None:
        raise NotImplementedError("slic: mask is not served")
    if slic_zero:
        raise NotImplementedError("slic: slic_zero is not served")
    image = _as_float(image)
    if image.ndim not in (2, 3) or (image.ndim == 3 and not multichannel):
        raise NotImplementedError(f"slic: volumes are not served (multichannel=False on a 3-D array or more than 3 dimensions), got "
                                  f"{image.shape}")
    if start_label is None:
        start_label = 0                                # skimage 0.18.3's default, which it announces with a FutureWarning
    if start_label not in [0, 1]:
        raise ValueError("start_label should be 0 or 1.")
    feats = slic_features(image, compactness, convert2lab if multichannel else False)
    H, W = feats.shape[:2]
    centres, step = grid_centroids(H, W, n_segments)
    dev = hip_device(device)
    labels, _, status, _, raw = _slic_batch(torch.from_numpy(feats)[None].to(dev), centres, step, max_iter, enforce_connectivity,
                                            min_size_factor, max_size_factor, start_label)
    st = int(status[0])
    if st & UNCOVERED:
        raise XaiHipError("slic: a pixel lies in no cluster's window; scikit-image leaves its label undefined, so there is nothing to equal")
    if st & EMPTY:
        raise XaiHipError("slic: a cluster has no pixel (its centre is 0 / 0); scikit-image leaves what follows undefined")
    if st & IRREGULAR:
        min_size, max_size = size_bounds(H, W, centres.shape[0], min_size_factor, max_size_factor)
        return _finish_on_host(raw[0].cpu().numpy().astype(np.int64) + start_label, min_size, max_size, start_label)
    return labels[0].cpu().numpy().astype(np.int64)
