"""The k-means of TIS on the HIP kernels K58 - K61 (include/xai_hip_ext7.h): the Euclidean Lloyd iteration of
tis.kmeans_centroids (TIS.py:150-155, fast_pytorch_kmeans.KMeans in the reference) in a stated arithmetic order.

What runs where
  xx_i, C = points[first], cc_j                                          K58  xai_kmeans_init_f32
  per iteration: the assignment (the score matrix is never stored)       K59
                 counts, sums, division, NaN -> +0, e_j, the next cc_j   K60
                 err in fp64, the counter, the `done` word               K61  (all three: xai_kmeans_iterate_f32)
  the loop: `check_every` iterations per call, then ONE read of the 24-byte state; launches after the stop change nothing

Parity: every sum starts from +0 and runs in ascending index with one accumulator, products and sums round separately, so the
centroids, assignments, counts, iterations and err equal a NumPy restatement of the header's contract bit for bit
(tests/kmeans_restated.py), on every run and machine.  tis.kmeans_centroids sums in rocBLAS's and torch's order instead: the two agree
to rounding, and a near-tie may fall differently.
"""
import numpy as np
import torch

from . import kernels as K
from ._lib import XaiHipError


def _first_indices(first, n, k, device):
    """the initial points as a checked (k,) int64 device tensor; None: the draw tis.kmeans_centroids makes"""
    if first is None:
        first = np.random.choice(n, size=[k], replace=False)
    if isinstance(first, torch.Tensor):
        if first.dtype != torch.int64:
            raise TypeError(f"first: expected torch.int64, got {first.dtype}")
        host = first.detach().cpu().numpy()
    else:
        host = np.asarray(first)
        if host.dtype.kind not in "iu":
            raise TypeError(f"first: expected integers, got {host.dtype}")
        host = host.astype(np.int64)
    if host.ndim != 1 or host.size < 1:
        raise ValueError(f"first must be (k,) with k >= 1, got {host.shape}")
    if k is not None and host.size != k:
        raise ValueError(f"first holds {host.size} indices, n_clusters is {k}")
    if host.size > n:
        raise ValueError(f"n_clusters must be in [1, n = {n}], got {host.size}")
    if host.min() < 0 or host.max() >= n:
        raise ValueError(f"first has an index outside [0, {n})")
    return torch.from_numpy(np.ascontiguousarray(host)).to(device)


def kmeans_device(points, n_clusters=None, *, first=None, max_iter=100, tol=1e-4, check_every=8, return_info=False):
    """points (n, d) fp32 on a HIP device -> centroids (k, d) on the device.  first: the k initial points (indices; None draws
    np.random.choice(n, size=[k], replace=False) from NumPy's global generator, as tis.kmeans_centroids does).  return_info: also a
    dict of assign (n,) int32 and counts (k,) int32 on the device, iterations and err (a Python float, fp64)."""
    if n_clusters is None and first is None:
        raise ValueError("give n_clusters or first")
    k = n_clusters if n_clusters is not None else (int(first.numel()) if isinstance(first, torch.Tensor) else int(np.size(first)))
    K._kmeans_stop(max_iter, tol)
    if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
        raise ValueError(f"check_every must be an int >= 1, got {check_every!r}")
    n, d, k = K._kmeans_extents(points, k)             # type, dtype, shape, k <= n, THE LIMITS, contiguity, the device
    first = _first_indices(first, n, k, points.device)
    dev = points.device
    ws = K.kmeans_workspace(points, k)
    C = torch.empty((k, d), dtype=torch.float32, device=dev)
    assign = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    state = torch.empty(K.KMEANS_STATE_WORDS, dtype=torch.int32, device=dev)
    K.kmeans_init(points, first, C, ws, state)
    issued = 0
    while True:
        chunk = min(check_every, max_iter - issued)
        K.kmeans_iterate(points, C, assign, counts, ws, state, max_iter, tol, chunk)
        issued += chunk
        host = state.cpu().numpy()                     # the one read-back of the chunk
        if host[2] != K.KMEANS_OK:
            raise XaiHipError(f"k-means: status {int(host[2])}, an initial index outside the points reached the device")
        if host[1] or issued >= max_iter:
            break
    if not host[1] or host[0] > issued:
        raise XaiHipError(f"k-means: {issued} iterations issued, the device reports {int(host[0])} run and done = {int(host[1])}")
    if not return_info:
        return C
    return C, {"assign": assign, "counts": counts, "iterations": int(host[0]), "err": float(host[4:6].view(np.float64)[0])}
