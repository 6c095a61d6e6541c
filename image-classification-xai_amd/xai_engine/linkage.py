"""Complete-linkage agglomerative clustering of a precomputed distance matrix on the HIP kernels K56 - K57
(include/xai_hip_ext6.h), defined by the two libraries ViT-CX calls for it: scipy.cluster.hierarchy.linkage(y, "complete") (the
nearest-neighbour chain, a stable sort by height, a union-find relabel) under scikit-learn's AgglomerativeClustering(n_clusters=None,
distance_threshold=t, metric="precomputed", linkage="complete") (the tree cut `_hc_cut`).

What runs where
  the symmetric working copy, the finite check, the chain loop      K56  xai_linkage_complete_f32 (one workgroup walks the chain)
  the stable sort of the n - 1 heights, the union-find relabel      K57  xai_linkage_sort_relabel_i32
  the cut: n_clusters and sklearn's `_hc_cut` on Python's heapq      host, on the 12 (n - 1) + 16 bytes read back in ONE copy

Parity: complete linkage does no arithmetic on distances (the update is `max`), so every height is one of the float32 inputs and every
fp32 comparison equals the libraries' fp64 one.  children, heights, n_clusters and labels are scikit-learn's children_, distances_,
n_clusters_ and labels_ bit for bit (tests/golden/linkage.npz holds the libraries' own runs).  The label of a cluster is its position
in CPython's heap list, which is why the cut stays Python's own heapq.
"""
from heapq import heappush, heappushpop

import numpy as np
import torch

from . import kernels as K
from ._lib import XaiHipError


def linkage_device(distance, lanes=0):
    """distance (n, n) fp32 on a HIP device, only the entries above the diagonal are read -> (children (n - 1, 2) int32, heights
    (n - 1,) fp32, info (4,) int32 = [status, row scans, pushes, merges]) as host arrays: three launches, one read-back.  A
    non-finite entry above the diagonal is a ValueError, as in sklearn's check_array."""
    ws = K.linkage_workspace(distance)                 # checks shape, dtype, the cap and the device
    n = int(distance.shape[0])
    m = n - 1
    out = torch.empty(3 * m + 4, dtype=torch.int32, device=distance.device)
    children, heights, info = out[:2 * m], out[2 * m:3 * m].view(torch.float32), out[3 * m:]
    K.linkage_complete(distance, ws, info, lanes)
    K.linkage_sort_relabel(n, ws, children, heights, info)
    host = out.cpu().numpy()                           # the one read-back of the step
    status = int(host[3 * m])
    if status == K.LINKAGE_NONFINITE:
        raise ValueError("distance has a non-finite entry above the diagonal (Input contains NaN or infinity)")
    if status != K.LINKAGE_OK:
        raise XaiHipError(f"complete linkage: the chain loop ended on a bound (status {status}, {host[3 * m + 1]} scans, "
                          f"{host[3 * m + 2]} pushes, {host[3 * m + 3]} of {m} merges): a logic error, not an input's fault")
    return host[:2 * m].reshape(m, 2).copy(), host[2 * m:3 * m].view(np.float32).copy(), host[3 * m:].copy()


def complete_linkage(distance):
    """-> (children (n - 1, 2) int32, heights (n - 1,) fp32): scikit-learn's children_ and distances_ for this matrix"""
    children, heights, _ = linkage_device(distance)
    return children, heights


def hc_cut(children, heights, distance_threshold):
    """-> (labels (n,) int64, n_clusters).  n_clusters = 1 + #{(double)height >= distance_threshold}: the threshold stays the Python
    double (float32(0.1) is not 0.1).  Then sklearn's `_hc_cut`: the n_clusters largest nodes on a heapq list of negated ids; the
    label of a cluster is its position in that list."""
    n = len(children) + 1
    n_clusters = int(np.count_nonzero(np.asarray(heights, dtype=np.float64) >= distance_threshold)) + 1
    rows = np.asarray(children).tolist()               # plain ints: the loops below are Python's
    nodes = [-(max(rows[-1]) + 1)]
    for _ in range(n_clusters - 1):
        a, b = rows[-nodes[0] - n]
        heappush(nodes, -a)
        heappushpop(nodes, -b)
    # labels[descendants(-node)] = i for i, node in enumerate(nodes), top down: a node's children were made before it, so one pass
    # over the ids in descending order hands every label to the leaves; the subtrees of the heap's nodes are disjoint
    label = [-1] * (2 * n - 1)
    for i, node in enumerate(nodes):
        label[-node] = i
    for node in range(2 * n - 2, n - 1, -1):
        if label[node] >= 0:
            a, b = rows[node - n]
            label[a] = label[b] = label[node]
    return np.array(label[:n], dtype=np.int64), n_clusters


def agglomerative_labels(distance, distance_threshold):
    """-> (labels (n,) int64 ndarray, n_clusters, children, heights): labels_, n_clusters_, children_ and distances_ of
    AgglomerativeClustering(n_clusters=None, distance_threshold=distance_threshold, metric="precomputed", linkage="complete")
    .fit(distance)"""
    children, heights = complete_linkage(distance)
    labels, n_clusters = hc_cut(children, heights, float(distance_threshold))
    return labels, n_clusters, children, heights
