"""Complete-linkage agglomerative clustering of a precomputed distance matrix, restated in NumPy from the two libraries that define
it for ViT-CX: scipy.cluster.hierarchy.linkage(y, "complete") (the nearest-neighbour chain of scipy/cluster/_hierarchy.pyx, `nn_chain`,
then a stable sort by height and `label`'s union-find) and scikit-learn's AgglomerativeClustering(n_clusters=None,
distance_threshold=t, metric="precomputed", linkage="complete") (sklearn/cluster/_agglomerative.py: linkage_tree reads
X[np.triu_indices(n, 1)], n_clusters_ = count_nonzero(distances_ >= t) + 1, `_hc_cut` on a heapq list).  Not the kernel source: this
is what K56 / K57 (include/xai_hip_ext6.h) and xai_engine/linkage.py are held to, bit for bit.

Complete linkage does no arithmetic on distances (the Lance-Williams update is `max`), so every height is one of the float32 inputs and
every fp32 comparison here equals the libraries' fp64 comparison of the same values.  The tie rules are the algorithm's: the row scan
takes the FIRST index of the strict minimum and prefers the chain predecessor on equality, the sort is stable.
"""
from heapq import heappush, heappushpop

import numpy as np


def nn_chain(distance):
    """distance (n, n) float32, only i < j read -> (merges (n-1, 2) int32 with x < y, heights (n-1,) float32, scans, pushes) in the
    order the chain finds them (scipy's Z before its sort)"""
    D = np.asarray(distance, dtype=np.float32)
    n = D.shape[0]
    if D.ndim != 2 or D.shape[1] != n or n < 2:
        raise ValueError(f"distance must be (n, n) with n >= 2, got {D.shape}")
    iu = np.triu_indices(n, 1)
    if not np.isfinite(D[iu]).all():
        raise ValueError("distance has a non-finite entry above the diagonal")
    W = np.zeros((n, n), np.float32)
    W[iu] = D[iu]
    W.T[iu] = D[iu]
    size = np.ones(n, np.int64)
    chain = []
    merges = np.zeros((n - 1, 2), np.int32)
    heights = np.zeros(n - 1, np.float32)
    scans = pushes = 0
    idx = np.arange(n)
    for k in range(n - 1):
        if not chain:
            chain.append(int(np.flatnonzero(size > 0)[0]))
            pushes += 1
        while True:
            x = chain[-1]
            if len(chain) >= 2:
                y = chain[-2]
                cur = W[x, y]
            else:
                y, cur = -1, np.float32(np.inf)
            live = (size > 0) & (idx != x)
            row = np.where(live, W[x], np.float32(np.inf))
            scans += 1
            i = int(np.argmin(row))               # the first index of the minimum
            if row[i] < cur:                      # strict: on equality the chain predecessor stays
                cur, y = row[i], i
            if len(chain) >= 2 and y == chain[-2]:
                break
            chain.append(y)
            pushes += 1
        del chain[-2:]
        if x > y:
            x, y = y, x
        merges[k] = (x, y)
        heights[k] = cur
        size[y] += size[x]
        size[x] = 0
        live = (size > 0) & (idx != y)
        new = np.where(W[live, y] > W[live, x], W[live, y], W[live, x])     # max(W[i][x], W[i][y]); W[i][x] on a signed-zero tie
        W[live, y] = new
        W[y, live] = new
    return merges, heights, scans, pushes


def sort_relabel(merges, heights, n):
    """the stable sort by height and scipy's `label` -> (children (n-1, 2) int32, ids ascending in a row; heights (n-1,) float32)"""
    order = np.argsort(heights, kind="stable")
    parent = np.arange(n)
    ident = np.arange(n)
    children = np.zeros((n - 1, 2), np.int32)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for k, j in enumerate(order):
        rx, ry = find(merges[j, 0]), find(merges[j, 1])
        a, b = ident[rx], ident[ry]
        children[k] = (min(a, b), max(a, b))
        parent[rx] = ry
        ident[ry] = n + k
    return children, heights[order]


def complete_linkage(distance):
    """-> (children (n-1, 2) int32, heights (n-1,) float32) = sklearn's children_ and distances_"""
    merges, heights, _, _ = nn_chain(distance)
    return sort_relabel(merges, heights, np.asarray(distance).shape[0])


def descendants(node, children, n):
    """the leaves below `node` (sklearn's _hc_get_descendent)"""
    out, stack = [], [int(node)]
    while stack:
        i = stack.pop()
        if i < n:
            out.append(i)
        else:
            stack.extend(int(c) for c in children[i - n])
    return out


def hc_cut(children, heights, distance_threshold):
    """-> (labels (n,) int64, n_clusters): n_clusters_ = 1 + #{(double)height >= threshold}, then sklearn's _hc_cut; the label of a
    cluster is its position in the heapq list, not in a sorted one"""
    n = len(children) + 1
    n_clusters = int(np.count_nonzero(np.asarray(heights, np.float64) >= distance_threshold)) + 1
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_clusters - 1):
        c = children[-nodes[0] - n]
        heappush(nodes, -int(c[0]))
        heappushpop(nodes, -int(c[1]))
    labels = np.zeros(n, np.int64)
    for i, node in enumerate(nodes):
        labels[descendants(-node, children, n)] = i
    return labels, n_clusters


def agglomerative_labels(distance, distance_threshold):
    """-> (labels, n_clusters, children, heights), sklearn's labels_, n_clusters_, children_, distances_"""
    children, heights = complete_linkage(distance)
    labels, n_clusters = hc_cut(children, heights, distance_threshold)
    return labels, n_clusters, children, heights


# ------------------------------------------------------------------------------------------------ the data kinds of the tests
def cosine_distance(rng, n, dim=16):
    """1 - cosine similarity of n random non-negative rows, float32, as ViT-CX forms it; the lower triangle holds the product's own
    (possibly not bit-symmetric) values"""
    v = rng.random((n, dim), dtype=np.float32) + np.float32(0.05)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (np.float32(1) - v @ v.T).astype(np.float32)


def quantised(rng, n, steps):
    """symmetric, every entry a multiple of 1 / steps in [0, 1]: ties everywhere"""
    d = rng.integers(0, steps + 1, size=(n, n)).astype(np.float32) / np.float32(steps)
    d = np.triu(d, 1)
    return (d + d.T).astype(np.float32)


def all_equal(n, value=0.25):
    d = np.full((n, n), value, np.float32)
    np.fill_diagonal(d, 0)
    return d


def duplicate_blocks(rng, n, blocks):
    """points that are exact copies of `blocks` prototypes: distance 0 inside a block, the prototypes' distance between blocks"""
    proto = cosine_distance(rng, blocks)
    proto = np.triu(proto, 1)
    proto = proto + proto.T
    of = rng.integers(0, blocks, size=n)
    return np.ascontiguousarray(proto[np.ix_(of, of)].astype(np.float32))


def other_lower_triangle(rng, d):
    """the same upper triangle over a lower triangle of different finite values, which no reader may look at"""
    n = d.shape[0]
    out = np.triu(d, 1) + np.tril(rng.random((n, n), dtype=np.float32) * np.float32(3) + np.float32(0.5), -1)
    return out.astype(np.float32)


def duplicated_pair_share(d):
    """the share of pairs i < j whose value some other pair has too"""
    v = d[np.triu_indices(d.shape[0], 1)]
    _, counts = np.unique(v, return_counts=True)
    return float(counts[counts > 1].sum()) / v.size


def from_condensed(y, n):
    """the symmetric (n, n) float32 matrix whose entries above the diagonal, in np.triu_indices(n, 1) order, are y; zero diagonal"""
    d = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    d[iu] = y
    d.T[iu] = y
    return d


def with_float32_tenth(rng, d):
    """a third of the pairs set to exactly float32(0.1), symmetrically"""
    n = d.shape[0]
    iu = np.triu_indices(n, 1)
    y = d[iu].copy()
    y[rng.random(y.size) < 1 / 3] = np.float32(0.1)
    return from_condensed(y, n)


def big_matrix(seed, n=768):
    """the n = 768 case of tests/golden/linkage.npz, redrawn: np.random.RandomState's stream is frozen, and a product, a sum and a
    rounding to float32 are the same on every machine.  Values in [0.02, 0.37)."""
    u = np.random.RandomState(seed).random_sample(n * (n - 1) // 2)
    return from_condensed((0.02 + 0.35 * u * u).astype(np.float32), n)
