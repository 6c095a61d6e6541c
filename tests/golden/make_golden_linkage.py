"""Regenerate tests/golden/linkage.npz from scipy's and scikit-learn's own complete-linkage clustering.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_linkage.py        (an interpreter that has scipy and scikit-learn)

scipy.cluster.hierarchy.linkage(y, "complete") and sklearn.cluster.AgglomerativeClustering(n_clusters=None, distance_threshold=t,
metric="precomputed", linkage="complete").fit(matrix) run unmodified on the host; `scipy_version` and `sklearn_version` in the file
name the releases.

Cases (`names`), per case <tag> = <kind>_<n>:
  <tag>_y           the entries above the diagonal in np.triu_indices(n, 1) order, float32 (tests/linkage_restated.from_condensed makes
                    the symmetric matrix; the `lower` kind gets a lower triangle of other finite values, drawn by the test, which no
                    reader may look at, so its upper triangle and its results are those of generic_<n>)
  <tag>_thresholds  float64: 0.1, a merge height, the double just above it, 0.0 (n clusters), above the largest height (one cluster)
  <tag>_Z           scipy's linkage output (n - 1, 4) float64
  <tag>_children, <tag>_distances   sklearn's children_ (int32) and distances_ (float64)
  <tag>_labels (T, n) int32, <tag>_n_clusters (T,) int32   sklearn's labels_ and n_clusters_ per threshold
    generic   1 - cosine similarity of random rows                       n in 2, 3, 5, 63, 64, 65, 127, 129
    q16, q64  distances quantised to 1/16 and 1/64: ties everywhere      the same sizes
    equal     every pair at the same distance: every comparison a tie    the same sizes
    blocks    exact duplicates of a few prototypes: distance 0 inside    the same sizes
    f32tenth_33   a third of the pairs at exactly float32(0.1); its thresholds add float32(0.1) as a double and the double just above
                  it, where a threshold rounded to fp32 would count one merge height more
    big_768   n = 768, not stored: tests/linkage_restated.big_matrix(big_768_seed) redraws it from np.random.RandomState, whose
              stream is frozen, and big_768_sha256 is the digest of its bytes
The generator asserts on every case that the NumPy restatement (tests/linkage_restated.py) equals the libraries bit for bit (Z,
children_, distances_, labels_, n_clusters_) and that every tie case (q16, q64, equal, blocks, f32tenth) with more than three points
has at least 10 % duplicated pair values.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import linkage_restated as R  # noqa: E402

try:
    import scipy
    import sklearn
    from scipy.cluster.hierarchy import linkage
    from sklearn.cluster import AgglomerativeClustering
except ImportError:
    sys.exit("make_golden_linkage.py: needs scipy and scikit-learn")

SIZES = (2, 3, 5, 63, 64, 65, 127, 129)
TIE_KINDS = ("q16", "q64", "equal", "blocks", "f32tenth")
BIG_SEED = 768


def matrix_of(kind, n, rng):
    if kind == "generic":
        return R.cosine_distance(rng, n)
    if kind in ("q16", "q64"):
        return R.quantised(rng, n, int(kind[1:]))
    if kind == "equal":
        return R.all_equal(n)
    if kind == "blocks":
        return R.duplicate_blocks(rng, n, max(1, n // 6))
    if kind == "f32tenth":
        return R.with_float32_tenth(rng, R.cosine_distance(rng, n))
    raise ValueError(kind)


def run_case(tag, d, extra_thresholds=()):
    """the libraries on one matrix, the restatement held to them -> the arrays to store (without the matrix)"""
    n = d.shape[0]
    y = d[np.triu_indices(n, 1)]
    Z = linkage(y, "complete")
    children, heights = R.complete_linkage(d)
    assert np.array_equal(children, Z[:, :2].astype(np.int64)) and np.array_equal(heights.astype(np.float64), Z[:, 2]), tag
    assert np.isin(heights, y).all(), tag                                  # every height is one of the inputs
    mid = float(heights[(n - 1) // 2])
    thresholds = np.array([0.1, mid, np.nextafter(mid, np.inf), 0.0, float(heights.max()) + 1.0, *extra_thresholds], np.float64)
    labels, counts = [], []
    for t in thresholds:
        m = AgglomerativeClustering(n_clusters=None, distance_threshold=float(t), metric="precomputed", linkage="complete").fit(d)
        assert np.array_equal(m.children_, children) and np.array_equal(m.distances_, Z[:, 2]), tag
        lab, k = R.hc_cut(children, heights, float(t))
        assert np.array_equal(lab, m.labels_) and k == m.n_clusters_, (tag, t)
        labels.append(m.labels_.astype(np.int32))
        counts.append(m.n_clusters_)
    assert heights.min() >= 0 and counts[3] == n and counts[4] == 1, (tag, counts)           # 0.0: n clusters; above the top: one
    assert counts[2] == counts[1] - np.count_nonzero(heights == np.float32(mid)), tag      # the double above the height drops exactly its ties
    return {f"{tag}_thresholds": thresholds, f"{tag}_Z": Z, f"{tag}_children": children.astype(np.int32), f"{tag}_distances": Z[:, 2].copy(),
            f"{tag}_labels": np.stack(labels), f"{tag}_n_clusters": np.array(counts, np.int32)}, counts


def main():
    out = {"scipy_version": np.array(scipy.__version__), "sklearn_version": np.array(sklearn.__version__)}
    names = []
    rng = np.random.default_rng(20)
    for kind in ("generic", "q16", "q64", "equal", "blocks"):
        for n in SIZES:
            tag = f"{kind}_{n}"
            d = matrix_of(kind, n, rng)
            share = R.duplicated_pair_share(d)
            if kind in TIE_KINDS and n > 3:
                assert share >= 0.1, (tag, share)
            arrays, counts = run_case(tag, d)
            out.update(arrays)
            out[f"{tag}_y"] = d[np.triu_indices(n, 1)]
            names.append(tag)
            print(f"{tag}: duplicated pairs {share:.2f} n_clusters {counts}")
    tag, tenth = "f32tenth_33", float(np.float32(0.1))
    d = matrix_of("f32tenth", 33, rng)
    assert R.duplicated_pair_share(d) >= 0.1
    arrays, counts = run_case(tag, d, extra_thresholds=(tenth, np.nextafter(tenth, np.inf)))
    heights = arrays[f"{tag}_distances"].astype(np.float32)
    above = float(arrays[f"{tag}_thresholds"][6])
    assert (heights == np.float32(0.1)).sum() >= 1 and np.float32(above) == np.float32(0.1)
    assert counts[6] == counts[5] - (heights == np.float32(0.1)).sum() < counts[5]       # in fp32 the two thresholds would count alike
    out.update(arrays)
    out[f"{tag}_y"] = d[np.triu_indices(33, 1)]
    names.append(tag)
    print(f"{tag}: n_clusters {counts}")
    d = R.big_matrix(BIG_SEED)
    arrays, counts = run_case("big_768", d)
    out.update(arrays)
    out["big_768_seed"] = np.array(BIG_SEED)
    out["big_768_sha256"] = np.array(hashlib.sha256(d.tobytes()).hexdigest())
    names.append("big_768")
    print(f"big_768: duplicated pairs {R.duplicated_pair_share(d):.2f} n_clusters {counts}")
    out["names"] = np.array(names)
    path = os.path.join(HERE, "linkage.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
