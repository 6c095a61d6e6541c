"""The arithmetic contract of include/xai_hip_ext7.h (K58-K61, the k-means of TIS) restated in NumPy, fp32 and fp64 exactly where the
header says so.  Every sum starts from +0 and runs sequentially in ascending index, one accumulator per result; products and sums round
separately (NumPy never fuses them).  The loops run over t with the (n, k) arrays vectorised, over i for the sums, over t (every j at
once, each j its own accumulator) for e_j and over j for err: elementwise vector operations keep one accumulator per result, so the
order of every single sum is the header's."""
import numpy as np

F32 = np.float32


def kmeans(X, first, max_iter=100, tol=1e-4):
    """X (n, d) fp32, first (k,) indices -> (centroids (k, d) fp32, assign (n,) int32, counts (k,) int32, iterations, err (np.float64))"""
    X = np.ascontiguousarray(X, dtype=F32)
    first = np.asarray(first, dtype=np.int64)
    n, d = X.shape
    k = len(first)
    assert 1 <= k <= n and max_iter >= 1 and first.min() >= 0 and first.max() < n
    C = X[first].copy()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        xx = np.zeros(n, F32)
        for t in range(d):
            xx = xx + X[:, t] * X[:, t]
        iterations, err = 0, np.float64(0.0)
        while True:
            cc = np.zeros(k, F32)
            for t in range(d):
                cc = cc + C[:, t] * C[:, t]
            dot = np.zeros((n, k), F32)
            for t in range(d):
                dot = dot + X[:, t, None] * C[None, :, t]
            s = ((F32(2) * dot) - xx[:, None]) - cc[None, :]
            assert s.dtype == F32
            assign = np.argmax(s, axis=1).astype(np.int32)          # the first NaN, else the first maximal value
            counts = np.zeros(k, np.int32)
            sums = np.zeros((k, d), F32)
            for i in range(n):
                counts[assign[i]] += 1
                sums[assign[i]] = sums[assign[i]] + X[i]
            new = sums / counts.astype(F32)[:, None]
            new[new != new] = 0
            q = new - C
            q = q * q
            assert new.dtype == F32 and q.dtype == F32
            e = np.zeros(k, np.float64)
            for t in range(d):
                e = e + q[:, t].astype(np.float64)
            err = np.float64(0.0)
            for j in range(k):
                err = err + e[j]
            C = new
            iterations += 1
            if err <= tol or iterations >= max_iter:
                break
    return C, assign, counts, iterations, err
