"""Plain NumPy fp64 restatement of LIME for images as the reference's harness runs it (limeAttr.py:23-36 -> lime_image.py
explain_instance -> lime_base.py explain_instance_with_data with 'highest_weights'), written from the description of what those
lines compute, the yardstick of the LIME tests wherever no fixture of the reference itself exists.

sklearn's pieces are closed forms here: the cosine distance of a 0/1 row with k ones to the all-ones row is 1 - sqrt(k / D) (1 for
k = 0), and Ridge(alpha, fit_intercept=True).fit(X, y, sample_weight=w) is, with the weighted means xbar and ybar,
coef = (sum w (x - xbar)(x - xbar)^T + alpha I)^-1 sum w (x - xbar)(y - ybar), intercept = ybar - xbar . coef.
tests/golden/lime.npz holds the reference's own numbers and the measured error of this restatement against them.
"""
import numpy as np

from xrai_restated import voronoi_labels

ALPHA_SELECT, ALPHA = 0.01, 1.0
GOLDEN_CASES = "abcd"                 # the cases of tests/golden/lime.npz


def distances(data):
    data = np.asarray(data)
    return 1.0 - np.sqrt((data != 0).sum(1) / data.shape[1])


def kernel_weights(d, kernel_width=0.25):
    return np.sqrt(np.exp(-(d ** 2) / kernel_width ** 2))


def weighted_means(X, y, w):
    """Weighted column means, every column (and the all-ones column that gives the sum of the weights) added in one order, rows
    ascending: a column of ones has the mean 1 exactly, a column of zeros 0, so their centred columns and coefficients are exact
    zeros -- the exact ties the order tests use."""
    cols = np.column_stack([np.ones(len(w)), X]) * w[:, None]
    s = np.zeros(cols.shape[1])
    for row in cols:
        s = s + row
    return s[1:] / s[0], float((w * y).sum() / s[0])


def ridge(X, y, w, alpha):
    X, y, w = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(w, np.float64)
    xbar, ybar = weighted_means(X, y, w)
    Xc, yc = X - xbar, y - ybar
    A = (Xc * w[:, None]).T @ Xc + alpha * np.eye(X.shape[1])
    coef = np.linalg.solve(A, (Xc * w[:, None]).T @ yc)
    return coef, ybar - float(xbar @ coef), ybar


def r2(y, pred, w, ybar):
    if len(y) < 2:
        return float("nan")
    num, den = float((w * (y - pred) ** 2).sum()), float((w * (y - ybar) ** 2).sum())
    if den == 0.0:
        return 1.0 if num == 0.0 else 0.0
    return 1.0 - num / den


def explain_label(data, y, w):
    """One label: -> coef (D,) indexed by feature, order (D,) the features by descending |coef| as the reference lists them,
    intercept, score, local_pred.  Both sorts are Python's stable `sorted(..., reverse=True)`: ties keep their earlier order."""
    X = (np.asarray(data) != 0).astype(np.float64)
    D = X.shape[1]
    c1, _, _ = ridge(X, y, w, ALPHA_SELECT)
    used = sorted(range(D), key=lambda j: abs(c1[j] * X[0, j]), reverse=True)
    c2, icpt, ybar = ridge(X[:, used], y, w, ALPHA)
    final = sorted(range(D), key=lambda i: abs(c2[i]), reverse=True)
    coef = np.zeros(D)
    coef[used] = c2
    pred = X[:, used] @ c2 + icpt
    return dict(coef=coef, order=np.array([used[i] for i in final], np.int32), intercept=icpt, score=r2(y, pred, w, ybar),
                local_pred=float(pred[0]))


def explain(data, Y, kernel_width=0.25):
    """data (N, D) 0/1, Y (N, L) the label columns -> dict: dist, weight (N,), coef (L, D), order (L, D), intercept, score,
    local_pred (L,)."""
    Y = np.asarray(Y, np.float64)
    d = distances(data)
    w = kernel_weights(d, kernel_width)
    per = [explain_label(data, Y[:, l], w) for l in range(Y.shape[1])]
    out = {k: np.array([p[k] for p in per]) for k in ("coef", "order", "intercept", "score", "local_pred")}
    out.update(dist=d, weight=w)
    return out


def chosen_features(order, coef, num_features=5):
    """get_image_and_mask(positive_only=True, min_weight=0): the first num_features features of the sorted explanation with a
    weight above 0."""
    return [int(f) for f in order if coef[f] > 0][:num_features]


def mask_of(segments, order, coef, num_features=5):
    mask = np.zeros(np.shape(segments), np.int64)
    for f in chosen_features(order, coef, num_features):
        mask[np.asarray(segments) == f] = 1
    return mask


def top_labels(probs_row0, n):
    return np.argsort(probs_row0)[-n:][::-1]


def perturbed(x_chw, segments, row, fill):
    """One perturbed image: the pixels of the superpixels with row[z] == 0 take `fill` (broadcastable to (C, H, W)), the others
    keep x, as a select (NaN and Inf of kept pixels pass); an id outside [0, len(row)) is never switched off."""
    seg = np.asarray(segments)
    inside = (seg >= 0) & (seg < len(row))
    off = np.zeros(seg.shape, bool)
    off[inside] = np.asarray(row)[seg[inside]] == 0
    return np.where(off[None], np.broadcast_to(fill, x_chw.shape), x_chw).astype(np.float32)


def segment_means(image_hwc, segments):
    """hide_color=None: every superpixel filled with its per-channel mean colour."""
    out = image_hwc.copy()
    for s in np.unique(segments):
        sel = segments == s
        out[sel] = [np.mean(image_hwc[sel][:, c]) for c in range(image_hwc.shape[2])]
    return out


def pack(data, words=None):
    """(N, D) 0/1 -> (N, words) uint64, column z = bit z % 64 of word z // 64."""
    data = np.asarray(data)
    N, D = data.shape
    words = (D + 63) // 64 if words is None else words
    out = np.zeros((N, words), np.uint64)
    for z in range(D):
        out[:, z // 64] |= (data[:, z] != 0).astype(np.uint64) << np.uint64(z % 64)
    return out


def seeded_case(H, W, cells, seed):
    """-> segments (H, W) int16 (the Voronoi cells of `cells` seeded points, ids 0 .. D - 1) and an (H, W, 3) float32 image in [0, 1]."""
    rng = np.random.default_rng(seed)
    seg = voronoi_labels(H, W, cells, rng)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([np.sin(yy / 5.0 + c) * np.cos(xx / 7.0 - c) for c in range(3)], -1)
    img = 0.5 + 0.25 * base + 0.25 * (rng.random((H, W, 3)) - 0.5)
    return seg, np.clip(img, 0.0, 1.0).astype(np.float32)


def seeded_fit_case(N, D, L, seed, zero_rows=0):
    """-> data (N, D) 0/1 with row 0 all ones (and `zero_rows` all-zero rows behind it) and Y (N, L) float32: a linear response
    to the bits plus noise, squashed into (0, 1)."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, (N, D))
    data[0] = 1
    data[1:1 + zero_rows] = 0
    beta = rng.standard_normal((D, L)) * np.linspace(1.0, 0.2, D)[:, None]
    z = (data - 0.5) @ beta / np.sqrt(D) + 0.1 * rng.standard_normal((N, L))
    return data, (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def conditioned(result, err, ranks=None):
    """Is the order of `result` (from `explain`) decided by the arithmetic's margin: every gap between neighbours of the sorted
    |coef| (the first `ranks` neighbours, default all) is at least 100 x `err`, the measured difference of the two arithmetics
    compared.  A gap of exactly 0 between two coefficients that are exactly 0 is a structural tie (constant columns, or no
    response at all): both arithmetics compute those zeros exactly and the stable order decides, so it does not count."""
    for coef, order in zip(result["coef"], result["order"]):
        a = np.abs(coef[order])
        n = len(a) - 1 if ranks is None else min(ranks, len(a) - 1)
        for i in range(n):
            if a[i] == 0.0 and a[i + 1] == 0.0:
                continue
            if a[i] - a[i + 1] < 100.0 * err:
                return False
    return True


def golden_case(g, tag):
    """-> dict of a stored case: seg, image, data (N, D), labels (N, 10), top, hide (None or number), seed, and the reference's
    coef (5, D) indexed by feature next to its stored lists."""
    i, n, seed, hide = g[f"{tag}_params"].tolist()
    seg, image = g[f"in{int(i)}_seg"], g[f"in{int(i)}_image"]
    D, n = int(seg.max()) + 1, int(n)
    data = np.unpackbits(g[f"{tag}_data"])[:n * D].reshape(n, D).astype(np.int64)
    feats, wts = g[f"{tag}_features"].astype(np.int64), g[f"{tag}_weights"]
    coef = np.zeros(wts.shape)
    for l in range(len(wts)):
        coef[l, feats[l]] = wts[l]
    return dict(seg=seg, image=image, data=data, labels=g[f"{tag}_labels"], top=g[f"{tag}_top"].astype(np.int64), seed=int(seed),
                hide=None if np.isnan(hide) else hide, coef=coef, order=feats, N=n, D=D)
