"""NumPy restatement of include/xai_hip_slic.h: the k-means of scikit-image 0.18.3's SLIC in T = float32 or float64 with every
operation rounded once (THE K-MEANS CONTRACT) and the regular case of its connectivity pass (THE CONNECTIVITY CONTRACT).  What the
kernels K65 - K68 are held to bit for bit, and what tests/golden/make_golden_slic.py holds to skimage's binary.

centres are (S, 2 + C): (y, x, c_0 ..), skimage's `segments` without the z column."""
import numpy as np

UNCOVERED, EMPTY, IRREGULAR = 1, 2, 4
MAX_SWEEPS = 64


def bounds(c, two_step, n):
    """[lo, hi) of a window along an axis of n pixels, computed in the dtype of c; a NaN centre has the empty window"""
    T = type(c)
    if c != c:
        return 0, 0
    a = c - two_step
    a = a if a > T(0) else T(0)
    a = a if a < T(n) else T(n)
    b = (c + two_step) + T(1)
    b = b if b < T(n) else T(n)
    b = b if b > T(0) else T(0)
    return int(a), int(b)


def assign(feat, centres, step):
    """feat (H, W, C) T, centres (S, 2 + C) T -> (labels (H, W) int32 with -1 where no window holds the pixel, status)"""
    T = feat.dtype.type
    H, W, C = feat.shape
    step = T(step)
    sw = T(1) / (step * step)
    two_step = T(2) * step
    far = np.finfo(np.float64).max if T is np.float64 else np.inf
    dist = np.full((H, W), far, dtype=T)
    labels = np.full((H, W), -1, dtype=np.int32)
    yy, xx = np.arange(H, dtype=T), np.arange(W, dtype=T)
    with np.errstate(all="ignore"):
        for k in range(centres.shape[0]):
            cy, cx = centres[k, 0], centres[k, 1]
            y0, y1 = bounds(cy, two_step, H)
            x0, x1 = bounds(cx, two_step, W)
            if y0 >= y1 or x0 >= x1:
                continue
            dy = cy - yy[y0:y1]
            dx = cx - xx[x0:x1]
            d = ((dy * dy)[:, None] + (dx * dx)[None, :]) * sw
            dc = np.zeros((y1 - y0, x1 - x0), dtype=T)
            for c in range(C):
                q = feat[y0:y1, x0:x1, c] - centres[k, 2 + c]
                dc = dc + q * q
            d = d + dc
            sub = dist[y0:y1, x0:x1]
            m = sub > d
            sub[m] = d[m]
            labels[y0:y1, x0:x1][m] = k
    return labels, (UNCOVERED if (labels < 0).any() else 0)


def update(feat, labels, centres):
    """-> (the new centres, status): per cluster the sums of (y, x, features) over its pixels in raster order, sequentially from
    +0 in T (np.add.accumulate is that chain), then / T(count); 0 / 0 for a cluster without a pixel"""
    T = feat.dtype.type
    H, W, C = feat.shape
    flat = labels.ravel()
    ys, xs = np.divmod(np.arange(H * W), W)
    rows = np.concatenate([ys[:, None].astype(T), xs[:, None].astype(T), feat.reshape(-1, C)], axis=1)
    new = np.empty_like(centres)
    status = 0
    with np.errstate(all="ignore"):
        for k in range(centres.shape[0]):
            mine = rows[flat == k]
            n = mine.shape[0]
            if n == 0:
                status |= EMPTY
                acc = np.zeros(2 + C, dtype=T)
            else:
                acc = np.add.accumulate(np.concatenate([np.zeros((1, 2 + C), dtype=T), mine]), axis=0, dtype=T)[-1]
            new[k] = acc / T(n)
    return new, status


def kmeans(feat, centres, step, max_iter=10):
    """-> (labels of the last assignment, the centres after every iteration (max_iter, S, 2 + C), status)"""
    centres = np.array(centres, dtype=feat.dtype)
    trace, status = [], 0
    for _ in range(max_iter):
        labels, st = assign(feat, centres, step)
        status |= st
        centres, st = update(feat, labels, centres)
        status |= st
        trace.append(centres)
    return labels, np.stack(trace), status


def initial(centres_yx, C, dtype):
    """(S, 2) grid centres -> (S, 2 + C) with zero colour, as skimage starts"""
    out = np.zeros((len(centres_yx), 2 + C), dtype=dtype)
    out[:, :2] = centres_yx
    return out


def sweep(labels, src):
    """one sweep of K67: every pixel takes the least root among itself and its equal 4-neighbours, each root followed once; the
    two sides are separate arrays"""
    H, W = labels.shape
    flat = src.ravel()
    jump = flat[flat].reshape(H, W)
    best = jump.copy()
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        a = (slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0)))          # the neighbour
        p = (slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0)))      # the pixel
        same = labels[p] == labels[a]
        best[p] = np.where(same, np.minimum(best[p], jump[a]), best[p])
    return best


def components(labels, min_size, max_size):
    """-> (comp (H, W) int32: the least flat index of each pixel's 4-connected component of equal label, status, sweeps run).  With
    the sweeps run out: IRREGULAR and the array as it stands."""
    H, W = labels.shape
    src = np.arange(H * W, dtype=np.int32).reshape(H, W)
    for n in range(1, MAX_SWEEPS + 1):
        dst = sweep(labels, src)
        same = np.array_equal(dst, src)
        src = dst
        if same:
            break
    else:
        return src, IRREGULAR, MAX_SWEEPS
    sizes = np.bincount(src.ravel(), minlength=H * W)
    roots = np.flatnonzero(src.ravel() == np.arange(H * W))
    bad = ((sizes[roots] < min_size) | (sizes[roots] >= max_size)).any()
    return src, (IRREGULAR if bad else 0), n


def number(comp, start_label=0):
    """-> (start_label + the rank of a component's first pixel among all first pixels in raster order (H, W) int32, their count)"""
    flat = comp.ravel()
    first = flat == np.arange(flat.size)
    rank = np.cumsum(first) - 1
    return (start_label + rank[flat]).astype(np.int32).reshape(comp.shape), int(first.sum())


def slic(feat, centres_yx, step, max_iter, min_size, max_size, start_label=0):
    """the whole device call on one image -> (labels, count, status, final centres, raw labels)"""
    raw, trace, status = kmeans(feat, initial(centres_yx, feat.shape[2], feat.dtype), step, max_iter)
    comp, st, _ = components(raw, min_size, max_size)
    labels, count = number(comp, start_label)
    return labels, count, status | st, trace[-1], raw
