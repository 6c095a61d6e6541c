"""Plain NumPy restatement of XRAI's segment handling and greedy loops (reference util/attribution_methods/XRAIBuilder.py:
_unpack_segs_to_masks :287-292, the dilation of :256-258, XRAI._xrai :649-711, _xrai_fast :745-789), the yardstick of the XRAI
tests wherever no fixture of the reference itself exists.

Two arithmetics for a gain: `np.float32` is the reference's own expression, attr[mask].mean() on the float32 attribution (with
it the restatement reproduces tests/golden/xrai.npz bit for bit); `np.float64` is what K30 states, float32(fp64 sum / count).
The two select the same masks wherever the margin between the winner and the best candidate with a DIFFERENT pixel set is far
above their difference; `xrai` measures both numbers (`margin`, `gain_err`) so that a test can hold its inputs to that.
"""
import numpy as np
from scipy import ndimage


def disk(r):
    """skimage.morphology.disk(r): the offsets with dx*dx + dy*dy <= r*r."""
    ax = np.arange(-r, r + 1)
    return (ax[:, None] ** 2 + ax[None, :] ** 2) <= r * r


def unpack(label_maps):
    """One boolean mask per integer in [min, max] of every label map, in order; absent labels give empty masks."""
    return [seg == l for seg in label_maps for l in range(int(seg.min()), int(seg.max()) + 1)]


def dilate(masks, r):
    """Binary dilation with disk(r), neighbours outside the image false (equal to skimage's reflecting border for this footprint)."""
    if not r:
        return [np.asarray(m, bool) for m in masks]
    fp = disk(r)
    return [ndimage.binary_dilation(m, structure=fp) for m in masks]


def pack_bits(masks, shape):
    """(M, ceil(H*W/64)) uint64: pixel p = y*W + x is bit p % 64 of word p // 64, the tail bits zero."""
    hw = shape[0] * shape[1]
    nw = (hw + 63) // 64
    out = np.zeros((len(masks), nw), np.uint64)
    for i, m in enumerate(masks):
        flat = np.zeros(nw * 64, np.uint8)
        flat[:hw] = np.asarray(m, bool).reshape(-1)
        out[i] = np.packbits(flat, bitorder="little").view(np.uint64)
    return out


def spans(bits):
    """(M, 2) int32: first and last non-empty word of every plane, (n_words, -1) for an empty one."""
    out = np.empty((len(bits), 2), np.int32)
    for i, b in enumerate(bits):
        nz = np.flatnonzero(b)
        out[i] = (nz[0], nz[-1]) if len(nz) else (bits.shape[1], -1)
    return out


def _gain(attr, attr64, sel, dtype):
    if dtype == np.float32:
        return attr[sel].mean()
    return np.float32(attr64[sel].sum() / np.count_nonzero(sel))


def _finish(attr, attr64, out, pixel_iter, keys, gains, dtype, extra):
    unc = pixel_iter < 0
    if unc.any():
        out[unc] = _gain(attr, attr64, unc, dtype)
    order = np.argsort(-np.asarray(gains, np.float32), kind="stable")
    ranks = np.zeros(attr.shape, dtype=int)
    for i, s in enumerate(order):
        ranks[pixel_iter == s] = i + 1
    if unc.any():
        ranks[unc] = len(order) + 1
    return dict(out=out, keys=np.asarray(keys, np.int32), gains=np.asarray(gains, np.float32), pixel_iter=pixel_iter, ranks=ranks,
                n_uncomputed=int(unc.sum()), **extra)


def xrai(attr, masks, area_threshold=1.0, min_pixel_diff=50, dtype=np.float64):
    """XRAI._xrai.  attr: (H, W) float32; masks: list of (H, W) bool.  -> dict: out (float64 array of float32 values), keys and gains
    in selection order, pixel_iter (the selection that covered a pixel, -1 uncomputed), ranks (the reference's integer segments),
    n_uncomputed, margin (smallest winner-minus-runner-up over the iterations, the runner-up being the best candidate whose
    remainder is a different pixel set; inf when there never was one) and gain_err (largest |float32 gain - fp64 gain| over every
    candidate evaluated).  Raises KeyError where the reference does (masks remain, none has a gain above -inf)."""
    assert min_pixel_diff >= 1
    attr = np.asarray(attr, np.float32)
    attr64 = attr.astype(np.float64)
    out = np.full(attr.shape, -np.inf)
    pixel_iter = np.full(attr.shape, -1, np.int32)
    current = np.zeros(attr.shape, bool)
    remaining = {k: np.asarray(m, bool) for k, m in enumerate(masks)}
    keys, gains = [], []
    margin, gain_err = np.inf, 0.0
    area = 0.0
    while area <= area_threshold:
        best_gain, best_key, cands = -np.inf, None, []
        for k in list(remaining):
            diff = remaining[k] & ~current
            if np.count_nonzero(diff) < min_pixel_diff:
                del remaining[k]
                continue
            g = _gain(attr, attr64, diff, dtype)
            g32, g64 = float(attr[diff].mean()), float(attr64[diff].sum() / np.count_nonzero(diff))
            gain_err = max(gain_err, abs(g32 - g64))
            cands.append((k, g64, diff))
            if g > best_gain:
                best_gain, best_key = g, k
        if not remaining:
            break
        if best_key is None:
            raise KeyError(best_key)
        win = next(c for c in cands if c[0] == best_key)
        others = [c[1] for c in cands if c[0] != best_key and not np.array_equal(c[2], win[2])]
        if others:
            margin = min(margin, win[1] - max(others))
        diff = win[2]
        out[diff] = best_gain
        pixel_iter[diff] = len(keys)
        keys.append(best_key)
        gains.append(best_gain)
        current |= remaining.pop(best_key)
        area = np.mean(current)
    return _finish(attr, attr64, out, pixel_iter, keys, gains, dtype, dict(margin=float(margin), gain_err=float(gain_err)))


def xrai_fast(attr, masks, min_pixel_diff=50, dtype=np.float64):
    """_xrai_fast: full-mask gains once (an empty mask: -inf), a stable sort by descending gain, one pass with the drop rule.
    margin: the smallest gap between two neighbours of the sorted order that are different pixel sets."""
    assert min_pixel_diff >= 1
    attr = np.asarray(attr, np.float32)
    attr64 = attr.astype(np.float64)
    masks = [np.asarray(m, bool) for m in masks]
    full = [(_gain(attr, attr64, m, dtype) if m.any() else -np.inf) for m in masks]
    full64 = [(attr64[m].sum() / np.count_nonzero(m) if m.any() else -np.inf) for m in masks]
    gain_err = max([abs(float(attr[m].mean()) - g) for m, g in zip(masks, full64) if m.any()], default=0.0)
    if any(g != g for g in full):
        raise ValueError("a NaN gain: the order of the reference's sort is undefined")
    order = sorted(range(len(masks)), key=lambda k: -full[k])
    o64 = sorted(range(len(masks)), key=lambda k: -full64[k])
    margin = np.inf
    for a, b in zip(o64, o64[1:]):
        if np.isfinite(full64[b]) and not np.array_equal(masks[a], masks[b]):
            margin = min(margin, full64[a] - full64[b])
    out = np.full(attr.shape, -np.inf)
    pixel_iter = np.full(attr.shape, -1, np.int32)
    current = np.zeros(attr.shape, bool)
    keys, gains = [], []
    for k in order:
        diff = masks[k] & ~current
        if np.count_nonzero(diff) < min_pixel_diff:
            continue
        g = _gain(attr, attr64, diff, dtype)
        gain_err = max(gain_err, abs(float(attr[diff].mean()) - float(attr64[diff].sum() / np.count_nonzero(diff))))
        out[diff] = g
        pixel_iter[diff] = len(keys)
        keys.append(k)
        gains.append(g)
        current |= masks[k]
    return _finish(attr, attr64, out, pixel_iter, keys, gains, dtype, dict(margin=float(margin), gain_err=float(gain_err)))


# ---- seeded inputs (the fixtures' generator and the GPU tests draw theirs from here) --------------------------------------
def voronoi_labels(H, W, n, rng):
    """(H, W) label map of the Voronoi cells of n random points, relabelled 0 .. cells - 1."""
    pts = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2
    _, lab = np.unique(d.argmin(-1), return_inverse=True)
    return lab.reshape(H, W).astype(np.int16)


def seeded_case(H, W, counts, seed, channels=3):
    """-> label maps (S, H, W) int16 at the granularities `counts`, and a smoothed (H, W, channels) float32 attribution."""
    rng = np.random.default_rng(seed)
    maps = np.stack([voronoi_labels(H, W, n, rng) for n in counts])
    attr = ndimage.gaussian_filter(rng.standard_normal((H, W, channels)), (3, 3, 0)).astype(np.float32)
    return maps, attr


def conditioned(res):
    """The condition every stored and seeded case is held to: the distinct-set margin is at least 100 times the largest
    difference between the reference's float32 gain and the fp64 gain of any candidate."""
    return res["margin"] >= 100.0 * res["gain_err"]
