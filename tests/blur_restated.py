"""K7 (csrc/blur_kernels.hip) restated on the host: the zero-padded separable cross-correlation in fp64, the forward error bound
of the kernel's fp32 arithmetic, and the inputs of the edge tests (tests/test_cpu_blur.py checks all of it without a GPU,
tests/test_gpu_blur_edges.py holds the kernels to it).

What K7 computes, per channel plane:  t[y, x] = sum_j k[j] * x[y, x + j - r]   (horizontal pass, zero outside the image)
                                      out[y, x] = sum_i k[i] * t[y + i - r, x] (vertical pass),  r = klen // 2
a cross-correlation (the taps are NOT flipped -- conv2d's meaning), each sum one chain of klen fp32 FMAs in ascending tap order
starting from +0.  K7 always uses one tap vector for both passes; the restatement takes two so that it knows its axes."""
import numpy as np

U = 2.0 ** -24            # unit round-off of fp32

# the matrix of tests/test_gpu_blur_edges.py: klen at 1, around 31 (the specialised form), at the largest length whose 32-row
# tile fits LDS (57), the first that does not (59) and the largest fused one (63); images smaller than the radius in either
# axis, H at both sides of the 16- and 32-row tile heights, W at both sides of the 64-column tile width
KLENS = (1, 3, 29, 31, 33, 57, 59, 63)
SHAPES = ((1, 1), (1, 130), (130, 1), (5, 7), (15, 63), (16, 64), (17, 65), (33, 129), (40, 52))
LONG_KLENS = (65, 67, 101)                     # K.blur_sep hands these to two blur_1d_kernel passes
LONG_SHAPES = ((40, 52), (17, 65))
PLANES = (2, 2)                                # images x channels of every cell: the plane offset is not zero
FORMS = ("sep", "two_pass")                    # K.blur_sep, and xai_blur_1d_f32 along W then along H


def cells():
    return [(k, s) for k in KLENS for s in SHAPES] + [(k, s) for k in LONG_KLENS for s in LONG_SHAPES]


def ledger_name(klen, shape, form):
    return f"blur_edges/{klen}/{shape[0]}x{shape[1]}/{form}"


def correlate(a, k, axis):
    """sum_j k[j] * a[.. p + j - r ..] along `axis`, zero outside, in a's dtype: explicit shifted sums, ascending j."""
    a = np.moveaxis(a, axis, -1)
    n, r = a.shape[-1], len(k) // 2
    out = np.zeros_like(a)
    for j in range(len(k)):
        s = j - r
        lo, hi = max(0, -s), min(n, n - s)
        if lo < hi:
            out[..., lo:hi] += k[j] * a[..., lo + s:hi + s]
    return np.moveaxis(out, -1, axis)


def blur64(x, k_h, k_v):
    """(..., H, W) -> the zero-padded cross-correlation in fp64: k_h along W first, then k_v along H."""
    t = correlate(np.asarray(x, np.float64), np.asarray(k_h, np.float64), -1)
    return correlate(t, np.asarray(k_v, np.float64), -2)


def bound(x, k):
    """Per-pixel bound on |K7(x, k) - blur64(x, k, k)|, derived and not measured.  A chain of n FMAs s_j = fl(k_j x_j + s_{j-1})
    from s = 0 returns sum_j k_j x_j (1 + th_j) with |th_j| <= g = n u / (1 - n u): term j goes through at most n roundings
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  So the horizontal pass is off by at most
    e1 = g (|k| *h |x|); the vertical pass runs on t^ with |t^| <= |t| + e1, adds g (|k| *v |t^|) of its own and carries the
    first pass's error through as |k| *v e1.  2 klen 2^-149 covers the roundings that land among the subnormals, where the
    relative model does not hold.  The same holds for a separate multiply and add per tap: the first add (to +0) is exact, so a
    term still sees at most n roundings."""
    x, k = np.asarray(x, np.float64), np.asarray(k, np.float64)
    ka, n = np.abs(k), len(k)
    g = n * U / (1 - n * U)
    e1 = g * correlate(np.abs(x), ka, -1)
    t_hat = np.abs(correlate(x, k, -1)) + e1
    e2 = g * correlate(t_hat, ka, -2) + correlate(e1, ka, -2)
    return e2 + 2 * n * 2.0 ** -149


def chain32(x, k):
    """The tap chains in numpy fp32 with a separate multiply and add per tap (two roundings where the kernel's FMA has one):
    never more accurate than K7, and inside bound() all the same -- the bound is checked on this before a kernel sees it."""
    x, k = np.asarray(x, np.float32), np.asarray(k, np.float32)
    return correlate(correlate(x, k, -1), k, -2)


def taps(klen, seed):
    """Random fp32 taps in [-1, 1] with |k| >= 2^-10 and no symmetry (klen > 1): reversing them, or running the passes along
    the wrong axes, changes the result.  The floor keeps every product of two taps a normal number."""
    rng = np.random.default_rng([seed, klen])
    while True:
        k = rng.uniform(-1, 1, klen).astype(np.float32)
        if (np.abs(k) >= 2.0 ** -10).all() and (klen == 1 or not np.array_equal(k, k[::-1])):
            return k


def normal_case(klen, shape, seed):
    """-> (N(0, 1) fp32 data of `shape`, taps(klen, seed)): the inputs of the bitwise and the bound comparisons."""
    rng = np.random.default_rng([seed, klen, *shape])
    return rng.standard_normal(shape).astype(np.float32), taps(klen, seed)


def exact_case(klen, shape, seed):
    """-> (x fp32, k fp32, the int64 correlation).  Integer data for which every partial sum of either pass is an integer below
    2^24 in magnitude: fp32 holds each exactly, so the result is the same in any order and with or without FMA, and the kernel
    must return it element for element.  The taps are klen distinct non-zero integers out of +-1 .. +-ceil(klen / 2), shuffled:
    signed and without symmetry (one tap cannot be asymmetric)."""
    rng = np.random.default_rng([seed, klen, *shape])
    m = (klen + 1) // 2
    pool = np.concatenate([np.arange(1, m + 1), -np.arange(1, m + 1)])
    while True:
        k = rng.permutation(pool)[:klen].astype(np.int64)
        if klen == 1 or not np.array_equal(k, k[::-1]):
            break
    x = rng.integers(-2, 3, size=shape).astype(np.int64)
    assert len(set(k.tolist())) == klen and (k != 0).all()
    assert klen == 1 or not np.array_equal(k, k[::-1])
    assert int(np.abs(k).sum()) ** 2 * int(np.abs(x).max(initial=0)) < 2 ** 24
    want = correlate(correlate(x, k, -1), k, -2)
    return x.astype(np.float32), k.astype(np.float32), want


def impulse_positions(H, W):
    """The four corners, both sides of the tile seams (rows 15 | 16 and 31 | 32, columns 63 | 64) where the image has them, and
    one pixel off both centre lines; no position twice."""
    at = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (15, 63), (16, 64), (31, 63), (32, 64), (H // 3, (2 * W) // 3)]
    seen = []
    for p in at:
        if p[0] < H and p[1] < W and p not in seen:
            seen.append(p)
    return seen


def impulse_response(k, H, W, py, px):
    """What a 1.0 at (py, px) of a zero (H, W) plane must give, to the bit: the horizontal chain leaves k[px - x + r] in row py
    (k * 1 + 0, then + 0 * k'), the vertical one rounds one product k[py - y + r] * k[px - x + r]; +0.0 outside the clipped
    klen x klen footprint (a chain that starts at +0 and adds -0 stays +0).  -> (fp32 plane, bool footprint)."""
    k = np.asarray(k, np.float32)
    r = len(k) // 2
    iy, ix = py - np.arange(H) + r, px - np.arange(W) + r
    in_y, in_x = (iy >= 0) & (iy < len(k)), (ix >= 0) & (ix < len(k))
    kv, kh = k[np.clip(iy, 0, len(k) - 1)], k[np.clip(ix, 0, len(k) - 1)]
    foot = in_y[:, None] & in_x[None, :]
    return np.where(foot, kv[:, None] * kh[None, :], np.float32(0)).astype(np.float32), foot
