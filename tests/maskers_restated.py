"""K11-K14 and K16 (csrc/masker_kernels.hip) restated on the host in numpy fp32, every operation rounded on its own (the file
is built with -ffp-contract=off), with the matrices of cells and the inputs of the edge tests.  tests/test_cpu_maskers.py checks
all of it without a GPU, tests/test_gpu_masker_edges.py holds the kernels to it bit for bit.

K11 restates torch's non-antialiased fp32 bilinear formula (align_corners = False; aten's area_pixel_compute_source_index and
compute_source_index_and_lambda) and the reference's norm_matrix (ViT_CX.py:29-34) -- not the kernel source:
    ratio = f32(n_in) / f32(n_out);  f = max(ratio * (o + 0.5) - 0.5, 0);  i0 = int(f);  i1 = i0 + (i0 < n_in - 1)
    l1 = f - i0;  l0 = 1 - l1
    tmp[y][ox] = s[y][x0] * lx0 + s[y][x1] * lx1;  v[oy][ox] = tmp[y0][ox] * ly0 + tmp[y1][ox] * ly1
    out = (v - min v) / (max v - min v), the IEEE quotient
The reference itself resizes with antialias = True, which is this formula only when up-sampling (H >= h and W >= w); smaller
targets are refused by the entry point."""
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64

# ---- K11: (R, h, w, H, W) ------------------------------------------------------------------------------------------------------
K11_CELLS = (
    (3, 1, 1, 4, 4),             # constant map: all NaN, as in the reference
    (3, 1, 2, 1, 4),             # H = 1
    (5, 2, 2, 8, 8),             # Q = 16 < 256, dyadic
    (2, 6, 8, 6, 8),             # identity: equals rownorm of the input
    (3, 3, 5, 9, 7),             # scalar form, h*W = 21: the tap table is re-aligned
    (3, 3, 7, 30, 45),           # scalar form, W < 256
    (2, 7, 3, 5, 259),           # scalar form, W > 256 -- H < h: refused since the entry point takes up-sampling only
    (2, 5, 3, 7, 259),           # ... so the scalar form's second column pass runs here
    (2, 4, 4, 32, 12),           # W4 = 3
    (3, 14, 14, 28, 28),         # W4 = 7
    (2, 4, 4, 100, 12),          # W4 = 3 again with Q = 300 > 256: d_col = 1 is walked, which the two cells above never do
    (2, 14, 14, 56, 28),         # W4 = 7 with Q = 392: d_col = 4, the column wraps on the second step
    (2, 14, 14, 224, 224),       # the production shape
    (2, 8, 5, 16, 1024),         # W4 = 256, h*W = 8192
    (2, 7, 5, 9, 1028),          # W4 = 257, d_row = 0
    (1, 64, 64, 1024, 128),      # all three LDS limits at once: 16 416 B static + 49 152 B dynamic
)
K11_ALIGNMENT_CELLS = ((2, 4, 4, 32, 12), (2, 14, 14, 224, 224))       # run again with `out` 4 bytes off
K11_LIMITS = {"src": 4096, "stretch": 8192, "taps": 1024}              # h*w, h*W, H
# status -3 (XAI_E_UNSUPPORTED) and nothing written; the last two are new with the up-sampling-only rule
K11_REFUSED = {"h*w = 4097": (1, 1, 4097, 1, 4097), "h*W = 8193": (1, 3, 1, 3, 2731), "H = 1025": (1, 1, 1, 1025, 1),
               "H < h": (1, 4, 4, 2, 8), "W < w": (1, 4, 4, 8, 2)}


def k11_refuses(cell):
    _, h, w, H, W = cell
    return h * w > K11_LIMITS["src"] or h * W > K11_LIMITS["stretch"] or H > K11_LIMITS["taps"] or H < h or W < w


def k11_is_dyadic(cell):
    _, h, w, H, W = cell
    pow2 = lambda a, b: a % b == 0 and (a // b) & (a // b - 1) == 0           # noqa: E731
    return pow2(H, h) and pow2(W, w)


def k11_is_constant(cell):
    """Maps of one source pixel: every up-sampled value is that pixel, 0/0 in the reference and in the kernel."""
    return cell[1] * cell[2] == 1


def k11_name(cell):
    return "x".join(str(c) for c in cell)


def ledger_name(cell):
    return f"masker_edges/up_rownorm/{k11_name(cell)}"


def k11_maps(cell, kind="normal"):
    """(R, h, w) fp32.  "normal": N(0, 1) with another offset and scale per map, so that a map written to another map's rows
    shows.  "integer": integers in [-8, 8], min and max in another place per map -- with dyadic ratios every product and sum of
    the up-sampling is then exact."""
    R, h, w = cell[:3]
    rng = np.random.default_rng([11, *cell, kind == "integer"])
    if kind == "integer":
        return rng.integers(-8, 9, size=(R, h, w)).astype(F32)
    x = rng.standard_normal((R, h, w))
    return (x * (1.0 + 0.5 * np.arange(R))[:, None, None] + np.arange(R)[:, None, None]).astype(F32)


def taps(n_in, n_out):
    """-> i0, i1 (int), l0, l1 (fp32) per output index, each operation in fp32."""
    ratio = F32(n_in) / F32(n_out)
    o = np.arange(n_out, dtype=F32)
    f = np.maximum((ratio * (o + F32(0.5))).astype(F32) - F32(0.5), F32(0)).astype(F32)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (f - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def upsample(fmap, H, W):
    """(R, h, w) -> (R, H, W): horizontal pass, then vertical pass; product, product, sum, each rounded to fp32."""
    s = np.asarray(fmap, F32)
    x0, x1, lx0, lx1 = taps(s.shape[2], W)
    y0, y1, ly0, ly1 = taps(s.shape[1], H)
    tmp = ((s[:, :, x0] * lx0).astype(F32) + (s[:, :, x1] * lx1).astype(F32)).astype(F32)
    return ((tmp[:, y0, :] * ly0[:, None]).astype(F32) + (tmp[:, y1, :] * ly1[:, None]).astype(F32)).astype(F32)


def up_rownorm(fmap, H, W):
    """K11: (R, h, w) -> (R, H*W)."""
    return rownorm(upsample(fmap, H, W).reshape(len(fmap), H * W))


def taps_exact(n_in, n_out):
    """The tap formula in rationals (ratio = n_in / n_out exactly)."""
    out = []
    for o in range(n_out):
        f = max(Fraction(n_in, n_out) * (Fraction(o) + Fraction(1, 2)) - Fraction(1, 2), Fraction(0))
        i0 = int(f)
        out.append((i0, i0 + (i0 < n_in - 1), 1 - (f - i0), f - i0))
    return out


def upsample_exact(fmap, H, W):
    """upsample() in rationals, as an object array of Fractions: no rounding anywhere, and written as the textbook sum of four
    weighted corners, not as two passes."""
    s = np.asarray(fmap, F32)
    R, h, w = s.shape
    sf = np.array([Fraction(float(v)) for v in s.ravel()], dtype=object).reshape(R, h, w)
    ty, tx = taps_exact(h, H), taps_exact(w, W)
    out = np.empty((R, H, W), dtype=object)
    for oy, (y0, y1, ly0, ly1) in enumerate(ty):
        for ox, (x0, x1, lx0, lx1) in enumerate(tx):
            out[:, oy, ox] = (sf[:, y0, x0] * (ly0 * lx0) + sf[:, y0, x1] * (ly0 * lx1)
                              + sf[:, y1, x0] * (ly1 * lx0) + sf[:, y1, x1] * (ly1 * lx1))
    return out


# ---- K12: (R, P) ---------------------------------------------------------------------------------------------------------------
K12_CELLS = ((1, 1), (1, 2), (9, 1000), (3, 4100), (3, 4099), (8, 1028), (17, 2049), (2, 40000), (600, 2052))
K12_MAX_SLICES, K12_BLOCK = 32, 256


def rownorm(x):
    """K12 (and K11's second half): (x - lo) / (hi - lo) per row, lo / hi with fminf / fmaxf semantics."""
    x = np.asarray(x, F32)
    lo = np.fmin.reduce(x, axis=1, keepdims=True)
    hi = np.fmax.reduce(x, axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((x - lo).astype(F32) / (hi - lo).astype(F32)).astype(F32)


def k12_slices(R, P, cus):
    """Workgroups per row of an out-of-place call: enough for two workgroups per compute unit, at least 4 elements per lane and
    slice, at most 32 (the rule of xai_rownorm_f32's comment; an in-place call has one)."""
    want, most = -(-2 * cus // R), -(-P // (4 * K12_BLOCK))
    return max(1, min(want, most, K12_MAX_SLICES))


def k12_seams(P, slices, vec):
    """-> (first element of every slice after the first, elements of the last slice, elements of a full slice)."""
    n = P // 4 if vec else P
    per = -(-n // slices)
    unit = 4 if vec else 1
    return [unit * per * s for s in range(1, slices) if per * s < n], unit * (n - per * (slices - 1)), unit * per


def k12_positions(P, seams):
    """Where a row's min and max are put in turn: first, last, inside the last float4, both sides of every slice seam."""
    at = [0, P - 1, P - 3]
    for s in seams:
        at += [s - 1, s]
    seen = []
    for p in at:
        if 0 <= p < P and p not in seen:
            seen.append(p)
    return seen


def k12_special_rows(R):
    """-> (row holding +-inf or None, row whose min is -0.0 or None): the last rows of a cell with rows to spare."""
    if R >= 3:
        return R - 1, R - 2
    return None, (1 if R == 2 else None)


def k12_rounds(R, P, seams):
    inf_row, zero_row = k12_special_rows(R)
    plain = R - (inf_row is not None) - (zero_row is not None)
    return -(-len(k12_positions(P, seams)) // plain) if P > 2 else 1


def k12_rows(R, P, seams, rnd):
    """Round `rnd` of a cell: U(-1, 1) rows with another scale per row; plain row i holds its min at position (rnd * plain + i)
    of k12_positions and its max half the list further on; one row holds +inf and -inf (inf - inf and inf / inf: all NaN), one
    has -0.0 as its only zero and its minimum (x - (-0.0) = x, and -0.0 - (-0.0) = +0.0)."""
    rng = np.random.default_rng([12, R, P, rnd])
    x = (rng.uniform(-1, 1, (R, P)) * (1.0 + 0.25 * (np.arange(R) % 7))[:, None]).astype(F32)
    inf_row, zero_row = k12_special_rows(R)
    at = k12_positions(P, seams)
    i = 0
    for r in range(R):
        if r == inf_row:
            x[r, P // 3], x[r, (2 * P) // 3] = np.inf, -np.inf
        elif r == zero_row:
            x[r] = np.abs(x[r]) + F32(0.125)
            x[r, P // 2] = -0.0
        elif P > 2:
            k = (rnd * (R - (inf_row is not None) - (zero_row is not None)) + i) % len(at)
            x[r, at[k]] = -4.0 - 0.5 * (r % 5)
            x[r, at[(k + len(at) // 2) % len(at)]] = 4.0 + 0.25 * (r % 3)
            i += 1
    return x


# ---- K13 -----------------------------------------------------------------------------------------------------------------------
K13_PS = (4, 1023, 1024, 1028)
K13_ROWS = 12
# one singleton, one empty cluster (offs[k] == offs[k + 1]), one holding most rows and not contiguous, one pair
K13_MEMBERS = np.array([5, 0, 2, 3, 6, 7, 9, 10, 11, 1, 8], np.int32)
K13_OFFS = np.array([0, 1, 1, 9, 11], np.int32)


def k13_rows(P):
    """Magnitudes 1e8, 1, -1e8, ... down the rows, shifted along the columns: 1e8 + 1 - 1e8 is 0 in fp32 and 1 in another order."""
    rng = np.random.default_rng([13, P])
    mag = np.array([1e8, 1.0, -1e8, 3.0, 1e-3, -1e8, 7.0, 1e8, -1.0, 1e4, -1e4, 0.5])
    x = mag[(np.arange(K13_ROWS)[:, None] + np.arange(P)[None, :]) % len(mag)] * rng.uniform(1.0, 1.5, (K13_ROWS, P))
    return x.astype(F32)


def cluster_sum(rows, members, offs):
    """K13: sequential fp32 += in member order, from +0."""
    rows = np.asarray(rows, F32)
    out = np.zeros((len(offs) - 1, rows.shape[1]), F32)
    for k in range(len(offs) - 1):
        for m in members[offs[k]:offs[k + 1]]:
            out[k] += rows[m]
    return out


# ---- K14: (N, C, HW) -----------------------------------------------------------------------------------------------------------
K14_CELLS = ((1, 1, 1), (2, 3, 4), (3, 3, 1023), (3, 3, 1024), (2, 3, 1028), (9, 3, 1350), (2, 4, 1028))
K14_MISALIGNED_CELL = (2, 3, 1028)
K14_SCALES = (0.1, 0.0, -0.25)


def k14_case(cell):
    """-> x (C, HW), masks (N, HW), noise (N, C, HW): masks in [-0.25, 1.25] with exact 0 and exact 1 among them."""
    N, C, HW = cell
    rng = np.random.default_rng([14, *cell])
    x = rng.standard_normal((C, HW)).astype(F32)
    m = rng.uniform(-0.25, 1.25, (N, HW)).astype(F32)
    m.reshape(-1)[::5] = 0.0
    m.reshape(-1)[2::7] = 1.0
    noise = rng.standard_normal((N, C, HW)).astype(F32)
    while N * C * HW == 1 and not all(k14_contraction_sensitive(x, m, noise, s) for s in K14_SCALES if s):
        x, noise = rng.standard_normal((C, HW)).astype(F32), rng.standard_normal((N, C, HW)).astype(F32)
        m = rng.uniform(0.25, 0.75, (N, HW)).astype(F32)       # the one element must itself tell x * m + add from an fma
    return x, m, noise


def causal_stack(x, masks, noise, noise_scale):
    """K14: oracle.vit_cx.causal_stack with any noise_scale; x (C, HW), masks (N, HW), noise (N, C, HW) -> (2N, C, HW)."""
    x, m = np.asarray(x, F32), np.asarray(masks, F32)[:, None, :]
    inv = (F32(1) - m).astype(F32)
    add = ((np.asarray(noise, F32) * F32(noise_scale)).astype(F32) * inv).astype(F32)
    masked = ((x[None] * m).astype(F32) + add).astype(F32)
    return np.concatenate([masked, (x[None] + add).astype(F32)], axis=0)


def k14_contraction_sensitive(x, masks, noise, noise_scale):
    """How many elements of the masked half have fl(fl(x m) + add) != fma(x, m, add): what a bit comparison needs to see a
    contracted multiply-add (at noise_scale 0 add is +-0 and there are none)."""
    x, m = np.asarray(x, F32), np.asarray(masks, F32)[:, None, :]
    add = ((np.asarray(noise, F32) * F32(noise_scale)).astype(F32) * (F32(1) - m).astype(F32)).astype(F32)
    two = ((x[None] * m).astype(F32) + add).astype(F32)
    return int((two.view(np.int32) != fma32(x[None], m, add).view(np.int32)).sum())


# ---- K16 -----------------------------------------------------------------------------------------------------------------------
K16_NS, K16_PS = (1, 7, 8, 9, 16, 17), (4, 1023, 1028)


def k16_case(N, P):
    """-> rows (N, P), weights (N,); drawn again until a chain of FMAs would give other bits (four elements may not on the
    first draw; one row never does: fl(v w) + 0 is the FMA)."""
    rng = np.random.default_rng([16, N, P])
    while True:
        rows = (rng.random((N, P)) * (1.0 + np.arange(N))[:, None]).astype(F32)
        w = rng.standard_normal(N).astype(F32)
        if N == 1 or (masked_sums(rows, w)[0].view(np.int32) != masked_sums(rows, w, fused=True)[0].view(np.int32)).any():
            return rows, w


def masked_sums(rows, w, fused=False):
    """K16: n ascending, the product rounded before the add (fused=True: one rounding, what a contraction would give)."""
    rows, w = np.asarray(rows, F32), np.asarray(w, F32)
    aw, ap = np.zeros(rows.shape[1], F32), np.zeros(rows.shape[1], F32)
    for n in range(len(rows)):
        aw = fma32(rows[n], w[n], aw) if fused else (aw + (rows[n] * w[n]).astype(F32)).astype(F32)
        ap = (ap + rows[n]).astype(F32)
    return (aw / F32(len(rows))).astype(F32), (ap / F32(len(rows))).astype(F32)


# ---- exact fp32 arithmetic: one rounding of a rational, fma, K11's division ----------------------------------------------------
def rn32(x):
    """A Fraction rounded to the nearest fp32 (ties to even, subnormals included); no overflow."""
    x = Fraction(x)
    if x == 0:
        return F32(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = round(a / quantum)                                      # Python rounds a Fraction half to even
    r = F32(float(n * quantum))                                 # 25 bits at most: exact in a double, and then in fp32
    assert np.isfinite(r)
    return -r if x < 0 else r


def fma32(a, b, c):
    """RN32(a * b + c) with one rounding, element-wise on finite fp32 arrays.  a * b is exact in fp64 (48 bits); the fp64 sum
    s = RN64(a b + c) rounds to fp32 as the exact sum does unless s lies exactly half-way between two fp32 numbers while the
    exact sum does not (TwoSum's error term is non-zero) -- those elements are redone in rationals."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p, c64 = a.astype(F64) * b.astype(F64), c.astype(F64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    with np.errstate(over="raise"):
        r = s.astype(F32)
    back = r.astype(F64)
    other = np.nextafter(r, np.where(s > back, F32(np.inf), F32(-np.inf)).astype(F32)).astype(F64)
    redo = (s != back) & (np.abs(s - back) == np.abs(other - s)) & (err != 0)
    r = np.array(r)
    for i in np.argwhere(redo):
        i = tuple(i)
        r[i] = rn32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def div_by_model(num, span):
    """K11's div_by, each of its three roundings applied to the exact value: y = RN(1 / span), q = RN(num y),
    r = RN(num - q span) (fma), RN(q + r y) (fma)."""
    num, span = np.asarray(num, F32), np.asarray(span, F32)
    y = (F32(1) / span).astype(F32)
    q = (num * y).astype(F32)
    r = fma32(-q, span, num)
    return fma32(r, y, q)


def div_by_exact(num, span):
    """The same for one pair of scalars, in rationals throughout (what div_by_model is checked against)."""
    fn, fs = Fraction(float(num)), Fraction(float(span))
    y = Fraction(float(rn32(1 / fs)))
    q = Fraction(float(rn32(fn * y)))
    r = Fraction(float(rn32(fn - q * fs)))
    return rn32(q + r * y)


def div_by_cases(seed=7, random_per_scale=4000):
    """-> (num, span) fp32 with 0 <= num <= span.  Spans: significands all ones and all ones less 1 .. 4 ulps, 1.0 (powers of
    two) and 1.0 plus 1 .. 4 ulps, and random ones, at exponents -10 .. 3 and again scaled by 2^60 and 2^-60; per span num =
    span, nextafter(span, 0), 0, span / 2, the neighbours of span / 2, significands near all ones below span, and random draws."""
    rng = np.random.default_rng(seed)
    ones = np.uint32(0x7FFFFF)
    sig = [ones - np.uint32(k) for k in range(5)] + [np.uint32(k) for k in range(5)]
    spans = []
    for e in range(-10, 4):
        base = np.uint32((127 + e) << 23)
        spans += [(base | s) for s in sig]
        spans += [(base | np.uint32(s)) for s in rng.integers(0, 1 << 23, 6)]
    spans = np.array(spans, np.uint32).view(F32)
    spans = np.concatenate([spans, spans * F32(2.0 ** 60), spans * F32(2.0 ** -60)])
    nums, dens = [], []
    for s in spans:
        half = F32(s / 2)
        mine = [s, np.nextafter(s, F32(0)), F32(0), half, np.nextafter(half, F32(0)), np.nextafter(half, s)]
        top = (s.view(np.uint32) & np.uint32(0xFF800000))
        for k in range(4):                                   # significands all ones (less k ulps) one and two binades below span
            for down in (1, 2):
                mine.append(np.uint32((top - np.uint32(down << 23)) | (ones - np.uint32(k))).view(F32))
        mine += list((rng.random(12) * float(s)).astype(F32))
        nums += mine
        dens += [s] * len(mine)
    for scale in (1.0, 2.0 ** 60, 2.0 ** -60):
        s = (rng.uniform(1e-3, 16, random_per_scale)).astype(F32)
        n = (rng.random(random_per_scale) * s).astype(F32)
        nums += list(n * F32(scale))
        dens += list(s * F32(scale))
    num, span = np.array(nums, F32), np.array(dens, F32)
    assert ((num >= 0) & (num <= span)).all() and np.isfinite(span).all() and (span > 0).all()
    return num, span
