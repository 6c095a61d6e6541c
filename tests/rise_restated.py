"""K4 / K5 (csrc/rise_kernels.hip) restated on the host in numpy, with the host code's dispatch and launch plans, the derived
bounds and the matrix of cells of the edge tests.  tests/test_cpu_rise.py checks all of it without a GPU,
tests/test_gpu_rise_edges.py holds the kernels to it.

What the kernel file promises (its header, and -ffp-contract=off in the Makefile) and this module restates:
    ratio = f64(s) / f64(up);  c = |(j + 0.5) * ratio - 0.5|;  i0 = floor(c);  i1 = i0 + 1, mirrored about s - 1, at least 0
    t = f32(c - i0): the tap in fp64, rounded once
    wr0 = 1 - tr, wr1 = tr, wc0 = 1 - tc, wc1 = tc                                   (fp32)
    v = [g00] wr0 wc0;  v += [g01] wr0 wc1;  v += [g10] wr1 wc0;  v += [g11] wr1 wc1   (every product and sum rounded to fp32)
    mask = min(max(v, lo), hi), lo / hi the smallest / largest value of the mask's own grid
    masked = image * mask (one fp32 product);  acc += scale * sum_n f64(score_n) * f64(mask_n), n ascending within a slice"""
import numpy as np

F32, F64 = np.float32, np.float64
U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoffs
BLOCK, STAGE_MAX, LDS_BYTES, TAP_BYTES = 256, 256, 64 * 1024, 12
MAX_S, MAX_MASKS = 64, 65535
NT_BYTES = 128 << 20                       # K4, s == 8: outputs above this go out with non-temporal stores


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------

def taps(n_in, n_out):
    """make_tap for every output index of an n_in -> n_out up-sampling: i0, i1 (int64), t (fp32)."""
    ratio = F64(n_in) / F64(n_out)
    j = np.arange(n_out, dtype=F64)
    c = (j + F64(0.5)) * ratio - F64(0.5)
    c = np.where(c < 0, -c, c)                              # mirror about sample 0
    i0 = np.floor(c).astype(np.int64)
    i1 = i0 + 1
    i1 = np.where(i1 >= n_in, 2 * n_in - 2 - i1, i1)        # mirror about sample n_in - 1
    i1 = np.maximum(i1, 0)                                  # n_in == 1
    return i0, i1, (c - i0.astype(F64)).astype(F32)


def upsampled32(grid, cell):
    """The whole (s + 1) * cell up-sampling of one s x s grid as the kernels form each of its pixels."""
    g = np.asarray(grid) != 0
    s = g.shape[0]
    r0, r1, tr = taps(s, (s + 1) * int(cell[0]))
    c0, c1, tc = taps(s, (s + 1) * int(cell[1]))
    wr0, wr1 = (F32(1) - tr).astype(F32)[:, None], tr[:, None]
    wc0, wc1 = (F32(1) - tc).astype(F32)[None, :], tc[None, :]
    zero = F32(0)
    v = np.where(g[r0][:, c0], (wr0 * wc0).astype(F32), zero)
    v = (v + np.where(g[r0][:, c1], (wr0 * wc1).astype(F32), zero)).astype(F32)
    v = (v + np.where(g[r1][:, c0], (wr1 * wc0).astype(F32), zero)).astype(F32)
    v = (v + np.where(g[r1][:, c1], (wr1 * wc1).astype(F32), zero)).astype(F32)
    lo, hi = F32(0 if (~g).any() else 1), F32(1 if g.any() else 0)
    return np.minimum(np.maximum(v, lo), hi).astype(F32)


def raw_blend32(grid, cell):
    """upsampled32 without the clip: what all-one grids need the clip for."""
    g = np.asarray(grid) != 0
    s = g.shape[0]
    r0, r1, tr = taps(s, (s + 1) * int(cell[0]))
    c0, c1, tc = taps(s, (s + 1) * int(cell[1]))
    wr0, wr1 = (F32(1) - tr).astype(F32)[:, None], tr[:, None]
    wc0, wc1 = (F32(1) - tc).astype(F32)[None, :], tc[None, :]
    v = np.where(g[r0][:, c0], (wr0 * wc0).astype(F32), F32(0))
    for rows, cols, w in ((r0, c1, wr0 * wc1), (r1, c0, wr1 * wc0), (r1, c1, wr1 * wc1)):
        v = (v + np.where(g[rows][:, cols], w.astype(F32), F32(0))).astype(F32)
    return v


def mask32(grid, shift, cell, H, W):
    """One mask: the crop of the up-sampling at (shift[0], shift[1])."""
    up = upsampled32(grid, cell)
    y, x = int(shift[0]), int(shift[1])
    assert 0 <= y and y + H <= up.shape[0] and 0 <= x and x + W <= up.shape[1]
    return up[y:y + H, x:x + W]


def masks32(grid, shifts, cell, H, W):
    """(N, H, W): mask32 per mask; masks that repeat a (grid, shift) pair are formed once."""
    grid, shifts = np.asarray(grid, np.uint8), np.asarray(shifts, np.int32)
    keys = np.concatenate([grid.reshape(len(grid), -1), shifts.view(np.uint8).reshape(len(grid), -1)], axis=1)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    ups = {}
    uniq = np.empty((len(first), H, W), F32)
    for k, n in enumerate(first):
        gb = grid[n].tobytes()
        if gb not in ups:
            ups[gb] = upsampled32(grid[n], cell)
        y, x = int(shifts[n, 0]), int(shifts[n, 1])
        uniq[k] = ups[gb][y:y + H, x:x + W]
    return uniq[np.asarray(inverse).ravel()]


def accum64(grid, shifts, scores, cell, H, W, scale, acc0=None, rows=None):
    """K5 with one slice: sum_n f64(score_n) * f64(mask_n) in ascending n from +0, times scale, added to acc0.
    rows: restrict to these pixel rows (the result has len(rows) rows)."""
    scores = np.asarray(scores, F32)
    pick = slice(None) if rows is None else np.asarray(rows)
    acc = np.zeros((H, W), F64)[pick]
    ups = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(len(scores)):
            gb = np.asarray(grid[n], np.uint8).tobytes()
            if gb not in ups:
                if len(ups) > 64:
                    ups.clear()
                ups[gb] = upsampled32(grid[n], cell)
            y, x = int(shifts[n][0]), int(shifts[n][1])
            acc += F64(scores[n]) * ups[gb][y:y + H, x:x + W][pick].astype(F64)
        out = acc * F64(scale)
        return out if acc0 is None else np.asarray(acc0, F64)[pick] + out


def accum_magnitude(grid, shifts, scores, cell, H, W, scale, rows=None):
    """scale * sum_n |score_n| * mask_n per pixel: what the K5 bound is relative to."""
    return accum64(grid, shifts, np.abs(np.asarray(scores, F32)), cell, H, W, abs(scale), rows=rows)


def accum_bound(n_masks, magnitude):
    """|K5 - accum64| <= (n_masks + 2) * 2^-53 * magnitude per pixel, magnitude = accum_magnitude(...), acc carried in as 0.

    Every product f64(score) * f64(mask) is exact: two 24-bit significands give at most 48 bits.  K5 then adds the n products of
    a pixel with n - 1 fp64 additions in some order (sequentially inside a slice, the slices by atomics in any order; the first
    addition onto +0 is exact) and multiplies by scale once: every term passes through at most n - 1 + 1 roundings, each
    (1 + d) with |d| <= u = 2^-53, so K5 is within ((1 + u)^n - 1) <= (n + 1) u of the exact sum, relative to
    scale * sum |score_n| mask_n (n u << 1: the second-order part is below u for n <= 65 535, which makes it n + 2).  That is
    the stated condition.  accum64 is itself such a sum and carries the same kind of error, so against accum64 the worst case
    over all data is twice that; what makes n + 2 sound for the cells of this module is the running-error bound below, which
    tests/test_cpu_rise.py evaluates for every bounded cell: it stays below (n + 2) u everywhere, because the partial sums of
    scores spread over the masks are far below the final magnitude for most of the run."""
    return (n_masks + 2) * U64 * np.asarray(magnitude, F64)


def running_error(grid, shifts, scores, cell, H, W, scale, plan, rows=None):
    """A rigorous first-order bound on |K5 - accum64| per pixel for the slice plan `plan`, from the data alone: an fp64 addition
    errs by at most u |its result|, so a sequential sum errs by at most u * (sum of the absolute partial sums after the first);
    accum64 is one such run over all n, K5 one per slice; each product by scale adds u |result|; merging J slices onto +0 by
    atomics in any order adds at most (J - 1) u * sum_j |slice_j| * scale.  Partial sums are bounded by the partial sums of
    |score_n| mask_n, which is what is accumulated here (times 1 + 2^-40 for the second-order terms).  A plan of one slice runs
    accum64's own operations in accum64's order: no difference at all."""
    if plan["slices"] == 1:
        return np.zeros((H, W))[slice(None) if rows is None else np.asarray(rows)]
    scores = np.abs(np.asarray(scores, F32)).astype(F64)
    pick = slice(None) if rows is None else np.asarray(rows)
    shape = np.zeros((H, W))[pick].shape
    seq, seq_err = np.zeros(shape), np.zeros(shape)
    sl, sl_err, merged = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    per, ups = plan["per_slice"], {}
    for n in range(len(scores)):
        gb = np.asarray(grid[n], np.uint8).tobytes()
        if gb not in ups:
            if len(ups) > 64:
                ups.clear()
            ups[gb] = upsampled32(grid[n], cell)
        y, x = int(shifts[n][0]), int(shifts[n][1])
        t = scores[n] * ups[gb][y:y + H, x:x + W][pick].astype(F64)
        seq += t
        if n > 0:
            seq_err += seq
        if n % per == 0:
            merged += sl
            sl = np.zeros(shape)
        sl += t
        if n % per:
            sl_err += sl
    merged += sl
    total = seq_err + seq + sl_err + merged + (plan["slices"] - 1) * merged        # + seq, + merged: the products by scale
    return U64 * abs(scale) * total * (1 + 2.0 ** -40)


# |mask32 - oracle.rise.upsample_grid| on grids of 0 and 1.  With u = 2^-24 (fp32 numbers below 1 are spaced 2^-24 or closer, so
# rounding a value below 1 errs by at most u / 2; between 1 and 2 by at most u):
#   t = f32(c - i0) with 0 <= t < 1:            |t - tau| <= u / 2      (tau the real tap; c's own fp64 error, about s * 2^-53, below)
#   1 - t, rounded, in (0, 1]:                  |w0 - (1 - tau)| <= u / 2 + u / 2 = u
#   the four products of exact weights sum to at most 1; with the computed weights, the sum over the corners of
#   |e_r| w_c + |e_c| w_r is at most e_r0 + e_r1 + e_c0 + e_c1 = u + u / 2 + u + u / 2 = 3 u       (first order)
#   four products, each below 1 or exactly 1, each rounded:                       4 * u / 2 = 2 u
#   three additions with results below 2:                                         3 * u
#   the clip to [lo, hi] moves a value only towards the real value, which lies in [lo, hi]
#   scipy's zoom works in fp64 and rounds its result once to fp32:                u / 2
# together 8.5 u; 2^-40 covers the second-order products of these errors and the fp64 roundings of c on both sides.
ORACLE_BOUND = 8.5 * U32 + 2.0 ** -40


# ---- the host code's decisions ---------------------------------------------------------------------------------------------------

def cell_of(H, W, s):
    return (-(-H // s), -(-W // s))


def apply_path(s, W, aligned16=True, grid_aligned8=True):
    """xai_rise_apply_f32's choice: "s8" (no LDS, 4 pixels a lane), "v4" (4 pixels a lane, grid in LDS) or "scalar"."""
    vec = W % 4 == 0 and aligned16
    if vec and s == 8 and grid_aligned8:
        return "s8"
    return "v4" if vec else "scalar"


def apply_flavour(n_masks, C, H, W, masked, masks):
    """(NT, C3) of rise_apply_kernel_s8 for a call."""
    out_bytes = n_masks * H * W * 4 * ((C if masked else 0) + (1 if masks else 0))
    return out_bytes > NT_BYTES, C == 3


def accum_kernel(s, grid_aligned8=True):
    return "s8" if s == 8 and grid_aligned8 else "generic"


def accum_stage(s, cell, kernel=None):
    """Masks staged in LDS per round: 256 for the s == 8 kernel; for the generic one what 64 KiB hold next to the tap tables at
    20 + s * s bytes a mask, 256 at most.  0: even one does not fit (XAI_E_UNSUPPORTED)."""
    tap_bytes = (s + 1) * (int(cell[0]) + int(cell[1])) * TAP_BYTES
    if (kernel or accum_kernel(s)) == "s8":
        return STAGE_MAX if STAGE_MAX * 16 + tap_bytes <= LDS_BYTES else 0
    room = max(0, LDS_BYTES - tap_bytes)
    return min(STAGE_MAX, room // (20 + s * s))


def accum_plan(n_masks, H, W, stage=STAGE_MAX):
    """xai_rise_accum_f64's launch plan: slices, per_slice, last_slice (masks in the last slice), rounds (staging rounds of a
    full slice), last_round (masks in the last round of the last slice)."""
    tiles = -(-H * W // BLOCK)
    slices = max(1, min(-(-n_masks // 64), -(-2048 // tiles)))
    per = -(-n_masks // slices)
    slices = -(-n_masks // per)
    last = n_masks - per * (slices - 1)
    return {"slices": slices, "per_slice": per, "last_slice": last, "rounds": -(-per // stage),
            "last_round": last - stage * ((last - 1) // stage), "stage": stage}


# ---- the matrix ------------------------------------------------------------------------------------------------------------------

# K4: (H, W, s)
K4_CELLS = (
    (8, 8, 8),            # cell 1: less than one workgroup
    (32, 32, 8),          # exactly one workgroup of 4-pixel lanes; H % s == 0
    (36, 52, 8),          # cells (5, 7); ragged last workgroup
    (5, 12, 8),           # H < s
    (30, 45, 7),          # scalar kernel
    (33, 36, 8),          # with cell (4, 5): H = s * cell_h + 1, the crop reaches the last up-sampled row
    (9, 12, 2),
    (5, 9, 1),            # n_in == 1
    (40, 36, 17),         # s * s > 256: the strided staging loop
    (64, 128, 64),        # the largest s
    (16, 25, 8),          # s == 8 with odd W: scalar kernel; with cell (2, 3): W = s * cell_w + 1, the last up-sampled column
)
# With cell = ceil(H / s), what the reference draws, H <= s * cell and the last row a crop reads is H - 1 + cell - 1 <= up_h - 2:
# row up_h - 1 is read only when the caller passes a smaller cell with H = s * cell + 1, the largest H the entry points accept
# (H + cell - 1 <= (s + 1) * cell).  Two cells do.
K4_CELL_OVERRIDE = {(33, 36, 8): (4, 5), (16, 25, 8): (2, 3)}
K4_CHANNELS = (1, 3, 4)
GRID_FAMILIES = ("zero", "one", "impulse00", "impulse0e", "impulsee0", "impulseee", "impulsemid", "hole", "checker",
                 "p0.1", "p0.5", "p0.9")
N_SHIFTS = 5              # the four extremes and one random shift per grid


def family_grid(family, s, seed=0):
    g = np.zeros((s, s), np.uint8)
    e, m = s - 1, s // 2
    if family == "one":
        g[:] = 1
    elif family.startswith("impulse"):
        g[{"00": (0, 0), "0e": (0, e), "e0": (e, 0), "ee": (e, e), "mid": (m, m)}[family[7:]]] = 1
    elif family == "hole":
        g[:] = 1
        g[m, (m + 1) % s] = 0
    elif family == "checker":
        g[:] = (np.add.outer(np.arange(s), np.arange(s)) % 2).astype(np.uint8)
    elif family.startswith("p"):
        rng = np.random.default_rng([4, s, seed, int(float(family[1:]) * 10)])
        g[:] = rng.random((s, s)) < float(family[1:])
    return g


def k4_cell(cell3):
    return K4_CELL_OVERRIDE.get(tuple(cell3), cell_of(*cell3))


def k4_case(cell3):
    """-> grid (N, s, s) uint8, shifts (N, 2) int32, cell: every grid family at the four extreme shifts and a random one."""
    H, W, s = cell3
    cell = k4_cell(cell3)
    rng = np.random.default_rng([4, H, W, s])
    grids, shifts = [], []
    for f in GRID_FAMILIES:
        for k in range(N_SHIFTS):
            grids.append(family_grid(f, s, seed=k))
            if k < 4:
                shifts.append(((cell[0] - 1) * (k >> 1), (cell[1] - 1) * (k & 1)))
            else:
                shifts.append((int(rng.integers(0, cell[0])), int(rng.integers(0, cell[1]))))
    return np.stack(grids), np.array(shifts, np.int32), cell


def k4_image(C, H, W):
    return np.random.default_rng([44, C, H, W]).standard_normal((C, H, W)).astype(F32)


def k4_name(cell3):
    return "{}x{}s{}".format(*cell3)


def reaches_last_row(cell3):
    """Some mask of the cell reads the last up-sampled row / column: (rows, columns)."""
    H, W, s = cell3
    _, shifts, cell = k4_case(cell3)
    return (bool((H - 1 + shifts[:, 0] == (s + 1) * cell[0] - 1).any()), bool((W - 1 + shifts[:, 1] == (s + 1) * cell[1] - 1).any()))


# K5, exactly one slice (bit for bit): (H, W, s, n_masks)
K5_ONE_SLICE = ((32, 32, 8, 64), (30, 45, 8, 40), (30, 45, 7, 64), (9, 12, 2, 33), (5, 9, 1, 7), (32, 32, 3, 1))
# K5, several slices and / or rounds (within accum_bound): (H, W, s, n_masks)
K5_BOUNDED = tuple((H, W, s, n) for (H, W) in ((32, 32), (30, 45)) for s in (8, 7, 3) for n in (65, 130, 255, 256, 257, 513))
# per_slice > 256 with more than one slice: 1024 tiles allow two slices, so 514 masks run as 257 + 257 in rounds of 256 + 1
K5_LONG = ((512, 512, 8, 514), (512, 512, 7, 514))
LONG_ROWS = (0, 1, 63, 64, 255, 256, 447, 448, 510, 511)        # the pixel rows of a K5_LONG cell held to accum64
# large s: the generic kernel stages fewer than 256 masks a round
K5_LARGE_S = ((224, 224, 15, 300), (64, 64, 16, 500), (64, 64, 17, 70), (66, 66, 33, 64), (64, 128, 64, 40))
PAD_MASKS = 16            # masks' worth of in-range filler (grid 1, shift 0, score NaN) behind every K5 input


def k5_case(cell4, signed=True):
    """-> grid, shifts, scores, cell, scale.  Random grids at p = 0.5 with an all-zero and an all-one grid among them, shifts over
    the whole range with both extremes forced, scores N(0, 1) (or U(0, 1))."""
    H, W, s, n = cell4
    cell = cell_of(H, W, s)
    rng = np.random.default_rng([5, H, W, s, n])
    grid = (rng.random((n, s, s)) < 0.5).astype(np.uint8)
    if H * W > 100000:                                      # 16 distinct grids: the host forms each up-sampling once
        grid = grid[:16][rng.integers(0, 16, n)]
    shifts = np.stack([rng.integers(0, cell[0], n), rng.integers(0, cell[1], n)], axis=1).astype(np.int32)
    if n >= 4:
        grid[n // 3], grid[(2 * n) // 3] = 0, 1
        shifts[0], shifts[n - 1] = (0, 0), (cell[0] - 1, cell[1] - 1)
    scores = (rng.standard_normal(n) if signed else rng.random(n)).astype(F32)
    return grid, shifts, scores, cell, 1.0 / n / 0.5


def k5_name(cell4, kernel):
    return "{}/{}x{}s{}n{}".format(kernel, *cell4)


def k5_kernels(cell4):
    """The accumulate kernels a cell runs on: s == 8 cells run on both (the generic one through a grid one byte off)."""
    return ("s8", "generic") if cell4[2] == 8 else ("generic",)


def bounded_rows():
    """(cell, kernel) of every comparison that goes through accum_bound."""
    return [(c, k) for c in K5_BOUNDED + K5_LONG + K5_LARGE_S for k in k5_kernels(c)]


def mask_ledger_name(cell3):
    return f"rise_edges/mask_vs_oracle/{k4_name(cell3)}"


def accum_ledger_name(cell4, kernel):
    return f"rise_edges/accum/{k5_name(cell4, kernel)}"


def ledger_names():
    return sorted([mask_ledger_name(c) for c in K4_CELLS] + [accum_ledger_name(c, k) for c, k in bounded_rows()])
