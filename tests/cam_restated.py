"""K3 (csrc/cam_kernels.hip: gradcam_kernel<PPL>, gradcam_finish_kernel, bilinear_up_kernel) restated in NumPy, for
tests/test_cpu_cam.py (which proves the restatements on the host) and tests/test_gpu_cam_edges.py (which holds the kernels to them).

Three things per kernel: the kernel's own arithmetic in the kernel's own order, all in fp32 (`cam_fp32`, `bilinear_fp32`: the
kernel must return these BITS); the definition in float64 (`cam64`, `bilinear64`); and a derived per-pixel bound on the distance
between the two (`cam_bound`, `bilinear_bound`).  `exact_case` builds integer data on which every summation order is exact, so a
channel or pixel left out, read twice or mixed up shows element for element whatever the order.  The file header of
cam_kernels.hip is the specification of the order: "a wave owns channels {wave, wave+16, ...} of its workgroup's channel slice",
"the 16 wave partials ... summed in wave order", "sums the slice partials in slice order"."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32
WAVES, LANES = 16, 64               # kWaves, kWave
MAX_HW = 1024


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): a product of n factors (1 + d_i)^(+-1), |d_i| <= u, is 1 + t with |t| <= gamma_n."""
    return n * U / (1.0 - n * U)


# ---- host choices ----------------------------------------------------------------------------------------------------------------

def ppl_for(hw):
    """pixels per lane of the instantiation xai_gradcam_f32 launches: h*w <= 64 * PPL"""
    assert 1 <= hw <= MAX_HW
    return 1 if hw <= 64 else 2 if hw <= 128 else 4 if hw <= 256 else 8 if hw <= 512 else 16


def unroll_for(ppl):
    """UC: channels per wave and trip (a trip of the workgroup is 16 * UC channels)"""
    return 8 if ppl <= 2 else 4 if ppl <= 4 else 2


def slices_for(B, C, have_ws=True):
    """-> (slices, per): cam_slices (1 from 64 images on, else C / 64 clipped to 1 .. 16), one slice without (enough) workspace,
    then per = ceil(C / slices) and slices = ceil(C / per)."""
    slices = 1 if B >= 64 else max(1, min(16, C // 64))
    if not have_ws:
        slices = 1
    per = -(-C // slices)
    return -(-C // per), per


def workspace_floats(B, C, hw):
    """xai_gradcam_workspace_bytes / 4: sized by cam_slices, before per is known"""
    g = 1 if B >= 64 else max(1, min(16, C // 64))
    return 0 if g == 1 else B * g * hw


def slice_lengths(B, C, have_ws=True):
    slices, per = slices_for(B, C, have_ws)
    return [min(C, (s + 1) * per) - s * per for s in range(slices)]


# ---- Grad-CAM --------------------------------------------------------------------------------------------------------------------

def cam_fp32(act, grad, relu, have_ws=True):
    """(B, C, h, w) x 2 -> (B, h, w): the kernel's arithmetic in the kernel's order, every operation rounded to fp32.

    Per image and slice, wave v takes channels c_begin + v, c_begin + v + 16, ... in ascending order (round r of the loop below
    is channel c_begin + 16 r + v of every wave at once).  Per channel: lane l adds its PPL gradients ((0 + g[l]) + g[l + 64]) +
    ..., pixels past h*w being 0; the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (addition commutes, so all 64 lanes end with
    the same bits); a true division by float(hw); acc[p] = acc[p] + fl(w * a[p]).  Channels past the slice's end are loaded as
    zeros by the kernel: they add +0.0 to an accumulator that is never -0.0 (it starts at +0.0, and x + y is -0.0 only when both
    are), so padding the slice with zero channels is the same arithmetic.  Then the 16 wave accumulators are added from 0 in wave
    order and, with several slices, the slice partials from 0 in slice order; ReLU is max(v, 0) at the very end."""
    act, grad = np.ascontiguousarray(act, F32), np.ascontiguousarray(grad, F32)
    B, C, h, w = act.shape
    hw = h * w
    ppl = ppl_for(hw)
    slices, per = slices_for(B, C, have_ws)
    rounds = -(-per // WAVES)
    lane = np.arange(LANES)

    def laid_out(x, width):                      # (B, C, hw) -> (B, slices, rounds, WAVES, width), zeros where nothing is
        full = np.zeros((B, slices * per, width), F32)
        full[:, :C, :hw] = x.reshape(B, C, hw)
        out = np.zeros((B, slices, rounds * WAVES, width), F32)
        out[:, :, :per] = full.reshape(B, slices, per, width)
        return out.reshape(B, slices, rounds, WAVES, width)

    g = laid_out(grad, ppl * LANES).reshape(B, slices, rounds, WAVES, ppl, LANES)
    a = laid_out(act, hw)
    n = F32(hw)
    acc = np.zeros((B, slices, WAVES, hw), F32)
    for r in range(rounds):
        s = np.zeros((B, slices, WAVES, LANES), F32)
        for k in range(ppl):
            s = s + g[:, :, r, :, k]
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[..., lane ^ off]
        wgt = s[..., :1] / n
        acc = acc + wgt * a[:, :, r]
    part = np.zeros((B, slices, hw), F32)
    for v in range(WAVES):
        part = part + acc[:, :, v]
    if slices == 1:
        cam = part[:, 0]
    else:
        cam = np.zeros((B, hw), F32)
        for s_ in range(slices):
            cam = cam + part[:, s_]
    assert cam.dtype == F32
    cam = cam.reshape(B, h, w)
    return np.maximum(cam, F32(0)) if relu else cam


def cam64(act, grad, relu):
    """The definition in float64: the gradient's mean over the pixels weighs the activation, summed over the channels."""
    a, g = np.asarray(act, np.float64), np.asarray(grad, np.float64)
    cam = (g.mean(axis=(2, 3), keepdims=True) * a).sum(axis=1)
    return np.maximum(cam, 0.0) if relu else cam


def cam_chain(B, C, hw, have_ws=True):
    """n of cam_bound: the longest chain of fp32 roundings one input value g[c][q] * a[c][p] passes through."""
    slices, per = slices_for(B, C, have_ws)
    return ppl_for(hw) + 6 + 1 + 1 + -(-per // WAVES) + WAVES + (slices if slices > 1 else 0)


def cam_bound(act, grad, have_ws=True):
    """(B, h, w): |cam_fp32 - cam64| <= gamma_n * sum_c mean_q |g[c][q]| * |a[c][p]|, for any data.

    Every fp32 operation returns its exact result times (1 + d), |d| <= u = 2^-24 (no underflow at these magnitudes; float(hw) is
    exact for hw <= 1024 and the inputs are fp32 already).  Follow one product g[c][q] * a[c][p] / hw through the kernel; the
    factors (1 + d) it collects are
        PPL        the lane's additions (the first one, to 0, is exact and is counted all the same),
        6          the butterfly,
        1          the division by hw,
        1          the product w * a[p],
        ceil(per / 16)   additions into the wave's accumulator (one per channel of that wave from c on, at most all of them),
        16         the wave partials added from 0,
        slices     the slice partials added from 0 (none with one slice),
    so the computed cam[p] is sum_c sum_q g[c][q] a[c][p] / hw * (1 + t_cq) with |t_cq| <= gamma_n for that n (Higham, Accuracy
    and Stability of Numerical Algorithms, Lemma 3.1), hence the bound.  ReLU is 1-Lipschitz, so the bound holds after it too.
    float64 carries the same chain at 2^-53: below 2^-29 of this bound, which is not added."""
    a, g = np.abs(np.asarray(act, np.float64)), np.abs(np.asarray(grad, np.float64))
    B, C, h, w = a.shape
    return gamma(cam_chain(B, C, h * w, have_ws)) * (g.mean(axis=(2, 3), keepdims=True) * a).sum(axis=1)


def normal_case(B, C, h, w, seed=0):
    """N(0, 1) activations and gradients"""
    rng = np.random.default_rng([11, B, C, h, w, seed])
    return rng.standard_normal((B, C, h, w)).astype(F32), rng.standard_normal((B, C, h, w)).astype(F32)


def exact_case(B, C, h, w, seed=0):
    """-> act, grad (fp32, integer-valued), weights (B, C) int64, cam (B, h, w) int64, on which every order of addition is exact.

    act is integers in [-8, 8]; the weight of a channel is drawn in [-4, 4] and its gradient in [-16, 16], and the channel's last
    pixel is then set so that the gradients sum to weight * hw.  Every partial sum of a channel's gradients is an integer of
    magnitude <= 16 (hw - 1) + (4 hw + 16 (hw - 1)) < 2^16, the division is exact, and every partial sum of w * a is an integer of
    magnitude <= 32 C: all below 2^24, so fp32 holds each one exactly in any order."""
    rng = np.random.default_rng([12, B, C, h, w, seed])
    hw = h * w
    act = rng.integers(-8, 9, (B, C, h, w))
    weights = rng.integers(-4, 5, (B, C))
    grad = rng.integers(-16, 17, (B, C, hw))
    grad[:, :, -1] = weights * hw - grad[:, :, :-1].sum(axis=2)
    cam = (weights[:, :, None, None] * act).sum(axis=1)
    return act.astype(F32), grad.reshape(B, C, h, w).astype(F32), weights.astype(np.int64), cam.astype(np.int64)


def exact_case_holds(act, grad, weights, cam):
    """the conditions exact_case states, checked on the data itself"""
    B, C, h, w = act.shape
    hw = h * w
    a, g = act.astype(np.int64), grad.astype(np.int64).reshape(B, C, hw)
    assert (a == act).all() and (g.reshape(grad.shape) == grad).all() and np.abs(a).max() <= 8
    assert (g.sum(axis=2) == weights * hw).all() and np.abs(weights).max() <= 4
    assert np.abs(g).sum(axis=2).max() < 2 ** 24 and (np.abs(weights)[:, :, None, None] * np.abs(a)).sum(axis=1).max() < 2 ** 24
    assert (cam == (weights[:, :, None, None] * a).sum(axis=1)).all()
    return True


# hw as (h, w), non-square wherever hw is not 1, a square handed over by the classifiers (49) or a prime
CAM_HW = ((1, 1), (7, 7), (7, 9), (4, 16), (5, 13), (1, 127), (8, 16), (3, 43), (15, 17), (8, 32), (1, 257), (7, 73), (16, 32),
          (19, 27), (31, 33), (16, 64))
CAM_BUDGET = 2 ** 18                # C * hw per image ...
# ... but 16 slices need C >= 1024, which passes the budget from hw = 257 on: the C = 1030 cells of PPL 8 and 16 sit at the
# smallest hw of their class and are the only cells above it (2.1 MB per tensor)
CAM_OVER_BUDGET = ((1, 257), (19, 27))
TRIP_INSIDE = {8: 100, 4: 50, 2: 27}           # UC -> a C that ends inside the first trip of 16 * UC channels, in one slice
B64_CELLS = ((64, 256, 7, 7), (63, 256, 7, 7))


def trip_exact(ppl):
    """A C whose slices all end exactly on a trip: 16 * UC channels in one slice where that is below 128 (UC = 4, 2); with UC = 8
    a single slice holds at most 127 channels, so C = 2048 = 16 slices of one trip each."""
    uc = unroll_for(ppl)
    return 2048 if uc == 8 else WAVES * uc


def cam_cells():
    """(B, C, h, w) of the Grad-CAM matrix: per hw the channel counts 1, 17, inside a trip, exactly on a trip, 129 (2 slices of 65
    + 64), 200 (3 slices, the last ragged) and 1030 (16 slices of 65, the last with 55) within the budget; B = 3 where the slices
    are ragged or a wave runs dry (17, 200), B = 1 elsewhere; then C = 256 at B = 64 (one slice) and B = 63 (four)."""
    cells = []
    for h, w in CAM_HW:
        hw = h * w
        ppl = ppl_for(hw)
        for C in (1, 17, TRIP_INSIDE[unroll_for(ppl)], trip_exact(ppl), 129, 200, 1030):
            if C * hw <= CAM_BUDGET or (C == 1030 and (h, w) in CAM_OVER_BUDGET):
                cells.append((3 if C in (17, 200) else 1, C, h, w))
    return cells + list(B64_CELLS)


def cam_name(cell):
    return "B{}_C{}_{}x{}".format(*cell)


# ---- bilinear --------------------------------------------------------------------------------------------------------------------

def taps32(n_in, n_out):
    """the kernel's source taps in fp32: scale = fl(in / out), s = max(fl(fl(scale * (d + 0.5)) - 0.5), 0), i0 = int(s), the
    neighbour clamped, l1 = s - i0 (exact), l0 = fl(1 - l1)"""
    scale = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32)
    s = np.maximum((d + F32(0.5)) * scale - F32(0.5), F32(0))
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(F32)
    return i0, i1, F32(1) - l1, l1


def bilinear_fp32(src, H, W, mult=1.0, take_abs=False):
    """(B, h, w) -> (B, H, W), bilinear_up_kernel term for term: top = s00 * lx0 + s01 * lx1, bot likewise on row y1,
    v = (top * ly0 + bot * ly1) * mult, then |v| -- products and sums rounded separately."""
    src = np.ascontiguousarray(src, F32)
    B, h, w = src.shape
    y0, y1, ly0, ly1 = taps32(h, H)
    x0, x1, lx0, lx1 = taps32(w, W)
    top = src[:, y0][:, :, x0] * lx0 + src[:, y0][:, :, x1] * lx1
    bot = src[:, y1][:, :, x0] * lx0 + src[:, y1][:, :, x1] * lx1
    v = (top * ly0[None, :, None] + bot * ly1[None, :, None]) * F32(mult)
    assert v.dtype == F32
    return np.abs(v) if take_abs else v


def taps64(n_in, n_out):
    """exact source coordinate max((d + 0.5) * in / out - 0.5, 0) (in float64: exact to 2^-53 relative), neighbour clamped"""
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0, s


def bilinear64(src, H, W):
    """plain (not antialiased) align_corners=False bilinear interpolation in float64 at exact coordinates"""
    src = np.asarray(src, np.float64)
    B, h, w = src.shape
    y0, y1, ly1, _ = taps64(h, H)
    x0, x1, lx1, _ = taps64(w, W)
    top = src[:, y0][:, :, x0] * (1 - lx1) + src[:, y0][:, :, x1] * lx1
    bot = src[:, y1][:, :, x0] * (1 - lx1) + src[:, y1][:, :, x1] * lx1
    return top * (1 - ly1)[None, :, None] + bot * ly1[None, :, None]


COORD_ULPS = 5          # |s32 - s| <= 5 u max(s, 1), below
BLEND_ROUNDINGS = 7     # roundings on the longest path of the blend, below


def bilinear_bound(src, H, W, mult=1.0):
    """(B, H, W): |bilinear_fp32(src, H, W, mult) - mult * bilinear64(src, H, W)| <= this, for any data (|.| of both is closer still).

    Coordinate.  s = (d + 0.5) * in / out - 0.5.  fp32 rounds in / out (1 + d1), the product with the exact d + 0.5 (1 + d2) and the
    subtraction (1 + d3): |s32 - s| <= (2u + u^2) (s + 0.5) + u |s32| <= 3 u (s + 0.5) (1 + 2u) <= 4.5 u max(s, 1) (1 + 2u)
    < COORD_ULPS * u * max(s, 1); max(., 0) does not increase a distance.
    Lipschitz.  The interpolant f(y, x) is continuous and piecewise linear along each axis; its slope along x is a convex
    combination of differences of horizontal neighbours, so |f(y, x32) - f(y, x)| <= Dx |x32 - x| with Dx the largest
    |src[i][j + 1] - src[i][j]| of the image, and likewise along y with Dy.  That holds across a cell boundary, so a tap index
    that flips because of the coordinate's rounding is covered.
    Blend, at the fp32 coordinate.  i0 = int(s32) and l1 = s32 - i0 are exact.  l0 = fl(1 - l1) (1), s00 * lx0 (1), the sum with
    s01 * lx1 (1): top carries at most 3 roundings; ly0 (1) -- or the product's own 1, whichever path is longer stays <= 3 --
    top * ly0 (1), the sum with bot * ly1 (1), the product with mult (1): at most BLEND_ROUNDINGS = 7 on any path, on a convex
    combination of the four taps, so the error is <= gamma_7 * max |tap| * |mult|.  mult itself (1, 3, -2) is exact in fp32.
    ATen's CPU kernel rounds the same coordinate expression in fp32 and blends with no more roundings, so the same bound holds
    between `F.interpolate(antialias=False)` and bilinear64."""
    s = np.asarray(src, np.float64)
    B, h, w = s.shape
    y0, y1, _, sy = taps64(h, H)
    x0, x1, _, sx = taps64(w, W)
    dy = np.abs(np.diff(s, axis=1)).max(axis=(1, 2)) if h > 1 else np.zeros(B)
    dx = np.abs(np.diff(s, axis=2)).max(axis=(1, 2)) if w > 1 else np.zeros(B)
    # the blend happens at the fp32 coordinate, whose taps may lie one row / column beside the exact ones: every magnitude is
    # replaced by the largest of its 3 x 3 neighbourhood before the four exact taps are looked up
    pad = np.pad(np.abs(s), ((0, 0), (1, 1), (1, 1)), mode="edge")
    a = np.max([pad[:, i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    tap = np.maximum(np.maximum(a[:, y0][:, :, x0], a[:, y0][:, :, x1]), np.maximum(a[:, y1][:, :, x0], a[:, y1][:, :, x1]))
    coord = COORD_ULPS * U * (dy[:, None, None] * np.maximum(sy, 1.0)[None, :, None] + dx[:, None, None] * np.maximum(sx, 1.0)[None, None, :])
    return abs(float(mult)) * (coord + gamma(BLEND_ROUNDINGS) * tap)


def degenerate_axis_holds(src, up, axis, mult=1.0):
    """What is true of an up-sampling along an axis of source length 1 (axis 1: h = 1, axis 2: w = 1), in this arithmetic.  Both
    taps of that axis are the same value t, blended as fl(fl(t * l0) + fl(t * l1)): where l1 == 0 (the coordinate clamped at 0,
    which includes index 0) that is t bit for bit, so those rows (columns) are bitwise equal; elsewhere it is t only to
    rounding, so every row lies within 2 * gamma_7 * |mult| * max |src| of row 0 -- each is within gamma_7 (bilinear_bound's
    blend term) of the one exact value they share.  Bitwise equality of ALL rows does not hold, in the oracle or in ATen."""
    assert src.shape[axis] == 1
    up = np.ascontiguousarray(up, F32)
    first = up.take([0], axis=axis)
    l1 = taps32(1, up.shape[axis])[3]
    assert l1[0] == 0
    same = np.flatnonzero(l1 == 0)
    assert (up.take(same, axis=axis).view(np.int32) == first.view(np.int32)).all(), "rows / columns of weight 0 differ in their bits"
    slack = 2 * gamma(BLEND_ROUNDINGS) * abs(float(mult)) * np.abs(np.asarray(src, np.float64)).max(axis=(1, 2))[:, None, None]
    assert (np.abs(up.astype(np.float64) - first) <= slack).all()
    return True


BILINEAR_SHAPES = ((7, 7, 224, 224), (14, 14, 224, 224), (7, 7, 30, 45), (31, 33, 224, 224), (8, 8, 8, 8), (1, 9, 5, 65), (9, 1, 63, 4),
                   (1, 1, 3, 64), (14, 14, 7, 7), (9, 13, 4, 5), (5, 5, 1, 1)) + tuple((6, 7, H, W) for H in (3, 4, 5) for W in (63, 64, 65))
SHRINKING = ((14, 14, 7, 7), (9, 13, 4, 5), (5, 5, 1, 1))                      # the cells that pin the kernel as plain bilinear
SHRINKS = tuple(s for s in BILINEAR_SHAPES if s[2] < s[0] or s[3] < s[1])       # ... and the tile-edge cells, whose 6 rows become 3, 4, 5
WITH_MULT = ((7, 7, 224, 224), (8, 8, 8, 8), (14, 14, 7, 7), (6, 7, 5, 65), (1, 1, 3, 64))       # mult 3 and -2, with and without abs


def bilinear_cells():
    """(B, h, w, H, W, mult, take_abs): every shape at B = 1 and 3 with mult 1; on WITH_MULT also (3, abs) -- the Grad-CAM row's
    own call -- (-2, no abs), (-2, abs) and (1, abs)."""
    cells = []
    for shape in BILINEAR_SHAPES:
        for B in (1, 3):
            cells.append((B,) + shape + (1.0, 0))
        if shape in WITH_MULT:
            cells += [(3,) + shape + (3.0, 1), (1,) + shape + (-2.0, 0), (3,) + shape + (-2.0, 1), (1,) + shape + (1.0, 1)]
    return cells


def bilinear_name(cell):
    return "B{}_{}x{}_to_{}x{}_mult{:g}_abs{}".format(*cell)


def bilinear_case(cell):
    B, h, w = cell[:3]
    return np.random.default_rng([13, B, h, w, cell[3], cell[4]]).standard_normal((B, h, w)).astype(F32)


def ledger_names():
    """every row tests/test_gpu_cam_edges.py leaves in its ledger (profiles/cam_edges_parity.json): per comparison the error in
    the project's norm at BAR and, under /bound, the largest |error| / derived bound at 1.0"""
    names = [f"cam_edges/cam/{cam_name(c)}/relu{r}" for c in cam_cells() for r in (0, 1)]
    names += [f"cam_edges/cam_no_workspace/{k}" for k in ("none", "short", "full")]
    names += [f"cam_edges/bilinear/{bilinear_name(c)}" for c in bilinear_cells()]
    names += [f"cam_edges/bilinear_plain_vs_torch/{bilinear_name(c)}" for c in bilinear_cells() if c[1:5] in SHRINKING and c[5] == 1.0 and not c[6]]
    names = names + [n + "/bound" for n in names]
    names += ["cam_edges/resize_antialiased/{}x{}_to_{}x{}".format(*s) for s in SHRINKS]
    names += ["cam_edges/ablation_map/shared", "cam_edges/ablation_map/per_channel", "cam_edges/shrinking_layer/eager", "cam_edges/shrinking_layer/graphs", "cam_edges/shrinking_layer/graphs_second_input"]
    return sorted(names)
