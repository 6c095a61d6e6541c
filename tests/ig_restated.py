"""The IG family of csrc/ig_kernels.hip (ig_accum_stream_kernel<256,4,1,C,WT> and <64,1,5,C,WT>, ig_accum_kernel<4 | 1, WT>,
ig_accum_add_kernel, ig_finish_kernel, store_stream_kernel / _scalar_kernel, ig_cutoff_kernel, sumsq_kernel, idgi_accum_kernel)
restated in NumPy, for tests/test_cpu_ig.py (which proves the restatements on the host) and tests/test_gpu_ig_edges.py (which
holds the kernels to them).

Per kernel: the kernel's own arithmetic in the kernel's own order, every operation rounded to fp32 (`accum_fp32`, `finish_fp32`,
`accum_add_fp32`, `sumsq_fp32`, `idgi_fp32`: the kernel must return these BITS -- the library is built with -ffp-contract=off and
its division is a true division); the definition in float64 (`accum64`, `sumsq64`, `idgi64`); a derived bound on the distance
between the two in Higham's gamma; and the host's launch choice (`accum_kernel_for`, `sumsq_is_vector`, `store_kernel_for`).
`exact_accum_case` builds integer data on which every order of addition is exact and on which a step row read past n_use shows
element for element.  `cutoff` is the Left-IG cutoff of the reference."""
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32
LANES = 64                          # kWave
POISON_ROW = 2 ** 20 + 1            # what exact_accum_case puts into every step row from n_use on


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): a product of n factors (1 + d_i)^(+-1), |d_i| <= u, is 1 + t with |t| <= gamma_n."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


# ---- host choices ----------------------------------------------------------------------------------------------------------------

Launch = namedtuple("Launch", "kernel args grid per")       # grid, per: None for ig_accum_kernel (one lane per pixel / float4)


def accum_kernel_for(n_img, C, hw, aligned, weighted, cus):
    """What ig_accum_impl launches.  float4 lanes need hw % 4 == 0 and every pointer on a 16-byte boundary (`aligned`); with
    those and C in {1, 3} it is the step-outer stream kernel: items = n_img * hw / 4, big = items >= cus * 2 * 256 * 2, the big
    mapping <256, 4, 1, C, WT> on cus * 2 workgroups, the small one <64, 1, 5, C, WT> on ceil(items / 64); `per` is the items of
    one workgroup, ceil(items / grid), as the kernel computes it.  Everything else is ig_accum_kernel<4 | 1, WT>."""
    vec = hw % 4 == 0 and bool(aligned)
    if vec and C in (1, 3):
        items = n_img * (hw // 4)
        big = items >= cus * 2 * 256 * 2
        grid = cus * 2 if big else -(-items // 64)
        args = (256, 4, 1, C, bool(weighted)) if big else (64, 1, 5, C, bool(weighted))
        return Launch("ig_accum_stream_kernel", args, grid, -(-items // grid))
    return Launch("ig_accum_kernel", (4 if vec else 1, bool(weighted)), None, None)


def spellings(kernel, args):
    """The two forms a profiler reports an instantiation in, spaces removed: demangled, and the Itanium mangling."""
    plain = ",".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in args)
    mangled = "".join(f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E" for a in args)
    return f"{kernel}<{plain}>", f"{kernel}I{mangled}E"


def ran(names, launch):
    """Exactly one accumulate kernel is among `names`, and it is `launch`."""
    mine = [n for n in names if "ig_accum_stream_kernel" in n or "ig_accum_kernel" in n]
    return len(mine) == 1 and any(s in mine[0] for s in spellings(launch.kernel, launch.args))


def stream_lanes(n_img, hw, nu_img, launch, workgroup):
    """The stream kernel's index arithmetic.  Per round of `workgroup`'s `first += BLOCK * ITEMS` loop: which of a lane's ITEMS
    slots are live, and the (clamped) cutoff each slot holds -- an idle slot shadows item `lo` and holds that image's
    -> list over rounds of (live (BLOCK, ITEMS) bool, nu (BLOCK, ITEMS))."""
    block, n_items = launch.args[0], launch.args[1]
    hw4 = hw // 4
    items = n_img * hw4
    lo = workgroup * launch.per
    hi = min(lo + launch.per, items)
    nu_img = np.asarray(nu_img)
    rounds = []
    for first in range(lo, hi, block * n_items):
        it = first + np.arange(n_items)[None, :] * block + np.arange(block)[:, None]
        live = it < hi
        rounds.append((live, nu_img[np.where(live, it, lo) // hw4]))
    return rounds


def store_kernel_for(n, src_aligned, dst_aligned):
    return "store_stream_kernel" if n % 4 == 0 and src_aligned and dst_aligned else "store_stream_scalar_kernel"


def sumsq_is_vector(n_elem, aligned):
    """sumsq_kernel's own choice, per row: n % 4 == 0 and the row on a 16-byte boundary (with n % 4 == 0 every row of a buffer
    has the alignment of the first)."""
    return n_elem % 4 == 0 and bool(aligned)


# ---- accumulate ------------------------------------------------------------------------------------------------------------------

def clamp_n_use(n_use, n_img, n_steps):
    """None: all steps; an int or one int per image -> (n_img,) int64, clamped to [1, n_steps] as every kernel clamps it"""
    nu = np.broadcast_to(np.asarray(n_steps if n_use is None else n_use, np.int64), (n_img,))
    return np.clip(nu, 1, n_steps)


def _base(base, shape):
    return F32(base) if np.isscalar(base) else np.asarray(base, F32).reshape(shape)


def accum_fp32(grads, n_use, x, base, w1=None, w2=None):
    """grads (n_img, n_steps, C, hw), x (n_img, C, hw), base a scalar or like x, w1 / w2 (n_img, n_steps) or None
    -> out (n_img, C, hw), out_abs (n_img, hw), fp32.

    n_use is clamped to [1, n_steps].  Per (image, channel, pixel): acc = 0; for s ascending below n_use: t = g[s], t = fl(t *
    w1[s]), t = fl(t * w2[s]) where present, acc = fl(acc + t); o = fl(fl(acc / denom) * fl(x - b)) with denom = float(n_steps)
    when weighted, else float(n_use); abs = |((0 + o_0) + o_1) + ...| over the channels.  The unrolled loops of the three kernels
    load ahead but add in this order, so all three must return these bits."""
    g, x = np.asarray(grads, F32), np.asarray(x, F32)
    n_img, n_steps, C, hw = g.shape
    nu = clamp_n_use(n_use, n_img, n_steps)
    assert w1 is not None or w2 is None
    acc = np.zeros((n_img, C, hw), F32)
    for s in range(int(nu.max())):
        live = nu > s
        t = g[live, s]
        if w1 is not None:
            t = t * np.asarray(w1, F32)[live, s][:, None, None]
            if w2 is not None:
                t = t * np.asarray(w2, F32)[live, s][:, None, None]
        acc[live] = acc[live] + t
    denom = F32(n_steps) if w1 is not None else nu.astype(F32)[:, None, None]
    return finish_fp32(acc, denom, x, base)


def finish_fp32(acc, denom, x, base):
    """ig_finish_kernel, and the tail of every accumulate kernel: o = fl(fl(acc / denom) * fl(x - b)); abs as in accum_fp32.
    denom: n_steps (an int), or an fp32 array that broadcasts."""
    acc, x = np.asarray(acc, F32), np.asarray(x, F32)
    n_img, C, hw = acc.shape
    denom = F32(denom) if np.isscalar(denom) else denom
    o = (acc / denom) * (x.reshape(acc.shape) - _base(base, acc.shape))
    tot = np.zeros((n_img, hw), F32)
    for c in range(C):
        tot = tot + o[:, c]
    assert o.dtype == F32 and tot.dtype == F32
    return o, np.abs(tot)


def accum_add_fp32(grads, acc):
    """ig_accum_add_kernel: a = acc; a = fl(a + g[b]), b ascending.  grads (n_batch, n_elem), acc (n_elem,)."""
    a = np.array(acc, F32)
    for row in np.asarray(grads, F32):
        a = a + row
    return a


def accum64(grads, n_use, x, base, w1=None, w2=None):
    """-> out, out_abs in float64: sum_{s < n_use} g w1 w2 / denom * (x - b), |sum over the channels|; and the sum of the
    magnitudes sum_s |g w1 w2| / denom * |x - b| the bound is made of."""
    g = np.asarray(grads)
    n_img, n_steps, C, hw = g.shape
    nu = clamp_n_use(n_use, n_img, n_steps)
    acc, mag = np.zeros((n_img, C, hw)), np.zeros((n_img, C, hw))
    for s in range(int(nu.max())):
        live = nu > s
        t = g[live, s].astype(np.float64)
        for w in (w1, w2):
            if w is not None:
                t = t * np.asarray(w, np.float64)[live, s][:, None, None]
        acc[live] += t
        mag[live] += np.abs(t)
    denom = float(n_steps) if w1 is not None else nu.astype(np.float64)[:, None, None]
    d = np.asarray(x, np.float64).reshape(acc.shape) - (float(F32(base)) if np.isscalar(base) else np.asarray(base, np.float64).reshape(acc.shape))
    o = acc / denom * d
    return o, np.abs(o.sum(axis=1)), mag / denom * np.abs(d)


def accum_chain(n_use, n_weights):
    """n of accum_bound: the fp32 roundings one g[s] passes through on its way into out -- one per weight, at most n_use
    additions (the first, to 0, is exact and is counted all the same), the division, x - b, the product."""
    return n_use + n_weights + 3


def accum_bound(grads, n_use, x, base, w1=None, w2=None):
    """-> bound on |out - out64| (n_img, C, hw) and on |abs - abs64| (n_img, hw), for any data.

    Every fp32 operation returns its exact result times (1 + d), |d| <= u (no underflow at these magnitudes; float(n_use) and
    float(n_steps) are exact).  g[s] collects accum_chain(n_use, weights) such factors, so out = sum_s g w1 w2 / denom (x - b)
    (1 + t_s) with |t_s| <= gamma_n (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1): the bound is gamma_n
    sum_s |g w1 w2| / denom |x - b|, n = n_use + 5 at most.  The abs map adds the C channel values from 0: C more factors on
    each, and | |a| - |b| | <= |a - b|.  float64 carries the same chains at 2^-53, below 2^-29 of this bound: not added."""
    g = np.asarray(grads)
    n_img, n_steps, C, hw = g.shape
    nu = clamp_n_use(n_use, n_img, n_steps)
    n_w = (w1 is not None) + (w2 is not None)
    mag = accum64(grads, n_use, x, base, w1, w2)[2]
    return gamma(accum_chain(nu, n_w))[:, None, None] * mag, gamma(accum_chain(nu, n_w) + C)[:, None] * mag.sum(axis=1)


def normal_accum_case(n_img, n_steps, C, hw, seed=0):
    """N(0, 1) gradients, images, tensor baselines and step weights"""
    rng = np.random.default_rng([31, n_img % 65536, n_steps, C, hw, seed])
    f = lambda *shape: rng.standard_normal(shape, dtype=F32)
    return {"grads": f(n_img, n_steps, C, hw), "x": f(n_img, C, hw), "base": f(n_img, C, hw), "w1": f(n_img, n_steps), "w2": f(n_img, n_steps)}


def exact_accum_case(n_img, n_steps, C, hw, n_use, seed=0):
    """-> grads, x, base (fp32, integer-valued), out (n_img, C, hw) int64, out_abs (n_img, hw) int64, for the unweighted call.

    Gradients are integers in [-8, 8]; per (image, channel, pixel) a mean m in [-4, 4] is drawn and step n_use - 1 is set so
    that the first n_use steps sum to m * n_use: every partial sum is an integer below 2^12 in magnitude, the division by
    float(n_use) is exact and returns m.  x and the tensor baseline are integers in [-8, 8], so x - b and m (x - b) and the sum
    over the channels are exact.  Every step row from n_use on holds 2^20 + 1: one of them added changes the quotient by more
    than 2^20 / n_steps, whatever the order."""
    rng = np.random.default_rng([32, n_img % 65536, n_steps, C, hw, seed])
    nu = clamp_n_use(n_use, n_img, n_steps)
    g = rng.integers(-8, 9, (n_img, n_steps, C, hw))
    m = rng.integers(-4, 5, (n_img, C, hw))
    x, b = rng.integers(-8, 9, (n_img, C, hw)), rng.integers(-8, 9, (n_img, C, hw))
    for i in range(n_img):
        g[i, nu[i]:] = POISON_ROW
        g[i, nu[i] - 1] = m[i] * nu[i] - g[i, :nu[i] - 1].sum(axis=0)
    out = m * (x - b)
    return g.astype(F32), x.astype(F32), b.astype(F32), out.astype(np.int64), np.abs(out.sum(axis=1)).astype(np.int64)


def exact_accum_case_holds(grads, x, base, out, out_abs, n_use):
    """the conditions exact_accum_case states, checked on the data itself"""
    n_img, n_steps, C, hw = grads.shape
    nu = clamp_n_use(n_use, n_img, n_steps)
    g, xi, bi = grads.astype(np.int64), x.astype(np.int64), base.astype(np.int64)
    assert (g == grads).all() and (xi == x).all() and (bi == base).all()
    for i in range(n_img):
        used = g[i, :nu[i]]
        assert (g[i, nu[i]:] == POISON_ROW).all() and np.abs(used[:-1]).max(initial=0) <= 8
        assert np.abs(used).sum(axis=0).max() < 2 ** 12
        total = used.sum(axis=0)
        assert (total % nu[i] == 0).all() and np.abs(total // nu[i]).max() <= 4
        assert (out[i] == total // nu[i] * (xi[i] - bi[i])).all()
    assert np.abs(xi).max() <= 8 and np.abs(bi).max() <= 8 and np.abs(out).sum(axis=1).max() < 2 ** 24
    assert (out_abs == np.abs(out.sum(axis=1))).all()
    return True


# ---- the accumulate matrix ---------------------------------------------------------------------------------------------------------

# name; n_img (an int, or a function of cus); n_steps; C; hw; mode: "dev" (n_use per image on the device), "host" (one int) or
# "none" (all steps); n_use: the values the images cycle through (dev) / the int (host); weights: 0, 1 (w1) or 2 (w1 and w2);
# base: "scalar" or "tensor"; off: the operand one word past a 16-byte boundary, or None
Cell = namedtuple("Cell", "name n_img n_steps C hw mode n_use weights base off")
SMALL_USE = (1, 4, 5, 6, 9, 10, 11, 12)                 # around the 5-step unroll of the small stream kernel, n_steps = 12
SMALL_HW = (4, 8 * 9, 16 * 16, 4 * 65)
V4_USE = (7, 8, 9, 16, 17)                              # around the 8-step unroll of ig_accum_kernel, n_steps = 17
BIG_HW, BIG_STEPS, TWO_ROUND_STEPS = 512, 7, 3
OPERANDS = ("grads", "x", "base", "out", "out_abs")
SCALAR_BASE = 0.25


def n_img_of(cell, cus):
    return cell.n_img(cus) if callable(cell.n_img) else cell.n_img


def _over(cus):
    return cus * 8 + 1          # 128 items per image at hw = 512: cus * 1024 items is the threshold


def _under(cus):
    return cus * 8 - 1


def _two_rounds(cus):
    return cus * 16 + 4         # per = 1025: one item more than a round of 256 lanes x 4


def accum_cells():
    """The accumulate matrix of the issue; the big cells' image counts are functions of the device's CU count."""
    cells = []
    k = 0
    for C in (3, 1):
        for hw in SMALL_HW:
            for n_img in (1, 3):
                for mode in ("dev", "host", "none"):
                    use = tuple(SMALL_USE[(k + j) % 8] for j in range(n_img)) if mode == "dev" else SMALL_USE[k % 8] if mode == "host" else None
                    cells.append(Cell(f"small_C{C}_hw{hw}_B{n_img}_{mode}", n_img, 12, C, hw, mode, use, 0, ("scalar", "tensor")[k % 2], None))
                    k += 3
    big_use = tuple(range(1, BIG_STEPS + 1))
    cells.append(Cell("big_C3_over", _over, BIG_STEPS, 3, BIG_HW, "dev", big_use, 0, "tensor", None))
    cells.append(Cell("big_C3_under", _under, BIG_STEPS, 3, BIG_HW, "dev", big_use, 0, "tensor", None))
    cells.append(Cell("big_C1_two_rounds", _two_rounds, TWO_ROUND_STEPS, 1, BIG_HW, "dev", (3, 1, 2, 2, 3, 1, 1), 0, "scalar", None))
    for w in (1, 2):
        cells.append(Cell(f"weighted_small_w{w}", 3, 12, 3, 72, "dev", (4, 11, 6), w, "scalar", None))
        cells.append(Cell(f"weighted_big_w{w}", _over, BIG_STEPS, 3, BIG_HW, "dev", (2, 5, 6, 3, 1), w, "scalar", None))
        cells.append(Cell(f"weighted_v4_w{w}", 2, 17, 2, 64, "dev", (9, 16), w, "tensor", None))
        cells.append(Cell(f"weighted_v1_w{w}", 2, 12, 3, 197, "host", 7, w, "tensor", None))
    cells.append(Cell("weighted_small_C1_w2", 3, 12, 1, 260, "dev", (5, 10, 9), 2, "tensor", None))
    cells.append(Cell("weighted_big_C1_w1", _two_rounds, TWO_ROUND_STEPS, 1, BIG_HW, "dev", (2, 3, 1), 1, "tensor", None))
    k = 0
    for C in (2, 4):
        for hw in (8 * 8, 4 * 257):
            for use in V4_USE:
                mode = "none" if use == 17 else ("host", "dev")[k % 2]
                cells.append(Cell(f"v4_C{C}_hw{hw}_use{use}", 2, 17, C, hw, mode, None if mode == "none" else (use, 1 + k % 5) if mode == "dev" else use,
                                  0, ("tensor", "scalar")[k % 2], None))
                k += 1
    cells.append(Cell("v1_C3_hw197", 2, 12, 3, 197, "dev", (9, 11), 0, "scalar", None))
    cells.append(Cell("v1_C1_hw197", 3, 12, 1, 197, "dev", (12, 5, 8), 0, "tensor", None))
    cells.append(Cell("v1_C3_hw63", 2, 12, 3, 7 * 9, "host", 10, 0, "tensor", None))
    for op in OPERANDS:
        cells.append(Cell(f"v1_C3_hw256_off_{op}", 2, 12, 3, 256, "dev", (9, 11), 0, "tensor", op))
    return cells


def cell_n_use(cell, n_img):
    """-> what the kernel is told (per-image int32 array, an int, or None) and the same as accum_fp32's n_use argument"""
    if cell.mode == "dev":
        return np.asarray([cell.n_use[i % len(cell.n_use)] for i in range(n_img)], np.int32)
    return cell.n_use


def cell_launch(cell, cus):
    return accum_kernel_for(n_img_of(cell, cus), cell.C, cell.hw, cell.off is None, cell.weights > 0, cus)


# the cells the clamp, baseline and exact-integer tests run on: one per kernel
PER_KERNEL = ("small_C3_hw72_B3_dev", "big_C3_over", "v4_C2_hw64_use9", "v1_C3_hw197")
CLAMPED = (0, -3, None)             # None: n_steps + 5; must equal (1, 1, n_steps)


def accum_name(cell):
    return cell.name


# ---- accum_add / finish ------------------------------------------------------------------------------------------------------------

ADD_BATCHES = (1, 7, 8, 9, 17)
ADD_ELEMS = (1, 4, 1023, 1024 * 4 + 4)
# (n_batch, n_elem, off of grads, off of acc): every pair, and the aligned length with either operand one word off
ADD_CELLS = tuple((b, n, 0, 0) for b in ADD_BATCHES for n in ADD_ELEMS) + ((9, 4100, 1, 0), (9, 4100, 0, 1), (8, 4, 1, 1))
FINISH_CELLS = tuple((2, C, hw) for C in (1, 3, 4) for hw in (4, 63, 256))          # (n_img, C, hw), with and without out_abs
CHAINED_CELLS = ((2, 3, 64, (8, 9)), (1, 1, 63, (17,)), (3, 4, 256, (1, 7, 8)))     # (n_img, C, hw, batch sizes fed one after the other)


def add_name(cell):
    return "B{}_n{}_goff{}_aoff{}".format(*cell)


def finish_name(cell):
    return "B{}_C{}_hw{}".format(*cell)


def chained_name(cell):
    return "B{}_C{}_hw{}_batches{}".format(cell[0], cell[1], cell[2], "+".join(map(str, cell[3])))


# ---- store_grads -------------------------------------------------------------------------------------------------------------------

def store_cells(cus):
    """(n, src off, dst off).  One trip of the grid-stride loop moves cus * 8 * 256 lanes: the first two large cells are the
    second trip of the float4 and of the scalar form."""
    trip = cus * 8 * 256
    return [(n, 0, 0) for n in (1, 3, 4, 5, 1023, 1024)] + [(trip * 4 + 4, 0, 0), (trip + 1, 0, 1), (4096, 1, 0), (4096, 0, 1)]


def store_payload(n, seed=0):
    """random int32 words, with quiet and signalling NaN payloads, -0.0, both infinities and subnormals planted"""
    rng = np.random.default_rng([33, n % 65536, seed])
    w = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    special = np.array([0x7FC0BEEF, 0x7F800001, -0x7FFFFF, -2 ** 31, 0x7F800000, -0x800000, 1, -2 ** 31 + 1, 0x007FFFFF], np.int64).astype(np.int32)
    at = rng.permutation(n)[:min(n, special.size)]
    w[at] = special[:at.size]
    return w


# ---- cutoff ------------------------------------------------------------------------------------------------------------------------

def cutoff(logits, alpha_star):
    """Left-IG's number of leading steps, /util/attribution_methods/saliencyMethods.py:48-67 of the reference:
    `max_perc = torch.max(logits)`, `cutoff_perc = max_perc * alpha_star` (:48-49, an fp32 product); `alpha_star == 1` takes all
    steps (:52-53); else `torch.where(logits > cutoff_perc)[0]`, strictly above (:56), its first index (:59), 1 when there is
    none (:61) and 1 instead of 0 (:64-65).  torch.max propagates a NaN, and nothing is above a NaN threshold: a NaN anywhere in
    the row gives 1."""
    lg = np.asarray(logits, F32)
    if F32(alpha_star) == F32(1):
        return lg.size
    if np.isnan(lg).any():
        return 1
    thr = F32(lg.max() * F32(alpha_star))
    hit = np.flatnonzero(lg > thr)
    return max(int(hit[0]), 1) if hit.size else 1


CUTOFF_ALPHAS = (0.9, 0.5, 1.0)
CUTOFF_STEPS = (1, 2, 63, 64, 65, 128, 129, 200)
NO_HIT_ALPHA = 1.0 - 2.0 ** -20


def cutoff_rows(n, alpha_star):
    """-> labels, rows (R, n) fp32: the planted rows of the issue that fit n steps.  max = 8 (a power of two, so thr is exact at
    alpha 0.5), `above` is the fp32 next after thr, the background 1 lies below thr."""
    top, bg = F32(8), F32(1)
    thr = F32(top * F32(alpha_star))
    above = np.nextafter(thr, F32(np.inf)) if thr < top else top
    rows, labels = [], []

    def plant(label, values, fill=bg):
        row = np.full(n, fill, F32)
        for i, v in values.items():
            assert 0 <= i < n
            row[i] = v
        rows.append(row)
        labels.append(label)

    for h in sorted({0, 1, 63, 64, n - 1}):
        if h < n:
            plant(f"hit_at_{h}", {n - 1: top, h: above} if h < n - 1 else {h: top})
    for a, b in ((63, 64), (65, 70), (70, 129), (5, 64), (64 + 9, 128 + 2)):       # the later hit in a lane that meets it sooner
        if b < n:
            plant(f"hits_{a}_{b}", {a: above, b: top})
    plant("all_equal", {}, fill=F32(3))
    plant("negative_max", {i: F32(-1 - (i * 7) % 5) for i in range(n)})
    plant("zero_max", {n // 2: F32(0)}, fill=F32(-2))
    plant("all_minus_inf", {}, fill=F32(-np.inf))
    if n >= 4:
        plant("equal_to_thr_first", {1: thr, n - 2: above, n - 1: top})
        plant("several_maxima", {n // 2: top, n - 1: top, n // 2 + 1: top})
        h = n - 2
        plant("nan_before_hit", {h - 1: F32(np.nan), h: above, n - 1: top})
        plant("nan_after_hit", {h: top, h + 1: F32(np.nan)})
        plant("nan_at_0", {0: F32(np.nan), h: top})
    rng = np.random.default_rng([34, n])
    for j in range(3):
        rows.append(rng.standard_normal(n, dtype=F32) + F32(j))
        labels.append(f"random_{j}")
    return labels, np.stack(rows)


# ---- sumsq -------------------------------------------------------------------------------------------------------------------------

SUMSQ_THREADS, SUMSQ_WAVES = 1024, 16


def _butterfly(s):
    """wave_sum: the xor butterfly 32, 16, 8, 4, 2, 1 over the last axis of 64 lanes (a + b on both partners: all lanes agree)"""
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ off]
    return s


def sumsq_trips(n_elem, vector):
    """additions per thread: the trips of its loop, times 4 in the float4 form"""
    return -(-n_elem // (4 * SUMSQ_THREADS)) * 4 if vector else -(-n_elem // SUMSQ_THREADS)


def sumsq_fp32(rows, aligned=True):
    """(n_rows, n_elem) -> (n_rows,): sumsq_kernel.  Vector form (n % 4 == 0 and the row 16-byte aligned): thread t walks i = 4t,
    4t + 4096, ..., adding fl(v * v) in x, y, z, w order; scalar form: thread t walks i = t, t + 1024, ....  Then the butterfly
    inside each of the 16 waves, the 16 partials padded with zeros to 64 lanes, and the butterfly again (block_sum_lane0<16>).
    A thread past the row's end adds nothing; adding fl(0 * 0) = +0.0 instead leaves every bit alone, because an accumulator of
    squares is never -0.0."""
    rows = np.ascontiguousarray(rows, F32)
    n_rows, n = rows.shape
    vector = sumsq_is_vector(n, aligned)
    width = 4 if vector else 1
    trips = -(-n // (width * SUMSQ_THREADS))
    sq = np.zeros((n_rows, trips * SUMSQ_THREADS * width), F32)
    sq[:, :n] = rows * rows
    sq = sq.reshape(n_rows, trips, SUMSQ_THREADS, width)
    acc = np.zeros((n_rows, SUMSQ_THREADS), F32)
    for k in range(trips):
        for j in range(width):
            acc = acc + sq[:, k, :, j]
    part = _butterfly(acc.reshape(n_rows, SUMSQ_WAVES, LANES))[..., 0]
    lanes = np.zeros((n_rows, LANES), F32)
    lanes[:, :SUMSQ_WAVES] = part
    out = _butterfly(lanes)[:, 0]
    assert out.dtype == F32
    return out


def sumsq64(rows):
    r = np.asarray(rows, np.float64)
    return (r * r).sum(axis=1)


def sumsq_chain(n_elem, vector):
    """the square, the thread's additions, 6 + 6 butterfly steps"""
    return sumsq_trips(n_elem, vector) + 1 + 12


def sumsq_bound(rows, aligned=True):
    """|sumsq_fp32 - sumsq64| <= gamma_n * sumsq64, n = sumsq_chain: every term is positive, and a value passes through its own
    square (1), at most `trips` additions of its thread and the 12 additions of the two butterflies."""
    n = np.asarray(rows).shape[1]
    return gamma(sumsq_chain(n, sumsq_is_vector(n, aligned))) * sumsq64(rows)


SUMSQ_ROWS = (1, 3)
SUMSQ_ELEMS = (1, 3, 4, 1023, 1024, 4096, 4100, 4097, 150528)
SUMSQ_CELLS = tuple((r, n, 0) for r in SUMSQ_ROWS for n in SUMSQ_ELEMS) + ((3, 4096, 1),)      # (n_rows, n_elem, off)


def sumsq_name(cell):
    return "R{}_n{}_off{}".format(*cell)


def sumsq_case(cell, integer=False):
    rng = np.random.default_rng([35, cell[0], cell[1], cell[2], int(integer)])
    if integer:
        return rng.integers(-3, 4, cell[:2]).astype(F32)            # squares sum to at most 9 * 150528 < 2^24: exact in any order
    return rng.standard_normal(cell[:2], dtype=F32)


# ---- IDGI --------------------------------------------------------------------------------------------------------------------------

def idgi_fp32(grads, logits, sumsq):
    """grads (n_steps, n_elem), logits (n_steps,), sumsq (n_steps,) fp32 -> (n_elem,): idgi_accum_kernel,
    acc = fl(acc + fl(fl(fl(g * g) * fl(l[s + 1] - l[s])) / sumsq[s])), s ascending, the last step dropped."""
    g, lg, sq = np.asarray(grads, F32), np.asarray(logits, F32), np.asarray(sumsq, F32)
    acc = np.zeros(g.shape[1], F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(g.shape[0] - 1):
            acc = acc + ((g[s] * g[s]) * (lg[s + 1] - lg[s])) / sq[s]
    assert acc.dtype == F32
    return acc


def idgi64(grads, logits, sumsq):
    """-> the definition in float64 on the given fp32 sumsq, and sum_s |term_s|"""
    g, lg, sq = np.asarray(grads, np.float64), np.asarray(logits, np.float64), np.asarray(sumsq, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = g[:-1] * g[:-1] * (lg[1:] - lg[:-1])[:, None] / sq[:-1, None]
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def idgi_chain(n_steps):
    """g * g, l[s + 1] - l[s], their product, the division, at most n_steps - 1 additions"""
    return n_steps + 3


def idgi_bound(grads, logits, sumsq):
    """|idgi_fp32 - idgi64| <= gamma(n_steps + 3) * sum_s |term_s|: each term collects the four roundings idgi_chain names and
    one per addition it takes part in; the difference of two fp32 logits is their exact difference times (1 + d)."""
    return gamma(idgi_chain(np.asarray(grads).shape[0])) * idgi64(grads, logits, sumsq)[1]


IDGI_STEPS = (2, 3, 20)
IDGI_ELEMS = (1, 4, 63, 3 * 32 * 32, 4 * 1025)
IDGI_CELLS = tuple((s, n, 0) for s in IDGI_STEPS for n in IDGI_ELEMS) + ((3, 4 * 1025, 1), (20, 256, 1))       # (n_steps, n_elem, off of out)
IDGI_ZERO_STEP = (5, 256, 0)                # the middle step's gradient is all zero: 0 * d / 0
IDGI_CHAINED = (20, 3 * 32 * 32, 0)         # K.sumsq feeds K.idgi_accum


def idgi_name(cell):
    return "S{}_n{}_off{}".format(*cell)


def idgi_case(cell, zero_step=None):
    """N(0, 1) gradients; logits that rise along the path as a classifier's do, with one step down"""
    n_steps, n = cell[:2]
    rng = np.random.default_rng([36, n_steps, n, cell[2]])
    g = rng.standard_normal((n_steps, n), dtype=F32)
    lg = np.sort(rng.standard_normal(n_steps, dtype=F32) * F32(3))
    if n_steps >= 3:
        lg[[1, 2]] = lg[[2, 1]]
    if zero_step is not None:
        g[zero_step] = 0
    return g, lg


# ---- the ledger --------------------------------------------------------------------------------------------------------------------

def ledger_names():
    """every row tests/test_gpu_ig_edges.py leaves in its ledger (profiles/ig_edges_parity.json): per comparison the error in the
    project's norm at BAR and, under /bound, the largest |error| / derived bound at 1.0.  Bit-for-bit and int64 comparisons
    (store_grads, the cutoff, accum_add and finish on their own, the clamp and the exact cases) leave no row."""
    names = [f"ig_edges/accum/{c.name}/{part}" for c in accum_cells() for part in ("out", "abs")]
    names += [f"ig_edges/stream/{chained_name(c)}/{part}" for c in CHAINED_CELLS for part in ("out", "abs")]
    names += [f"ig_edges/sumsq/{sumsq_name(c)}" for c in SUMSQ_CELLS]
    names += [f"ig_edges/idgi/{idgi_name(c)}" for c in IDGI_CELLS] + ["ig_edges/idgi_chained/" + idgi_name(IDGI_CHAINED)]
    return sorted(names + [n + "/bound" for n in names])
