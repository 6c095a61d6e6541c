"""The edge matrix of the Guided IG step kernel K22 (csrc/gig_kernels.hip): seeded inputs, gradients and cases, shared by the CPU
tests (tests/test_cpu_gig.py: the two restatements against each other, no GPU) and the GPU tests (tests/test_gpu_gig_edges.py: K22
against both restatements).  Every expectation is computed live by tests/gig_restated.py; nothing here is a recorded result.

Inputs lie on a 1/256 grid and baselines on a 1/16 grid (or are zero), so that x_baseline + (x_input - x_baseline) * 1.0 is x_input
exactly and the reference loop ends on the last step, where l1_target is 0."""
import os
import zlib

import numpy as np
import torch

import gig_restated

SCALE = int(os.environ.get("XAI_FUZZ_SCALE", "1"))       # multiplies the random part of the matrix, as in tests/test_gpu_fuzz.py

FRACTIONS = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 1.0)
MAX_DISTS = (0.0, 0.02, 0.3, 1.0, 2.0)
STEPS = (1, 2, 7, 20)
BASELINES = ("zero", "grid", "grid_eq30")
GRADS = ("normal", "ties", "zeros", "band", "mid_band", "pow2", "subnormal", "all_equal")
# n_elem: the scalar path <1> (n % 4 != 0), and <4>; below one sweep of 1024 lanes (x 4), around it, odd image shapes
# (3x30x45, 3x33x33), and n - 1 a multiple of 10 and of 3 (11, 31, 1021, 3001) for the fp32 rank product
SIZES_1 = (1, 2, 3, 5, 63, 1023, 1025, 4050, 3267, 11, 31, 1021, 3001)
SIZES_4 = (4, 64, 1024, 4092, 4096, 4100, 3 * 32 * 32)
FULL = 3 * 224 * 224

# |x - x_ref| / |x_input - x_baseline| and rel_inf of the running attribution, K22's arithmetic (sums in fp64, rounded) against the
# reference's (torch's fp32 sums), over this matrix.  Measured, not chosen: restatement-fp64 against restatement-fp32 on the CPU
# (tests/test_cpu_gig.py::test_edge_matrix_fp32_sums_against_fp64_sums) gives MEASURED_CPU, K22 against restatement-fp32 on an
# MI355X (profiles/gig_edges_parity.json) gives MEASURED_GPU; the asserted tolerance is 2 x the larger.
MEASURED_CPU = {"x_over_span": 1.52587890625e-05, "attr": 8.942704094864205e-06}
MEASURED_GPU = {"x_over_span": 1.52587890625e-05, "attr": 8.942704094864205e-06}
TOL = {k: 2.0 * max(MEASURED_CPU[k], MEASURED_GPU[k]) for k in MEASURED_CPU}
# steps on which the two restatements themselves disagree about the selection count or the moved set (an isclose or a gamma > 1
# that flips on the last bit of a sum) are left out of the fp32 comparison, counted, and capped
MAX_DISAGREE = 0.02


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def image(n, baseline, seed):
    """-> (x_input, x_baseline), fp32 torch vectors of n: input on the 1/256 grid and never 0, baseline by kind."""
    rng = np.random.default_rng(seed)
    xin = (rng.integers(1, 513, n) * rng.choice((-1, 1), n)).astype(np.float32) / np.float32(256)
    if baseline == "generic":                            # off the grids: the last step's x_max is not x_input to the bit (status rows)
        return (torch.from_numpy(rng.standard_normal(n).astype(np.float32)),
                torch.from_numpy(rng.standard_normal(n).astype(np.float32)))
    if baseline == "same":                               # x_input == x_baseline: l1_total is 0 and the attribution is zero (:222-225)
        return torch.from_numpy(xin), torch.from_numpy(xin.copy())
    if baseline == "zero":
        xb = np.zeros(n, np.float32)
    else:
        xb = rng.integers(-16, 17, n).astype(np.float32) / np.float32(16)
        if baseline == "grid_eq30":                      # x_input == x_baseline inside a moving image: d == 0 -> NaN alpha -> alpha_max
            same = rng.random(n) < 0.3
            same[0] = False
            xb[same] = xin[same]
        elif baseline != "grid":
            raise ValueError(baseline)
    return torch.from_numpy(xin), torch.from_numpy(xb)


def gradient(kind, n, rng):
    """One step's gradient of `kind` from the numpy generator `rng`, an fp32 torch vector of n."""
    g = rng.standard_normal(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if kind == "normal":
        out = g
    elif kind == "ties":
        out = np.round(2 * g) / 2
    elif kind == "zeros":
        u = rng.random(n)
        out = np.where(u < 0.6, 0.0, np.where(u < 0.7, -0.0, g))
    elif kind == "band":                                 # the keys share their top 22 bits: the last radix pass decides
        out = sign * (1.0 + rng.integers(0, 512, n) * 2.0 ** -23)
    elif kind == "mid_band":                             # the top 11 bits are shared: the second and third pass decide
        out = sign * (1.0 + rng.integers(0, 512, n) * 2.0 ** -13)
    elif kind == "pow2":                                 # keys on both sides of digit boundaries
        out = sign * 2.0 ** rng.integers(-20, 3, n) * (1.0 + rng.integers(-1, 2, n) * 2.0 ** -23)
    elif kind == "subnormal":
        out = g * 1e-41
    elif kind == "all_equal":
        out = sign * 0.75
    elif kind == "all_zero":                             # not an axis value: two rows of their own, +0 and -0 mixed
        out = sign * 0.0
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.asarray(out, np.float64).astype(np.float32))


class Case:
    """One launch sequence: `images` = [(baseline kind, gradient kind)], all of n elements, sharing steps / fraction / max_dist."""

    def __init__(self, name, n, steps, fraction, max_dist, images, tamper=None):
        self.name, self.n, self.steps, self.fraction, self.max_dist, self.images = name, n, steps, fraction, max_dist, list(images)
        self.tamper = dict(tamper or {})                  # {(image, step): function that edits that step's gradient in place}

    def __repr__(self):
        return self.name

    def inputs(self, i):
        return image(self.n, self.images[i][0], _seed(self.name, i, "image"))

    def gradients(self, i):
        """The generator of image i's gradients, one draw per step; the same in a batch and alone."""
        rng = np.random.default_rng(_seed(self.name, i, "grad"))
        at = [0]

        def draw():
            g = gradient(self.images[i][1], self.n, rng)
            edit = self.tamper.get((i, at[0]))
            if edit is not None:
                edit(g)
            at[0] += 1
            return g
        return draw

    def solo(self, i):
        """Image i alone: the same input, baseline and gradients as in the batch."""
        c = Case(self.name, self.n, self.steps, self.fraction, self.max_dist, [self.images[i]])
        c.inputs = lambda _: self.inputs(i)
        c.gradients = lambda _: self.gradients(i)
        return c


def _settle(n, steps, fraction, max_dist, grad):
    """The combinations for which the reference loop cannot end within the cap are moved to their neighbours:
    max_dist 0 (x_min == x_max: nothing is left to select, the loop ends only through isclose) needs alpha * d exact, so steps 1 or 2;
    fraction 0 selects one tie level per quantile, so above 32 elements every gradient is one of a few levels."""
    if max_dist == 0.0 and steps not in (1, 2):
        steps = 1 if steps == 7 else 2
    if fraction == 0.0 and n > 32 and grad not in ("ties", "all_equal"):
        grad = "ties"
    return steps, grad


def _case(tag, n, fi, mi, si, bi, gi):
    fraction, max_dist = FRACTIONS[fi % 7], MAX_DISTS[mi % 5]
    steps, grad = _settle(n, STEPS[si % 4], fraction, max_dist, GRADS[gi % 8])
    base = BASELINES[bi % 3]
    name = f"{tag}/n{n}/f{fraction:.3g}/d{max_dist:g}/s{steps}/{base}/{grad}"
    return Case(name, n, steps, fraction, max_dist, [(base, grad)])


def matrix(scale=SCALE):
    """The cases; sizes divisible by 4 run on both kernel instantiations on the GPU (aligned: <4>; one float into a buffer: <1>)."""
    out = []
    # every axis value once at a size divisible by 4 (so with both paths) ...
    for k in range(8):
        out.append(_case("axes4", SIZES_4[k % len(SIZES_4)], k, k, k, k, k))
    # ... and once at a size that is not
    for k in range(8):
        out.append(_case("axes1", SIZES_1[(k + 4) % len(SIZES_1)], k, k + 2, k + 1, k + 1, k + 3))
    # every size against every gradient kind and, cycling, the other axes
    i = 0
    for n in SIZES_1 + SIZES_4:
        for gi in range(8):
            out.append(_case("size", n, i, i // 2, i // 3, i // 5, gi))
            i += 1
    for n in (63, 1024):
        out.append(Case(f"size/n{n}/f0.25/d0.3/s7/grid/all_zero", n, 7, 0.25, 0.3, [("grid", "all_zero")]))
    # the rank: every fraction at the sizes whose n - 1 is a multiple of 10 and of 3
    for n in (11, 31, 1021, 3001):
        for fi in range(7):
            out.append(_case("rank", n, fi, 3, 2, 1, 0 if n <= 32 else fi))
    # the random part
    rng = np.random.default_rng(22)
    for r in range(24 * scale):
        n = int(rng.integers(1, 4200)) if r % 3 else 4 * int(rng.integers(1, 1050))
        out.append(_case(f"random{r}", n, *(int(v) for v in rng.integers(0, 840, 5))))
    # batches whose images differ (baseline and gradient kind), so that the selection counts differ inside one launch
    kinds = [(BASELINES[j % 3], GRADS[(3 * j) % 8]) for j in range(7)]
    for n, steps, fraction, max_dist, B in ((1025, 7, 0.25, 0.02, 2), (3 * 32 * 32, 7, 0.1, 0.02, 2), (4096, 7, 0.5, 1.0, 7),
                                            (63, 20, 0.1, 0.3, 7), (4100, 2, 0.9, 2.0, 7)):
        out.append(Case(f"batch{B}/n{n}/f{fraction:.3g}/d{max_dist:g}/s{steps}", n, steps, fraction, max_dist, kinds[:B]))
    names = [c.name for c in out]
    keep = [c for j, c in enumerate(out) if c.name not in names[:j]]
    return keep


def full_size():
    """150 528 elements (3 x 224 x 224), run on the GPU through a view one float into a larger buffer: <1> at the product's size."""
    return Case("full/n150528/f0.25/d0.3/s7/grid/normal", FULL, 7, 0.25, 0.3, [("grid", "normal")])


def cap_cases():
    """Status 2, the selection cap.  Generic float inputs and baselines: on the last step x_baseline + d * 1.0 differs from x_input
    in some last bits, l1_current never is l1_target = 0, and once every feature is at x_max nothing is left to select;
    fraction 0 on 200 tie-free gradients selects one feature per quantile and the single step needs all 200."""
    return [Case("cap/generic/n1000", 1000, 7, 0.25, 0.3, [("generic", "normal")]),
            Case("cap/generic/n4096", 4096, 10, 0.25, 0.02, [("generic", "normal")]),
            Case("cap/fraction0/n200", 200, 1, 0.0, 2.0, [("grid", "normal")])]


def gamma_case():
    """Status 3, the reference's `assert gamma > 0`: an x ahead of the step's target (0.9 of the way at step 0 of 4, target 0.25)
    with max_dist 2, so x_max is x_input and every feature is still selectable.  -> (case, the x to start the step from)."""
    c = Case("gamma/n1025", 1025, 4, 0.25, 2.0, [("grid", "normal")])
    xin, xb = c.inputs(0)
    return c, xb + (xin - xb) * 0.9


def _put(value):
    """The gradient of the largest magnitude becomes `value`: that feature is among the last the quantile reaches."""
    def edit(g):
        g[int(g.abs().argmax())] = value
    return edit


def infinity_cases():
    """A single infinite gradient with the rank among the infinite keys (max_dist 2: x_max is x_input from the first step on).
    fraction 1 at step 0: the threshold is that infinity itself; +inf is never selected (:264, :268), -inf is, and both runs end.
    fraction 0.9 at the last step: the second quantile falls among the features already at x_max; -inf is selected with the rest
    and the run ends; +inf is never moved, so the reference loops on and the restatement raises its cap."""
    out = []
    for n in (63, 64):
        for name, value in (("neg", -np.inf), ("pos", np.inf)):
            out.append(Case(f"inf/{name}/n{n}/f1/step0", n, 2, 1.0, 2.0, [("grid", "normal")], {(0, 0): _put(value)}))
            out.append(Case(f"inf/{name}/n{n}/f0.9/step1", n, 2, 0.9, 2.0, [("grid", "normal")], {(0, 1): _put(value)}))
    return out


def mixed_batch():
    """Four images of one launch: image 1's gradient is NaN at step 2, image 3's input equals its baseline."""
    def nan(g):
        g[:] = np.nan
    return Case("mixed/n1025", 1025, 5, 0.25, 0.3, [("grid", "normal"), ("zero", "ties"), ("grid_eq30", "pow2"), ("same", "normal")],
                {(1, 2): nan})


def both(x, xin, xb, grad, s, case, l1_64, l1_32, attr0):
    """The step from x under K22's arithmetic and under the reference's.  -> ((x, attr, sel, moved) | RuntimeError text) x 2."""
    res = []
    for dt, l1t in ((torch.float64, l1_64), (torch.float32, l1_32)):
        try:
            res.append(gig_restated.step(x, xin, xb, grad, s, case.steps, case.fraction, case.max_dist, l1t, sum_dtype=dt, attr0=attr0))
        except RuntimeError as e:
            res.append(str(e))
    return res


def errors32(x_got, attr_got, ref32, xin, xb):
    """The two measured quantities of a step against the reference's arithmetic."""
    span = (xin - xb).abs().double()
    moving = span > 0
    ex = float(((x_got.double() - ref32[0].double()).abs()[moving] / span[moving]).max()) if moving.any() else 0.0
    # rel_inf, except that below 2^-125 (the `subnormal` gradients) the fp32 quantum 2^-149 is itself more than 2^-24 of the
    # value, so the error is taken against 2^-125 there
    ea = float((attr_got.double() - ref32[1].double()).abs().max()) / max(float(ref32[1].abs().max()), 2.0 ** -125)
    return ex, ea


def restated_run(case, i=0):
    """Image i of `case` through both restatements on the CPU, each step from the fp64-sum restatement's x (K22's chain).
    -> per step (ref64, ref32, x before, attr before, gradient)."""
    xin, xb = case.inputs(i)
    draw = case.gradients(i)
    l1_64, l1_32 = gig_restated.l1(xin, xb, torch.float64), gig_restated.l1(xin, xb, torch.float32)
    x, attr = xb.clone(), torch.zeros_like(xb)
    log = []
    for s in range(case.steps):
        g = draw()
        if float(l1_64) == 0.0:                           # input == baseline: the reference returns zeros before its loop (:222-225)
            log.append(((x, attr, 0, torch.zeros_like(x, dtype=torch.bool)),) * 2 + (x, attr, g))
            continue
        r64, r32 = both(x, xin, xb, g, s, case, l1_64, l1_32, attr)
        log.append((r64, r32, x, attr, g))
        if isinstance(r64, str):
            break
        x, attr = r64[0], r64[1]
    return log
