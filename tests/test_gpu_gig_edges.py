"""K22 (csrc/gig_kernels.hip, xai_gig_init_f32 / xai_gig_step_f32) on the MI355X against the restated reference loop
(tests/gig_restated.py) over the edge matrix of tests/gig_edges.py, its status words, the mixed batch and GuidedIG.GetMask's
eager path.

Every sequence is *driven*: before each launch the current x and attribution are copied to the host, that step's gradient is drawn
from the case's seeded generator, K22 runs the step once, and the restatement runs the same step from the same bytes -- with the
kernel's arithmetic (the two sums in fp64, rounded to fp32), where everything must agree bit for bit, and with the reference's
(torch's fp32 sums), where the selections must agree and x and the attribution lie within the measured tolerance E.TOL."""
import numpy as np
import pytest
import torch

import gig_edges as E
import gig_restated
from conftest import check, load_golden
from helpers import tiny_from

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGAINST = "restatement, fp32 sums"


def _view(numel, off):
    """`numel` floats starting `off` floats into a fresh (256-byte aligned) allocation: off = 1 defeats xai_can_vec4."""
    return torch.zeros(numel + 4, dtype=torch.float32, device=DEV)[off:off + numel]


def _same(got, want, what, nan_ok=False):
    a, b = got.numpy().view(np.int32), want.numpy().view(np.int32)
    if nan_ok:          # 0 * inf: the bits of a NaN (sign, payload) are the machine's, not the operation's
        ok = (a == b) | (torch.isnan(got) & torch.isnan(want)).numpy()
        assert ok.all(), what
    else:
        np.testing.assert_array_equal(a, b, err_msg=str(what))


def drive(case, offs=(0, 0, 0, 0, 0), extra=0):
    """Run the case's launches; offs: float offsets of x_input, x_baseline, grad, x, attr into their allocations (the five
    pointers xai_can_vec4 looks at).  -> everything the kernel read and wrote, on the host."""
    from xai_engine import kernels as K
    B, n = len(case.images), case.n
    pairs = [case.inputs(i) for i in range(B)]
    xin_h, xb_h = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    xin, base, grad, x, attr = (_view(B * n, o).view(B, n) for o in offs)
    xin.copy_(xin_h)
    base.copy_(xb_h)
    x.fill_(7.0)                                          # init must overwrite every element
    attr.fill_(7.0)
    l1 = torch.full((B,), -1.0, dtype=torch.float32, device=DEV)
    state = torch.full((B, 4), -1, dtype=torch.int32, device=DEV)
    K.gig_init(xin, base, x, attr, l1, state)
    _same(x.cpu(), xb_h, (case, "init x"))
    _same(attr.cpu(), torch.zeros_like(xb_h), (case, "init attr"))
    assert not state.cpu().any(), (case, state)
    draws = [case.gradients(i) for i in range(B)]
    log = []
    for s in range(case.steps + extra):
        x0, a0, st0 = x.cpu(), attr.cpu(), state.cpu()
        g = torch.stack([d() for d in draws])
        grad.copy_(g)
        K.gig_step(xin, base, grad, case.steps, case.fraction, case.max_dist, x, attr, l1, state)
        log.append({"x0": x0, "a0": a0, "state0": st0, "g": g, "x1": x.cpu(), "a1": attr.cpu(), "state": state.cpu()})
    _same(xin.cpu(), xin_h, (case, "x_input is read only"))
    _same(base.cpu(), xb_h, (case, "x_baseline is read only"))
    return {"xin": xin_h, "xb": xb_h, "l1": l1.cpu(), "steps": log}


def _identical(run_a, run_b, i=0, j=0, what=""):
    """Image i of run_a and image j of run_b: the same bytes after every launch."""
    assert float(run_a["l1"][i]) == float(run_b["l1"][j]), what
    for s, (p, q) in enumerate(zip(run_a["steps"], run_b["steps"])):
        _same(p["x1"][i], q["x1"][j], (what, s, "x"), nan_ok=True)
        _same(p["a1"][i], q["a1"][j], (what, s, "attr"), nan_ok=True)
        assert p["state"][i].tolist() == q["state"][j].tolist(), (what, s)


class Tally:
    """What a test measured against the reference's arithmetic: the worst of the two quantities, for K22 and for the fp64-sum
    restatement, and the steps left out because the two restatements disagree on the selection."""

    def __init__(self):
        self.steps = self.left_out = 0
        self.k22 = {"x_over_span": 0.0, "attr": 0.0}
        self.cpu = {"x_over_span": 0.0, "attr": 0.0}

    def report(self, name):
        print(f"{name}: {self.steps} steps, {self.left_out} left out, K22 {self.k22}, restated64 {self.cpu}")
        assert self.left_out <= E.MAX_DISAGREE * self.steps, (self.left_out, self.steps)
        for k in ("x_over_span", "attr"):
            check(f"gig/edges/{name}/restated64_vs_restated32/{k}", self.cpu[k], 0.0, E.TOL[k], against=AGAINST, absolute=True)
            check(f"gig/edges/{name}/k22_vs_restated32/{k}", self.k22[k], 0.0, E.TOL[k], against=AGAINST, absolute=True)


def compare(case, run, tally, nan_ok=False):
    """Every image and step of a driven run against the two restatements.  A step on which the fp64-sum restatement raises its cap
    must end with status 2 (words [step, 2, 64, step]); an image with a status is not touched by later launches."""
    for i in range(len(case.images)):
        xin, xb = run["xin"][i], run["xb"][i]
        l1_64, l1_32 = gig_restated.l1(xin, xb, torch.float64), gig_restated.l1(xin, xb, torch.float32)
        _same(run["l1"][i], l1_64, (case, i, "l1_total"))
        dead = None
        for s, rec in enumerate(run["steps"]):
            x0, a0, g, x1, a1, st = rec["x0"][i], rec["a0"][i], rec["g"][i], rec["x1"][i], rec["a1"][i], rec["state"][i].tolist()
            at = (case, i, s)
            if dead is not None:                          # "a failed image is left as it stands"
                _same(x1, x0, at, nan_ok)
                _same(a1, a0, at, nan_ok)
                assert st == dead, at
                continue
            if float(l1_64) == 0.0:                       # input == baseline (:222-225)
                assert st == [s + 1, 0, 0, 0] and torch.equal(x1, xb) and not a1.any(), at
                continue
            r64, r32 = E.both(x0, xin, xb, g, s, case, l1_64, l1_32, a0)
            if isinstance(r64, str):
                assert st == [s, 2, 64, s], (at, st, r64)
                dead = st
                continue
            assert st == [s + 1, 0, r64[2], int(rec["state0"][i, 3])], (at, st, r64[2])
            assert torch.equal(x1 != x0, r64[3]), (at, "moved set")
            _same(x1, r64[0], (at, "x"), nan_ok)
            _same(a1, r64[1], (at, "attr"), nan_ok)
            tally.steps += 1
            if isinstance(r32, str) or r32[2] != r64[2] or not torch.equal(r32[3], r64[3]):
                assert case.images[i][1] != "normal", at
                tally.left_out += 1
                continue
            if nan_ok:
                continue
            for into, got in ((tally.k22, (x1, a1)), (tally.cpu, r64[:2])):
                ex, ea = E.errors32(got[0], got[1], r32, xin, xb)
                into["x_over_span"], into["attr"] = max(into["x_over_span"], ex), max(into["attr"], ea)


def _cases_of(group, path):
    return [c for c in E.matrix() if c.name.startswith(group) and (c.n % 4 != 0) == (path == "scalar")]


GROUPS = [(g, p) for g in ("axes4", "axes1", "size", "rank", "random") for p in ("vec4", "scalar", "scalar_by_misalignment")
          if _cases_of(g, p)]


@pytest.mark.parametrize("group,path", GROUPS)
def test_k22_over_the_edge_matrix(group, path):
    """gig_init_kernel / gig_step_kernel <4> (n % 4 == 0, aligned), <1> (n % 4 != 0) and <1> at the sizes of <4> (every pointer one
    float into its allocation).  The matrix (tests/gig_edges.py): n from 1 to 4100 -- below one sweep (idle lanes in the
    histograms, the prefix scan and the block sums), around 1024 and 4096, odd image shapes; fractions 0 .. 1 with n - 1 a multiple
    of 10 and 3 (the fp32 rank product); max_dist 0 (alpha_min == alpha_max, the straight-line limit), 0.02, 0.3, 1 and 2; steps 1,
    2, 7, 20; x_input == x_baseline inside a moving image (d == 0 -> NaN alpha -> alpha_max); gradients with ties at the threshold,
    +0 / -0, all zero, all equal, subnormal, keys sharing their top 22 / 11 bits (radix passes C / B decide), keys at both sides of
    digit boundaries, ranks that are the first / last element of a bin; and, with max_dist >= 1 and fractions 0.9 and 1, the rank
    falling among the +inf keys of the features already at x_max (threshold inf: everything not at x_max is selected)."""
    cases = _cases_of(group, path)
    offs = (1,) * 5 if path == "scalar_by_misalignment" else (0,) * 5
    tally = Tally()
    for c in cases:
        compare(c, drive(c, offs), tally)
    tally.report(f"{group}/{path}")


def test_k22_full_size_on_the_scalar_path():
    """150 528 elements (a 3 x 224 x 224 image) through views that start one float into larger buffers: gig_step_kernel<1> at the
    product's size, 147 sweeps of 1024 lanes."""
    c = E.full_size()
    tally = Tally()
    compare(c, drive(c, (1,) * 5), tally)
    tally.report("full/scalar_by_misalignment")


@pytest.mark.parametrize("n", [64, 1024])
def test_each_misaligned_pointer_alone_selects_the_scalar_path_with_identical_results(n):
    """xai_can_vec4 looks at x_input, x_baseline, grad, x and attr: each of them misaligned alone (and all together) gives the bytes of
    the aligned run, on a case whose steps take several selections with ties at the threshold."""
    c = E.Case(f"misalign/n{n}", n, 7, 0.25, 0.3, [("grid_eq30", "ties")])
    aligned = drive(c)
    compare(c, aligned, Tally())
    for k in range(5):
        _identical(drive(c, tuple(int(j == k) for j in range(5))), aligned, what=(c, "pointer", k))
    _identical(drive(c, (1,) * 5), aligned, what=(c, "all pointers"))


@pytest.mark.parametrize("path", ["aligned", "misaligned"])
def test_batches_of_different_images_equal_their_solo_runs(path):
    """1, 2 and 7 images per launch that differ in baseline and gradient kind, so that the workgroups of one launch need different
    numbers of selections: every image against the reference loop per step, and bit for bit against its run alone."""
    offs = (1,) * 5 if path == "misaligned" else (0,) * 5
    tally = Tally()
    seen = set()
    for c in [c for c in E.matrix() if c.name.startswith("batch")]:
        run = drive(c, offs)
        compare(c, run, tally)
        counts = {tuple(int(rec["state"][i, 2]) for rec in run["steps"]) for i in range(len(c.images))}
        assert len(counts) > 1, (c, "the images of the launch need the same selections")
        seen.add(len(c.images))
        for i in range(len(c.images)):
            _identical(run, drive(c.solo(i), offs), i, 0, what=(c, i))
    assert seen == {2, 7}
    tally.report(f"batch/{path}")


def test_infinite_gradients_are_selected_as_the_reference_selects_them():
    """One -inf or +inf gradient with the rank among the infinite keys: +inf is never selected, -inf is once the threshold is
    infinite (`|grad| <= threshold and grad != inf`), on <1> (n = 63) and <4> (n = 64); where +inf keeps the reference from ever
    reaching its target, the restatement raises its cap and K22 reports status 2.  x bit for bit; attr too, NaN for NaN."""
    statuses = set()
    for c in E.infinity_cases():
        run = drive(c)
        compare(c, run, Tally(), nan_ok=True)
        statuses.add((c.name.split("/")[1], c.fraction, int(run["steps"][-1]["state"][0, 1])))
        if "neg" in c.name:                               # the -inf feature was moved to x_input: its attribution is not finite
            at = int(torch.isinf(run["steps"][int("step1" in c.name)]["g"][0]).nonzero()[0])
            assert not torch.isfinite(run["steps"][-1]["a1"][0, at]) and run["steps"][-1]["x1"][0, at] == run["xin"][0, at], c
    assert statuses == {("neg", 1.0, 0), ("neg", 0.9, 0), ("pos", 1.0, 0), ("pos", 0.9, 2)}, statuses


def test_status_2_the_selection_cap():
    """kCap: generic float inputs and baselines (off the grids: the last step cannot reach l1_target = 0) on <1> and <4>, every
    step run -- status 2 exactly on the step on which the restatement raises, bit-equal before; and fraction 0 on 200 tie-free
    gradients.  Words [step unchanged, 2, 64, step]; nothing non-finite is written."""
    for c, at in zip(E.cap_cases(), (6, 9, 0)):
        run = drive(c)
        compare(c, run, Tally())
        last = run["steps"][-1]
        assert last["state"][0].tolist() == [at, 2, 64, at], (c, last["state"])
        assert torch.isfinite(last["x1"]).all() and torch.isfinite(last["a1"]).all(), c


def test_status_3_gamma_not_positive():
    """kGamma: an x ahead of the step's target with features left to select (the inputs with which the restatement's
    `assert gamma > 0` fires, tests/test_cpu_gig.py): words [0, 3, 1, 0], x and attr as they were."""
    from xai_engine import kernels as K
    c, ahead = E.gamma_case()
    xin_h, xb_h = c.inputs(0)
    g = c.gradients(0)()
    with pytest.raises(AssertionError):
        gig_restated.step(ahead, xin_h, xb_h, g, 0, c.steps, c.fraction, c.max_dist, gig_restated.l1(xin_h, xb_h, torch.float64),
                          sum_dtype=torch.float64)
    xin, base, grad = xin_h.view(1, -1).to(DEV), xb_h.view(1, -1).to(DEV), g.view(1, -1).to(DEV)
    x, attr = torch.empty_like(xin), torch.empty_like(xin)
    l1 = torch.empty(1, dtype=torch.float32, device=DEV)
    state = torch.empty((1, 4), dtype=torch.int32, device=DEV)
    K.gig_init(xin, base, x, attr, l1, state)
    x.copy_(ahead.view(1, -1))
    K.gig_step(xin, base, grad, c.steps, c.fraction, c.max_dist, x, attr, l1, state)
    assert state.cpu()[0].tolist() == [0, 3, 1, 0], state
    _same(x.cpu()[0], ahead, "x")
    assert not attr.cpu().any()
    K.gig_step(xin, base, grad, c.steps, c.fraction, c.max_dist, x, attr, l1, state)        # and it stays as it stands
    assert state.cpu()[0].tolist() == [0, 3, 1, 0], state
    _same(x.cpu()[0], ahead, "x")


@pytest.mark.parametrize("n", [63, 1024])
def test_status_4_more_launches_than_steps(n):
    """kSteps: launch steps + 1 writes [steps, 4, the last step's selections, steps] and leaves x and attr untouched bit for bit."""
    c = E.Case(f"launches/n{n}", n, 2, 0.5, 1.0, [("grid", "normal")])
    run = drive(c, extra=1)
    done, extra = run["steps"][-2], run["steps"][-1]
    assert done["state"][0].tolist()[:2] == [2, 0]
    assert extra["state"][0].tolist() == [2, 4, int(done["state"][0, 2]), 2], extra["state"]
    _same(extra["x1"][0], done["x1"][0], "x")
    _same(extra["a1"][0], done["a1"][0], "attr")


def test_a_failed_image_stands_while_the_others_of_its_launch_go_on():
    """`if (st[1] != kOk) return;` -- four images per launch: image 1's gradient is NaN at step 2 (status 1, kNanKey, its x and
    attr stay those of the end of step 1), images 0 and 2 equal their solo runs bit for bit and the reference loop, image 3's
    input equals its baseline (zeros, status 0)."""
    c = E.mixed_batch()
    run = drive(c)
    last = run["steps"][-1]
    assert last["state"][:, 1].tolist() == [0, 1, 0, 0], last["state"]
    assert last["state"][1].tolist() == [2, 1, 0, 2], last["state"]
    _same(last["x1"][1], run["steps"][1]["x1"][1], "image 1: x of the end of step 1")
    _same(last["a1"][1], run["steps"][1]["a1"][1], "image 1: attr of the end of step 1")
    assert torch.isfinite(last["a1"]).all()
    for i in (0, 2):
        solo = drive(c.solo(i))
        _identical(run, solo, i, 0, what=(c, i))
        compare(c.solo(i), solo, Tally())
        assert last["state"][i].tolist()[:2] == [c.steps, 0]
    assert last["state"][3].tolist() == [c.steps, 0, 0, 0] and not last["a1"][3].any()
    _same(last["x1"][3], run["xb"][3], "image 3 never moves")
    # the healthy steps of image 1 are the reference's too
    for s in range(2):
        rec = run["steps"][s]
        r64 = gig_restated.step(rec["x0"][1], run["xin"][1], run["xb"][1], rec["g"][1], s, c.steps, c.fraction, c.max_dist,
                                gig_restated.l1(run["xin"][1], run["xb"][1], torch.float64), sum_dtype=torch.float64, attr0=rec["a0"][1])
        _same(rec["x1"][1], r64[0], ("image 1", s, "x"))
        _same(rec["a1"][1], r64[1], ("image 1", s, "attr"))


class _NaNForOne(torch.nn.Module):
    def __init__(self, inner, which):
        super().__init__()
        self.inner, self.which = inner, which

    def forward(self, x):
        y = self.inner(x)
        scale = torch.ones(y.shape[0], 1, device=y.device)
        scale[self.which] = float("nan")
        return y * scale


def test_guided_ig_batch_names_the_image_that_failed():
    """A classifier that returns NaN for image 1 of 3 only: XaiHipError names image 1 and status 1; the others were healthy."""
    from xai_engine import XaiHipError
    from xai_engine.guided_ig import guided_ig_batch
    model = tiny_from(load_golden("gig.npz"), DEV)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    t = torch.zeros(3, dtype=torch.long, device=DEV)
    with pytest.raises(XaiHipError, match=r"image 1: status 1 at step 0 .*NaN"):
        guided_ig_batch(x, _NaNForOne(model, 1), t, steps=5, fraction=0.5, max_dist=1.0, graphs=False)


# ---- GuidedIG.GetMask with a caller's own gradient function: the eager per-step path of guided_ig.py ----------------------------

def _weights(shape):
    return torch.from_numpy(np.random.default_rng(31).standard_normal(shape).astype(np.float32))


def _closed_form(w, seen):
    """call_model_function of f(x) = sum(w * x^2): the gradient 2 w x, exact to one rounding on either device."""
    from xai_engine.guided_ig import INPUT_OUTPUT_GRADIENTS

    def fn(images, model, device, call_model_args=None, expected_keys=None):
        seen.append(images.device.type)
        g = (w.to(images.device) * images) * 2.0
        if call_model_args and call_model_args.get("answer_on_host") and len(seen) % 2:
            g = g.cpu()
        return {INPUT_OUTPUT_GRADIENTS: g}
    return fn


def _restated_getmask(xin, xb, w, steps, fraction, max_dist):
    """The whole tensor as one point (one l1_total, one quantile), the gradient 2 w x at the fp64-sum restatement's x.
    -> (attribution with K22's sums; the last step's attribution with torch's fp32 sums from the same x)."""
    shape = xin.shape
    xin, xb, w = xin.reshape(-1), xb.reshape(-1), w.reshape(-1)
    l1_64, l1_32 = gig_restated.l1(xin, xb, torch.float64), gig_restated.l1(xin, xb, torch.float32)
    x, attr = xb.clone(), torch.zeros_like(xb)
    for s in range(steps):
        g = (w * x) * 2.0
        if s == steps - 1:
            last32 = gig_restated.step(x, xin, xb, g, s, steps, fraction, max_dist, l1_32, sum_dtype=torch.float32, attr0=attr)[1]
        x, attr, _, _ = gig_restated.step(x, xin, xb, g, s, steps, fraction, max_dist, l1_64, sum_dtype=torch.float64, attr0=attr)
    return attr.view(shape), last32.view(shape)


def _getmask_inputs(shape, seed):
    n = int(np.prod(shape))
    xin, xb = E.image(n, "grid", seed)
    return xin.view(shape), xb.view(shape)


def test_getmask_with_a_callers_gradient_function_on_an_odd_shape():
    """guided_ig.py's eager path, one call of the caller's function and one K22 launch per step: a (1, 3, 15, 17) input (765
    elements, gig_step_kernel<1>) equals the step-by-step restatement with K22's sums bit for bit, and the reference's arithmetic
    within the tolerance measured over the edge matrix.  The function gets its tensor on x_value's device (the host here)."""
    from util.attribution_methods import GIGBuilder as GIG
    shape, steps, fraction, max_dist = (1, 3, 15, 17), 7, 0.25, 0.3
    xin, xb = _getmask_inputs(shape, 41)
    w, seen = _weights(shape), []
    got = GIG.GuidedIG().GetMask(xin, None, DEV, _closed_form(w, seen), {}, x_baseline=xb, x_steps=steps, fraction=fraction,
                                 max_dist=max_dist)
    assert got.shape == xin.shape and got.device == xin.device and seen == ["cpu"] * steps
    want64, last32 = _restated_getmask(xin, xb, w, steps, fraction, max_dist)
    _same(got, want64, "GetMask, eager path")
    check("gig/edges/getmask/odd_shape/attr", got.numpy(), last32.numpy(), E.TOL["attr"], against=AGAINST)


def test_getmask_treats_a_batch_of_two_as_one_point():
    """A (2, 3, 5, 7) x_value is ONE point of the path, as in the reference: one l1_total and one quantile over both images."""
    from util.attribution_methods import GIGBuilder as GIG
    shape, steps, fraction, max_dist = (2, 3, 5, 7), 7, 0.5, 0.02
    xin, xb = _getmask_inputs(shape, 42)
    w = _weights(shape)
    w[1] *= 100.0                                         # image 1's gradients are the larger ones: per-image quantiles would differ
    got = GIG.GuidedIG().GetMask(xin, None, DEV, _closed_form(w, []), {}, x_baseline=xb, x_steps=steps, fraction=fraction,
                                 max_dist=max_dist)
    want64, _ = _restated_getmask(xin, xb, w, steps, fraction, max_dist)
    _same(got, want64, "GetMask, batch of two")
    halves = torch.cat([_restated_getmask(xin[i:i + 1], xb[i:i + 1], w[i:i + 1], steps, fraction, max_dist)[0] for i in range(2)])
    assert not torch.equal(halves, want64), "the case cannot tell one point from two images"


def test_getmask_hands_the_function_a_tensor_on_the_device_of_x_value():
    """x_value on the GPU: the function receives device tensors and may answer on either device (here: alternating); the result
    is on x_value's device and is the restatement's bit for bit."""
    from util.attribution_methods import GIGBuilder as GIG
    shape, steps, fraction, max_dist = (1, 3, 15, 17), 7, 0.25, 0.3
    xin, xb = _getmask_inputs(shape, 41)
    w, seen = _weights(shape), []
    got = GIG.GuidedIG().GetMask(xin.to(DEV), None, DEV, _closed_form(w, seen), {"answer_on_host": True}, x_baseline=xb.to(DEV),
                                 x_steps=steps, fraction=fraction, max_dist=max_dist)
    assert got.is_cuda and seen == ["cuda"] * steps
    _same(got.cpu(), _restated_getmask(xin, xb, w, steps, fraction, max_dist)[0], "GetMask, x_value on the device")
