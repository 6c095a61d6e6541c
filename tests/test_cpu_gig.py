"""Guided IG without a GPU: the harness row, the mirror module's interface and resolution, the argument checks of the
K22 entry points (made before any HIP call), and the yardstick of the GPU tests: tests/gig_restated.py replays the reference's
recorded run bit for bit, and the edge matrix of tests/gig_edges.py is run through its two arithmetics."""
import inspect
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import gig_edges as E
import gig_restated
from conftest import GOLDEN, PKG, check, load_golden

with open(os.path.join(GOLDEN, "gig_api.json")) as _f:
    API = json.load(_f)


def test_gig_is_a_cnn_attribution_of_the_harness():
    from xai_engine.sweep import CNN_ATTR_FUNCS
    assert "gig" in CNN_ATTR_FUNCS


@pytest.mark.parametrize("name", sorted(API))
def test_mirror_has_the_reference_signature(name):
    from util.attribution_methods import GIGBuilder
    if name == "GuidedIG.GetMask":
        params = list(inspect.signature(GIGBuilder.GuidedIG.GetMask).parameters.values())[1:]
    else:
        params = list(inspect.signature(getattr(GIGBuilder, name)).parameters.values())
    want = API[name]
    assert [p.name for p in params] == [w["name"] for w in want]
    for p, w in zip(params, want):
        assert (p.default is not inspect.Parameter.empty) == w["has_default"], (name, p.name)
        if w["has_default"]:
            assert p.default == w["default"] and type(p.default) is type(w["default"]), (name, p.name, p.default, w["default"])


SIBLING = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])          # build first, sibling tree after it
    from util.attribution_methods import GIGBuilder as GIG_Builder            # evaluatePerturbation.py:41
    import xai_engine.guided_ig as g
    assert GIG_Builder.GuidedIG is g.GuidedIG and GIG_Builder.call_model_function is g.call_model_function
    assert GIG_Builder.WHO == "sibling" and GIG_Builder.CoreSaliency.WHO == "sibling core"
    assert GIG_Builder.VisualizeImageGrayscale() == "sibling grayscale"
    print("gig imports ok")
""")


def test_guided_ig_resolves_to_the_engine_and_the_rest_falls_through(tmp_path):
    root = tmp_path / "sibling" / "util"
    (root / "attribution_methods").mkdir(parents=True)
    (root / "__init__.py").write_text("")
    (root / "attribution_methods" / "__init__.py").write_text("")
    (root / "attribution_methods" / "GIGBuilder.py").write_text(
        "WHO = 'sibling'\nclass CoreSaliency:\n    WHO = 'sibling core'\nclass GuidedIG:\n    WHO = 'sibling'\n"
        "def VisualizeImageGrayscale():\n    return 'sibling grayscale'\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", SIBLING, PKG, str(tmp_path / "sibling")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gig imports ok" in r.stdout


def test_k22_entry_points_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    lib = _lib.load()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first
    assert lib.xai_gig_init_f32(None, p, 1, 4, p, p, p, p, None) == -1
    assert lib.xai_gig_init_f32(p, p, 1, 4, p, p, p, None, None) == -1
    assert lib.xai_gig_init_f32(p, p, 0, 4, p, p, p, p, None) == -2
    assert lib.xai_gig_init_f32(p, p, 1, 0, p, p, p, p, None) == -2
    args = dict(n_img=1, n_elem=4, steps=50, fraction=0.5, max_dist=1.0)

    def step(ptrs=(p,) * 7, **kw):
        a = dict(args, **kw)
        return lib.xai_gig_step_f32(ptrs[0], ptrs[1], ptrs[2], a["n_img"], a["n_elem"], a["steps"], a["fraction"], a["max_dist"],
                                    ptrs[3], ptrs[4], ptrs[5], ptrs[6], None)
    for i in range(7):
        assert step(ptrs=tuple(None if j == i else p for j in range(7))) == -1, i
    assert step(n_img=0) == -2 and step(n_elem=0) == -2 and step(steps=0) == -2
    assert step(fraction=1.5) == -2 and step(fraction=-0.1) == -2 and step(max_dist=float("nan")) == -2
    assert step(n_img=70000) == -3
    # torch.quantile's own limit; above it fp32(n_elem - 1) can round up to n_elem and the rank would leave the image
    assert step(n_elem=2 ** 24 + 1) == -3 and step(n_elem=2 ** 24 + 4, fraction=1.0) == -3 and step(n_elem=2 ** 31) == -3
    assert lib.xai_gig_init_f32(p, p, 1, 2 ** 24 + 1, p, p, p, p, None) == -3


def test_guided_ig_refuses_the_cpu():
    from xai_engine import XaiHipError
    from xai_engine.guided_ig import guided_ig_batch
    from util.attribution_methods import GIGBuilder
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(XaiHipError):
        GIGBuilder.GuidedIG().GetMask(x, torch.nn.Identity(), "cpu", GIGBuilder.call_model_function, {"class_idx_str": 0})
    with pytest.raises(XaiHipError):
        guided_ig_batch(x, torch.nn.Identity(), torch.zeros(1, dtype=torch.long))


def _bits(t):
    return (t.numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_replays_the_reference_bit_for_bit(tag):
    """tests/golden/gig.npz holds the reference's own x and gradient of every step; gig_restated.step with torch's fp32 sums, from
    the recorded x[s] and g[s], gives x[s + 1] to the bit, the recorded number of quantile calls, and -- accumulated into the
    running total iteration by iteration, as the reference's `attr +=` does -- the reference's mask to the bit.  (The increments
    of the steps summed afterwards are NOT bit-equal for b, whose steps take two iterations: (T + a1) + a2 is not T + (a1 + a2).)"""
    g = load_golden("gig.npz")
    steps, fraction, max_dist = g[f"{tag}_params"].tolist()
    steps = int(steps)
    xin = torch.from_numpy(g[f"{tag}_input"])
    xb = torch.from_numpy(g["b_baseline"]) if tag == "b" else torch.zeros_like(xin)
    l1_total = gig_restated.l1(xin, xb)
    attr = torch.zeros_like(xin)
    for s in range(steps):
        x0 = torch.from_numpy(g[f"{tag}_x"][s])
        x, attr, sel, moved = gig_restated.step(x0, xin, xb, torch.from_numpy(g[f"{tag}_g"][s]), s, steps, fraction, max_dist, l1_total,
                                                sum_dtype=torch.float32, attr0=attr)
        np.testing.assert_array_equal(_bits(x), _bits(g[f"{tag}_x"][s + 1]), err_msg=f"x after step {s}")
        assert sel == g[f"{tag}_iters"][s], (s, sel)
        assert torch.equal(moved, x != x0)
    np.testing.assert_array_equal(_bits(attr), _bits(g[f"{tag}_mask"]))


def test_edge_matrix_covers_every_axis_value_on_both_paths():
    """Sizes divisible by 4 run on <4> and, through a misaligned view, on <1>: every fraction, max_dist, steps, baseline and gradient
    kind of the issue's matrix occurs among them, and among the sizes that only <1> can take."""
    cases = E.matrix(1)
    for div4 in (True, False):
        sub = [c for c in cases if (c.n % 4 == 0) == div4 and len(c.images) == 1]
        assert {c.fraction for c in sub} == set(E.FRACTIONS) and {c.max_dist for c in sub} == set(E.MAX_DISTS)
        assert {c.steps for c in sub} == set(E.STEPS)
        assert {c.images[0][0] for c in sub} == set(E.BASELINES) and {c.images[0][1] for c in sub} >= set(E.GRADS)
    assert {c.n for c in cases} >= set(E.SIZES_1) | set(E.SIZES_4)
    assert {len(c.images) for c in cases} == {1, 2, 7}


def test_edge_matrix_fp32_sums_against_fp64_sums():
    """The reference side alone: every case of the matrix through the restatement with K22's sums (fp64, rounded) and with torch's
    fp32 sums, each step from the same x.  The loop ends within the cap everywhere; the steps on which the two disagree about the
    selection count or the moved set are at most 2 % (none with `normal` gradients); on the others |x64 - x32| / |x_input - baseline|
    and the rel_inf of the running attribution are the CPU half of the tolerance the GPU tests assert (E.MEASURED_CPU)."""
    steps = out = 0
    worst = {"x_over_span": 0.0, "attr": 0.0}
    for c in E.matrix() + [E.full_size()]:
        for i in range(len(c.images)):
            xin, xb = c.inputs(i)
            for s, (r64, r32, x, attr, g) in enumerate(E.restated_run(c, i)):
                assert not isinstance(r64, str) and not isinstance(r32, str), (c, i, s, r64, r32)
                steps += 1
                if r64[2] != r32[2] or not torch.equal(r64[3], r32[3]):
                    assert c.images[i][1] != "normal", (c, i, s)
                    out += 1
                    continue
                ex, ea = E.errors32(r64[0], r64[1], r32, xin, xb)
                worst["x_over_span"], worst["attr"] = max(worst["x_over_span"], ex), max(worst["attr"], ea)
    print(f"steps {steps}, left out {out}, worst {worst}")
    assert steps >= 1500 and out <= E.MAX_DISAGREE * steps, (out, steps)
    for k, v in worst.items():
        check(f"gig/edges/cpu/restated64_vs_restated32/{k}", v, 0.0, E.TOL[k], against="restatement, fp32 sums", absolute=True)
    if E.SCALE == 1:                                      # the tolerance stays tied to what the default matrix measures here and now
        for k, v in worst.items():
            assert E.TOL[k] <= 2 * max(v, E.MEASURED_GPU[k]) * (1 + 1e-9), (k, v, E.TOL[k])


def test_cap_and_gamma_paths_of_the_restatement():
    """The inputs with which the GPU tests expect K22's status 2 and 3 (E.cap_cases, E.gamma_case) do raise the restatement's cap
    RuntimeError, on the step stated and not before, and its `assert gamma > 0`, with either arithmetic."""
    for c, at in zip(E.cap_cases(), (6, 9, 0)):
        log = E.restated_run(c)
        assert len(log) == at + 1 == c.steps, (c, len(log))
        assert all(not isinstance(r, str) for step in log[:-1] for r in step[:2]), c
        assert all(isinstance(r, str) and f"step {at}: 64 selections" in r for r in log[-1][:2]), (c, log[-1][:2])
    c, x = E.gamma_case()
    xin, xb = c.inputs(0)
    g = c.gradients(0)()
    for dt in (torch.float32, torch.float64):
        with pytest.raises(AssertionError):
            gig_restated.step(x, xin, xb, g, 0, c.steps, c.fraction, c.max_dist, gig_restated.l1(xin, xb, dt), sum_dtype=dt)
