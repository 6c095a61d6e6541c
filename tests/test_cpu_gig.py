"""Guided IG without a GPU: the harness row, the mirror module's interface and resolution, and the argument checks of the
K22 entry points (made before any HIP call)."""
import inspect
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import GOLDEN, PKG

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


def test_guided_ig_refuses_the_cpu():
    from xai_engine import XaiHipError
    from xai_engine.guided_ig import guided_ig_batch
    from util.attribution_methods import GIGBuilder
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(XaiHipError):
        GIGBuilder.GuidedIG().GetMask(x, torch.nn.Identity(), "cpu", GIGBuilder.call_model_function, {"class_idx_str": 0})
    with pytest.raises(XaiHipError):
        guided_ig_batch(x, torch.nn.Identity(), torch.zeros(1, dtype=torch.long))
