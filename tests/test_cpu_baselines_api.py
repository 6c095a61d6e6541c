"""The mirror's Baselines serves every method of the reference's Baselines with the reference's parameters (no GPU needed).

tests/golden/baselines_api.json lists, for every public method of the reference's class, its parameter names and defaults
(tests/golden/make_golden_rave.py).  The evaluation scripts call these methods positionally and by keyword, so the reference's
parameters must be a prefix of the mirror's, with equal defaults; the mirror may only append keyword parameters."""
import inspect
import json
import os
import re

import pytest

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("xai_attn_head_importance_workspace_bytes", "xai_attn_head_importance_f32", "xai_rave_matrices_f32", "xai_rollout_row_f32",
               "xai_residual_shares_f32", "xai_attn_cam_f32")

with open(os.path.join(GOLDEN, "baselines_api.json")) as _f:
    API = json.load(_f)


@pytest.mark.parametrize("method", sorted(API))
def test_mirror_baselines_has_the_reference_signature(method):
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import Baselines
    assert hasattr(Baselines, method), f"Baselines.{method} is missing"
    params = list(inspect.signature(getattr(Baselines, method)).parameters.values())[1:]
    want = API[method]
    assert [p.name for p in params[:len(want)]] == [w["name"] for w in want]
    for p, w in zip(params, want):
        assert (p.default is not inspect.Parameter.empty) == w["has_default"], (method, p.name)
        if w["has_default"]:
            assert p.default == w["default"] and type(p.default) is type(w["default"]), (method, p.name, p.default, w["default"])
    for p in params[len(want):]:
        assert p.default is not inspect.Parameter.empty or p.kind is inspect.Parameter.KEYWORD_ONLY, (method, p.name)


def test_reference_call_sites_of_the_new_methods_bind():
    """imagenet_seg_eval.py:122 and the InFlow rows of the evaluation scripts; option='b' is not a parameter of the reference's
    generate_RAVE either, so it stays a TypeError."""
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import Baselines
    inspect.signature(Baselines.generate_cam_attn).bind(None, "x", 3, "cuda:0")
    inspect.signature(Baselines.generate_RAVE).bind(None, "x", 3, device="cuda:0")
    with pytest.raises(TypeError):
        inspect.signature(Baselines.generate_RAVE).bind(None, "x", 3, option="b", device="cuda:0")


def test_new_kernels_are_declared_in_the_header_and_bound():
    from xai_engine import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xai_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/xai_hip.h"
        assert name in _lib.SIGNATURES


def test_inflow_is_a_vit_attribution_of_the_harness():
    from xai_engine.sweep import VIT_ATTR_FUNCS
    assert "InFlow" in VIT_ATTR_FUNCS and "attn_gradcam" not in VIT_ATTR_FUNCS


def test_rave_argument_errors_come_before_any_device_work():
    import torch
    from xai_engine import XaiHipError
    from xai_engine.vit_attr import Baselines
    b = Baselines(torch.nn.Module())
    with pytest.raises(ValueError):
        b.generate_RAVE(torch.zeros(1, 3, 8, 8), 0, ablate=2)
    with pytest.raises(XaiHipError):
        b.generate_RAVE(torch.zeros(1, 3, 8, 8), 0, device="cpu")
    with pytest.raises(XaiHipError):
        b.generate_cam_attn(torch.zeros(1, 3, 8, 8), 0, "cpu")
