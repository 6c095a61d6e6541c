"""Transformer Attribution (t_attr) without a GPU: the module path and signature of the reference's LRP, the harness tuples and CLIs,
the fourth extension header (include/xai_hip_ext4.h) and its library, the argument checks K46-K52 make before any HIP call, the
methods that are refused, and the closed-form flow of tests/lrp_restated.py against the reference-made goldens (tests/golden/lrp.npz)."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import lrp_restated as R
from abi_libs import PINNED, built, declared, exported, exported_elsewhere
from conftest import GOLDEN, ROOT

EXT4_HEADER = os.path.join(ROOT, "include", "xai_hip_ext4.h")
ENTRIES = ["xai_lrp_add_chunk", "xai_lrp_add_parts_f32", "xai_lrp_add_scale_f32", "xai_lrp_add_workspace_bytes",
           "xai_lrp_attn_matrices_f32", "xai_lrp_clone_f32", "xai_lrp_gather_f32", "xai_lrp_half_product_f32", "xai_lrp_ratio_f32",
           "xai_lrp_split_f32"]
_p, _i, _l, _z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


# ------------------------------------------------------------------------------------------------ module path, tuples, CLIs
def test_lrp_is_importable_at_the_reference_path_with_the_reference_signature():
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import LRP
    import xai_engine.lrp
    assert LRP is xai_engine.lrp.LRP
    api = json.load(open(os.path.join(GOLDEN, "lrp_api.json")))["generate_LRP"]
    sig = inspect.signature(LRP.generate_LRP)
    got = [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in sig.parameters.items()]
    assert got == api
    assert [n for n, _ in api] == ["self", "input", "target_class", "method", "is_ablation", "start_layer", "withgrad", "device"]
    p = inspect.signature(xai_engine.lrp.transformer_attribution_batch).parameters
    assert list(p)[:8] == ["x", "model", "targets", "method", "withgrad", "start_layer", "is_ablation", "graphs"]
    assert (p["method"].default, p["withgrad"].default, p["start_layer"].default, p["is_ablation"].default, p["graphs"].default) == \
        ("transformer_attribution", True, 0, False, True)
    assert callable(xai_engine.lrp.clear_cache)
    assert set(xai_engine.lrp.LRP_COUNTS) == {"captures", "captures_refused", "replayed", "eager"}


def test_the_harness_tuples():
    from xai_engine import sweep
    assert sweep.VIT_LRP_ATTR_FUNCS == ("t_attr",)
    assert sweep.VIT_TRANS_ATTR_FUNCS == ("MDA",) and len(sweep.VIT_ATTR_FUNCS) == 10
    assert "t_attr" not in sweep.VIT_ATTR_FUNCS and "t_attr" not in sweep.CNN_ATTR_FUNCS


class _Passed(Exception):
    pass


@pytest.mark.parametrize("cli", ["evaluate_perturbation", "evaluate_sanity"])
def test_both_clis_take_t_attr_for_vit_models_and_refuse_it_for_cnn_models(cli, monkeypatch, capsys):
    import importlib
    mod = importlib.import_module(f"xai_engine.{cli}")
    assert "t_attr" in mod.build_parser().format_help()

    def passed(*a, **k):
        raise _Passed
    # whatever a CLI does first after its model-attribution check touches the device: that is as far as a CPU test goes
    monkeypatch.setattr(torch.cuda, "set_device", passed)
    if cli == "evaluate_perturbation":
        monkeypatch.setattr(mod.xd, "init_from_env", passed)
    for model in ("VIT16", "VIT32"):
        with pytest.raises(_Passed):
            mod.main(["--model", model, "--attr_func", "t_attr"])
    for model in ("R50", "R101", "RNXT"):
        with pytest.raises(SystemExit) as e:
            mod.main(["--model", model, "--attr_func", "t_attr"])
        assert e.value.code == 1
    assert capsys.readouterr().out.count("Model-attribution mismatch") == 3


def test_the_segmentation_cli_still_refuses_t_attr_by_name():
    from xai_engine import evaluate_imagenet_seg, segeval
    assert "t_attr" in segeval.REFUSED
    with pytest.raises(SystemExit, match="t_attr is not served"):
        evaluate_imagenet_seg.main(["--model", "VIT16", "--attr_func", "t_attr"])


# ------------------------------------------------------------------------------------------------ header and library
def test_ext4_header_parses_at_1_0_and_cites_the_reference():
    from xai_engine import _lib
    text = open(EXT4_HEADER).read()
    args, ret, version = _lib.parse_header(text, _lib.LIBRARIES["ext4"].defines)
    assert version == (1, 0) and (_lib.LIBRARIES["ext4"].version, _lib.LIBRARIES["ext4"].minor) == PINNED["ext4"] == (1, 0)
    assert sorted(args) == declared(EXT4_HEADER) == sorted(ENTRIES + ["xai_ext4_version", "xai_ext4_version_minor"])
    assert args["xai_lrp_split_f32"] == [_p, _i, _l, _p, _p, _p]
    assert args["xai_lrp_ratio_f32"] == [_p, _p, _p, _i, _l, _p, _p]
    assert args["xai_lrp_half_product_f32"] == [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]
    assert args["xai_lrp_add_parts_f32"] == [_p, _p, _p, _i, _l, _p, _p, _p, _z, _p]
    assert args["xai_lrp_add_scale_f32"] == [_p, _p, _i, _l, _p, _z, _p]
    assert args["xai_lrp_attn_matrices_f32"] == [_p, _p, _i, _i, _i, _i, _i, _p, _p]
    assert ret["xai_lrp_add_workspace_bytes"] is _z and all(t is _i for n, t in ret.items() if n != "xai_lrp_add_workspace_bytes")
    listed = text[text.index(" *   0 = "):text.index("#define XAI_EXT4_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    for name in ENTRIES:
        if name.endswith("_f32") and name != "xai_lrp_add_scale_f32":            # the two launches of K50 share one comment
            at = text.index(name + "(")
            comment = text[text.rfind("/*", 0, at):at]
            assert re.search(r"(replaces\s+|\()(layers_ours|ViT_LRP_timm)\.py:\d+", comment), name
    assert "starting from +0.0" in text and "ascending p" in text               # K50's summation order is stated


def test_ext4_library_exports_exactly_its_header_and_the_other_four_are_unchanged():
    from xai_engine import _lib
    assert exported(built("ext4")) == declared(EXT4_HEADER) == sorted(_lib.LIBRARIES["ext4"].signatures)
    lib = _lib.load("ext4")
    assert (lib.xai_ext4_version(), lib.xai_ext4_version_minor()) == (1, 0)
    assert lib.xai_lrp_add_chunk() == R.ADD_CHUNK == 4096
    # each other library exports exactly its own header (exported_elsewhere), none of them an entry of this feature
    assert not [(o, n) for o, n in exported_elsewhere("ext4") if n.startswith("xai_lrp_") or "ext4" in n]
    assert {k: (rec.version, rec.minor) for k, rec in _lib.LIBRARIES.items()} == PINNED


def test_k46_to_k52_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext4")
    lib = _lib.load("ext4")
    p = 16                               # a non-NULL, 16-byte aligned pointer that is never dereferenced: validation comes first
    assert lib.xai_lrp_split_f32(None, 1, 4, p, p, None) == lib.xai_lrp_split_f32(p, 1, 4, None, p, None) == -1
    assert [lib.xai_lrp_split_f32(p, 0, 4, p, p, None), lib.xai_lrp_split_f32(p, 1, 0, p, p, None)] == [-2, -2]
    assert [lib.xai_lrp_ratio_f32(None, p, None, 1, 4, p, None), lib.xai_lrp_ratio_f32(p, None, None, 1, 4, p, None)] == [-1, -1]
    assert lib.xai_lrp_ratio_f32(p, p, None, 1, -1, p, None) == -2
    assert lib.xai_lrp_gather_f32(p, p, None, 1, 4, p, None) == lib.xai_lrp_clone_f32(p, None, p, 1, 4, p, None) == -1
    assert lib.xai_lrp_gather_f32(p, p, p, -1, 4, p, None) == lib.xai_lrp_clone_f32(p, p, p, 1, 0, p, None) == -2

    def half(B=1, h=2, N=3, d=4, slots=3, slot=0, out=p):
        return lib.xai_lrp_half_product_f32(p, p, B, h, N, d, slots, slot, out, None)
    assert half(out=None) == -1
    assert [half(B=0), half(h=0), half(N=0), half(d=0), half(slots=2), half(slot=3), half(slot=-1), half(slots=1, slot=1)] == [-2] * 8

    assert lib.xai_lrp_add_workspace_bytes(1, 1) == lib.xai_lrp_add_workspace_bytes(1, 4096) == 24
    assert lib.xai_lrp_add_workspace_bytes(3, 4097) == 3 * 2 * 24
    assert lib.xai_lrp_add_workspace_bytes(0, 5) == lib.xai_lrp_add_workspace_bytes(1, 1 << 31) == lib.xai_lrp_add_workspace_bytes(65536, 5) == 0

    def parts(x0=p, ws=p, B=1, n=5000, nbytes=48):
        return lib.xai_lrp_add_parts_f32(x0, p, p, B, n, p, p, ws, nbytes, None)
    assert [parts(x0=None), parts(ws=None)] == [-1, -1]
    assert [parts(B=0), parts(n=0), parts(nbytes=47), parts(ws=20)] == [-2, -2, -2, -2]
    assert [parts(n=1 << 31), parts(B=65536, nbytes=1 << 40)] == [-3, -3]
    assert lib.xai_lrp_add_scale_f32(p, None, 1, 5000, p, 48, None) == -1
    assert lib.xai_lrp_add_scale_f32(p, p, 1, 5000, p, 24, None) == -2

    def mats(cam=p, out=p, L=1, B=1, h=1, S=5, mode=0):
        return lib.xai_lrp_attn_matrices_f32(cam, None, L, B, h, S, mode, out, None)
    assert [mats(cam=None), mats(out=None)] == [-1, -1]
    assert [mats(L=0), mats(B=0), mats(h=0), mats(S=0), mats(mode=3), mats(mode=-1)] == [-2] * 6
    assert [mats(L=65536), mats(B=65536)] == [-3, -3]


# ------------------------------------------------------------------------------------------------ the driver's refusals
def test_full_and_inflow_are_not_implemented_and_other_names_are_value_errors():
    from xai_engine import zoo
    from xai_engine.lrp import LRP, blocks_needed, transformer_attribution_batch
    model = zoo.vit_base_patch16_224(0, img=32, patch=8, dim=32, depth=1, heads=4, num_classes=10)
    x = torch.zeros(1, 3, 32, 32)
    for method in ("full", "InFlow"):
        with pytest.raises(NotImplementedError, match=method):
            LRP(model).generate_LRP(x, 0, method=method)
        with pytest.raises(NotImplementedError, match=method):
            transformer_attribution_batch(x, model, 0, method=method)
    with pytest.raises(ValueError, match="unknown method 'attn'"):
        LRP(model).generate_LRP(x, 0, method="attn")
    with pytest.raises(IndexError):                                       # the reference's self.blocks[1] on a one-block model
        blocks_needed("second_layer", 1, 0)
    with pytest.raises(IndexError):
        blocks_needed("transformer_attribution", 2, 2)
    assert blocks_needed("transformer_attribution", 3, 1) == [1, 2] and blocks_needed("last_layer", 3, 0) == [2]
    assert blocks_needed("second_layer", 3, 0) == [1] and blocks_needed("last_layer_attn", 3, 0) == []


def test_a_model_of_another_layout_is_a_type_error_naming_what_is_missing():
    from xai_engine import zoo
    from xai_engine.lrp import LRP
    with pytest.raises(TypeError, match="`patch_embed`"):
        LRP(torch.nn.Linear(2, 2))
    model = zoo.vit_base_patch16_224(0, img=32, patch=8, dim=32, depth=2, heads=4, num_classes=10)
    del model.blocks[1].mlp.fc2
    with pytest.raises(TypeError, match=r"`blocks\[1\]\.mlp\.fc2`"):
        LRP(model)


# ------------------------------------------------------------------------------------------------ the restated flow
def test_the_pinned_sum_is_the_stated_tree():
    rng = np.random.default_rng(0)
    for n in (1, 5, 4095, 4096, 4097, 10000):
        v = rng.standard_normal(n).astype(np.float32)
        lanes = [0.0] * (-(-n // 4096) * 256)
        for i in range(n):                                                # lane (i / 4) % 256 of chunk i / 4096, ascending i
            lanes[(i // 4096) * 256 + (i % 4096 // 4) % 256] += float(v[i])
        total = 0.0
        for c in range(len(lanes) // 256):
            part = 0.0
            for w in range(4):
                t = lanes[c * 256 + w * 64:c * 256 + w * 64 + 64]
                for off in (32, 16, 8, 4, 2, 1):
                    t = [t[k] + t[k ^ off] for k in range(64)]
                part += t[0]
            total += part
        assert R.pinned_sum(v) == total
    assert abs(R.pinned_sum(np.ones(10000, np.float32)) - 10000.0) == 0.0


@pytest.fixture(scope="module", params=list(R.FIXTURES))
def fixture(request):
    return (request.param,) + R.load_fixture(request.param, GOLDEN)


def test_every_stored_fixture_has_a_gap_of_at_most_1e_5(fixture):
    name, _, _, _, g = fixture
    gaps = [k for k in g.files if k.startswith(name + "/") and k.endswith("/gap")]
    assert len(gaps) >= R.IMAGES * len(R.CALLS)
    for k in gaps:
        f32, f64 = g[k[:-3] + "f32"], g[k[:-3] + "f64"]
        assert f32.dtype == np.float32 and f64.dtype == np.float64
        assert float(g[k]) == R.rel_err(f32, f64) <= 1e-5, k


def test_the_restated_flow_meets_the_reference_fp64_goldens(fixture):
    """tests/lrp_restated.py in fp32 on the CPU against the reference's own fp64 result: at most max(1e-5, 4 x the reference's own
    fp32-to-fp64 gap) (lrp_restated.bound has the reasoning)."""
    name, model, xs, targets, g = fixture
    torch.set_num_threads(min(8, torch.get_num_threads()))
    for j in range(R.IMAGES):
        for key, kw in R.CALLS.items():
            got, cams = R.generate(model, xs[j:j + 1], targets[j:j + 1], **kw)
            want, gap = g[f"{name}/{j}/{key}/f64"], g[f"{name}/{j}/{key}/gap"]
            assert got.shape == want.shape
            err = R.rel_err(got.numpy(), want)
            assert err <= R.bound(gap), (name, j, key, err, float(gap))
            if name == "mini" and key == "transformer_attribution":
                for i, cam in cams.items():
                    err = R.rel_err(cam.numpy(), g[f"{name}/{j}/cam{i}/f64"])
                    assert err <= R.bound(g[f"{name}/{j}/cam{i}/gap"]), (name, j, f"cam{i}", err)


def test_the_restated_flow_gives_each_image_of_a_batch_its_own_result():
    name = "mini"
    model, xs, targets, g = R.load_fixture(name, GOLDEN)
    got, _ = R.generate(model, xs, targets)
    for j in range(R.IMAGES):
        err = R.rel_err(got[j:j + 1].numpy(), g[f"{name}/{j}/transformer_attribution/f64"])
        assert err <= R.bound(g[f"{name}/{j}/transformer_attribution/gap"]), (j, err)
    none, _ = R.generate(model, xs, None)                                  # the fixtures' targets are the argmax
    assert torch.equal(none, got)
