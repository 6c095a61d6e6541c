"""The sanity test without a GPU: the grown second extension header (include/xai_hip_ext2.h at minor 1) and its library, the
argument checks K39-K43 make before any HIP call, the yardstick itself (tests/sanity_restated.py; against skimage where that is
installed), the two randomisers against a transcription of the reference's traversal, and the reference's Counter fold."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sanity_restated as R
from abi_libs import PINNED, built, declared, exported
from conftest import ROOT

EXT2_HEADER = os.path.join(ROOT, "include", "xai_hip_ext2.h")
NEW = ["xai_hog_f32", "xai_hog_workspace_bytes", "xai_rank_corr_f64", "xai_rank_corr_max_n", "xai_sanity_normalize_f32", "xai_ssim_f32",
       "xai_ssim_tile", "xai_ssim_workspace_bytes", "xai_tie_ranks_chunk", "xai_tie_ranks_i32"]
_p, _i, _l, _f, _d, _z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t


# ------------------------------------------------------------------------------------------------ header and library
def test_ext2_header_parses_at_minor_1_with_the_sanity_entries():
    from xai_engine import _lib
    text = open(EXT2_HEADER).read()
    args, ret, version = _lib.parse_header(text, _lib.LIBRARIES["ext2"].defines)
    assert version == (1, 1) == PINNED["ext2"] and _lib.LIBRARIES["ext2"].minor == 1
    assert set(NEW) <= set(args) and sorted(args) == declared(EXT2_HEADER)
    assert args["xai_sanity_normalize_f32"] == [_p, _i, _l, _i, _p, _p]
    assert args["xai_ssim_f32"] == [_p, _p, _i, _i, _i] + [_d] * 6 + [_f, _f, _p, _p, _p, _z, _p]
    assert args["xai_tie_ranks_i32"] == [_p, _p, _i, _l, _p, _p]
    assert args["xai_rank_corr_f64"] == [_p, _p, _p, _p, _i, _l, _p, _p]
    assert args["xai_hog_f32"] == [_p, _i, _i, _i, _i, _i, _p, _p, _z, _p]
    assert all(t is _i for t in ret.values())
    # the minor's comment lists every new entry, and every launch entry cites the reference lines it replaces
    listed = text[text.index(" *   1 = "):text.index("#define XAI_EXT2_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == NEW
    for name in NEW:
        if name.endswith(("_f32", "_f64", "_i32")):
            at = text.index(name + "(")
            comment = text[text.rfind("/*", 0, at):at]
            assert re.search(r"replaces\s+evaluateSanity\.py:\d+", comment), name


def test_ext2_library_exports_exactly_the_declared_symbols():
    from xai_engine import _lib
    assert exported(built("ext2")) == declared(EXT2_HEADER) == sorted(_lib.LIBRARIES["ext2"].signatures)
    lib = _lib.load("ext2")
    assert (lib.xai_ext2_version(), lib.xai_ext2_version_minor()) == (1, 1)
    assert lib.xai_ssim_tile() >= 11 and lib.xai_tie_ranks_chunk() >= 64 and lib.xai_rank_corr_max_n() == 131072


def test_the_five_kernels_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext2")
    lib = _lib.load("ext2")
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def norm(x=p, out=p, n=1, hw=64):
        return lib.xai_sanity_normalize_f32(x, n, hw, 1, out, None)
    assert [norm(x=None), norm(out=None), norm(n=0), norm(hw=0)] == [-1, -1, -2, -2]

    assert lib.xai_ssim_workspace_bytes(3, 224, 224) == 3 * 7 * 7 * 8 and lib.xai_ssim_workspace_bytes(0, 224, 224) == 0

    def ssim(x=p, y=p, mean=p, ws=p, n=1, H=16, W=16, nbytes=8):
        return lib.xai_ssim_f32(x, y, n, H, W, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 1e-4, 1e-3, mean, None, ws, nbytes, None)
    assert [ssim(**{k: None}) for k in ("x", "y", "mean", "ws")] == [-1] * 4
    assert ssim(H=10) == -2 and ssim(W=10) == -2 and ssim(n=0) == -2           # skimage raises below 11 x 11
    assert ssim(nbytes=7) == -2 and ssim(ws=20) == -2 and ssim(n=65536, nbytes=1 << 20) == -3

    def tie(vals=p, order=p, out=p, rows=1, n=8):
        return lib.xai_tie_ranks_i32(vals, order, rows, n, out, None)
    assert [tie(vals=None), tie(order=None), tie(out=None), tie(rows=0), tie(n=0), tie(rows=65536)] == [-1, -1, -1, -2, -2, -3]

    def corr(ra=p, rb=p, out=p, pairs=1, n=8):
        return lib.xai_rank_corr_f64(ra, rb, None, None, pairs, n, out, None)
    assert [corr(ra=None), corr(rb=None), corr(out=None), corr(pairs=0), corr(n=1)] == [-1, -1, -1, -2, -2]
    assert corr(n=131073) == -3                                                 # XAI_E_UNSUPPORTED: the driver goes to scipy

    assert lib.xai_hog_workspace_bytes(2, 224, 224, 16, 16) == 2 * 14 * 14 * 9 * 8

    def hog(img=p, out=p, ws=p, n=1, H=48, W=48, ch=16, cw=16, nbytes=9 * 9 * 8):
        return lib.xai_hog_f32(img, n, H, W, ch, cw, out, ws, nbytes, None)
    assert [hog(img=None), hog(out=None), hog(ws=None)] == [-1] * 3
    assert hog(H=47) == -2 and hog(W=47) == -2 and hog(ch=0) == -2 and hog(nbytes=9 * 9 * 8 - 1) == -2


# ------------------------------------------------------------------------------------------------ the yardstick
def test_restated_ssim_is_one_for_identical_maps_and_hog_has_the_documented_length():
    rng = np.random.default_rng(0)
    x = rng.random((40, 52), dtype=np.float32)
    mean, S = R.ssim(x, x.copy())
    assert abs(mean - 1.0) <= 1e-6 and S.shape == x.shape and S.dtype == np.float32
    with pytest.raises(ValueError):
        R.ssim(x[:10], x[:10])
    for H, W, cell in ((48, 48, (16, 16)), (50, 70, (16, 16)), (24, 40, (8, 8)), (224, 224, (16, 16))):
        f = R.hog(rng.random((H, W), dtype=np.float32), cell)
        assert f.shape == (R.hog_length(H, W, cell),) and f.dtype == np.float32
    assert R.hog_length(224, 224) == 11664
    with pytest.raises(ValueError):
        R.hog(x[:, :47])


def test_restated_hog_bins_of_an_axis_aligned_step():
    img = np.zeros((48, 48), np.float32)
    img[:, 24:] = 1.0                                    # g_col = +1 at columns 23, 24: orientation exactly 0
    mag, ori = R.hog_gradients(img)
    assert set(np.unique(ori[mag > 0])) == {0.0}
    mag, ori = R.hog_gradients(img.T.copy())             # g_row = +1: exactly 90
    assert set(np.unique(ori[mag > 0])) == {90.0}
    mag, ori = R.hog_gradients(1 - img)                  # g_col = -1: atan2 gives pi, 180 % 180 = 0
    assert set(np.unique(ori[mag > 0])) == {0.0}


def test_restated_normalize_image_has_both_variants():
    x = np.full((4, 4), 3.0, np.float32)
    assert np.array_equal(R.normalize_image(x, guard=True), x) and np.isnan(R.normalize_image(x, guard=False)).all()
    y = np.array([[1.0, np.inf], [-np.inf, 3.0]], np.float32)
    assert np.array_equal(R.normalize_image(y), np.array([[1 / 3, 0], [0, 1]], np.float32))


def test_restated_ssim_and_hog_against_skimage():
    metrics = pytest.importorskip("skimage.metrics")
    feature = pytest.importorskip("skimage.feature")
    rng = np.random.default_rng(1)
    for H, W in ((48, 48), (50, 70), (224, 224)):
        a, b = rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32)
        want, S = metrics.structural_similarity(a, b, gaussian_weights=True, data_range=2.0, full=True)
        got, S_got = R.ssim(a, b, 2.0)
        assert np.array_equal(S_got, S) and got == want
        want = feature.hog(a, pixels_per_cell=(16, 16))
        assert np.abs(R.hog(a) - want).max() <= 2.4e-7


# ------------------------------------------------------------------------------------------------ the randomisers
def _transcribed_cnn(model):
    """evaluateSanity.py:108-120, the traversal as the reference walks it"""
    for _, layer in model.named_modules():
        if isinstance(layer, torch.nn.Module) and len(list(layer.parameters())) > 0:
            with torch.no_grad():
                if isinstance(layer, torch.nn.Conv2d):
                    torch.nn.init.kaiming_uniform_(layer.weight, nonlinearity="relu")
                elif isinstance(layer, torch.nn.Linear):
                    torch.nn.init.xavier_uniform_(layer.weight)
    return model


def _transcribed_vit(model, fn=torch.nn.init.normal_):
    """evaluateSanity.py:122-130"""
    for _, layer in model.named_modules():
        if isinstance(layer, torch.nn.Module) and len(list(layer.parameters())) > 0:
            with torch.no_grad():
                for param in layer.parameters():
                    fn(param)
    return model


def _small_cnn():
    from xai_engine.zoo import resnet50
    return resnet50(seed=0, width=8, num_classes=10)


def _small_vit():
    from xai_engine.zoo import VisionTransformer
    torch.manual_seed(0)
    return VisionTransformer(img=32, patch=8, dim=32, depth=2, heads=4, num_classes=10)


@pytest.mark.parametrize("kind", ["cnn", "vit"])
def test_randomisers_draw_what_the_references_traversal_draws(kind):
    from xai_engine import sanity
    make, ours, theirs = ((_small_cnn, sanity.randomize_CNN_model, _transcribed_cnn) if kind == "cnn" else
                          (_small_vit, sanity.randomize_VIT_model, _transcribed_vit))
    base = make()
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    torch.manual_seed(123)
    assert ours(a) is a
    after_ours = torch.rand(4)
    torch.manual_seed(123)
    theirs(b)
    after_theirs = torch.rand(4)
    assert torch.equal(after_ours, after_theirs)                     # the generator was consumed identically
    changed = []
    for (name, p0), p1, p2 in zip(base.state_dict().items(), a.state_dict().values(), b.state_dict().values()):
        assert torch.equal(p1, p2), name                             # the same tensors, the same values
        if not torch.equal(p0, p1):
            changed.append(name)
    if kind == "cnn":
        weights = {n + ".weight" for n, m in base.named_modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))}
        assert set(changed) == weights and len(weights) > 50         # no bias, no BatchNorm tensor
    else:
        assert set(changed) == {n for n, _ in base.named_parameters()}


# ------------------------------------------------------------------------------------------------ the fold and the CSV
def test_reference_counter_fold_drops_a_negative_spr(tmp_path):
    from xai_engine import sanity
    rows = [(0.5, -0.2, 0.3), (0.4, 0.1, 0.2), (0.3, 0.3, float("nan"))]
    total = sanity.fold_reference_counter(rows)
    # SPR: -0.2 + 0.1 < 0 is dropped at the second image and starts again from 0.3, at the end; HOG: the NaN sum is dropped
    assert list(total) == ["SSIM", "SPR"] and total["SSIM"] == 0.5 + 0.4 + 0.3 and total["SPR"] == 0.3
    assert sanity.fold_reference_counter([(0.5, -0.2, 0.3)]) == {"SSIM": 0.5, "SPR": -0.2, "HOG": 0.3}      # the first as it is
    path = tmp_path / "out" / "R50" / "gc_3_images.csv"
    sanity.write_csv(str(path), total, 3, 1.5)
    assert open(path).read().splitlines() == [f"SSIM,{total['SSIM'] / 3}", f"SPR,{0.3 / 3}", "Total Runtime,1.5"]


def test_cli_has_the_references_flags_and_refuses_clip():
    from xai_engine import evaluate_sanity, evaluate_perturbation
    opts = {a.dest for a in evaluate_sanity.build_parser()._actions}
    assert {"image_count", "model", "attr_func", "cuda_num", "dataset_path", "weights", "class_map", "out_dir", "reference_counter"} <= opts
    for cli in (evaluate_sanity, evaluate_perturbation):
        with pytest.raises(SystemExit, match="unknown --model CLIP16"):
            cli.main(["--model", "CLIP16"])


def test_mirrored_module_serves_the_references_names():
    from util.test_methods import sanityForMethods as M
    for name in ("get_layers", "independent_layer_rand", "cascading_layer_rand", "normalize_image", "evaluate"):
        assert callable(getattr(M, name))
    model, empty = _small_vit(), _small_vit()
    layers = M.get_layers(model)
    assert layers[0] == next(iter(model.state_dict())).split(".")[0] and len(layers) == len(set(layers))
    with torch.no_grad():
        for p in empty.parameters():
            p.fill_(0.5)
        first = next(n for n, _ in model.named_parameters() if n.startswith(layers[0]))
        empty.state_dict()[first].zero_()
    before = copy.deepcopy(model.state_dict())
    torch.manual_seed(3)
    M.independent_layer_rand(model, empty, layers[0])
    torch.manual_seed(3)
    want_rand = torch.rand(before[first].shape)
    for n, v in model.state_dict().items():
        if n == first:
            assert torch.equal(v, want_rand)                         # all-zero in empty_model: torch.rand of the shape
        elif n.startswith(layers[0]) and n in dict(model.named_parameters()):
            assert torch.equal(v, torch.full_like(v, 0.5))
        else:
            assert torch.equal(v, before[n]), n
    M.cascading_layer_rand(model, empty, layers, 1)
    assert all(torch.equal(v, torch.full_like(v, 0.5)) for n, v in model.named_parameters() if n.startswith(layers[1]))
