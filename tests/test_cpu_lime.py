"""LIME without a GPU: the yardstick of the GPU tests (tests/lime_restated.py against the reference's recorded runs,
tests/golden/lime.npz), the host side of xai_engine/lime.py (the data draw, the bit packing, the host fit, the argument checks),
the mirror package's interface and resolution, the harness row and the argument checks of the K31 - K33 entry points (made before
any HIP call)."""
import inspect
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import lime_restated as R
from conftest import BAR, GOLDEN, PKG, check, load_golden

with open(os.path.join(GOLDEN, "lime_api.json")) as _f:
    API = json.load(_f)
CASES = R.GOLDEN_CASES
golden_case = R.golden_case


@pytest.mark.parametrize("tag", CASES)
def test_restatement_meets_the_reference(tag):
    g = load_golden("lime.npz")
    c = golden_case(g, tag)
    mine = R.explain(c["data"], c["labels"][:, c["top"]])
    check(f"lime_restated/{tag}/dist", mine["dist"], g[f"{tag}_dist"], BAR, against="reference LIME")
    check(f"lime_restated/{tag}/coef", mine["coef"], c["coef"], BAR, against="reference LIME")
    for k in ("intercept", "score", "local_pred"):
        check(f"lime_restated/{tag}/{k}", mine[k], g[f"{tag}_{k}"], BAR, against="reference LIME")
    err = float(g[f"{tag}_err"])
    assert err <= 1e-12 and R.conditioned(mine, err)
    np.testing.assert_array_equal(mine["order"], c["order"])
    np.testing.assert_array_equal(R.mask_of(c["seg"], mine["order"][0], mine["coef"][0]), g[f"{tag}_mask"])
    np.testing.assert_array_equal(R.top_labels(c["labels"][0], 5), c["top"])


def test_fixture_is_small_and_covers_the_cases():
    g = load_golden("lime.npz")
    assert os.path.getsize(os.path.join(GOLDEN, "lime.npz")) < 200 * 1024
    assert [tuple(g[f"in{i}_seg"].shape) for i in range(2)] == [(40, 36), (65, 63)]
    assert all(g[f"in{i}_seg"].dtype == np.int16 for i in range(2))
    got = {t: golden_case(g, t) for t in CASES}
    assert [(c["N"], c["D"], c["hide"]) for c in got.values()] == [(200, 24, 0.0), (200, 24, None), (300, 70, 0.0), (300, 70, None)]
    assert all(c["labels"].dtype == np.float32 and c["labels"].shape == (c["N"], 10) for c in got.values())
    assert all((c["data"][0] == 1).all() for c in got.values())


@pytest.mark.parametrize("tag", CASES)
def test_host_draw_is_the_references_matrix(tag):
    """RandomState(seed): the seed draw of lime_image.py:174-175 first, then the matrix of :249-252."""
    from xai_engine import lime
    c = golden_case(load_golden("lime.npz"), tag)
    rs = lime._random_state(c["seed"])
    assert 0 <= lime.draw_seed(rs) < 1000
    np.testing.assert_array_equal(lime.draw_data(rs, c["N"], c["D"]), c["data"])
    rs = np.random.RandomState(c["seed"])
    assert not np.array_equal(lime.draw_data(rs, c["N"], c["D"]), c["data"])          # without the seed draw it is another matrix
    assert lime._random_state(rs) is rs and lime._random_state(None) is np.random.mtrand._rand


@pytest.mark.parametrize("D", [1, 63, 64, 65, 130])
def test_rows_are_packed_bit_z_of_word_z_div_64(D):
    from xai_engine import lime
    data = np.random.default_rng(D).integers(0, 2, (7, D))
    data[0] = 1
    got = lime.pack_rows(data)
    assert got.dtype == np.uint64 and got.shape == (7, (D + 63) // 64)
    np.testing.assert_array_equal(got, R.pack(data))
    for z in range(D):
        np.testing.assert_array_equal((got[:, z // 64] >> np.uint64(z % 64)) & np.uint64(1), data[:, z].astype(np.uint64))
    assert int(got[0, -1]) == (1 << (D - 64 * (got.shape[1] - 1))) - 1                # the bits behind D are zero
    wide = lime.pack_rows(data, got.shape[1] + 1)
    np.testing.assert_array_equal(wide[:, :-1], got)
    assert not wide[:, -1].any()
    with pytest.raises(ValueError, match="words"):
        lime.pack_rows(np.ones((2, 65), int), 1)


@pytest.mark.parametrize("shape", [(200, 24, 5), (50, 128, 2), (8, 3, 1), (1, 5, 2), (300, 130, 3)])
def test_host_fit_meets_the_restatement(shape):
    """The fit `lime_batch` falls back to above K32's cap: the same closed form, the same two stable sorts."""
    from xai_engine import lime
    N, D, L = shape
    data, Y = R.seeded_fit_case(N, D, L, seed=N + D, zero_rows=1 if N == 8 else 0)
    got, want = lime.host_fit(data, Y), R.explain(data, Y)
    for k in ("dist", "weight", "coef", "intercept", "local_pred"):
        check(f"lime_host_fit/{shape}/{k}", got[k], want[k], BAR, against="restated LIME")
    np.testing.assert_array_equal(got["order"], want["order"])
    if N == 1:
        assert np.isnan(got["score"]).all() and np.isnan(want["score"]).all() and not got["coef"].any()
        assert got["order"].tolist() == [list(range(D))] * L
    else:
        check(f"lime_host_fit/{shape}/score", got["score"], want["score"], BAR, against="restated LIME")
        assert R.conditioned(want, np.abs(got["coef"] - want["coef"]).max())


def test_get_image_and_mask_replays_the_references_masks():
    from xai_engine.lime import ImageExplanation
    g = load_golden("lime.npz")
    for tag in CASES:
        c = golden_case(g, tag)
        exp = ImageExplanation(c["image"], c["seg"].astype(np.int64))
        for l, label in enumerate(c["top"]):
            exp.local_exp[int(label)] = [(int(f), float(c["coef"][l, f])) for f in c["order"][l]]
        img, mask = exp.get_image_and_mask(int(c["top"][0]), positive_only=True, hide_rest=False)
        np.testing.assert_array_equal(mask, g[f"{tag}_mask"])
        assert mask.dtype == np.int64 and np.array_equal(img, c["image"])
        hidden, _ = exp.get_image_and_mask(int(c["top"][0]), positive_only=True, hide_rest=True)
        assert np.array_equal(hidden[mask == 1], c["image"][mask == 1]) and not hidden[mask == 0].any()
        _, neg = exp.get_image_and_mask(int(c["top"][0]), positive_only=False, negative_only=True, num_features=3)
        want = [f for f in c["order"][0] if c["coef"][0, f] < 0][:3]
        assert set(np.unique(c["seg"][neg == 1]).tolist()) == set(int(f) for f in want)
        _, both = exp.get_image_and_mask(int(c["top"][0]), positive_only=False, num_features=4)
        for f in c["order"][0][:4]:
            assert (both[c["seg"] == f] == (1 if c["coef"][0, f] >= 0 else -1)).all()
        with pytest.raises(KeyError):
            exp.get_image_and_mask(-1)
        with pytest.raises(ValueError, match="cannot be true at the same time"):
            exp.get_image_and_mask(int(c["top"][0]), positive_only=True, negative_only=True)


@pytest.mark.parametrize("name", sorted(API))
def test_mirror_has_the_reference_signature(name):
    from util.attribution_methods.lime import limeAttr, lime_image
    obj = lime_image if "." in name else limeAttr
    for part in name.split("."):
        obj = getattr(obj, part)
    params = list(inspect.signature(obj).parameters.values())[1 if "." in name else 0:]
    want = API[name]
    assert [p.name for p in params] == [w["name"] for w in want]
    for p, w in zip(params, want):
        assert (p.default is not inspect.Parameter.empty) == w["has_default"], (name, p.name)
        if w["has_default"]:
            default = list(p.default) if isinstance(p.default, tuple) else p.default
            assert default == w["default"] and type(default) is type(w["default"]), (name, p.name, p.default, w["default"])


def test_lime_is_a_cnn_attribution_of_the_harness_and_the_cli():
    from xai_engine.sweep import CNN_ATTR_FUNCS, TRANS_ATTR_FUNCS
    from xai_engine.evaluate_perturbation import build_parser
    assert "lime" in CNN_ATTR_FUNCS and "lime" in TRANS_ATTR_FUNCS
    assert " lime," in build_parser().format_help()


def test_arguments_the_device_path_does_not_serve_are_refused():
    from xai_engine import XaiHipError
    from xai_engine import lime
    img = np.zeros((8, 8, 3), np.float32)
    seg = np.arange(64).reshape(8, 8) // 16
    model = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="kernel"):
        lime.LimeImageExplainer(kernel=lambda d, kernel_width: d)
    for fs in ("forward_selection", "lasso_path", "none"):
        with pytest.raises(NotImplementedError, match="feature_selection"):
            lime.LimeImageExplainer(feature_selection=fs)
    ex = lime.LimeImageExplainer(feature_selection="highest_weights", random_state=3)
    with pytest.raises(NotImplementedError, match="batch_predict"):
        ex.explain_instance(img, lambda images, model, device: None, model, "cuda:0", segmentation_fn=lambda im: seg)
    with pytest.raises(NotImplementedError, match="model_regressor"):
        ex.explain_instance(img, lime.batch_predict, model, "cuda:0", segmentation_fn=lambda im: seg, model_regressor=object())
    with pytest.raises(NotImplementedError, match="distance_metric"):
        ex.explain_instance(img, lime.batch_predict, model, "cuda:0", segmentation_fn=lambda im: seg, distance_metric="euclidean")
    with pytest.raises(NotImplementedError, match="num_features"):
        ex.explain_instance(img, lime.batch_predict, model, "cuda:0", segmentation_fn=lambda im: seg, num_features=3)
    with pytest.raises(NotImplementedError, match="num_features"):
        lime.LimeImageExplainer().explain_instance(img, lime.batch_predict, model, "cuda:0", segmentation_fn=lambda im: seg, num_features=6)
    with pytest.raises(XaiHipError):
        ex.explain_instance(img, lime.batch_predict, model, "cpu", segmentation_fn=lambda im: seg)
    with pytest.raises(XaiHipError):
        lime.lime_batch(torch.zeros(1, 3, 8, 8), model, seg)
    with pytest.raises(ValueError, match="without gaps.*2 is missing.*lime_image.py"):
        lime.check_segments(np.where(seg == 2, 4, seg))
    with pytest.raises(ValueError, match="negative superpixel id -1.*never be perturbed"):
        lime.check_segments(seg - 1)
    with pytest.raises(ValueError, match="integer ids"):
        lime.check_segments(seg.astype(np.float32))
    s32, D = lime.check_segments(torch.from_numpy(seg))
    assert D == 4 and s32.dtype == np.int32


def test_segment_mean_image_is_the_references_expression():
    from xai_engine.lime import segment_mean_image
    seg, image = R.seeded_case(12, 9, 5, 2)
    got = segment_mean_image(image, seg)
    want = image.copy()
    for s in np.unique(seg):                     # lime_image.py:188-192, restated
        want[seg == s] = (np.mean(image[seg == s][:, 0]), np.mean(image[seg == s][:, 1]), np.mean(image[seg == s][:, 2]))
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(got, R.segment_means(image, seg))


def test_k31_k32_k33_entry_points_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    lib = _lib.load()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first
    assert lib.xai_lime_max_features() == 128

    def compose(ptrs=(p,) * 5, hide=p, fudged=None, words=1, B=2, C=3, H=5, W=7, N=10, first=0, n=4):
        x, seg, rows, D, out = ptrs
        return lib.xai_lime_compose_f32(x, seg, rows, D, words, hide, fudged, B, C, H, W, N, first, n, out, None)
    for i in range(5):
        assert compose(ptrs=tuple(None if j == i else p for j in range(5))) == -1, i
    assert compose(hide=None) == -1
    assert compose(B=0) == -2 and compose(C=0) == -2 and compose(H=0) == -2 and compose(W=-1) == -2 and compose(N=0) == -2
    assert compose(n=0) == -2 and compose(first=-1) == -2 and compose(words=0) == -2 and compose(first=17) == -2 and compose(n=21) == -2
    assert compose(words=2049) == -3 and compose(B=3, N=2 ** 30) == -3

    def fit(ptrs=(p,) * 10, words=1, B=2, N=10, L=5, stride=64, kw=0.25, a1=0.01, a2=1.0):
        rows, D, Y, coef, icpt, score, pred, order, dist, weight = ptrs
        return lib.xai_lime_fit_f64(rows, words, D, Y, B, N, L, stride, kw, a1, a2, coef, icpt, score, pred, order, dist, weight, None)
    for i in range(10):
        assert fit(ptrs=tuple(None if j == i else p for j in range(10))) == -1, i
    assert fit(B=0) == -2 and fit(N=0) == -2 and fit(L=0) == -2 and fit(words=0) == -2 and fit(stride=0) == -2
    assert fit(kw=0.0) == -2 and fit(kw=float("nan")) == -2 and fit(a1=0.0) == -2 and fit(a2=-1.0) == -2
    assert fit(B=3, N=2 ** 30) == -3

    def paint(table=p, seg=p, out=p, B=2, stride=64, H=5, W=7):
        return lib.xai_lime_paint_f32(table, seg, B, stride, H, W, out, None)
    assert paint(table=None) == -1 and paint(seg=None) == -1 and paint(out=None) == -1
    assert paint(B=0) == -2 and paint(stride=0) == -2 and paint(H=0) == -2 and paint(W=0) == -2


def test_quickshift_segments_without_skimage_says_what_still_works():
    from xai_engine.lime import quickshift_segments
    try:
        import skimage  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match=r"segments= / segmentation_fn="):
            quickshift_segments(np.zeros((8, 8, 3), np.float32), 1)
    else:
        assert quickshift_segments(np.random.default_rng(0).random((32, 32, 3)), 1).shape == (32, 32)


ALONE = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[1])
    from util.attribution_methods.lime import limeAttr, lime_image                # evaluatePerturbation.py:40
    import xai_engine.lime as x
    assert limeAttr.get_lime_attr is x.get_lime_attr and limeAttr.batch_predict is x.batch_predict and limeAttr.make_tensor is x.make_tensor
    assert lime_image.LimeImageExplainer is x.LimeImageExplainer and lime_image.ImageExplanation is x.ImageExplanation
    for mod in (limeAttr, lime_image):
        try:
            mod.WHO
        except AttributeError as e:
            assert "follows it on sys.path" in str(e), e
        else:
            raise AssertionError("expected AttributeError")
    try:
        from util.attribution_methods.lime import lime_base
    except ImportError:
        pass
    else:
        raise AssertionError("expected ImportError")
    print("alone ok")
""")
SIBLING = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])          # build first, sibling tree after it
    from util.attribution_methods.lime import limeAttr, lime_image, lime_base
    from util.attribution_methods.lime.wrappers.scikit_image import SegmentationAlgorithm
    from util.attribution_methods.lime.utils import generic_utils
    import xai_engine.lime as x
    assert limeAttr.get_lime_attr is x.get_lime_attr and lime_image.LimeImageExplainer is x.LimeImageExplainer
    assert limeAttr.WHO == "sibling" and lime_image.WHO == "sibling image" and lime_base.WHO == "sibling base"
    assert SegmentationAlgorithm.WHO == "sibling wrapper" and generic_utils.WHO == "sibling utils"
    assert limeAttr.lime_image_of_the_sibling is lime_image              # the sibling's `from . import lime_image` meets the mirror's
    print("lime imports ok")
""")


def _run(code, *args):
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    return subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, env=env, timeout=300)


def test_mirror_lime_package_alone():
    r = _run(ALONE, PKG)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "alone ok" in r.stdout


def test_mirror_lime_package_in_front_of_a_sibling_tree(tmp_path):
    root = tmp_path / "sibling" / "util" / "attribution_methods" / "lime"
    (root / "wrappers").mkdir(parents=True)
    (root / "utils").mkdir()
    for d in (root.parent.parent, root.parent, root, root / "wrappers", root / "utils"):
        (d / "__init__.py").write_text("")
    (root / "limeAttr.py").write_text("from . import lime_image\nWHO = 'sibling'\nlime_image_of_the_sibling = lime_image\n")
    (root / "lime_image.py").write_text("WHO = 'sibling image'\nclass LimeImageExplainer:\n    WHO = 'sibling'\n")
    (root / "lime_base.py").write_text("WHO = 'sibling base'\n")
    (root / "wrappers" / "scikit_image.py").write_text("class SegmentationAlgorithm:\n    WHO = 'sibling wrapper'\n")
    (root / "utils" / "generic_utils.py").write_text("WHO = 'sibling utils'\n")
    r = _run(SIBLING, PKG, str(tmp_path / "sibling"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lime imports ok" in r.stdout
