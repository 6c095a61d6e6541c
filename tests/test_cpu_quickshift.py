"""Device quickshift without a GPU: the NumPy restatement (tests/quickshift_restated.py) against scikit-image 0.18.3's recorded runs
(tests/golden/quickshift.npz), the host half of xai_engine/quickshift.py (features, tie noise), the decision margin of every stored
case, the fifth extension header (include/xai_hip_ext5.h) and its library, every refusal K53-K55 and the Python front make before
any HIP call, and the identity tokens of xai_engine/lime.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import quickshift_restated as R
from abi_libs import PINNED, built, declared, exported, exported_elsewhere
from conftest import ROOT, load_golden

EXT5_HEADER = os.path.join(ROOT, "include", "xai_hip_ext5.h")
ENTRIES = ["xai_quickshift_density_f64", "xai_quickshift_labels_i32", "xai_quickshift_lds_bytes", "xai_quickshift_parent_f64",
           "xai_quickshift_workspace_bytes"]
_p, _i, _d, _z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
SQRT_DBL_MAX = float(np.sqrt(np.finfo(np.float64).max))


def _case(g, tag):
    ratio, ks, md, seed = g[f"{tag}_params"].tolist()
    return dict(image=g[f"{tag}_image"], ratio=ratio, ks=ks, md=md, seed=int(seed), features=g[f"{tag}_features"],
                labels=g[f"{tag}_labels"], parent=g[f"{tag}_parent"], dist=g[f"{tag}_dist"], margin=g[f"{tag}_margin"])


TAGS = ["lime", "cut", "roots"]


# ------------------------------------------------------------------------------------------------ the restatement and the fixture
def test_fixture_is_small_names_its_release_and_covers_the_cases():
    g = load_golden("quickshift.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "quickshift.npz")) < 512 * 1024
    assert str(g["version"]) == "0.18.3" and list(g["names"]) == TAGS
    lime, cut, roots = (_case(g, t) for t in TAGS)
    assert (lime["ks"], lime["md"], lime["ratio"]) == (4, 200, 0.2) and lime["labels"].max() + 1 >= 4
    real = cut["dist"] < SQRT_DBL_MAX                                   # pixels that have a denser neighbour
    assert 0 < (cut["dist"][real] > cut["md"]).sum() < real.sum()        # the cut binds for some of them, not for all
    assert roots["labels"].max() + 1 == roots["labels"].size == 340      # every pixel is a root


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_skimage(tag):
    """labels and parent exactly, dist bit for bit, on skimage's own features and the RandomState draw"""
    c = _case(load_golden("quickshift.npz"), tag)
    noise = np.random.RandomState(c["seed"]).normal(scale=0.00001, size=c["image"].shape[:2])
    r = R.quickshift_from(c["features"], noise, c["ks"], c["md"])
    assert np.array_equal(r["labels"], c["labels"]) and r["D"] == c["labels"].max() + 1
    assert np.array_equal(r["tree"], c["parent"])
    assert r["dist"].tobytes() == c["dist"].tobytes()
    assert np.array_equal(r["parent"], np.where(c["dist"] > c["md"], np.arange(r["parent"].size).reshape(r["parent"].shape), c["parent"]))


@pytest.mark.parametrize("tag", TAGS)
def test_margin_condition_holds_on_every_stored_case(tag):
    """gap >= 100 * bound, recomputed here and as stored: no density comparison can be turned by one differing exp per term"""
    c = _case(load_golden("quickshift.npz"), tag)
    noise = np.random.RandomState(c["seed"]).normal(scale=0.00001, size=c["image"].shape[:2])
    bound, gap = R.margin(c["features"], R.density(c["features"], noise, c["ks"]), c["ks"])
    print(f"{tag}: bound {bound:.3e} gap {gap:.3e}; stored {c['margin']}")
    assert gap >= 100 * bound and c["margin"][1] >= 100 * c["margin"][0]
    assert bound == c["margin"][0] and abs(gap - c["margin"][1]) <= bound


@pytest.mark.parametrize("tag", TAGS)
def test_quickshift_features_against_skimage(tag):
    """<= 1e-12 absolute: Lab reaches 100, one ulp there is 1.4e-14, and the 3-term matrix product is the only unstated order"""
    from xai_engine import quickshift as Q
    c = _case(load_golden("quickshift.npz"), tag)
    got = Q.quickshift_features(c["image"], c["ratio"])
    assert got.dtype == np.float64 and got.flags.c_contiguous and got.shape == c["features"].shape
    err = np.abs(got - c["features"]).max()
    print(f"{tag}: max |features - skimage| = {err:.3e}")
    assert err <= 1e-12
    assert np.abs(R.features(c["image"], c["ratio"]) - c["features"]).max() <= 1e-12


def test_quickshift_features_without_lab_and_its_input_types():
    from xai_engine import quickshift as Q
    g = np.random.default_rng(0).random((5, 7))
    f = Q.quickshift_features(g, 0.5, convert2lab=False)
    assert f.shape == (5, 7, 1) and np.array_equal(f[..., 0], g * 0.5)
    u8 = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert np.array_equal(Q.quickshift_features(u8, 1.0, convert2lab=False), u8 / 255.0)
    f32 = g.astype(np.float32)
    assert np.array_equal(Q.quickshift_features(f32, 1.0, convert2lab=False)[..., 0], f32.astype(np.float64))
    with pytest.raises(TypeError, match="floating point or uint8"):
        Q.quickshift_features(np.zeros((4, 4, 3), np.int32), 1.0)
    with pytest.raises(ValueError, match=r"\(\.\.\., 3\)"):
        Q.quickshift_features(np.zeros((4, 4, 2)), 1.0)


def test_tie_noise_equals_the_two_numpy_draws():
    from xai_engine import quickshift as Q
    assert np.array_equal(Q.tie_noise(531, 9, 11), np.random.RandomState(531).normal(scale=0.00001, size=(9, 11)))
    assert np.array_equal(Q.tie_noise(531, 9, 11, "RandomState"), Q.tie_noise(531, 9, 11))
    assert np.array_equal(Q.tie_noise(531, 9, 11, "generator"), np.random.default_rng(531).normal(scale=0.00001, size=(9, 11)))
    assert not np.array_equal(Q.tie_noise(531, 9, 11, "generator"), Q.tie_noise(531, 9, 11))
    with pytest.raises(ValueError, match="RandomState.*generator"):
        Q.tie_noise(1, 4, 4, "legacy")


# ------------------------------------------------------------------------------------------------ header and library
def test_ext5_header_parses_at_1_0_and_cites_skimage():
    from xai_engine import _lib
    text = open(EXT5_HEADER).read()
    args, ret, version = _lib.parse_header(text, _lib.LIBRARIES["ext5"].defines)
    assert version == (1, 0) and (_lib.LIBRARIES["ext5"].version, _lib.LIBRARIES["ext5"].minor) == PINNED["ext5"] == (1, 0)
    assert sorted(args) == declared(EXT5_HEADER) == sorted(ENTRIES + ["xai_ext5_version", "xai_ext5_version_minor"])
    assert args["xai_quickshift_lds_bytes"] == [_i, _d]
    assert args["xai_quickshift_density_f64"] == [_p, _p, _i, _i, _i, _i, _d, _p, _p]
    assert args["xai_quickshift_parent_f64"] == [_p, _p, _i, _i, _i, _i, _d, _d, _p, _p, _p, _p, _p]
    assert args["xai_quickshift_workspace_bytes"] == [_i, _i, _i]
    assert args["xai_quickshift_labels_i32"] == [_p, _i, _i, _i, _p, _p, _p, _z, _p]
    sizes = ("xai_quickshift_lds_bytes", "xai_quickshift_workspace_bytes")
    assert all(ret[n] is _z for n in sizes) and all(t is _i for n, t in ret.items() if n not in sizes)
    listed = text[text.index(" *   0 = "):text.index("#define XAI_EXT5_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    for name in ("xai_quickshift_density_f64", "xai_quickshift_parent_f64", "xai_quickshift_labels_i32"):
        at = text.index(name + "(")
        comment = text[text.rfind("/*", 0, at):at]
        assert re.search(r"replaces\s+_quickshift_cy\.pyx", comment), name
    assert "_quickshift.py:71-73" in text and "THE CAP" in text and "65536" in text


def test_ext5_library_exports_exactly_its_header_and_the_other_five_are_unchanged():
    from xai_engine import _lib
    assert exported(built("ext5")) == declared(EXT5_HEADER) == sorted(_lib.LIBRARIES["ext5"].signatures)
    lib = _lib.load("ext5")
    assert (lib.xai_ext5_version(), lib.xai_ext5_version_minor()) == (1, 0)
    # each other library exports exactly its own header (exported_elsewhere), none of them an entry of this feature
    assert not [(o, n) for o, n in exported_elsewhere("ext5") if n.startswith("xai_quickshift_") or "ext5" in n]
    assert {k: (rec.version, rec.minor) for k, rec in _lib.LIBRARIES.items()} == PINNED


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_k53_to_k55_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext5")
    lib = _lib.load("ext5")
    p = 16                               # a non-NULL, aligned pointer that is never dereferenced: validation comes first
    nan = float("nan")

    # the LDS formula and the cap: (16 + 2 * ceil(3 * kernel_size))^2 * C * 8 <= 65536
    assert lib.xai_quickshift_lds_bytes(3, 4.0) == 40 * 40 * 3 * 8 == 38400
    assert lib.xai_quickshift_lds_bytes(1, 1.5) == (16 + 2 * 5) ** 2 * 8                         # kw = ceil(4.5) = 5
    assert lib.xai_quickshift_lds_bytes(3, 6.0) == 52 * 52 * 24 <= 65536 < lib.xai_quickshift_lds_bytes(3, 6.1)
    assert lib.xai_quickshift_lds_bytes(1, 37 / 3) <= 65536 < lib.xai_quickshift_lds_bytes(1, 12.5)
    assert [lib.xai_quickshift_lds_bytes(0, 4.0), lib.xai_quickshift_lds_bytes(3, 0.99), lib.xai_quickshift_lds_bytes(3, nan)] == [0] * 3
    assert lib.xai_quickshift_lds_bytes(3, 1e9) == C.c_size_t(-1).value

    def dens(f=p, noise=p, out=p, B=1, H=5, W=7, Cn=3, ks=4.0):
        return lib.xai_quickshift_density_f64(f, noise, B, H, W, Cn, ks, out, None)
    assert [dens(f=None), dens(noise=None), dens(out=None)] == [-1] * 3
    assert [dens(B=0), dens(H=0), dens(W=-1), dens(Cn=0), dens(ks=0.5), dens(ks=nan), dens(ks=-4.0)] == [-2] * 7
    assert [dens(ks=6.1), dens(ks=1e300), dens(ks=float("inf")), dens(Cn=4, ks=6.0), dens(B=65536), dens(H=1 << 16, W=1 << 15)] == [-3] * 6

    def par(f=p, d=p, parent=p, tree=p, closest=p, dist=p, B=1, H=5, W=7, Cn=3, ks=4.0, md=200.0):
        return lib.xai_quickshift_parent_f64(f, d, B, H, W, Cn, ks, md, parent, tree, closest, dist, None)
    assert [par(f=None), par(d=None), par(parent=None), par(closest=None), par(dist=None)] == [-1] * 5
    assert [par(B=0), par(H=0), par(W=0), par(Cn=-1), par(ks=0.0), par(ks=nan)] == [-2] * 6
    assert [par(ks=6.1), par(B=65536), par(H=1 << 16, W=1 << 15)] == [-3] * 3

    assert lib.xai_quickshift_workspace_bytes(2, 3, 4) == 2 * 3 * 4 * 2 * 4
    assert [lib.xai_quickshift_workspace_bytes(0, 3, 4), lib.xai_quickshift_workspace_bytes(1, 0, 4), lib.xai_quickshift_workspace_bytes(1, 3, -1),
            lib.xai_quickshift_workspace_bytes(65536, 3, 4), lib.xai_quickshift_workspace_bytes(1, 1 << 16, 1 << 15)] == [0] * 5

    def lab(parent=p, labels=p, D=p, ws=p, B=2, H=3, W=4, nbytes=192):
        return lib.xai_quickshift_labels_i32(parent, B, H, W, labels, D, ws, nbytes, None)
    assert [lab(parent=None), lab(labels=None), lab(D=None), lab(ws=None)] == [-1] * 4
    assert [lab(B=0), lab(H=0), lab(W=0), lab(nbytes=191), lab(ws=18)] == [-2] * 5
    assert [lab(B=65536, nbytes=1 << 40), lab(H=1 << 16, W=1 << 15, nbytes=1 << 40)] == [-3] * 2


def test_the_python_front_refuses_before_it_needs_a_device():
    from xai_engine import XaiHipError, kernels as K
    from xai_engine import quickshift as Q
    img = np.random.default_rng(1).random((6, 8, 3))
    sig = inspect.signature(Q.quickshift)
    skimage_0_18 = [("image", inspect.Parameter.empty), ("ratio", 1.0), ("kernel_size", 5), ("max_dist", 10), ("return_tree", False),
                    ("sigma", 0), ("convert2lab", True), ("random_seed", 42)]
    assert [(n, q.default) for n, q in sig.parameters.items()][:8] == skimage_0_18
    assert list(sig.parameters)[8:] == ["tie_noise", "device"] and sig.parameters["tie_noise"].default == "RandomState"
    with pytest.raises(NotImplementedError, match="sigma"):
        Q.quickshift(img, sigma=1.0)
    with pytest.raises(ValueError, match="tie_noise must be one of"):
        Q.quickshift(img, tie_noise="philox")
    with pytest.raises(ValueError, match="kernel_size"):
        Q.quickshift(img, kernel_size=0.5)
    with pytest.raises(XaiHipError):
        Q.quickshift(img, device="cpu")
    assert list(inspect.signature(Q.quickshift_features).parameters) == ["image", "ratio", "convert2lab"]
    assert list(inspect.signature(Q.tie_noise).parameters) == ["seed", "H", "W", "kind"]
    assert list(inspect.signature(Q.quickshift_batch).parameters) == ["features_dev", "noise_dev", "kernel_size", "max_dist", "return_tree"]
    f, n = torch.zeros(1, 6, 8, 3, dtype=torch.float64), torch.zeros(1, 6, 8, dtype=torch.float64)
    with pytest.raises(XaiHipError, match="no CPU fallback"):                       # a missing device is an error, never a fallback
        Q.quickshift_batch(f, n, 4, 200)
    with pytest.raises(XaiHipError):
        K.quickshift_labels(torch.zeros(1, 6, 8, dtype=torch.int32))
    assert K.quickshift_lds_bytes(3, 4) == 38400


# ------------------------------------------------------------------------------------------------ LIME's segmenters
def test_lime_quickshift_segments_and_both_defaults_are_unchanged():
    from xai_engine import lime
    assert list(inspect.signature(lime.quickshift_segments).parameters) == ["image", "random_seed"]
    assert list(inspect.signature(lime.device_quickshift_segments).parameters) == ["image", "random_seed"]
    assert inspect.signature(lime.LimeImageExplainer.explain_instance).parameters["segmentation_fn"].default is None
    assert inspect.signature(lime.lime_batch).parameters["segments"].default is inspect.Parameter.empty
    assert lime.QUICKSHIFT_ARGS == dict(kernel_size=4, max_dist=200, ratio=0.2)
    src = inspect.getsource(lime.quickshift_segments)
    assert "kernel_size=4, max_dist=200, ratio=0.2, random_seed=random_seed" in src and "from skimage.segmentation import quickshift" in src
    try:
        import skimage  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match=r"segments= / segmentation_fn="):
            lime.quickshift_segments(np.zeros((8, 8, 3), np.float32), 1)
        # the default of explain_instance is still skimage's quickshift: nothing falls over to the device segmenter by itself
        with pytest.raises(ImportError, match="scikit-image"):
            lime.LimeImageExplainer(random_state=1).explain_instance(np.zeros((8, 8, 3), np.float32), lime.batch_predict,
                                                                     torch.nn.Identity(), "cuda:0")


class _Passed(Exception):
    pass


def _restated_device_segments(calls):
    def fn(image, random_seed, dev):
        calls.append((np.array(image), random_seed, str(dev)))
        r = R.quickshift(image, ratio=0.2, kernel_size=4, max_dist=200, random_seed=random_seed)
        return torch.from_numpy(r["labels"].astype(np.int32)).to(dev), r["D"]
    return fn


def test_lime_batch_recognises_the_device_segmenter_by_identity(monkeypatch):
    """The restated segmenter stands in for the device call; the input check and K31 are stubbed, which is as far as a CPU test goes:
    the token reaches `_device_segments` with the (H, W, C) image and the drawn seed, per image, in the reference's draw order, and
    a wrapper around the same function is an ordinary host callable."""
    from xai_engine import lime
    calls, composed = [], []
    monkeypatch.setattr(lime, "_device_segments", _restated_device_segments(calls))
    monkeypatch.setattr(lime, "check_input", lambda x, name: x.detach().float().contiguous())

    def compose(x, seg_t, rows, D_t, *a, **k):
        composed.append((seg_t.clone(), D_t.clone(), rows.clone()))
        raise _Passed
    monkeypatch.setattr(lime.K, "lime_compose", compose)
    x = torch.from_numpy(np.random.default_rng(5).random((2, 3, 12, 14)).astype(np.float32))
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 12 * 14, 6))
    rs = np.random.RandomState(11)
    with pytest.raises(_Passed):
        lime.lime_batch(x, model, lime.device_quickshift_segments, num_samples=20, random_state=rs)
    want = np.random.RandomState(11)
    seeds, segs, mats = [], [], []
    for b in range(2):
        seeds.append(lime.draw_seed(want))
        r = R.quickshift(x[b].numpy().transpose(1, 2, 0), ratio=0.2, kernel_size=4, max_dist=200, random_seed=seeds[-1])
        segs.append(r["labels"])
        mats.append(lime.draw_data(want, 20, r["D"]))
    assert [c[1] for c in calls] == seeds and all(np.array_equal(c[0], x[b].numpy().transpose(1, 2, 0)) for b, c in enumerate(calls))
    seg_t, D_t, rows = composed[0]
    assert seg_t.dtype == torch.int32 and np.array_equal(seg_t.numpy(), np.stack(segs))
    assert D_t.tolist() == [int(s.max()) + 1 for s in segs]
    words = rows.shape[1]
    assert np.array_equal(rows.numpy().view(np.uint64), np.concatenate([lime.pack_rows(m, words) for m in mats]))
    assert want.randint(0, 1 << 30) == rs.randint(0, 1 << 30)                       # the RandomState is left in the same state

    # not the token itself: called on the host like any other callable, and its (H, W) host result goes through check_segments
    calls.clear()
    host_calls = []

    def host_fn(image, seed):
        host_calls.append(seed)
        return np.zeros(image.shape[:2], np.int64)
    with pytest.raises(_Passed):
        lime.lime_batch(x, model, host_fn, num_samples=20, random_state=np.random.RandomState(11))
    assert host_calls == seeds and calls == []


def test_explain_instance_recognises_the_device_segmenter_by_identity(monkeypatch):
    from xai_engine import lime
    calls, seen = [], {}
    monkeypatch.setattr(lime, "_device_segments", _restated_device_segments(calls))
    monkeypatch.setattr(lime, "hip_device", lambda device: torch.device("cpu"))

    def batch(x, model, segments, **kw):
        seen.update(segments=np.array(segments), data=kw["data"][0])
        raise _Passed
    monkeypatch.setattr(lime, "lime_batch", batch)
    image = np.random.default_rng(6).random((12, 14, 3))
    with pytest.raises(_Passed):
        lime.LimeImageExplainer(random_state=4).explain_instance(image, lime.batch_predict, torch.nn.Identity(), "cuda:0", hide_color=0,
                                                                 num_samples=15, segmentation_fn=lime.device_quickshift_segments)
    want = np.random.RandomState(4)
    seed = lime.draw_seed(want)
    r = R.quickshift(image, ratio=0.2, kernel_size=4, max_dist=200, random_seed=seed)
    assert len(calls) == 1 and calls[0][1] == seed and np.array_equal(calls[0][0], image)
    assert np.array_equal(seen["segments"], r["labels"]) and np.array_equal(seen["data"], lime.draw_data(want, 15, r["D"]))
    # an explicit random_seed is passed on as it is (lime_image.py:174-175 draws only for None)
    with pytest.raises(_Passed):
        lime.LimeImageExplainer(random_state=4).explain_instance(image, lime.batch_predict, torch.nn.Identity(), "cuda:0", hide_color=0,
                                                                 num_samples=15, segmentation_fn=lime.device_quickshift_segments, random_seed=77)
    assert calls[1][1] == 77


def test_the_harness_key_and_the_cli_flag():
    from xai_engine import evaluate_perturbation as cli
    from xai_engine import sweep
    args = cli.build_parser().parse_args([])
    assert args.lime_quickshift == "skimage"
    assert cli.build_parser().parse_args(["--lime_quickshift", "device"]).lime_quickshift == "device"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--lime_quickshift", "slic"])
    src = inspect.getsource(sweep)
    assert 'testing_dict.get("lime_quickshift", "skimage")' in src and "lime.device_quickshift_segments if which == \"device\"" in src
    assert '"lime_quickshift": args.lime_quickshift' in inspect.getsource(cli.main)
