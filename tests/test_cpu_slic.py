"""Device SLIC without a GPU: the NumPy restatement of include/xai_hip_slic.h (tests/slic_restated.py) and the host front of
xai_engine/slic.py against scikit-image 0.18.3's own runs (tests/golden/slic.npz), the header, its library's build line and names, every
refusal K65-K68 and the Python front make before any HIP call, and the option's way from the CLI flag to MDA."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import slic_restated as R
from abi_libs import built, declared, exported_elsewhere
from conftest import PKG, ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "xai_hip_slic.h")
ENTRIES = ["xai_slic_assign_f32", "xai_slic_assign_f64", "xai_slic_clear_i32", "xai_slic_components_i32", "xai_slic_iterate_f32",
           "xai_slic_iterate_f64", "xai_slic_max_channels", "xai_slic_max_clusters", "xai_slic_max_pixels", "xai_slic_number_i32",
           "xai_slic_update_f32", "xai_slic_update_f64", "xai_slic_workspace_bytes"]
TAGS = ["mda", "ragged", "colour", "wide", "one"]
DTYPES = {"f32": np.float32, "f64": np.float64}
_p, _i, _z = C.c_void_p, C.c_int, C.c_size_t


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("slic.npz")


@functools.lru_cache(maxsize=None)
def restated(tag, name):
    """the restatement's ten iterations on the fixture's own features; computed once, never modified"""
    g = golden()
    feat = g[f"{tag}_{name}_features"]
    return R.kmeans(feat, R.initial(g[f"{tag}_centroids"], feat.shape[2], feat.dtype), float(g[f"{tag}_step"]), 10)


# ------------------------------------------------------------------------------------------------ the restatement against skimage
def test_the_fixture_is_scikit_image_0_18_3_and_holds_the_stated_cases():
    g = golden()
    assert str(g["version"]) == "0.18.3" and list(g["names"]) == TAGS
    shapes = {"mda": (112, 112, 49, 10000.0), "ragged": (57, 43, 25, 10000.0), "colour": (40, 56, 12, 0.5), "wide": (33, 47, 20, 0.02),
              "one": (24, 24, 1, 10.0)}
    for tag, (H, W, n, comp) in shapes.items():
        assert g[f"{tag}_image"].shape == (H, W, 3) and g[f"{tag}_image"].dtype == np.float32 and g[f"{tag}_params"].tolist() == [n, comp]
        for name, T in DTYPES.items():
            assert g[f"{tag}_{name}_features"].dtype == T and g[f"{tag}_{name}_centres"].dtype == T
    assert g["mda_step"] == 16 and len(g["ragged_centroids"]) == 24 and len(g["one_centroids"]) == 1
    assert g["big_labels"].shape == (224, 224) and len(np.unique(g["big_labels"])) == 196
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "slic.npz")) < 1000000


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_skimage_raw_labels_and_centres_bit_for_bit(tag, name):
    g = golden()
    raw, trace, status = restated(tag, name)
    assert status == 0 and raw.dtype == np.int32 and trace.dtype == DTYPES[name] and trace.shape[0] == 10
    assert np.array_equal(raw, g[f"{tag}_{name}_raw"])
    assert trace[-1].tobytes() == g[f"{tag}_{name}_centres"].tobytes()       # skimage's `segments` after a direct _slic_cython call


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_regular_rule_equals_the_sequential_pass_and_the_host_pass_equals_skimage_everywhere(tag, name):
    from xai_engine.slic import enforce_connectivity_host, size_bounds
    g = golden()
    raw = g[f"{tag}_{name}_raw"].astype(np.int32)
    mn, mx = (int(v) for v in g[f"{tag}_sizes"])
    assert size_bounds(raw.shape[0], raw.shape[1], len(g[f"{tag}_centroids"])) == (mn, mx)
    comp, status, sweeps = R.components(raw, mn, mx)
    assert (status == 0) == bool(g[f"{tag}_{name}_regular"]) == (tag in ("mda", "ragged", "one")) and sweeps < R.MAX_SWEEPS
    want = g[f"{tag}_{name}_labels"]
    if status == 0:
        labels, count = R.number(comp, 0)
        assert np.array_equal(labels, want) and count == len(np.unique(want))
    else:
        assert status == R.IRREGULAR
    host = enforce_connectivity_host(raw, mn, mx, 0)
    assert host.dtype == np.int64 and np.array_equal(host, want)


def test_host_pass_equals_skimage_on_irregular_maps_that_keep_several_labels():
    from xai_engine.slic import enforce_connectivity_host
    g = golden()
    assert int(g["conn_count"]) == 3
    for i in range(3):
        raw, want = g[f"conn{i}_raw"].astype(np.int64), g[f"conn{i}_labels"]
        mn, mx = (int(v) for v in g[f"conn{i}_sizes"])
        assert R.components(raw.astype(np.int32), mn, mx)[1] == R.IRREGULAR and len(np.unique(want)) > 1
        assert np.array_equal(enforce_connectivity_host(raw, mn, mx, 0), want), i


def test_restatement_ties_the_uncovered_pixel_and_the_empty_cluster():
    feat = np.zeros((4, 9, 1), np.float32)
    cen = np.array([[1, 2, 0], [1, 6, 0]], np.float32)                       # pixel column 4 is exactly between the two centres
    labels, status = R.assign(feat, cen, 4)
    assert status == 0 and labels[:, 4].tolist() == [0] * 4 and labels[:, 5].tolist() == [1] * 4      # the lower k wins the tie
    labels, status = R.assign(np.zeros((4, 30, 1), np.float32), np.array([[1, 2, 0]], np.float32), 2)
    assert status == R.UNCOVERED and (labels[:, 7:] == -1).all() and (labels[:, :7] == 0).all()          # window columns [0, 7)
    feat = np.zeros((6, 6, 1), np.float32)
    cen = np.array([[2, 2, 0], [2, 2, 0]], np.float32)                        # the twin loses every tie
    labels, status = R.assign(feat, cen, 3)
    new, st = R.update(feat, labels, cen)
    assert status == 0 and st == R.EMPTY and (labels == 0).all() and np.isnan(new[1]).all() and new[0].tolist() == [2.5, 2.5, 0]
    assert R.assign(feat, new, 3)[0].tolist() == labels.tolist()              # a NaN centre has the empty window
    assert R.bounds(np.float32(np.nan), np.float32(6), 6) == (0, 0) and R.bounds(np.float32(1e30), np.float32(6), 6) == (6, 6)
    assert R.bounds(np.float32(2.5), np.float32(2), 100) == (0, 5) and R.bounds(np.float64(97.9), np.float64(2), 100) == (95, 100)


def test_components_and_numbering_of_the_restatement():
    lab = np.array([[5, 5, 2, 2], [5, 2, 2, 5], [7, 7, 7, 5]], np.int32)
    comp, status, sweeps = R.components(lab, 1, 5)
    assert comp.tolist() == [[0, 0, 2, 2], [0, 2, 2, 7], [8, 8, 8, 7]] and status == 0 and sweeps >= 2
    labels, count = R.number(comp, 1)
    assert labels.tolist() == [[1, 1, 2, 2], [1, 2, 2, 3], [4, 4, 4, 3]] and count == 4
    assert R.components(lab, 3, 5)[1] == R.IRREGULAR and R.components(lab, 1, 4)[1] == R.IRREGULAR      # the 2-component, the 4-component
    wide = np.zeros((400, 1), np.int32)
    comp, status, sweeps = R.components(wide, 1, 1000)                        # pointer following: far fewer sweeps than pixels
    assert status == 0 and (comp == 0).all() and sweeps <= 12


# ------------------------------------------------------------------------------------------------ the host front
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_features_against_skimages_within_the_rounding_bound(tag, name):
    """Both sides run the same NumPy operations in T; they may differ by the pow and cbrt of two libm builds and by the order (or the
    fusing) of the 3-term sums of `arr @ xyz_from_rgb.T` in two BLAS builds.  Count roundings of half an ulp on the way to x (and y):
    add, divide, pow (2: libm), three products and two sums, the division by the white point, cbrt (2: libm), 12 in all.  The
    matrix is positive, so nothing cancels before cbrt and cbrt divides a relative error by 3; x, y <= 1.  a = 500 (x - y) carries
    both errors 500-fold, 500 * 2 * 12 * eps / 2, and its own two roundings (the product and `* ratio`) bring the count to 13:
    |difference| <= 500 * 13 * eps * ratio.  L (116-fold) and b (200-fold) are inside it."""
    from xai_engine.slic import slic_features
    g = golden()
    T = DTYPES[name]
    ratio = 1.0 / float(g[f"{tag}_params"][1])
    got = slic_features(g[f"{tag}_image"].astype(T), float(g[f"{tag}_params"][1]))
    want = g[f"{tag}_{name}_features"]
    assert got.dtype == T and got.shape == want.shape and got.flags.c_contiguous
    diff, bound = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()), 500 * 13 * float(np.finfo(T).eps) * ratio
    print(f"{tag} {name}: |features - skimage's| = {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound


def test_grid_centroids_equal_skimages_and_the_front_refuses_what_it_does_not_serve():
    from xai_engine import slic as S
    g = golden()
    for tag in TAGS:
        H, W = g[f"{tag}_image"].shape[:2]
        centres, step = S.grid_centroids(H, W, int(g[f"{tag}_params"][0]))
        assert np.array_equal(centres, g[f"{tag}_centroids"]) and step == float(g[f"{tag}_step"]) and centres.dtype == np.int64
    assert S.grid_centroids(224, 224, 196)[0].shape == (196, 2) and S.grid_centroids(224, 224, 196)[1] == 16.0
    sig = inspect.signature(S.slic)
    assert list(sig.parameters) == ["image", "n_segments", "compactness", "max_iter", "sigma", "spacing", "multichannel", "convert2lab",
                                    "enforce_connectivity", "min_size_factor", "max_size_factor", "slic_zero", "start_label", "mask", "device"]
    assert [p.default for p in sig.parameters.values()][1:] == [100, 10., 10, 0, None, True, None, True, 0.5, 3, False, None, None, "cuda"]
    assert list(inspect.signature(S.slic_batch).parameters) == ["features_dev", "centres", "step", "max_iter", "enforce_connectivity",
                                                                "min_size_factor", "max_size_factor", "start_label"]
    img = np.zeros((8, 8, 3), np.float32)
    for kw, word in ((dict(sigma=1), "sigma"), (dict(spacing=[1, 1, 1]), "spacing"), (dict(mask=np.ones((8, 8), bool)), "mask"),
                     (dict(slic_zero=True), "slic_zero"), (dict(multichannel=False), "volumes")):
        with pytest.raises(NotImplementedError, match=word):
            S.slic(img, **kw)
    with pytest.raises(NotImplementedError, match="volumes"):
        S.slic(np.zeros((4, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="start_label"):
        S.slic(img, start_label=2)
    with pytest.raises(TypeError, match="float32, float64 or uint8"):
        S.slic(np.zeros((8, 8, 3), np.int32))
    with pytest.raises(S.XaiHipError, match="not a HIP GPU"):                 # never a CPU fallback
        S.slic(img, device="cpu")
    assert S.slic_features(np.full((2, 2, 3), 255, np.uint8), 1.0).dtype == np.float64          # uint8 becomes float64, as img_as_float


# ------------------------------------------------------------------------------------------------ the table, header and library
def test_the_makefile_builds_slic_from_its_kernel_file():
    assert "SRCS_slic := slic_kernels.hip\n" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_header_parses_at_1_0_cites_skimage_and_states_its_bound():
    from xai_engine import _lib
    text = open(HEADER).read()
    rec = _lib.LIBRARIES["slic"]
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert version == (rec.version, rec.minor) == (1, 0)
    assert sorted(args) == declared(HEADER) == sorted(ENTRIES + ["xai_slic_version", "xai_slic_version_minor"])
    assert args["xai_slic_workspace_bytes"] == [_i, _i, _i] and ret["xai_slic_workspace_bytes"] is _z
    assert args["xai_slic_clear_i32"] == [_p, _i, _p]
    for sfx in ("f32", "f64"):
        assert args[f"xai_slic_assign_{sfx}"] == [_p, _p] + [_i] * 6 + [_p, _p, _p]
        assert args[f"xai_slic_update_{sfx}"] == [_p, _p] + [_i] * 6 + [_p, _p, _p]
        assert args[f"xai_slic_iterate_{sfx}"] == [_p] + [_i] * 7 + [_p, _p, _p, _p]
    assert args["xai_slic_components_i32"] == [_p, _i, _i, _i, _i, _i, _p, _p, _p, _z, _p]
    assert args["xai_slic_number_i32"] == [_p, _i, _i, _i, _i, _p, _p, _p, _z, _p]
    listed = text[text.index(" *   0 = "):text.index("#define XAI_SLIC_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    flat = " ".join(text.split())
    assert "slic_superpixels.py:316-318" in text and "slic_superpixels.py:320-328" in text and "_slic.pyx" in text and "0.18.3" in text
    assert "#define XAI_SLIC_MAX_CLUSTERS 4096" in text and "#define XAI_SLIC_MAX_CHANNELS 8" in text and "THE LIMITS" in text
    assert "a lane visiting H * W / 1024 pixels per sweep" in flat                # the bound on H * W, derived from K67's layout
    for name in ("xai_slic_assign_f32", "xai_slic_update_f32", "xai_slic_iterate_f32", "xai_slic_components_i32", "xai_slic_number_i32"):
        at = text.index("int " + name + "(")
        assert re.search(r"replaces\s", text[text.rfind("/*", 0, at):at]), name


def test_no_other_library_exports_a_slic_name():
    assert not [(o, n) for o, n in exported_elsewhere("slic") if n.startswith("xai_slic_")]


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_k65_to_k68_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("slic")
    lib = _lib.load("slic")
    p = 16                               # a non-NULL, aligned pointer that is never dereferenced: validation comes first
    caps = lib.xai_slic_max_clusters(), lib.xai_slic_max_channels(), lib.xai_slic_max_pixels()
    assert caps == (4096, 8, 1 << 20) and caps[2] >= 224 * 224
    assert lib.xai_slic_workspace_bytes(32, 224, 224) == 3 * 4 * 32 * 224 * 224 and lib.xai_slic_workspace_bytes(1, 1, 1) == 12
    assert [lib.xai_slic_workspace_bytes(*s) for s in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 1025, 1024), (65536, 4, 4), (-1, -1, -1)]] == [0] * 6
    big = 1 << 40
    shapes = [dict(B=0), dict(H=0), dict(W=-3), dict(Cc=0), dict(S=0), dict(step=0)]
    overs = [dict(B=65536), dict(S=4097), dict(Cc=9), dict(H=1025, W=1024), dict(H=1 << 20, W=1 << 20),
             dict(H=16 * 65535 + 1, W=1)]                                         # 65536 rows of tiles: over K65's grid in y

    def entry(kind, sfx):
        fn = getattr(lib, f"xai_slic_{kind}_{sfx}")

        def call(a=p, b=p, B=2, H=8, W=9, Cc=3, S=4, step=2, c=p, status=p, iterations=2):
            if kind == "iterate":
                return fn(a, B, H, W, Cc, S, step, iterations, b, c, status, None)
            return fn(a, b, B, H, W, Cc, S, step, c, status, None)
        return call
    for sfx in ("f32", "f64"):
        for kind in ("assign", "update", "iterate"):
            fn = entry(kind, sfx)
            assert [fn(a=None), fn(b=None), fn(c=None), fn(status=None)] == [-1] * 4, (kind, sfx)
            assert [fn(**kw) for kw in shapes] == [-2] * len(shapes), (kind, sfx)
            assert [fn(**kw) for kw in overs] == [-3] * len(overs), (kind, sfx)
        assert [entry("iterate", sfx)(iterations=0), entry("iterate", sfx)(iterations=-1)] == [-2] * 2

    def components(labels=p, B=2, H=8, W=9, mn=1, mx=5, comp=p, status=p, ws=p, nbytes=big):
        return lib.xai_slic_components_i32(labels, B, H, W, mn, mx, comp, status, ws, nbytes, None)

    def number(comp=p, B=2, H=8, W=9, start=0, out=p, n=p, ws=p, nbytes=big):
        return lib.xai_slic_number_i32(comp, B, H, W, start, out, n, ws, nbytes, None)
    assert [components(labels=None), components(comp=None), components(status=None), components(ws=None)] == [-1] * 4
    assert [number(comp=None), number(out=None), number(n=None), number(ws=None)] == [-1] * 4
    for fn in (components, number):
        assert [fn(B=0), fn(H=0), fn(W=0), fn(nbytes=3 * 4 * 2 * 8 * 9 - 1), fn(ws=18)] == [-2] * 5, fn.__name__
        assert [fn(B=65536), fn(H=1025, W=1024)] == [-3] * 2, fn.__name__
    assert [components(mn=-1), components(mn=6, mx=5)] == [-2] * 2
    assert [lib.xai_slic_clear_i32(None, 1, None), lib.xai_slic_clear_i32(p, 0, None)] == [-1, -2]


def test_the_python_front_refuses_before_it_needs_a_device():
    from xai_engine import XaiHipError, kernels as K
    from xai_engine import slic as S
    built("slic")
    f = torch.zeros(1, 8, 8, 3)
    cen = np.array([[2, 2], [6, 6]])
    with pytest.raises(TypeError, match="torch.Tensor"):
        S.slic_batch(np.zeros((1, 8, 8, 3), np.float32), cen, 4)
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        S.slic_batch(f.half(), cen, 4)
    for shape in ((8, 8, 3), (1, 8, 8), (0, 8, 8, 3)):
        with pytest.raises(ValueError, match=r"\(B, H, W, C\)"):
            S.slic_batch(torch.zeros(*shape), cen, 4)
    with pytest.raises(ValueError, match="THE LIMITS"):
        S.slic_batch(torch.zeros(1, 4, 4, 9), cen, 4)
    with pytest.raises(ValueError, match="THE LIMITS"):                          # inside H * W, over K65's rows of tiles
        S.slic_batch(torch.zeros(1, 16 * 65535 + 1, 1, 1), cen, 4)
    with pytest.raises(ValueError, match="start_label"):
        S.slic_batch(f, cen, 4, start_label=2)
    for step in (0, 2.5, -1):
        with pytest.raises(ValueError, match="step must be"):
            S.slic_batch(f, cen, step)
    with pytest.raises(XaiHipError, match="no CPU fallback"):                  # a missing device is an error, never a fallback
        S.slic_batch(f, cen, 4)
    with pytest.raises(XaiHipError, match="no CPU fallback"):
        K.slic_assign(f, torch.zeros(1, 2, 5), 4)
    with pytest.raises(XaiHipError, match="no CPU fallback"):
        K.slic_components(torch.zeros(1, 4, 4, dtype=torch.int32), 1, 2)
    with pytest.raises(TypeError, match="torch.Tensor"):
        K.slic_number(None)


# ------------------------------------------------------------------------------------------------ the option, from the CLI to MDA
def test_the_slic_option_and_every_default():
    from xai_engine import evaluate_perturbation as cli
    from xai_engine import mda, sweep
    assert list(inspect.signature(mda.MDA).parameters)[-1] == "segments" and mda.SLIC == ("skimage", "device")      # the pinned signature
    assert inspect.signature(mda.slic_segments).parameters["which"].default == "skimage"
    for bad in ("gpu", None, ""):
        with pytest.raises(ValueError, match="slic must be one of"):
            mda.slic_segments(None, 4, bad)
        with pytest.raises(ValueError, match="slic must be one of"):            # before anything is computed
            mda.MDA(None, None, None, 4, None, None, "cuda", 8, segments=bad if bad is not None else "gpu")
    assert cli.build_parser().parse_args([]).mda_slic == "skimage"
    assert cli.build_parser().parse_args(["--mda_slic", "device"]).mda_slic == "device"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--mda_slic", "opencv"])
    assert '"mda_slic": args.mda_slic' in inspect.getsource(cli.main)
    src = inspect.getsource(sweep.get_VIT_attr)                                   # a bad key is refused by name (on the GPU: test_gpu_slic.py)
    assert 'which = testing_dict.get("mda_slic", "skimage")' in src and "testing_dict['mda_slic'] must be 'skimage' or 'device'" in src
    assert 'segments=testing_dict.get("mda_segments") if testing_dict.get("mda_segments") is not None else which)' in src
