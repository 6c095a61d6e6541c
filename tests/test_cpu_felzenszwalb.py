"""Device Felzenszwalb segmentation, what needs no GPU: the NumPy restatement of include/xai_hip_felz.h's contract
(tests/felzenszwalb_restated.py) against scikit-image 0.18.3's binary as tests/golden/felzenszwalb.npz recorded it, the Gaussian
weights, the header, the library's build line and names, every refusal by name and the option from the CLI down."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import felzenszwalb_restated as R
from abi_libs import built, declared, exported_elsewhere
from conftest import PKG, ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "xai_hip_felz.h")
ENTRIES = ["xai_felz_clear_i32", "xai_felz_costs_u64", "xai_felz_edges", "xai_felz_labels_i32", "xai_felz_max_channels",
           "xai_felz_max_pixels", "xai_felz_max_radius", "xai_felz_max_scales", "xai_felz_merge_f64", "xai_felz_smooth_f64",
           "xai_felz_sort_u64", "xai_felz_workspace_bytes"]
SMALL = {"a": (64, 48, 20), "b": (33, 47, 5), "c": (57, 43, 150), "d": (5, 9, 2), "e": (112, 112, 150),
         "d23": (2, 3, 1), "d17": (1, 7, 2), "d71": (7, 1, 2), "d11": (1, 1, 2)}             # H, W, min_size
XRAI_SCALES = [50, 100, 150, 250, 500, 1200]
_p, _i, _z = C.c_void_p, C.c_int, C.c_size_t


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("felzenszwalb.npz")


# ------------------------------------------------------------------------------------------------ the restatement against skimage
def test_the_fixture_is_scikit_image_0_18_3_and_holds_the_stated_cases():
    g = golden()
    assert (str(g["version_skimage"]), str(g["version_scipy"]), str(g["version_numpy"])) == ("0.18.3", "1.7.1", "1.26.4")
    assert list(g["names"]) == list(SMALL)
    for tag, (H, W, min_size) in SMALL.items():
        scales = g[f"{tag}_scales"].tolist()
        assert scales == (XRAI_SCALES + [1] if len(tag) == 1 else [50]), tag
        assert g[f"{tag}_image"].shape == (H, W, 3) and g[f"{tag}_image"].dtype == np.float32
        assert g[f"{tag}_params"].tolist() == [0.8, min_size] and g[f"{tag}_weights"].shape == (7,)
        assert g[f"{tag}_smoothed"].shape == (H, W, 3) and g[f"{tag}_smoothed"].dtype == np.float64
        assert g[f"{tag}_labels"].shape == (len(scales), H, W) and g[f"{tag}_labels"].dtype == np.int16
    assert g["big_labels"].shape == (6, 224, 224) and g["big_scales"].tolist() == XRAI_SCALES
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "felzenszwalb.npz")) < 1000000


@pytest.mark.parametrize("tag", SMALL)
def test_restatement_equals_skimage_labels_and_smoothed_bits(tag):
    g = golden()
    sigma, min_size = g[f"{tag}_params"]
    got = R.felzenszwalb(g[f"{tag}_image"].astype(np.float64), g[f"{tag}_scales"], float(sigma), int(min_size), weights=g[f"{tag}_weights"])
    assert np.array_equal(got.smoothed.view(np.int64), g[f"{tag}_smoothed"].view(np.int64))
    assert len(np.unique(got.costs)) == len(got.costs)                          # no two costs equal: skimage's order is pinned here
    assert np.array_equal(got.labels, g[f"{tag}_labels"])
    assert np.array_equal(got.counts, g[f"{tag}_labels"].reshape(len(got.counts), -1).max(1) + 1)
    assert np.all(got.merged <= got.tested) and np.all(got.tested <= len(got.costs))
    assert np.array_equal(np.sort(got.order), np.arange(len(got.costs))) and np.all(np.diff(got.costs[got.order]) > 0)


def test_restatement_orders_equal_costs_by_edge_index_and_numbers_segments_by_first_pixel():
    flat = R.felzenszwalb(np.zeros((3, 4, 2)), [1, 0], 0.8, 0)                  # every cost 0.0: the order is the edge index
    assert np.array_equal(flat.order, np.arange(6 + 9 + 8 + 8 - 2)) and flat.counts.tolist() == [1, 12]
    assert flat.tested.tolist() == [11, 29] and flat.merged.tolist() == [11, 0]   # scale 0: 0 < 0 never holds
    halves = np.zeros((4, 6, 1))
    halves[:, 3:] = 1.0
    got = R.felzenszwalb(halves, [1], 0, 2)
    assert np.array_equal(got.labels[0], np.repeat([[0, 0, 0, 1, 1, 1]], 4, 0)) and got.counts.tolist() == [2]
    a, b = R.edge_pixels(2, 3)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1), (1, 2), (3, 4), (4, 5), (0, 3), (1, 4), (2, 5), (0, 4), (1, 5), (1, 3), (2, 4)]
    assert R.reflect(np.array([-9, -1, 0, 2, 3, 5, 6]), 3).tolist() == [2, 0, 0, 2, 2, 0, 0]   # period 2 n, also for r >= n


def test_gaussian_weights_against_the_stored_ones():
    from xai_engine import felzenszwalb as F
    g = golden()
    w = F.gaussian_weights(0.8)
    stored = g["a_weights"]
    ulps = np.abs(w.view(np.int64) - stored.view(np.int64)).max()
    if ulps:
        print(f"gaussian_weights(0.8) is {ulps} ulp from the stored weights under NumPy {np.__version__}")
    assert w.shape == (7,) and ulps <= 1 and np.array_equal(w, w[::-1])
    assert np.array_equal(w, R.weights_of(0.8))
    assert F.gaussian_weights(0) is None and F.gaussian_weights(1e-16) is None and F.gaussian_weights(2.0).shape == (17,)
    assert not re.search(r"^\s*(import|from) (scipy|skimage)", inspect.getsource(F), flags=re.M)      # NumPy only at run time


# ------------------------------------------------------------------------------------------------ the table, header and library
def test_the_makefile_builds_felz_from_its_kernel_file():
    assert "SRCS_felz := felz_kernels.hip\n" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_header_parses_at_1_0_cites_what_it_replaces_and_derives_its_bound():
    from xai_engine import _lib
    text = open(HEADER).read()
    rec = _lib.LIBRARIES["felz"]
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert version == (rec.version, rec.minor) == (1, 0)
    assert sorted(args) == declared(HEADER) == sorted(ENTRIES + ["xai_felz_version", "xai_felz_version_minor"])
    assert args["xai_felz_workspace_bytes"] == [_i] * 4 and ret["xai_felz_workspace_bytes"] is _z
    assert args["xai_felz_edges"] == [_i, _i] and args["xai_felz_clear_i32"] == [_p, _i, _p]
    assert args["xai_felz_smooth_f64"] == [_p, _p] + [_i] * 6 + [_p, _p]
    assert args["xai_felz_costs_u64"] == [_p] + [_i] * 4 + [_p, _p, _p, _p]
    assert args["xai_felz_sort_u64"] == [_p, _p] + [_i] * 4 + [_p, _z, _p]
    assert args["xai_felz_merge_f64"] == [_p, _p, _p] + [_i] * 5 + [_p, _p, _p, _p, _z, _p]
    assert args["xai_felz_labels_i32"] == [_p, _i, _i, _p, _p, _p, _p]
    listed = text[text.index(" *   0 = "):text.index("#define XAI_FELZ_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    flat = " ".join(text.replace(" * ", " ").split())
    assert "_felzenszwalb_cy.pyx" in text and "0.18.3" in text and "scipy.ndimage.gaussian_filter" in text and "THE LIMITS" in text
    assert "#define XAI_FELZ_MAX_PIXELS 65536" in text and "#define XAI_FELZ_MAX_CHANNELS 8" in text
    assert "#define XAI_FELZ_MAX_SCALES 16" in text and "#define XAI_FELZ_MAX_RADIUS 64" in text
    assert "a 16-bit word names 65536 pixels" in flat and "224 x 224 = 50176" in flat             # the bound on H * W, from K73's layout
    for name in ("xai_felz_smooth_f64", "xai_felz_costs_u64", "xai_felz_sort_u64", "xai_felz_merge_f64", "xai_felz_labels_i32"):
        at = text.index("int " + name + "(")
        assert re.search(r"replaces\s", text[text.rfind("/*", 0, at):at]), name


def test_no_other_library_exports_a_felz_name():
    assert not [(o, n) for o, n in exported_elsewhere("felz") if n.startswith("xai_felz_")]


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_k69_to_k74_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("felz")
    lib = _lib.load("felz")
    p = 16                               # a non-NULL, aligned pointer that is never dereferenced: validation comes first
    assert (lib.xai_felz_max_pixels(), lib.xai_felz_max_channels(), lib.xai_felz_max_scales(), lib.xai_felz_max_radius()) == (65536, 8, 16, 64)
    assert lib.xai_felz_max_pixels() >= 224 * 224
    assert [lib.xai_felz_edges(*s) for s in [(224, 224), (2, 3), (1, 7), (7, 1), (1, 1), (0, 4), (257, 256)]] == [199362, 11, 6, 6, 0, 0, 0]
    E, n = 199362, 224 * 224
    sort = 32 * E * 8 + 32 * E * 4 + 32 * 256 * 195 * 4
    assert lib.xai_felz_workspace_bytes(32, 224, 224, 6) == max(sort, 32 * 6 * n * 12)
    assert lib.xai_felz_workspace_bytes(1, 1, 1, 1) == 12
    assert [lib.xai_felz_workspace_bytes(*s) for s in [(0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, 17), (1, 257, 256, 1),
                                                       (65536, 4, 4, 1), (-1, -1, -1, -1)]] == [0] * 8
    big = 1 << 40

    def smooth(src=p, w=p, r=3, axis=0, B=2, H=8, W=9, Cc=3, dst=32):
        return lib.xai_felz_smooth_f64(src, w, r, axis, B, H, W, Cc, dst, None)

    def costs(image=p, B=2, H=8, W=9, Cc=3, keys=p, index=p, status=p):
        return lib.xai_felz_costs_u64(image, B, H, W, Cc, keys, index, status, None)

    def sort_(keys=p, index=p, B=2, H=8, W=9, S=2, ws=p, nbytes=big):
        return lib.xai_felz_sort_u64(keys, index, B, H, W, S, ws, nbytes, None)

    def merge(keys=p, order=p, scales=p, B=2, S=2, H=8, W=9, mn=3, roots=p, stats=p, status=p, ws=p, nbytes=big):
        return lib.xai_felz_merge_f64(keys, order, scales, B, S, H, W, mn, roots, stats, status, ws, nbytes, None)

    def labels(roots=p, M=2, n=72, lab=32, counts=p, status=p):
        return lib.xai_felz_labels_i32(roots, M, n, lab, counts, status, None)
    assert [smooth(src=None), smooth(w=None), smooth(dst=None)] == [-1] * 3
    assert [smooth(B=0), smooth(H=0), smooth(W=-1), smooth(Cc=0), smooth(r=-1), smooth(axis=2), smooth(dst=p)] == [-2] * 7
    assert [smooth(B=65536), smooth(H=257, W=256), smooth(Cc=9), smooth(r=65)] == [-3] * 4
    assert [costs(image=None), costs(keys=None), costs(index=None), costs(status=None)] == [-1] * 4
    assert [costs(B=0), costs(H=0), costs(W=0), costs(Cc=0)] == [-2] * 4 and [costs(H=257, W=256), costs(Cc=9)] == [-3] * 2
    assert [sort_(keys=None), sort_(index=None), sort_(ws=None)] == [-1] * 3
    need = lib.xai_felz_workspace_bytes(2, 8, 9, 2)
    assert [sort_(B=0), sort_(H=0), sort_(S=0), sort_(nbytes=need - 1), sort_(ws=20)] == [-2] * 5 and sort_(nbytes=need) != -2
    assert [sort_(H=257, W=256), sort_(S=17)] == [-3] * 2
    assert [merge(keys=None), merge(order=None), merge(scales=None), merge(roots=None), merge(stats=None), merge(status=None),
            merge(ws=None)] == [-1] * 7
    assert [merge(B=0), merge(S=0), merge(H=0), merge(mn=-1), merge(nbytes=need - 1), merge(ws=20)] == [-2] * 6
    assert [merge(H=257, W=256), merge(S=17), merge(B=65536)] == [-3] * 3
    assert [labels(roots=None), labels(lab=None), labels(counts=None), labels(status=None)] == [-1] * 4
    assert [labels(M=0), labels(n=0), labels(lab=p)] == [-2] * 3 and [labels(n=65537), labels(M=(1 << 20) + 1)] == [-3] * 2
    assert [lib.xai_felz_clear_i32(None, 1, None), lib.xai_felz_clear_i32(p, 0, None)] == [-1, -2]


def test_the_python_front_refuses_by_name_before_it_needs_a_device():
    from xai_engine import XaiHipError, kernels as K
    from xai_engine import felzenszwalb as F
    built("felz")
    image = np.zeros((8, 8, 3))
    with pytest.raises(ValueError, match=re.escape("This algorithm works only on single or multi-channel 2d images. ")):   # skimage's text
        F.felzenszwalb(image, multichannel=False)
    with pytest.raises(ValueError, match="sigma must be >= 0"):
        F.felzenszwalb(image, sigma=-0.5)
    with pytest.raises(ValueError, match="sigma must be >= 0"):
        F.gaussian_weights(-1)
    for bad in (np.nan, np.inf, -np.inf):
        broken = image.copy()
        broken[3, 4, 1] = bad
        with pytest.raises(XaiHipError, match="NaN or an infinite pixel"):
            F.felzenszwalb(broken)
    with pytest.raises(TypeError, match="float or uint8"):
        F.felzenszwalb(np.zeros((8, 8, 3), np.int32))
    with pytest.raises(ValueError, match=r"\(H, W\) or \(H, W, C\)"):
        F.felzenszwalb(np.zeros((2, 8, 8, 3)))
    t = torch.zeros(1, 8, 8, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="min_size must be an integer >= 0"):
        F._stages(t, [50], 0.8, -1, None)
    with pytest.raises(ValueError, match="scales must be finite"):
        F._stages(t, [np.nan], 0.8, 20, None)
    with pytest.raises(ValueError, match="symmetric"):
        F._stages(t, [50], 0.8, 20, np.array([0.2, 0.5, 0.3]))
    with pytest.raises(ValueError, match="THE LIMITS"):
        F._stages(torch.zeros(1, 4, 4, 9, dtype=torch.float64), [50], 0.8, 20, None)
    with pytest.raises(ValueError, match="THE LIMITS"):
        F._stages(torch.zeros(1, 257, 256, 1, dtype=torch.float64), [50], 0.8, 20, None)
    with pytest.raises(ValueError, match=r"\(B, H, W, C\)"):
        F._stages(torch.zeros(8, 8, 3, dtype=torch.float64), [50], 0.8, 20, None)
    with pytest.raises(XaiHipError, match="no CPU fallback"):                  # a missing device is an error, never a fallback
        F._stages(t, [50], 0.8, 20, None)
    with pytest.raises(XaiHipError, match="no CPU fallback"):
        K.felz_labels(torch.zeros(1, 4, 4, dtype=torch.int32))
    with pytest.raises(TypeError, match="float tensor"):
        F.felzenszwalb_batch(torch.zeros(1, 8, 8, 3, dtype=torch.int32), [50])
    assert list(inspect.signature(F.felzenszwalb).parameters) == ["image", "scale", "sigma", "min_size", "multichannel", "device"]
    assert [p.default for p in inspect.signature(F.felzenszwalb).parameters.values()][1:] == [1, 0.8, 20, True, None]
    assert list(inspect.signature(F.felzenszwalb_batch).parameters)[:5] == ["images", "scales", "sigma", "min_size", "weights"]


# ------------------------------------------------------------------------------------------------ the option, from the CLI to XRAI
def test_the_felzenszwalb_option_and_every_default():
    from xai_engine import evaluate_perturbation as cli
    from xai_engine import sweep, xrai
    assert cli.build_parser().parse_args([]).xrai_felzenszwalb == "skimage"
    assert cli.build_parser().parse_args(["--xrai_felzenszwalb", "device"]).xrai_felzenszwalb == "device"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--xrai_felzenszwalb", "opencv"])
    assert '"xrai_felzenszwalb": args.xrai_felzenszwalb' in inspect.getsource(cli.main)
    src = inspect.getsource(sweep.get_CNN_attr)
    assert 'which = testing_dict.get("xrai_felzenszwalb", "skimage")' in src
    assert '(testing_dict.get("xrai_label_maps") or segmenter)' in src                 # an explicit xrai_label_maps wins
    # a bad key is refused by name, before the IG is computed (on the GPU: test_gpu_felzenszwalb.py)
    assert "testing_dict['xrai_felzenszwalb'] must be 'skimage' or 'device'" in src
    assert src.index("testing_dict['xrai_felzenszwalb'] must be") < src.index("ig = IG(input_tensor, model, steps, batch_size, 1, baseline")
    assert inspect.signature(xrai.device_felzenszwalb_label_maps).parameters["device"].default is None
    with pytest.raises(ValueError, match="'device'"):
        xrai.XRAI().GetMask(np.zeros((8, 8, 3), np.float32), segments="gpu", base_attribution=np.zeros((8, 8, 3), np.float32))
    try:
        import skimage  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="xrai_felzenszwalb"):              # the text names the opt-in
            xrai.felzenszwalb_label_maps(np.zeros((8, 8, 3), np.float32))
