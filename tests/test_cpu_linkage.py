"""Device complete linkage without a GPU: the NumPy restatement (tests/linkage_restated.py) against scipy and scikit-learn themselves
and against their recorded runs (tests/golden/linkage.npz), the host cut of xai_engine/linkage.py, the sixth extension header
(include/xai_hip_ext6.h) and its library, every refusal K56-K57 and the Python front make before any HIP call, and the option's way
from the CLI flag to ViT_CX."""
import ctypes as C
import hashlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import linkage_restated as R
from abi_libs import PINNED, built, declared, exported, exported_elsewhere
from conftest import ROOT, load_golden

EXT6_HEADER = os.path.join(ROOT, "include", "xai_hip_ext6.h")
ENTRIES = ["xai_linkage_complete_f32", "xai_linkage_max_n", "xai_linkage_sort_relabel_i32", "xai_linkage_workspace_bytes"]
_p, _i, _z = C.c_void_p, C.c_int, C.c_size_t
SIZES = (2, 3, 5, 63, 64, 65, 127, 129)
KINDS = ("generic", "q16", "q64", "equal", "blocks")


def _matrix(g, tag):
    if tag == "big_768":
        return R.big_matrix(int(g["big_768_seed"]))
    return R.from_condensed(g[f"{tag}_y"], int(tag.rsplit("_", 1)[1]))


# ------------------------------------------------------------------------------------------------ the restatement against the libraries
def _seeded(t):
    """matrix t of the 420: n in 2..33, a third generic, a third quantised to 1/16, a third to 1/64"""
    rng = np.random.default_rng(1000 + t)
    n = int(rng.integers(2, 34))
    return (R.cosine_distance(rng, n), R.quantised(rng, n, 16), R.quantised(rng, n, 64))[t % 3]


def test_restatement_equals_scipy_and_sklearn_on_420_seeded_matrices():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    cluster = pytest.importorskip("sklearn.cluster")
    tied = 0
    for t in range(420):
        d = _seeded(t)
        n = d.shape[0]
        Z = hierarchy.linkage(d[np.triu_indices(n, 1)], "complete")
        children, heights = R.complete_linkage(d)
        assert np.array_equal(children, Z[:, :2].astype(np.int64)) and heights.astype(np.float64).tobytes() == Z[:, 2].tobytes(), t
        tied += len(np.unique(heights)) < n - 1
        for thr in (0.1, float(heights[(n - 1) // 2]), 0.0):
            m = cluster.AgglomerativeClustering(n_clusters=None, distance_threshold=thr, metric="precomputed", linkage="complete").fit(d)
            labels, k = R.hc_cut(children, heights, thr)
            assert np.array_equal(m.children_, children) and np.array_equal(m.distances_, Z[:, 2]), t
            assert k == m.n_clusters_ and np.array_equal(labels, m.labels_), (t, thr)
    assert tied >= 200          # the quantised two thirds merge at repeated heights nearly always


def test_fixture_is_small_names_its_releases_and_covers_the_cases():
    g = load_golden("linkage.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "linkage.npz")) < 512 * 1024
    assert re.fullmatch(r"\d+\.\d+\.\d+.*", str(g["scipy_version"])) and re.fullmatch(r"\d+\.\d+\.\d+.*", str(g["sklearn_version"]))
    assert list(g["names"]) == [f"{k}_{n}" for k in KINDS for n in SIZES] + ["f32tenth_33", "big_768"]
    d = R.big_matrix(int(g["big_768_seed"]))
    assert d.shape == (768, 768) and hashlib.sha256(d.tobytes()).hexdigest() == str(g["big_768_sha256"])
    for kind in KINDS[1:]:
        for n in SIZES[2:]:
            assert R.duplicated_pair_share(_matrix(g, f"{kind}_{n}")) >= 0.1, (kind, n)
    assert R.duplicated_pair_share(_matrix(g, "f32tenth_33")) >= 0.1
    assert g["generic_129_y"].dtype == np.float32 and g["generic_129_Z"].shape == (128, 4) and g["generic_129_labels"].shape == (5, 129)


@pytest.mark.parametrize("tag", [f"{k}_{n}" for k in KINDS for n in SIZES] + ["f32tenth_33", "big_768"])
def test_restatement_equals_the_recorded_runs(tag):
    g = load_golden("linkage.npz")
    d = _matrix(g, tag)
    children, heights = R.complete_linkage(d)
    assert np.array_equal(children, g[f"{tag}_children"]) and np.array_equal(children, g[f"{tag}_Z"][:, :2].astype(np.int64))
    assert heights.astype(np.float64).tobytes() == g[f"{tag}_distances"].tobytes() == g[f"{tag}_Z"][:, 2].tobytes()
    assert np.isin(heights, d[np.triu_indices(d.shape[0], 1)]).all()          # no arithmetic: every height is an input value
    for t, labels, k in zip(g[f"{tag}_thresholds"], g[f"{tag}_labels"], g[f"{tag}_n_clusters"]):
        got, got_k = R.hc_cut(children, heights, float(t))
        assert got_k == k and np.array_equal(got, labels), (tag, t)


def test_the_lower_triangle_and_the_diagonal_are_not_read_and_a_non_finite_entry_is_refused():
    g = load_golden("linkage.npz")
    d = _matrix(g, "generic_65")
    other = R.other_lower_triangle(np.random.default_rng(65), d)
    np.fill_diagonal(other, np.nan)
    children, heights = R.complete_linkage(other)
    assert np.array_equal(children, g["generic_65_children"])
    for bad in (np.nan, np.inf, -np.inf):
        e = d.copy()
        e[3, 40] = bad
        with pytest.raises(ValueError, match="non-finite"):
            R.complete_linkage(e)
    with pytest.raises(ValueError, match="n >= 2"):
        R.complete_linkage(np.zeros((1, 1), np.float32))


def test_the_host_cut_of_the_engine_is_the_restated_one_and_keeps_the_threshold_a_double():
    from xai_engine import linkage as L
    g = load_golden("linkage.npz")
    for tag in ("q16_65", "blocks_129", "f32tenth_33", "generic_2"):
        children, heights = g[f"{tag}_children"], g[f"{tag}_distances"].astype(np.float32)
        for t, labels, k in zip(g[f"{tag}_thresholds"], g[f"{tag}_labels"], g[f"{tag}_n_clusters"]):
            got, got_k = L.hc_cut(children, heights, float(t))
            assert got_k == k and got.dtype == np.int64 and np.array_equal(got, labels), (tag, t)
    # the double just above float32(0.1) rounds to float32(0.1): an fp32 comparison would count the heights at float32(0.1)
    heights = g["f32tenth_33_distances"].astype(np.float32)
    t_above = float(g["f32tenth_33_thresholds"][6])
    assert np.float32(t_above) == np.float32(0.1) and t_above > float(np.float32(0.1))
    assert 1 + int((heights >= np.float32(t_above)).sum()) > L.hc_cut(g["f32tenth_33_children"], heights, t_above)[1]
    src = inspect.getsource(L)
    assert "from heapq import heappush, heappushpop" in src and src.count(".cpu()") == 1     # Python's own heap; one read-back


# ------------------------------------------------------------------------------------------------ header and library
def test_ext6_header_parses_at_1_0_and_cites_scipy_and_sklearn():
    from xai_engine import _lib
    text = open(EXT6_HEADER).read()
    args, ret, version = _lib.parse_header(text, _lib.LIBRARIES["ext6"].defines)
    assert version == (1, 0) and (_lib.LIBRARIES["ext6"].version, _lib.LIBRARIES["ext6"].minor) == PINNED["ext6"] == (1, 0)
    assert sorted(args) == declared(EXT6_HEADER) == sorted(ENTRIES + ["xai_ext6_version", "xai_ext6_version_minor"])
    assert args["xai_linkage_max_n"] == [] and args["xai_linkage_workspace_bytes"] == [_i]
    assert args["xai_linkage_complete_f32"] == [_p, _i, _p, _z, _p, _i, _p]
    assert args["xai_linkage_sort_relabel_i32"] == [_i, _p, _z, _p, _p, _p, _p]
    assert ret["xai_linkage_workspace_bytes"] is _z and all(t is _i for n, t in ret.items() if n != "xai_linkage_workspace_bytes")
    listed = text[text.index(" *   0 = "):text.index("#define XAI_EXT6_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    for name, cited in (("xai_linkage_complete_f32", r"replaces\s+scipy/cluster/_hierarchy\.pyx, `nn_chain`"),
                        ("xai_linkage_sort_relabel_i32", r"replaces\s+scipy/cluster/hierarchy\.py, linkage")):
        at = text.index("int " + name + "(")
        assert re.search(cited, text[text.rfind("/*", 0, at):at]), name
    assert "THE CAP" in text and "#define XAI_LINKAGE_MAX_N 2048" in text and "sklearn/cluster/_agglomerative.py" in text
    assert all(n.startswith(("xai_linkage_", "xai_ext6_")) for n in args)


def test_ext6_library_exports_exactly_its_header_and_the_other_six_are_unchanged():
    from xai_engine import _lib
    assert exported(built("ext6")) == declared(EXT6_HEADER) == sorted(_lib.LIBRARIES["ext6"].signatures)
    lib = _lib.load("ext6")
    assert (lib.xai_ext6_version(), lib.xai_ext6_version_minor()) == (1, 0)
    # each other library exports exactly its own header (exported_elsewhere), none of them an entry of this feature
    assert not [(o, n) for o, n in exported_elsewhere("ext6") if n.startswith("xai_linkage_") or "ext6" in n]
    assert {k: (rec.version, rec.minor) for k, rec in _lib.LIBRARIES.items()} == PINNED


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_k56_and_k57_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext6")
    lib = _lib.load("ext6")
    p = 16                               # a non-NULL, aligned pointer that is never dereferenced: validation comes first
    cap = lib.xai_linkage_max_n()
    assert cap == 2048 >= 1024

    def words(n):
        return n * n + n * -(-n // 256) + 3 * (n - 1)
    assert [lib.xai_linkage_workspace_bytes(n) for n in (2, 256, 257, 768, cap)] == [4 * words(n) for n in (2, 256, 257, 768, cap)]
    assert [lib.xai_linkage_workspace_bytes(n) for n in (1, 0, -3, cap + 1)] == [0] * 4
    big = 1 << 40

    def chain(d=p, n=5, ws=p, nbytes=big, info=p, lanes=0):
        return lib.xai_linkage_complete_f32(d, n, ws, nbytes, info, lanes, None)
    assert [chain(d=None), chain(ws=None), chain(info=None)] == [-1] * 3
    assert [chain(n=1), chain(n=0), chain(n=-2), chain(nbytes=4 * words(5) - 1), chain(ws=18), chain(lanes=128), chain(lanes=-64),
            chain(lanes=2048)] == [-2] * 8
    assert [chain(n=cap + 1), chain(n=1 << 30)] == [-3] * 2

    def sort(n=5, ws=p, nbytes=big, children=p, heights=p, info=p):
        return lib.xai_linkage_sort_relabel_i32(n, ws, nbytes, children, heights, info, None)
    assert [sort(ws=None), sort(children=None), sort(heights=None), sort(info=None)] == [-1] * 4
    assert [sort(n=1), sort(n=0), sort(nbytes=4 * words(5) - 1), sort(ws=18)] == [-2] * 4
    assert [sort(n=cap + 1)] == [-3]


def test_the_python_front_refuses_before_it_needs_a_device():
    from xai_engine import XaiHipError, kernels as K
    from xai_engine import linkage as L
    assert list(inspect.signature(L.complete_linkage).parameters) == ["distance"]
    assert list(inspect.signature(L.agglomerative_labels).parameters) == ["distance", "distance_threshold"]
    cap = K.linkage_max_n()
    with pytest.raises(ValueError, match="n >= 2"):
        L.complete_linkage(torch.zeros(1, 1))
    with pytest.raises(ValueError, match="n >= 2"):
        L.agglomerative_labels(torch.zeros(0, 0), 0.1)
    with pytest.raises(ValueError, match="THE CAP"):
        L.complete_linkage(torch.zeros(cap + 1, cap + 1))
    with pytest.raises(TypeError, match="float32"):
        L.complete_linkage(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(TypeError, match="torch.Tensor"):
        L.complete_linkage(np.zeros((4, 4), np.float32))
    for shape in ((4, 5), (16,), (2, 4, 4)):
        with pytest.raises(ValueError, match=r"\(n, n\)"):
            L.complete_linkage(torch.zeros(*shape))
    with pytest.raises(XaiHipError, match="no CPU fallback"):                       # a missing device is an error, never a fallback
        L.agglomerative_labels(torch.zeros(4, 4), 0.1)


def test_a_non_finite_status_from_the_device_is_a_value_error_and_a_bound_a_hip_error(monkeypatch):
    """the kernels stubbed, which is as far as a CPU test goes: how linkage_device reads the one buffer that comes back"""
    from xai_engine import XaiHipError, kernels as K
    from xai_engine import linkage as L
    g = load_golden("linkage.npz")
    d = _matrix(g, "q16_5")
    status = {"value": 0}
    monkeypatch.setattr(K, "linkage_workspace", lambda distance: torch.zeros(8, dtype=torch.uint8))
    monkeypatch.setattr(K, "linkage_complete", lambda distance, ws, info, lanes=0: info.copy_(torch.tensor([status["value"], 7, 6, 4], dtype=torch.int32)))

    def sort(n, ws, children, heights, info):
        c, h = R.complete_linkage(d)
        children.copy_(torch.from_numpy(c.reshape(-1)))
        heights.copy_(torch.from_numpy(h))
    monkeypatch.setattr(K, "linkage_sort_relabel", sort)
    labels, k, children, heights = L.agglomerative_labels(torch.from_numpy(d), float(g["q16_5_thresholds"][1]))
    assert np.array_equal(children, g["q16_5_children"]) and heights.dtype == np.float32 and children.dtype == np.int32
    assert k == g["q16_5_n_clusters"][1] and np.array_equal(labels, g["q16_5_labels"][1])
    status["value"] = K.LINKAGE_NONFINITE
    with pytest.raises(ValueError, match="non-finite"):
        L.complete_linkage(torch.from_numpy(d))
    status["value"] = K.LINKAGE_BOUND
    with pytest.raises(XaiHipError, match="bound"):
        L.complete_linkage(torch.from_numpy(d))


# ------------------------------------------------------------------------------------------------ the option, from the CLI to ViT_CX
def test_the_clustering_option_and_every_default():
    from xai_engine import evaluate_perturbation as cli
    from xai_engine import sweep, vit_cx
    assert inspect.signature(vit_cx.cluster_masks).parameters["clustering"].default == "sklearn"
    par = inspect.signature(vit_cx.ViT_CX).parameters["clustering"]
    assert par.default == "sklearn" and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(vit_cx.cluster_masks).parameters) == ["mask", "distance_threshold", "clustering"]
    for bad in ("scipy", "gpu", None, ""):
        with pytest.raises(ValueError, match="clustering must be one of"):
            vit_cx.cluster_masks(torch.zeros(4, 9), 0.1, clustering=bad)
        with pytest.raises(ValueError, match="clustering must be one of"):          # before the device, the model or the image is touched
            vit_cx.ViT_CX(None, None, None, clustering=bad)
    args = cli.build_parser().parse_args([])
    assert args.vit_cx_clustering == "sklearn" and args.lime_quickshift == "skimage"
    assert cli.build_parser().parse_args(["--vit_cx_clustering", "device"]).vit_cx_clustering == "device"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--vit_cx_clustering", "scipy"])
    assert 'testing_dict.get("vit_cx_clustering", "sklearn")' in inspect.getsource(sweep.get_VIT_attr)
    assert '"vit_cx_clustering": args.vit_cx_clustering' in inspect.getsource(cli.main)
    src = inspect.getsource(vit_cx.cluster_labels)
    assert 'AgglomerativeClustering(n_clusters=None, distance_threshold=distance_threshold, metric="precomputed", linkage="complete")' in src
