"""Device complete linkage on the MI355X: K56-K57 (include/xai_hip_ext6.h) and xai_engine/linkage.py against the NumPy restatement
of scipy's nearest-neighbour chain and scikit-learn's tree cut (tests/linkage_restated.py) and against the libraries' own recorded
runs (tests/golden/linkage.npz).

Everything is exact.  Complete linkage does no arithmetic on distances, so children, heights, n_clusters and labels are compared bit
for bit, ties included: most cases are nothing but ties."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import linkage_restated as R
from conftest import load_golden
from helpers import vit_mini_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (2, 3, 5, 63, 64, 65, 127, 129)
KINDS = ("generic", "q16", "q64", "equal", "blocks")
TENTH = float(np.float32(0.1))


@pytest.fixture(scope="module")
def L():
    from xai_engine import linkage
    return linkage


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden("linkage.npz")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(tag):
    """-> (matrix, dict of the libraries' results) of one stored case"""
    g = _golden()
    if tag == "big_768":
        d = R.big_matrix(int(g["big_768_seed"]))
        assert hashlib.sha256(d.tobytes()).hexdigest() == str(g["big_768_sha256"])
    else:
        d = R.from_condensed(g[f"{tag}_y"], int(tag.rsplit("_", 1)[1]))
    return d, {k: g[f"{tag}_{k}"] for k in ("thresholds", "Z", "children", "distances", "labels", "n_clusters")}


def _hold_tree(name, children, heights, want):
    assert children.dtype == np.int32 and heights.dtype == np.float32, name
    assert np.array_equal(children, want["children"]) and np.array_equal(children, want["Z"][:, :2].astype(np.int64)), name
    assert heights.astype(np.float64).tobytes() == want["distances"].tobytes() == want["Z"][:, 2].tobytes(), name


def _hold_case(L, name, d_host, d_dev, want):
    """the tree once, then every stored threshold: all bit for bit against the libraries' run and the restatement"""
    children, heights, info = L.linkage_device(d_dev)
    _hold_tree(name, children, heights, want)
    r_merges, r_heights, r_scans, r_pushes = R.nn_chain(d_host)
    r_children, r_sorted = R.sort_relabel(r_merges, r_heights, d_host.shape[0])
    assert np.array_equal(children, r_children) and heights.tobytes() == r_sorted.tobytes(), name
    assert info.tolist() == [0, r_scans, r_pushes, d_host.shape[0] - 1], (name, info)      # the same walk, scan for scan
    for t, labels, k in zip(want["thresholds"], want["labels"], want["n_clusters"]):
        got_labels, got_k, c2, h2 = L.agglomerative_labels(d_dev, float(t))
        assert got_k == int(k) and got_labels.dtype == np.int64 and np.array_equal(got_labels, labels), (name, t)
        assert np.array_equal(c2, children) and h2.tobytes() == heights.tobytes(), (name, t)
        r_labels, r_k = R.hc_cut(children, heights, float(t))
        assert r_k == got_k and np.array_equal(r_labels, got_labels), (name, t)
    print(f"{name}: n_clusters {want['n_clusters'].tolist()} scans {info[1]} pushes {info[2]}")


# ------------------------------------------------------------------------------------------------ the libraries' recorded runs
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_fixture_cases_equal_scipy_and_sklearn(L, kind, n):
    """every size around the wave (63, 64, 65) and over one pass of a 64-lane scan (127, 129), every data kind; the thresholds of
    each case: 0.1, exactly a merge height, the double just above it, 0.0 (n clusters), above the top (one cluster)"""
    tag = f"{kind}_{n}"
    d, want = _case(tag)
    assert want["n_clusters"][3] == n and want["n_clusters"][4] == 1
    _hold_case(L, tag, d, _dev(d), want)


@pytest.mark.parametrize("n", (5, 65, 129))
def test_the_lower_triangle_is_never_read(L, n):
    """the generic case's upper triangle over a lower triangle of other finite values: the generic case's results"""
    d, want = _case(f"generic_{n}")
    other = R.other_lower_triangle(np.random.default_rng(n), d)
    assert np.array_equal(np.triu(other, 1), np.triu(d, 1)) and not np.array_equal(np.tril(other, -1), np.tril(d, -1))
    _hold_case(L, f"lower_{n}", other, _dev(other), want)


def test_the_threshold_stays_a_double(L):
    """a third of the pairs are exactly float32(0.1).  The double just above float32(0.1) rounds to float32(0.1): compared in fp32 it
    would count those heights, compared as a double it does not"""
    d, want = _case("f32tenth_33")
    t_at, t_above = want["thresholds"][5:7]
    assert t_at == TENTH and t_above > TENTH and np.float32(t_above) == np.float32(0.1)
    heights32 = want["distances"].astype(np.float32)
    ties = int((heights32 == np.float32(0.1)).sum())
    assert ties >= 1 and want["n_clusters"][5] - want["n_clusters"][6] == ties
    assert 1 + int((heights32 >= np.float32(t_above)).sum()) == want["n_clusters"][5] != want["n_clusters"][6]      # what fp32 would say
    _hold_case(L, "f32tenth_33", d, _dev(d), want)


def test_n_768_equals_scipy_and_sklearn(L):
    d, want = _case("big_768")
    _hold_case(L, "big_768", d, _dev(d), want)


# ------------------------------------------------------------------------------------------------ the kernels' own contract
def test_a_second_launch_and_every_width_write_the_same_bytes():
    """K56 and K57 twice on the same buffers, then with 64 and 1024 lanes: `out` (children, heights, info) and the merges in `ws`
    hold the same bytes every time"""
    from xai_engine import kernels as K
    for tag in ("q16_129", "generic_65", "equal_64"):
        d, want = _case(tag)
        n = d.shape[0]
        m = n - 1
        dd = _dev(d)
        ws = K.linkage_workspace(dd)
        out = torch.empty(3 * m + 4, dtype=torch.int32, device=DEV)
        seen = []
        for lanes in (0, 0, 64, 256, 1024):
            K.linkage_complete(dd, ws, out[3 * m:], lanes)
            K.linkage_sort_relabel(n, ws, out[:2 * m], out[2 * m:3 * m].view(torch.float32), out[3 * m:])
            torch.cuda.synchronize()
            seen.append((out.cpu().numpy().tobytes(), ws[-12 * m:].cpu().numpy().tobytes()))
        assert all(s == seen[0] for s in seen), tag
        host = np.frombuffer(seen[0][0], np.int32)
        assert np.array_equal(host[:2 * m].reshape(m, 2), want["children"]) and host[3 * m] == 0
        assert np.array_equal(dd.cpu().numpy(), d)                                       # the input is only read


def test_a_non_finite_entry_above_the_diagonal_is_a_value_error(L):
    d, _ = _case("generic_65")
    for bad in (np.nan, np.inf, -np.inf):
        for i, j in ((0, 1), (63, 64), (7, 40)):
            e = d.copy()
            e[i, j] = bad
            with pytest.raises(ValueError, match="non-finite"):
                L.complete_linkage(_dev(e))
    e = d.copy()
    e[np.tril_indices(65)] = np.nan                                                     # below and on the diagonal: never read
    children, heights = L.complete_linkage(_dev(e))
    assert np.array_equal(children, _case("generic_65")[1]["children"])


def test_the_front_refuses_what_the_header_refuses(L):
    from xai_engine import kernels as K
    cap = K.linkage_max_n()
    assert cap >= 1024
    with pytest.raises(ValueError, match="n >= 2"):
        L.complete_linkage(torch.zeros(1, 1, device=DEV))
    with pytest.raises(ValueError, match="THE CAP"):
        L.complete_linkage(torch.zeros(cap + 1, cap + 1, device=DEV))
    with pytest.raises(TypeError):
        L.complete_linkage(torch.zeros(4, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(n, n\)"):
        L.complete_linkage(torch.zeros(4, 5, device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        L.complete_linkage(torch.zeros(8, 4, device=DEV)[::2])
    d = _dev(_case("generic_5")[0])
    with pytest.raises(ValueError, match="lanes"):
        K.linkage_complete(d, K.linkage_workspace(d), torch.zeros(4, dtype=torch.int32, device=DEV), lanes=128)


# ------------------------------------------------------------------------------------------------ ViT-CX end to end
def test_ViT_CX_with_device_clustering_equals_the_sklearn_path():
    """the suite's small hooked ViT, the same noise: the labels are equal and the saliency is the same bytes"""
    from xai_engine import vit_cx
    gv = load_golden("vit_mini.npz")
    model = vit_mini_from(gv, DEV)
    x = torch.from_numpy(gv["x"])
    layer = model.blocks[-1].norm1
    noise = torch.randn(32, 3, 32, 32, generator=torch.Generator().manual_seed(9))
    soft = torch.nn.Sequential(model, torch.nn.Softmax(dim=1))
    _, fmap = vit_cx.feature_maps(soft, x.to(DEV), layer, vit_cx.reshape_function_vit)
    mask = vit_cx.K.up_rownorm(fmap, 32, 32)
    for thr in (0.1, 0.02):
        m_host, l_host = vit_cx.cluster_masks(mask, thr)
        m_dev, l_dev = vit_cx.cluster_masks(mask, thr, clustering="device")
        assert np.array_equal(l_host, l_dev) and torch.equal(m_host, m_dev), thr
        n = m_host.shape[0]
        a, _ = vit_cx.ViT_CX(model, x, layer, distance_threshold=thr, gpu_batch=5, device=DEV, noise=noise[:n], return_feature_map=False)
        b, _ = vit_cx.ViT_CX(model, x, layer, distance_threshold=thr, gpu_batch=5, device=DEV, noise=noise[:n], return_feature_map=False,
                             clustering="device")
        assert a.numpy().tobytes() == b.numpy().tobytes(), thr
        print(f"ViT_CX thr {thr}: {n} clusters of {len(l_host)} maps")
    with pytest.raises(ValueError, match="clustering must be one of"):
        vit_cx.ViT_CX(model, x, layer, device=DEV, clustering="scipy")


def test_the_harness_key_selects_the_device_clustering():
    from xai_engine.sweep import get_VIT_attr
    gv = load_golden("vit_mini.npz")
    model = vit_mini_from(gv, DEV)
    x = torch.from_numpy(gv["x"])
    td = {"models": [model, model], "img_hw": 32, "batch_size": 25, "device": DEV, "num_patches": 4, "attr_func": "VIT_CX"}
    torch.manual_seed(1)
    a = get_VIT_attr(x.clone(), None, None, td)
    torch.manual_seed(1)
    b = get_VIT_attr(x.clone(), None, None, dict(td, vit_cx_clustering="device"))
    assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match="clustering must be one of"):
        get_VIT_attr(x.clone(), None, None, dict(td, vit_cx_clustering="gpu"))
