"""Device k-means on the MI355X: K58-K61 (include/xai_hip_ext7.h) and xai_engine/kmeans.py against the NumPy restatement of the
header's arithmetic contract (tests/kmeans_restated.py).

Everything against the restatement is exact: the contract fixes the order of every sum, so the centroids, assignments and counts are
compared as bytes, the iterations as integers and err as the bits of a double.  Only the comparison with the parent's torch loop,
whose order is rocBLAS's, has a bound: 0.05, the one tests/test_gpu_e2e.py holds that loop to on the same data."""
import functools

import numpy as np
import pytest
import torch

import kmeans_restated as R
from conftest import load_golden
from helpers import vit_mini_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def M():
    from xai_engine import kmeans
    return kmeans


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def planted():
    """the planted clusters of tests/test_gpu_e2e.py and tests/test_oracle_golden.py"""
    rng = np.random.RandomState(3)
    centres = rng.randn(5, 16).astype(np.float32) * 10
    return np.concatenate([c + 0.01 * rng.randn(40, 16).astype(np.float32) for c in centres])


@functools.lru_cache(maxsize=None)
def _data(name):
    """-> (X (n, d) fp32, first (k,) int64) of a named case; never modified"""
    if name == "planted":
        return planted(), np.random.RandomState(11).choice(200, size=[5], replace=False)
    if name == "integers":          # every product, sum and score is a small integer: exact, and ties are the rule
        rng = np.random.RandomState(7)
        X = rng.randint(-2, 3, size=(150, 7)).astype(np.float32)
        first = rng.choice(150, size=[30], replace=False)
        X[first[17]] = X[first[4]]                      # two identical initial points: the later one loses every tie
        return X, first
    if name == "overflow":          # squares are inf, scores NaN
        rng = np.random.RandomState(9)
        return (rng.randn(60, 5) * 1e20).astype(np.float32), rng.choice(60, size=[4], replace=False)
    n, d, k = {"ragged": (257, 49, 33), "tokens": (130, 196, 65), "d1": (70, 1, 3), "k_is_n": (40, 5, 40), "k1": (50, 6, 1),
               "tiles": (1100, 20, 300)}[name]
    rng = np.random.RandomState(n + d + k)
    return rng.randn(n, d).astype(np.float32), rng.choice(n, size=[k], replace=False)


@functools.lru_cache(maxsize=None)
def _want(name, max_iter=100):
    X, first = _data(name)
    return R.kmeans(X, first, max_iter=max_iter)


def _hold(M, name, max_iter=100, check_every=8):
    """one device run of a named case against the restatement: bytes, iterations, the bits of err"""
    X, first = _data(name)
    C, assign, counts, iterations, err = _want(name, max_iter)
    got, info = M.kmeans_device(_dev(X), len(first), first=first, max_iter=max_iter, check_every=check_every, return_info=True)
    tag = (name, max_iter, check_every)
    assert got.dtype == torch.float32 and info["assign"].dtype == torch.int32 and info["counts"].dtype == torch.int32, tag
    assert info["iterations"] == iterations, (tag, info["iterations"], iterations)
    assert info["assign"].cpu().numpy().tobytes() == assign.tobytes(), tag
    assert info["counts"].cpu().numpy().tobytes() == counts.tobytes(), tag
    assert got.cpu().numpy().tobytes() == C.tobytes(), (tag, np.abs(got.cpu().numpy() - C).max())
    assert np.float64(info["err"]).tobytes() == np.float64(err).tobytes(), (tag, info["err"], err)
    return got, info


def test_planted_clusters(M):
    _, info = _hold(M, "planted")
    assert 1 <= info["iterations"] < 100 and info["err"] <= 1e-4


def test_integer_points_one_iteration_leaves_the_duplicate_empty(M):
    X, first = _data("integers")
    assert np.array_equal(X[first[17]], X[first[4]])
    got, info = _hold(M, "integers", max_iter=1)
    assert info["iterations"] == 1 and int(info["counts"][17]) == 0 and int(info["counts"][4]) >= 2
    assert got[17].cpu().numpy().tobytes() == np.zeros(7, np.float32).tobytes()             # an empty cluster is a row of +0
    assert not (info["assign"] == 17).any()


def test_integer_points_to_convergence(M):
    _, info = _hold(M, "integers")
    assert 1 < info["iterations"] < 100


@pytest.mark.parametrize("name", ["ragged", "tokens", "d1", "k1", "tiles"])
def test_ragged_extents_and_several_tiles(M, name):
    _hold(M, name)


def test_k_equal_to_n_stops_after_one_iteration_with_err_zero(M):
    _, info = _hold(M, "k_is_n")
    assert info["iterations"] == 1 and info["err"] == 0.0 and info["counts"].tolist() == [1] * 40


def test_the_cap_and_the_launches_after_the_stop_change_nothing(M):
    _, capped = _hold(M, "ragged", max_iter=2)
    assert capped["iterations"] == 2
    runs = [_hold(M, "ragged", check_every=c) for c in (1, 3, 100)]        # 100: every launch after the stop is issued
    assert _want("ragged")[3] < 100
    for got, info in runs[1:]:
        assert torch.equal(got, runs[0][0]) and torch.equal(info["assign"], runs[0][1]["assign"])
        assert info["iterations"] == runs[0][1]["iterations"]
    for c in (1, 3, 100):
        _hold(M, "ragged", max_iter=2, check_every=c)


def test_overflow_nan_scores_and_nan_to_zero(M):
    C, assign, counts, iterations, err = _want("overflow", 3)
    X, _ = _data("overflow")
    with np.errstate(over="ignore"):
        assert np.isinf((X * X).sum(1)).all()
    assert not np.isnan(C).any() and not np.isnan(err)                  # err is inf, not NaN: its bits are defined
    assert (counts == 0).any()                          # 0 / 0 = NaN became +0 somewhere
    _hold(M, "overflow", max_iter=3)


def test_against_the_torch_loop_of_the_parent_on_the_planted_clusters(M):
    from xai_engine.tis import kmeans_centroids
    pts = _dev(planted())
    np.random.seed(11)
    got = M.kmeans_device(pts, 5)
    np.random.seed(11)
    want = kmeans_centroids(pts, 5)
    gap = float((got - want).abs().max())
    print("device k-means vs the torch loop:", gap)
    assert gap <= 0.05
    assert got.cpu().numpy().tobytes() == _want("planted")[0].tobytes()                       # the same draw as the restated case


def test_a_bad_argument_is_refused_on_the_device_too(M):
    x = _dev(planted())
    with pytest.raises(ValueError, match="outside"):
        M.kmeans_device(x, 2, first=torch.tensor([0, 200], device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        M.kmeans_device(x.t(), 2)
    with pytest.raises(ValueError, match="n_clusters must be in"):
        M.kmeans_device(x, 201)
    with pytest.raises(TypeError, match="float32"):
        M.kmeans_device(x.double(), 2)


def test_TIS_with_the_device_kmeans(M):
    from xai_engine.sweep import get_VIT_attr
    from xai_engine.tis import TIS
    gv = load_golden("vit_mini.npz")
    model = vit_mini_from(gv, DEV)
    x = torch.from_numpy(gv["x"]).to(DEV)
    np.random.seed(5)
    a = TIS(model, n_masks=6, batch_size=4, kmeans="device")(x)
    _, acts = TIS(model, n_masks=6).get_encoder_activations(x)
    channels = acts.squeeze(0)[1:].T.contiguous().float()
    np.random.seed(5)
    raw = M.kmeans_device(channels, 6)
    b = TIS(model, n_masks=6, batch_size=4, raw_masks=raw)(x)
    assert a.shape == (4, 4) and torch.equal(a, b) and torch.isfinite(a).all()
    np.random.seed(5)
    c = TIS(model, n_masks=6, batch_size=4, kmeans="torch")(x)
    np.random.seed(5)
    d = TIS(model, n_masks=6, batch_size=4)(x)
    assert torch.equal(c, d)
    with pytest.raises(ValueError, match="kmeans must be one of"):
        TIS(model, n_masks=6, kmeans="gpu")
    td = {"models": [model, model], "img_hw": 32, "batch_size": 25, "device": DEV, "num_patches": 4, "tis_n_masks": 8,
          "attr_func": "TIS", "tis_kmeans": "device"}
    np.random.seed(1)
    got = get_VIT_attr(torch.from_numpy(gv["x"]).clone(), None, torch.tensor(int(gv["target"])), td)
    assert got.shape == (32, 32) and got.dtype == np.float32 and np.isfinite(got).all() and (got >= 0).all()
    with pytest.raises(ValueError, match="kmeans must be one of"):
        get_VIT_attr(torch.from_numpy(gv["x"]).clone(), None, torch.tensor(int(gv["target"])), dict(td, tis_kmeans="sklearn"))
