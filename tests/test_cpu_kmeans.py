"""Device k-means without a GPU: the NumPy restatement of the contract (tests/kmeans_restated.py) against the oracle's Lloyd loop, the
seventh extension header (include/xai_hip_ext7.h), its library's build line and names, every refusal K58-K61
and the Python front make before any HIP call, and the option's way from the CLI flag to TIS."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import kmeans_restated as R
from abi_libs import PINNED, built, declared, exported_elsewhere
from conftest import PKG, ROOT

EXT7_HEADER = os.path.join(ROOT, "include", "xai_hip_ext7.h")
ENTRIES = ["xai_kmeans_assign_f32", "xai_kmeans_init_f32", "xai_kmeans_iterate_f32", "xai_kmeans_max_clusters", "xai_kmeans_max_features",
           "xai_kmeans_max_points", "xai_kmeans_update_f32", "xai_kmeans_workspace_bytes"]
_p, _i, _z, _d = C.c_void_p, C.c_int, C.c_size_t, C.c_double


def planted():
    """the planted clusters of tests/test_oracle_golden.py (test_kmeans_restatement_recovers_separated_clusters)"""
    rng = np.random.RandomState(3)
    centres = rng.randn(5, 16).astype(np.float32) * 10
    return np.concatenate([c + 0.01 * rng.randn(40, 16).astype(np.float32) for c in centres]), centres


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_against_the_oracle_loop_on_the_planted_clusters():
    """0.05 is the project's own bound for this comparison (tests/test_gpu_e2e.py, the torch loop against the oracle).  Measured on
    the CPU: 0.0088 apart, the restatement stops after 3 iterations."""
    from oracle import tis as otis
    pts, _ = planted()
    want = otis.kmeans_centroids(pts, 5, rng=np.random.RandomState(11))
    first = np.random.RandomState(11).choice(200, size=[5], replace=False)
    got, assign, counts, iterations, err = R.kmeans(pts, first)
    print("restatement vs oracle:", np.abs(got - want).max(), "iterations", iterations, "err", err)
    assert np.abs(got - want).max() <= 0.05
    assert got.dtype == np.float32 and assign.dtype == np.int32 and counts.dtype == np.int32 and type(err) is np.float64
    assert counts.sum() == 200 and np.array_equal(np.bincount(assign, minlength=5), counts) and 1 <= iterations < 100 and err <= 1e-4


def test_restatement_ties_nan_and_the_empty_cluster():
    X = np.array([[1, 0], [1, 0], [0, 1], [0, 2], [3, 3]], np.float32)
    got, assign, counts, iterations, err = R.kmeans(X, [0, 1, 2], max_iter=1)
    assert assign.tolist() == [0, 0, 2, 2, 0] and counts.tolist() == [3, 0, 2]           # the duplicate loses every tie: a zero row
    assert got[1].tobytes() == np.zeros(2, np.float32).tobytes() and iterations == 1
    big = (X * np.float32(1e20)).astype(np.float32)
    got, assign, counts, iterations, err = R.kmeans(big, [0, 2], max_iter=2)
    assert not np.isnan(got).any() and assign.tolist() == [0] * 5 and counts.tolist() == [5, 0]      # every score NaN: the first wins


# ------------------------------------------------------------------------------------------------ the table, header and library
def test_the_makefile_builds_ext7_from_the_kmeans_kernels():
    assert "SRCS_ext7 := kmeans_kernels.hip\n" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_ext7_header_parses_at_1_0_states_the_order_and_cites_tis():
    from xai_engine import _lib
    text = open(EXT7_HEADER).read()
    rec = _lib.LIBRARIES["ext7"]
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert version == (rec.version, rec.minor) == (1, 0)
    assert sorted(args) == declared(EXT7_HEADER) == sorted(ENTRIES + ["xai_ext7_version", "xai_ext7_version_minor"])
    # the literal argument types of each entry
    assert args["xai_kmeans_max_points"] == args["xai_kmeans_max_features"] == args["xai_kmeans_max_clusters"] == []
    assert args["xai_kmeans_workspace_bytes"] == [_i, _i, _i]
    assert args["xai_kmeans_init_f32"] == [_p, _p, _i, _i, _i, _p, _p, _z, _p, _p]
    assert args["xai_kmeans_assign_f32"] == [_p, _i, _i, _i, _p, _p, _p, _z, _p, _p]
    assert args["xai_kmeans_update_f32"] == [_p, _i, _i, _i, _p, _p, _p, _p, _z, _p, _i, _d, _p]
    assert args["xai_kmeans_iterate_f32"] == [_p, _i, _i, _i, _p, _p, _p, _p, _z, _p, _i, _d, _i, _p]
    assert ret["xai_kmeans_workspace_bytes"] is _z and all(t is _i for n, t in ret.items() if n != "xai_kmeans_workspace_bytes")
    listed = text[text.index(" *   0 = "):text.index("#define XAI_EXT7_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    assert "TIS.py:150-155" in text and "xai_engine/tis.py" in text and "THE ARITHMETIC CONTRACT" in text and "THE LIMITS" in text
    assert "starts from +0 and runs sequentially in ascending index, one accumulator per result" in " ".join(text.split())
    assert all(n.startswith(("xai_kmeans_", "xai_ext7_")) for n in args)
    for name in ENTRIES[:3] + ENTRIES[6:7]:
        at = text.index("int " + name + "(")
        assert re.search(r"replaces\s", text[text.rfind("/*", 0, at):at]), name


def test_no_other_library_exports_a_kmeans_or_ext7_name():
    from xai_engine import _lib
    assert not [(o, n) for o, n in exported_elsewhere("ext7") if n.startswith("xai_kmeans_") or "ext7" in n]
    assert {k: (r.version, r.minor) for k, r in _lib.LIBRARIES.items()} == PINNED


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_k58_to_k61_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext7")
    lib = _lib.load("ext7")
    p = 16                               # a non-NULL, aligned pointer that is never dereferenced: validation comes first
    caps = lib.xai_kmeans_max_points(), lib.xai_kmeans_max_features(), lib.xai_kmeans_max_clusters()
    assert caps == (65536, 4096, 16384) and caps[0] >= 9216 and caps[1] >= 196 and caps[2] >= 1024

    def nbytes(n, d, k):
        return 8 * k + 4 * (n + k)
    good = [(9216, 196, 1024), (1, 1, 1), (40, 5, 40), caps[:2] + (caps[2],)]
    assert [lib.xai_kmeans_workspace_bytes(*s) for s in good] == [nbytes(*s) for s in good]
    over = [(caps[0] + 1, 4, 2), (8, caps[1] + 1, 2), (caps[0], 4, caps[2] + 1)]
    assert [lib.xai_kmeans_workspace_bytes(*s) for s in [(0, 4, 1), (8, 0, 2), (8, 4, 0), (8, 4, 9), (-1, -1, -1)] + over] == [0] * 8
    big = 1 << 40
    shapes = [dict(n=0), dict(d=0), dict(k=0), dict(k=9), dict(n=-4), dict(nbytes=nbytes(8, 4, 3) - 1), dict(ws=20), dict(state=12)]
    overs = [dict(n=caps[0] + 1), dict(d=caps[1] + 1), dict(n=caps[0], k=caps[2] + 1), dict(n=1 << 30, k=1 << 29)]

    def init(X=p, first=p, n=8, d=4, k=3, Cc=p, ws=p, nbytes=big, state=p):
        return lib.xai_kmeans_init_f32(X, first, n, d, k, Cc, ws, nbytes, state, None)

    def assign(X=p, n=8, d=4, k=3, Cc=p, a=p, ws=p, nbytes=big, state=p):
        return lib.xai_kmeans_assign_f32(X, n, d, k, Cc, a, ws, nbytes, state, None)

    def update(X=p, n=8, d=4, k=3, Cc=p, a=p, counts=p, ws=p, nbytes=big, state=p, max_iter=5, tol=1e-4):
        return lib.xai_kmeans_update_f32(X, n, d, k, Cc, a, counts, ws, nbytes, state, max_iter, tol, None)

    def iterate(X=p, n=8, d=4, k=3, Cc=p, a=p, counts=p, ws=p, nbytes=big, state=p, max_iter=5, tol=1e-4, iterations=2):
        return lib.xai_kmeans_iterate_f32(X, n, d, k, Cc, a, counts, ws, nbytes, state, max_iter, tol, iterations, None)
    assert [init(X=None), init(first=None), init(Cc=None), init(ws=None), init(state=None)] == [-1] * 5
    assert [assign(X=None), assign(Cc=None), assign(a=None), assign(ws=None), assign(state=None)] == [-1] * 5
    for fn in (update, iterate):
        assert [fn(X=None), fn(Cc=None), fn(a=None), fn(counts=None), fn(ws=None), fn(state=None)] == [-1] * 6
        assert [fn(max_iter=0), fn(max_iter=-1)] == [-2] * 2
    for fn in (init, assign, update, iterate):
        assert [fn(**kw) for kw in shapes] == [-2] * len(shapes), fn.__name__
        assert [fn(**kw) for kw in overs] == [-3] * len(overs), fn.__name__
    assert [iterate(iterations=0), iterate(iterations=-2), iterate(iterations=6)] == [-2] * 3


def test_the_python_front_refuses_before_it_needs_a_device():
    from xai_engine import XaiHipError, kernels as K
    from xai_engine import kmeans as M
    sig = inspect.signature(M.kmeans_device)
    assert list(sig.parameters) == ["points", "n_clusters", "first", "max_iter", "tol", "check_every", "return_info"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, 100, 1e-4, 8, False]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[2:])
    caps = K.kmeans_limits()
    x = torch.zeros(8, 4)
    with pytest.raises(TypeError, match="torch.Tensor"):
        M.kmeans_device(np.zeros((8, 4), np.float32), 2)
    with pytest.raises(TypeError, match="float32"):
        M.kmeans_device(x.double(), 2)
    for shape in ((8,), (2, 4, 4), (0, 4), (4, 0)):
        with pytest.raises(ValueError, match=r"\(n, d\)"):
            M.kmeans_device(torch.zeros(*shape), 2)
    for k in (0, -1, 9):                                                    # k > n
        with pytest.raises(ValueError, match="n_clusters must be in"):
            M.kmeans_device(x, k)
    with pytest.raises(TypeError, match="n_clusters"):
        M.kmeans_device(x, 2.0)
    with pytest.raises(ValueError, match="n_clusters or first"):
        M.kmeans_device(x)
    with pytest.raises(ValueError, match="THE LIMITS"):
        M.kmeans_device(torch.zeros(2, caps[1] + 1), 2)
    with pytest.raises(ValueError, match="contiguous"):
        M.kmeans_device(torch.zeros(4, 8).t(), 2)
    with pytest.raises(XaiHipError, match="no CPU fallback"):               # a missing device is an error, never a fallback
        M.kmeans_device(x, 2)
    for kw in (dict(max_iter=0), dict(check_every=0), dict(check_every=-3)):
        with pytest.raises(ValueError, match="must be"):
            M.kmeans_device(x, 2, **kw)
    with pytest.raises(TypeError, match="max_iter"):
        M.kmeans_device(x, 2, max_iter=2.5)
    # the initial indices are checked on the host, before the points' device is asked for anything
    for bad in ([0, 8], [-1, 2], torch.tensor([0, 9])):
        with pytest.raises(ValueError, match="outside"):
            M._first_indices(bad, 8, 2, "cpu")
    with pytest.raises(ValueError, match="n_clusters is 3"):
        M._first_indices([0, 1], 8, 3, "cpu")
    with pytest.raises(TypeError, match="integers"):
        M._first_indices([0.5, 1.0], 8, 2, "cpu")
    with pytest.raises(TypeError, match="int64"):
        M._first_indices(torch.tensor([0, 1], dtype=torch.int32), 8, 2, "cpu")
    np.random.seed(11)
    want = np.random.choice(200, size=[5], replace=False)
    np.random.seed(11)
    got = M._first_indices(None, 200, 5, "cpu")                             # the draw tis.kmeans_centroids makes
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    # the thin wrappers say the same checks
    with pytest.raises(TypeError, match="torch.Tensor"):
        K.kmeans_workspace(None, 2)
    with pytest.raises(ValueError, match="n_clusters must be in"):
        K.kmeans_workspace(x, 9)
    with pytest.raises(XaiHipError, match="no CPU fallback"):
        K.kmeans_iterate(x, torch.zeros(2, 4), None, None, None, None, 5, 1e-4, 1)


# ------------------------------------------------------------------------------------------------ the option, from the CLI to TIS
def test_the_kmeans_option_and_every_default():
    from xai_engine import evaluate_perturbation as cli
    from xai_engine import sweep, tis
    par = inspect.signature(tis.TIS).parameters["kmeans"]
    assert par.default == "torch" and par.kind is inspect.Parameter.KEYWORD_ONLY and tis.KMEANS == ("torch", "device")
    for bad in ("gpu", "numpy", None, ""):
        with pytest.raises(ValueError, match="kmeans must be one of"):      # before the model is touched
            tis.TIS(None, kmeans=bad)
    assert tis.TIS(None).kmeans == "torch" and tis.TIS(None, kmeans="device").kmeans == "device"
    assert cli.build_parser().parse_args([]).tis_kmeans == "torch"
    assert cli.build_parser().parse_args(["--tis_kmeans", "device"]).tis_kmeans == "device"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--tis_kmeans", "sklearn"])
    assert 'kmeans=testing_dict.get("tis_kmeans", "torch")' in inspect.getsource(sweep.vit_patch_map)      # TIS validates the value
    assert '"tis_kmeans": args.tis_kmeans' in inspect.getsource(cli.main)
    # the default loop is what it was
    src = inspect.getsource(tis.kmeans_centroids)
    assert "sim = 2 * points @ c.T - x_sq - (c * c).sum(1)[None]" in src and "if float(err) <= tol:" in src
    assert "return kmeans_centroids(channels, self.n_masks)" in inspect.getsource(tis.TIS.generate_raw_masks)
