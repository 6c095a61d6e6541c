"""XRAI without a GPU: the yardstick of the GPU tests (tests/xrai_restated.py replays the reference's recorded runs bit for bit, and
its fp64 form -- what K30 states -- selects the same masks on well-conditioned inputs), the mirror module's interface and
resolution, the harness row, the argument checks of the K29 / K30 entry points (made before any HIP call) and the host side of
xai_engine/xrai.py."""
import inspect
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import xrai_restated as R
from conftest import GOLDEN, PKG, load_golden

with open(os.path.join(GOLDEN, "xrai_api.json")) as _f:
    API = json.load(_f)
CASES = "abcdef"


def golden_case(g, tag):
    """-> attr (H, W) float32, masks, min_pixel_diff, area_threshold, fast of a stored case."""
    i, radius, mpd, th, fast = g[f"{tag}_params"].tolist()
    maps, attr3 = g[f"in{int(i)}_maps"], g[f"in{int(i)}_attr"]
    return attr3.max(-1), R.dilate(R.unpack(maps), int(radius)), int(mpd), float(th), bool(fast)


def restated(g, tag, dtype):
    attr, masks, mpd, th, fast = golden_case(g, tag)
    return R.xrai_fast(attr, masks, mpd, dtype) if fast else R.xrai(attr, masks, th, mpd, dtype)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_replays_the_reference_bit_for_bit(tag):
    """With the reference's own float32 mean the restatement gives the reference's output, selection keys, gains and ranks to the
    bit; in fp64 (K30's arithmetic) it selects the same masks, and the stored case is well conditioned: its distinct-set margin is
    at least 100 times the largest float32-vs-fp64 gain difference the reference's run logged."""
    g = load_golden("xrai.npz")
    r32 = restated(g, tag, np.float32)
    assert r32["out"].dtype == np.float64
    np.testing.assert_array_equal(r32["out"].astype(np.float32).view(np.int32), g[f"{tag}_out"].view(np.int32))
    np.testing.assert_array_equal(r32["keys"], g[f"{tag}_keys"])
    np.testing.assert_array_equal(r32["gains"].view(np.int32), g[f"{tag}_gains"].view(np.int32))
    np.testing.assert_array_equal(r32["ranks"], g[f"{tag}_ranks"])
    r64 = restated(g, tag, np.float64)
    np.testing.assert_array_equal(r64["keys"], g[f"{tag}_keys"])
    np.testing.assert_array_equal(r64["pixel_iter"], r32["pixel_iter"])
    margin, gain_err = g[f"{tag}_cond"].tolist()
    assert margin >= 100 * gain_err and R.conditioned(r64), (margin, gain_err, r64["margin"], r64["gain_err"])
    assert r64["margin"] == margin


def test_fixture_is_small_and_covers_the_paths():
    g = load_golden("xrai.npz")
    assert os.path.getsize(os.path.join(GOLDEN, "xrai.npz")) < 300 * 1024
    assert {tuple(g[f"in{i}_maps"].shape[1:]) for i in range(4)} == {(40, 36), (65, 63)}
    assert all(g[f"in{i}_maps"].dtype == np.int16 for i in range(4))
    p = {t: g[f"{t}_params"].tolist() for t in CASES}
    assert {v[4] for v in p.values()} == {0.0, 1.0} and {v[2] for v in p.values()} == {1.0, 50.0} and {v[3] for v in p.values()} == {1.0, 0.3}
    unc = {t: int((g[f"{t}_ranks"] == len(g[f"{t}_keys"]) + 1).sum()) for t in CASES}
    assert unc["a"] == 0 and unc["c"] > 0 and unc["d"] > 1000               # coverage equal to 1, below 1, cut by the threshold


def test_restated_helpers_pack_and_dilate():
    m = np.zeros((5, 30), bool)
    m[2, 3] = m[4, 29] = True
    bits = R.pack_bits([m, np.zeros_like(m)], m.shape)
    assert bits.shape == (2, 3) and bits[0].tolist() == [1 << 63, 0, 1 << (149 - 128)] and not bits[1].any()
    assert R.spans(bits).tolist() == [[0, 2], [3, -1]]
    assert R.disk(5).sum() == 81 and R.disk(0).shape == (1, 1)
    d = R.dilate([m], 2)[0]
    assert d.sum() == 13 + 6 and d[0, 3] and d[2, 5] and not d[0, 4] and d[4, 27] and d[2, 29]
    maps = np.array([[[0, 2], [2, 0]], [[-1, -1], [1, 1]]])
    assert [u.sum() for u in R.unpack(maps)] == [2, 0, 2, 2, 0, 2]


@pytest.mark.parametrize("name", sorted(API))
def test_mirror_has_the_reference_signature(name):
    from util.attribution_methods import XRAIBuilder
    obj = XRAIBuilder
    for part in name.split("."):
        obj = getattr(obj, part)
    params = list(inspect.signature(obj).parameters.values())[1 if "." in name else 0:]
    want = API[name]
    assert [p.name for p in params] == [w["name"] for w in want]
    for p, w in zip(params, want):
        assert (p.default is not inspect.Parameter.empty) == w["has_default"], (name, p.name)
        if w["has_default"]:
            assert p.default == w["default"] and type(p.default) is type(w["default"]), (name, p.name, p.default, w["default"])
    assert XRAIBuilder.XRAIParameters().experimental_params == {"min_pixel_diff": 50}


SIBLING = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])          # build first, sibling tree after it
    from util.attribution_methods import XRAIBuilder as XRAI                  # evaluatePerturbation.py:44
    import xai_engine.xrai as x
    assert XRAI.XRAI is x.XRAI and XRAI.XRAIParameters is x.XRAIParameters and XRAI.XRAIOutput is x.XRAIOutput
    assert XRAI.call_model_function is x.call_model_function
    assert XRAI.WHO == "sibling" and XRAI.CoreSaliency.WHO == "sibling core"
    assert XRAI._get_segments_felzenszwalb() == "sibling segments"
    print("xrai imports ok")
""")


def test_xrai_resolves_to_the_engine_and_the_rest_falls_through(tmp_path):
    root = tmp_path / "sibling" / "util"
    (root / "attribution_methods").mkdir(parents=True)
    (root / "__init__.py").write_text("")
    (root / "attribution_methods" / "__init__.py").write_text("")
    (root / "attribution_methods" / "XRAIBuilder.py").write_text(
        "WHO = 'sibling'\nclass CoreSaliency:\n    WHO = 'sibling core'\nclass XRAI:\n    WHO = 'sibling'\n"
        "def _get_segments_felzenszwalb():\n    return 'sibling segments'\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", SIBLING, PKG, str(tmp_path / "sibling")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "xrai imports ok" in r.stdout


def test_xrai_is_a_cnn_attribution_of_the_harness_in_the_reference_order():
    from xai_engine.sweep import CNN_ATTR_FUNCS
    i = CNN_ATTR_FUNCS.index("xrai")
    assert CNN_ATTR_FUNCS[i - 1] == "sg" and CNN_ATTR_FUNCS[i + 1] == "gc"


def test_k29_k30_entry_points_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    lib = _lib.load()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def pack(labels=p, lo=p, hi=p, S=2, masks=None, M=5, H=8, W=9, radius=5, bits=p, span=p):
        return lib.xai_xrai_pack_u64(labels, lo, hi, S, masks, M, H, W, radius, bits, span, None)
    assert pack(labels=None) == -1 and pack(masks=p) == -1 and pack(lo=None) == -1 and pack(hi=None) == -1
    assert pack(bits=None) == -1 and pack(span=None) == -1
    assert pack(S=0) == -2 and pack(M=0) == -2 and pack(H=0) == -2 and pack(W=-1) == -2 and pack(radius=-1) == -2
    assert pack(labels=None, lo=None, hi=None, S=0, masks=p, M=0) == -2
    assert pack(radius=65) == -3 and pack(H=65536, W=65536) == -3

    ws = lib.xai_xrai_workspace_bytes(2, 8, 9, 5)
    assert ws >= 3 * 5 * 4 and ws % 16 == 0 and lib.xai_xrai_workspace_bytes(1, 8, 9, 0) > 0
    assert lib.xai_xrai_workspace_bytes(0, 8, 9, 5) == 0 and lib.xai_xrai_workspace_bytes(1, 8, 9, -1) == 0

    def rank(ptrs=(p,) * 9, n_img=2, M=5, H=8, W=9, mpd=50, th=1.0, fast=0, ws_ptr=p, ws_bytes=ws):
        attr, bits, span, first, out, it, key, gain, state = ptrs
        return lib.xai_xrai_rank_f32(attr, bits, span, first, n_img, M, H, W, mpd, th, fast, out, it, key, gain, state, ws_ptr, ws_bytes, None)
    for i in range(9):
        assert rank(ptrs=tuple(None if j == i else p for j in range(9))) == -1, i
    assert rank(ws_ptr=None) == -1
    assert rank(n_img=0) == -2 and rank(H=0) == -2 and rank(W=0) == -2 and rank(M=-1) == -2 and rank(th=float("nan")) == -2
    assert rank(ws_bytes=ws - 16) == -2 and rank(ws_ptr=24) == -2
    assert rank(mpd=0) == -3 and rank(H=512, W=513) == -3


def test_xrai_refuses_the_cpu_and_the_arguments_the_reference_dies_on():
    from xai_engine import XaiHipError
    from xai_engine.xrai import XRAI, pack_segments, xrai_batch
    attr = torch.zeros(1, 3, 8, 8)
    masks = np.ones((2, 8, 8), bool)
    with pytest.raises(XaiHipError):
        xrai_batch(attr, masks)
    with pytest.raises(XaiHipError):
        pack_segments(masks, device="cpu")
    with pytest.raises(XaiHipError):
        XRAI().GetMask(np.zeros((8, 8, 3), np.float32), segments=list(masks), base_attribution=np.zeros((8, 8, 3), np.float32))
    with pytest.raises(NotImplementedError, match="min_pixel_diff"):
        xrai_batch(attr, masks, min_pixel_diff=0)
    with pytest.raises(ValueError, match="Unknown algorithm type"):
        xrai_batch(attr, masks, algorithm="quick")
    with pytest.raises(ValueError, match="base attribution shape"):
        XRAI().GetMask(np.zeros((8, 8, 3), np.float32), segments=list(masks), base_attribution=np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError, match="base_attribution"):
        XRAI().GetMask(np.zeros((8, 8, 3), np.float32), segments=list(masks))


def test_ranked_segments_orders_the_selections_like_the_reference():
    """:702-711 from K30's outputs: a stable sort by descending gain (equal gains keep the selection order), the uncomputed last."""
    from xai_engine.xrai import ranked_segments
    g = load_golden("xrai.npz")
    for tag in CASES:
        r = restated(g, tag, np.float32)
        np.testing.assert_array_equal(ranked_segments(r["pixel_iter"], r["gains"]), g[f"{tag}_ranks"])
    pi = np.array([[0, 1, -1], [2, 2, 0]])
    assert ranked_segments(pi, [0.5, 2.0, 0.5]).tolist() == [[2, 1, 4], [3, 3, 2]]
    masks = ranked_segments(pi, [0.5, 2.0, 0.5], flatten=False)
    assert [m.sum() for m in masks] == [1, 2, 2, 1] and masks[0][0, 1] and masks[3][0, 2]
    assert len(ranked_segments(np.zeros((2, 2), int), [1.0], flatten=False)) == 1


def test_felzenszwalb_label_maps_without_skimage_says_what_still_works():
    from xai_engine.xrai import felzenszwalb_label_maps
    try:
        import skimage  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="segments="):
            felzenszwalb_label_maps(np.zeros((8, 8, 3), np.float32))
    else:
        assert felzenszwalb_label_maps(np.random.default_rng(0).random((32, 32, 3)).astype(np.float32)).shape == (6, 32, 32)


STUB_SKIMAGE = textwrap.dedent("""
    import numpy as np
    CALLS = []
    def felzenszwalb(im, scale=1, sigma=0.8, min_size=20):
        CALLS.append((np.array(im), scale, sigma, min_size))
        return np.full(im.shape[:2], len(CALLS), dtype=np.int64)
""")
WITH_STUB = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])
    import numpy as np, torch
    from xai_engine.xrai import felzenszwalb_label_maps
    x = np.random.default_rng(5).standard_normal((9, 7, 3)).astype(np.float32)
    maps = felzenszwalb_label_maps(torch.from_numpy(x))
    from skimage.segmentation import CALLS
    assert maps.shape == (6, 9, 7) and [int(m[0, 0]) for m in maps] == [1, 2, 3, 4, 5, 6]
    assert [c[1:] for c in CALLS] == [(s, 0.8, 150) for s in (50, 100, 150, 250, 500, 1200)], [c[1:] for c in CALLS]
    t = torch.from_numpy(x)                                  # _normalize_image, XRAIBuilder.py:186-189, restated
    want = ((t - torch.min(t)) / (torch.max(t) - torch.min(t))) * (1.0 - -1.0) + -1.0
    for c in CALLS:
        assert c[0].dtype == np.float32 and np.array_equal(c[0], want.numpy())
    assert want.min() == -1.0 and want.max() == 1.0
    assert np.array_equal(felzenszwalb_label_maps(x), maps + 6)      # an array works like a tensor
    print("stub ok")
""")


def test_felzenszwalb_label_maps_calls_the_segmenter_like_the_reference(tmp_path):
    pkg = tmp_path / "site" / "skimage"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    (pkg / "segmentation.py").write_text(STUB_SKIMAGE)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", WITH_STUB, PKG, str(tmp_path / "site")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stub ok" in r.stdout
