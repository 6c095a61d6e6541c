"""AGI without a GPU: the harness row and the CLI, the interface of xai_engine.agi, the argument checks of K23-K25 (made before
any HIP call), and the NumPy restatement (tests/agi_restated.py) against the reference's own recorded runs (tests/golden/agi.npz)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import agi_restated as R
from conftest import GOLDEN, check, load_golden
from helpers import tiny_from

with open(os.path.join(GOLDEN, "agi_api.json")) as _f:
    API = json.load(_f)
CASES = ("a", "b", "c", "d", "e")


def test_agi_is_a_cnn_attribution_of_the_harness_and_the_cli():
    from xai_engine.sweep import CNN_ATTR_FUNCS, TRANS_ATTR_FUNCS
    from xai_engine.evaluate_perturbation import build_parser
    assert "agi" in CNN_ATTR_FUNCS and "agi" in TRANS_ATTR_FUNCS
    assert "agi" in build_parser().format_help()


@pytest.mark.parametrize("name", sorted(API))
def test_engine_has_the_reference_signature(name):
    from xai_engine import agi
    if "." in name:
        cls, meth = name.split(".")
        params = list(inspect.signature(getattr(getattr(agi, cls), meth)).parameters.values())[1:]
    else:
        params = list(inspect.signature(getattr(agi, name)).parameters.values())
    want = API[name]
    assert [p.name for p in params] == [w["name"] for w in want]
    for p, w in zip(params, want):
        assert (p.default is not inspect.Parameter.empty) == w["has_default"], (name, p.name)
        if w["has_default"]:
            assert p.default == w["default"], (name, p.name)


def test_k23_k25_entry_points_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    lib = _lib.load()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def init(ptrs=(p,) * 7, n_img=1, n_cls=1, n_out=10, n=4):
        return lib.xai_agi_init_f32(ptrs[0], ptrs[1], ptrs[2], n_img, n_cls, n_out, n, ptrs[3], ptrs[4], ptrs[5], ptrs[6], None)
    for i in range(7):
        assert init(ptrs=tuple(None if j == i else p for j in range(7))) == -1, i
    assert init(n_img=0) == -2 and init(n_cls=0) == -2 and init(n_out=0) == -2 and init(n=0) == -2
    assert init(n_img=300, n_cls=300) == -3

    def step(ptrs=(p,) * 8, n_img=1, n_cls=1, n_out=10, n=4, eps=0.05, max_iter=20):
        return lib.xai_agi_step_f32(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], n_img, n_cls, n_out, n, eps, max_iter, ptrs[5], ptrs[6],
                                    ptrs[7], None)
    for i in range(8):
        assert step(ptrs=tuple(None if j == i else p for j in range(8))) == -1, i
    assert step(n_img=0) == -2 and step(n_cls=0) == -2 and step(n=0) == -2 and step(max_iter=0) == -2
    assert step(eps=float("nan")) == -2 and step(n_img=70000) == -3

    def heat(cd=p, out=p, n_img=1, n_cls=1, C=3, HW=256, lo=80.0, hi=99.0):
        return lib.xai_agi_heatmap_f32(cd, n_img, n_cls, C, HW, lo, hi, out, None, None, None)
    assert heat(cd=None) == -1 and heat(out=None) == -1
    assert heat(n_img=0) == -2 and heat(n_cls=0) == -2 and heat(C=0) == -2 and heat(HW=0) == -2
    assert heat(lo=-1.0) == -2 and heat(hi=100.5) == -2 and heat(lo=float("nan")) == -2
    assert heat(HW=1 << 24) == -3


def test_engine_refuses_the_cpu_and_bad_arguments():
    from xai_engine import XaiHipError
    from xai_engine import agi
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(XaiHipError):
        agi.agi_batch(x, torch.nn.Identity(), [0])
    with pytest.raises(XaiHipError):
        agi.test(torch.nn.Identity(), "cpu", np.zeros((8, 8, 3), np.float32), 0.05, 1, [0], 20)
    with pytest.raises(XaiHipError):
        agi.fgsm_step(x, 0.05, x, x)
    from xai_engine import kernels as K
    with pytest.raises(XaiHipError):
        K.agi_heatmap(torch.zeros(1, 3, 4, 4), 1)


def _recorded_oracles(g, tag):
    """oracle_of(k) serving the reference's own logits and gradients of the k-th class's attack, and checking that each forward
    runs on the x the reference ran it on"""
    pair, fx, fl, fga, fgl = (g[f"{tag}_{k}"] for k in ("pair", "fx", "fl", "fga", "fgl"))
    classes = g[f"{tag}_classes"].tolist()

    def oracle_of(k):
        idx = np.flatnonzero(pair == classes[k])

        def oracle(i, x):
            j = idx[i]
            np.testing.assert_array_equal(x.view(np.int32), fx[j].view(np.int32), err_msg=f"x of forward {i}, class {classes[k]}")
            return fl[j], fga[j], fgl[j]
        return oracle
    return oracle_of


@pytest.mark.parametrize("tag", CASES)
def test_restatement_replays_the_reference_bit_for_bit(tag):
    """Fed the recorded logits and gradients, the restated loop reproduces every x_i, the number of forwards of every attack (its
    break iteration), step_grad and the harness map bit for bit; case (e) is the reference's (0, 0, 0)."""
    g = load_golden("agi.npz")
    eps, max_iter = g[f"{tag}_params"].tolist()
    data = g[f"{tag}_data"][0]
    classes = g[f"{tag}_classes"].tolist()
    pairs, step_grad = R.run(data, classes, int(g[f"{tag}_init_pred"]), eps, int(max_iter), _recorded_oracles(g, tag))
    for k, cls in enumerate(classes):
        n_fwd = int((g[f"{tag}_pair"] == cls).sum())
        if pairs[k] is None:
            assert n_fwd == 0
            continue
        seen, c, n, broke = pairs[k]
        assert len(seen) == n_fwd and n == n_fwd - int(broke), (tag, cls)
    if g[f"{tag}_zero"]:
        assert step_grad is None
        return
    np.testing.assert_array_equal(step_grad.view(np.int32), g[f"{tag}_adv"].view(np.int32))
    hm = R.harness_map(step_grad)
    np.testing.assert_array_equal(hm.view(np.int32), g[f"{tag}_hm"].view(np.int32))


@pytest.mark.parametrize("tag", CASES)
def test_restatement_as_a_whole_loop_on_the_cpu(tag):
    """The restated loop driving TinyNet itself (torch on the CPU) ends where the reference ended: same forwards per attack,
    step_grad and the map within the 1e-5 bar."""
    g = load_golden("agi.npz")
    model = tiny_from(g)
    eps, max_iter = g[f"{tag}_params"].tolist()
    data = g[f"{tag}_data"][0]
    classes = g[f"{tag}_classes"].tolist()
    ip = int(g[f"{tag}_init_pred"])
    pairs, step_grad = R.run(data, classes, ip, eps, int(max_iter),
                             lambda k: R.torch_oracle(model, g["mean"], g["std"], ip, classes[k]))
    for k, cls in enumerate(classes):
        if pairs[k] is not None:
            assert len(pairs[k][0]) == int((g[f"{tag}_pair"] == cls).sum()), (tag, cls)
    if g[f"{tag}_zero"]:
        assert step_grad is None
        return
    check(f"agi/restated_loop/{tag}/step_grad", step_grad, g[f"{tag}_adv"], 1e-5, against="reference AGI.test")
    check(f"agi/restated_loop/{tag}/map", R.harness_map(step_grad), g[f"{tag}_hm"], 1e-5, against="reference AGI.test")
