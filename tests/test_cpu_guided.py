"""Guided Backprop / Guided Grad-CAM without a GPU: the harness rows and the CLI, the captum-shaped classes, the refusals, the
three new ABI entries and their argument checks (made before any HIP call), the thread-local guided switch, and the restatement
(tests/guided_restated.py) against the DEFINITION of the method computed by an independent float64 backward -- not against captum,
which is on neither machine (parity with captum itself is unpinned: DESIGN.md)."""
import inspect
import os
import re
import subprocess
import sys
import textwrap
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guided_restated as R
from conftest import PKG, ROOT
from helpers import TinyNet


def test_gbp_and_ggc_are_cnn_attributions_of_the_harness_and_the_cli():
    from xai_engine.sweep import CNN_ATTR_FUNCS
    from xai_engine.evaluate_perturbation import build_parser
    assert CNN_ATTR_FUNCS[-5:] == ("gc", "gbp", "ggc", "fa", "occ")              # the reference's order (:147-176)
    text = build_parser().format_help()
    assert " gbp," in text and " ggc," in text


def test_classes_carry_captums_parameter_names():
    from xai_engine import guided
    p = inspect.signature(guided.GuidedBackprop.attribute).parameters
    assert list(p) == ["self", "inputs", "target", "additional_forward_args"]
    p = inspect.signature(guided.GuidedGradCam.attribute).parameters
    assert list(p) == ["self", "inputs", "target", "additional_forward_args", "interpolate_mode", "attribute_to_layer_input"]
    assert p["interpolate_mode"].default == "nearest" and p["attribute_to_layer_input"].default is False
    assert list(inspect.signature(guided.GuidedBackprop.__init__).parameters) == ["self", "model"]
    p = inspect.signature(guided.GuidedGradCam.__init__).parameters
    assert list(p) == ["self", "model", "layer", "device_ids"] and p["device_ids"].default is None
    p = inspect.signature(guided.guided_backprop_batch).parameters
    assert list(p) == ["x", "model", "targets", "layer", "want_attr", "want_map", "graphs"]
    assert (p["layer"].default, p["want_attr"].default, p["want_map"].default, p["graphs"].default) == (None, True, False, True)
    from xai_engine import kernels as K
    assert inspect.signature(K.bn_relu_bwd_mask).parameters["guided"].default is False
    assert inspect.signature(K.bn_relu_maxpool_bwd).parameters["guided"].default is False
    p = inspect.signature(K.guided_map).parameters
    assert list(p)[:4] == ["grad", "cam", "want_attr", "want_map"] and p["cam"].default is None


def test_engine_refuses_the_cpu():
    from xai_engine import XaiHipError, guided
    from xai_engine import kernels as K
    x, net = torch.zeros(1, 3, 8, 8), TinyNet().eval()
    with pytest.raises(XaiHipError):
        guided.guided_backprop_batch(x, net, 0)
    with pytest.raises(XaiHipError):
        guided.guided_backprop_batch(x, net, 0, layer=net.conv, want_map=True)
    with pytest.raises(XaiHipError):
        guided.GuidedBackprop(net).attribute(x, target=0)
    with pytest.raises(XaiHipError):
        guided.GuidedGradCam(net, net.conv).attribute(x, 0)
    with pytest.raises(XaiHipError):
        guided.GuidedGradCam(net, net.conv).attribute(x, 0, interpolate_mode="bilinear")
    with pytest.raises(XaiHipError):
        K.guided_map(torch.zeros(1, 3, 8, 8))
    with pytest.raises(XaiHipError):
        K.bn_relu_bwd_mask(torch.zeros(1, 3, 8, 8), torch.zeros(32, dtype=torch.uint8), torch.ones(3), torch.ones(3), 1e-5, 9, guided=True)
    with pytest.raises(NotImplementedError):
        guided.guided_backprop_batch((x, x), net, 0)


def test_inplace_relu_modules_are_refused_on_the_compatibility_path_only():
    from xai_engine import XaiHipError, guided
    from xai_engine.prepare import fuse_bn_relu
    from xai_engine.zoo import resnet50
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.ReLU(inplace=True))
    with pytest.raises(XaiHipError, match="fuse_bn_relu"):
        guided._refuse_inplace(net)
    with pytest.raises(XaiHipError, match="inplace"):
        with guided._guided_modules(net):
            pass
    assert not net[1]._forward_hooks                                             # nothing left behind
    model = resnet50(seed=0, width=8, num_classes=10)
    assert len(guided._refuse_inplace(model)) == 17                              # stem + 16 blocks, all hooked when unfused
    for m in model.modules():
        if isinstance(m, torch.nn.ReLU):
            m.inplace = True                                                     # torchvision's own definition
    with pytest.raises(XaiHipError):
        guided._refuse_inplace(model)
    assert guided._refuse_inplace(fuse_bn_relu(model)) == []                     # the fused path never calls them
    ok = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.ReLU())
    with guided._guided_modules(ok):
        assert len(ok[1]._forward_hooks) == 1
    assert not ok[1]._forward_hooks


def test_guided_relu_is_a_thread_local_switch_read_in_the_forward():
    from xai_engine import prepare
    assert not prepare.guided_active()
    seen = {}
    with prepare.guided_relu():
        assert prepare.guided_active()
        t = threading.Thread(target=lambda: seen.__setitem__("other", prepare.guided_active()))
        t.start()
        t.join()
        with prepare.guided_relu():
            pass
        assert prepare.guided_active()                                           # the inner exit restores, it does not clear
    assert not prepare.guided_active() and seen["other"] is False
    with pytest.raises(RuntimeError):
        with prepare.guided_relu():
            raise RuntimeError("x")
    assert not prepare.guided_active()
    # the torch-op form that non-fusable sites take (CPU tensors here): relu forward, clamp-then-gate backward
    bn = torch.nn.BatchNorm2d(2).eval()
    x = torch.tensor([[-1.0, 2.0], [3.0, 0.5]]).view(1, 2, 2, 1).requires_grad_(True)
    gy = torch.tensor([[5.0, -7.0], [float("nan"), 0.25]]).view(1, 2, 2, 1)
    with prepare.guided_relu():
        y = prepare.bn_relu(x, bn)
    (g,) = torch.autograd.grad(y, x, gy)                                         # backward OUTSIDE the context: the site remembers
    s = float(1 / np.sqrt(np.float32(1 + 1e-5)))
    want = torch.tensor([[0.0, 0.0], [float("nan"), 0.25 * s]]).view(1, 2, 2, 1)
    assert torch.allclose(g, want, rtol=1e-6, atol=0, equal_nan=True)
    (g_plain,) = torch.autograd.grad(prepare.bn_relu(x, bn), x, gy)
    assert float(g_plain[0, 0, 1, 0]) == pytest.approx(-7.0 * s, rel=1e-6)       # and outside nothing changes


def _declared():
    src = open(os.path.join(ROOT, "include", "xai_hip.h")).read()
    return src, set(re.findall(r"\b(xai_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


NEW = ("xai_bn_relu_bwd_mask_guided_f32", "xai_bn_relu_maxpool_bwd_guided_f32", "xai_guided_map_f32")


def test_the_three_new_symbols_are_declared_exported_and_bound():
    from xai_engine import _lib, LIB_PATH
    src, names = _declared()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and re.search(rf" T {n}$", out, flags=re.M), n
        at = src.index(n + "(")
        assert re.search(r"evaluatePerturbation\.py:15[49]-1(58|63)", src[src.rfind("/*", 0, at):at]), n
    assert "evaluatePerturbation.py:159-163" in src and ":181" in src[src.index("K28"):]
    assert _lib.SIGNATURES[NEW[0]] == _lib.SIGNATURES["xai_bn_relu_bwd_mask_f32"]
    assert _lib.SIGNATURES[NEW[1]] == _lib.SIGNATURES["xai_bn_relu_maxpool_bwd_f32"]
    assert lib.xai_version_minor() == _lib.ABI_MINOR >= 9


def test_new_entry_points_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    lib = _lib.load()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def mask(gy=p, m=p, w=p, var=p, gx=p, w2=None, var2=None, gid=None, variant=9, N=1, C=3, HW=49):
        return lib.xai_bn_relu_bwd_mask_guided_f32(gy, None, m, w, var, 1e-5, w2, var2, 1e-5, variant, N, C, HW, gx, gid, None)
    assert mask(gy=None) == -1 and mask(m=None) == -1 and mask(w=None) == -1 and mask(var=None) == -1 and mask(gx=None) == -1
    assert mask(N=0) == -2 and mask(C=0) == -2 and mask(HW=0) == -2 and mask(variant=16) == -2 and mask(m=12) == -2
    assert mask(w2=p) == -1 and mask(w2=p, gid=p) == -1                         # the second BatchNorm needs g_identity and var2

    def stem(gy=p, code=p, w=p, var=p, gx=p, N=1, C=3, H=8, W=8, PH=4, PW=4, k=3, s=2, pad=1):
        return lib.xai_bn_relu_maxpool_bwd_guided_f32(gy, None, code, w, var, 1e-5, 9, N, C, H, W, PH, PW, k, s, pad, gx, None)
    assert stem(gy=None) == -1 and stem(code=None) == -1 and stem(w=None) == -1 and stem(var=None) == -1 and stem(gx=None) == -1
    assert stem(N=0) == -2 and stem(PH=5) == -2 and stem(pad=2) == -2 and stem(s=0) == -2
    assert stem(s=1, PH=8, PW=8) == -3 and stem(N=70000) == -3                               # three windows per axis; planes beyond grid.y

    def gmap(grad=p, cam=p, attr=p, out=p, B=1, C=3, H=8, W=8, h=2, w=2):
        return lib.xai_guided_map_f32(grad, cam, B, C, H, W, h, w, attr, out, None)
    assert gmap(grad=None) == -1 and gmap(attr=None, out=None) == -1
    assert gmap(B=0) == -2 and gmap(C=0) == -2 and gmap(H=0) == -2 and gmap(W=0) == -2 and gmap(h=0) == -2 and gmap(w=-1) == -2
    assert gmap(cam=None, attr=None, out=None, h=0, w=0) == -1


CAPTUM = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])
    import captum.attr
    before = dict(vars(captum.attr))
    from util import model_utils
    import xai_engine.guided as gd
    assert captum.attr.GuidedBackprop.WHO == "captum" and captum.attr.GuidedGradCam.WHO == "captum"      # not asked: untouched
    assert gd.patch_captum() == (before["GuidedBackprop"], before["GuidedGradCam"])
    from captum.attr import GuidedBackprop, GuidedGradCam, LayerGradCam
    assert GuidedBackprop is gd.GuidedBackprop and GuidedGradCam is gd.GuidedGradCam and LayerGradCam.WHO == "captum"
    changed = sorted(k for k, v in vars(captum.attr).items() if before.get(k) is not v)
    assert changed == ["GuidedBackprop", "GuidedGradCam"], changed
    assert gd.patch_captum() == (gd.GuidedBackprop, gd.GuidedGradCam)
    print("captum ok")
""")


def test_patch_captum_rebinds_exactly_the_two_names(tmp_path):
    pkg = tmp_path / "site" / "captum" / "attr"
    pkg.mkdir(parents=True)
    (tmp_path / "site" / "captum" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("".join(f"class {n}: WHO = 'captum'\n" for n in ("LayerGradCam", "GuidedBackprop", "GuidedGradCam")))
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "XAI_PATCH_CAPTUM")}
    r = subprocess.run([sys.executable, "-c", CAPTUM, PKG, str(tmp_path / "site")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "captum ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the restatement vs the definition
def _tiny64(seed):
    torch.manual_seed(seed)
    return TinyNet().eval().double()


def _manual_guided_backward(net, x, t, guided=True):
    """TinyNet (conv 3x3 pad 1 -> ReLU -> 4 x 4 average pool -> fc) backwards, layer by layer in float64 loops, the clamp put in by
    hand between the pool's gradient and the ReLU's gate."""
    w, b = net.conv.weight.detach().numpy(), net.conv.bias.detach().numpy()
    fw = net.fc.weight.detach().numpy()
    B, C, H, W = x.shape
    O, bh, bw = w.shape[0], H // 4, W // 4
    out = np.zeros((B, C, H, W))
    for n in range(B):
        xp = np.zeros((C, H + 2, W + 2))
        xp[:, 1:-1, 1:-1] = x[n].numpy()
        z = np.zeros((O, H, W))
        for o in range(O):
            for i in range(H):
                for j in range(W):
                    z[o, i, j] = b[o] + (w[o] * xp[:, i:i + 3, j:j + 3]).sum()
        g_pool = fw[int(t[n])].reshape(O, 4, 4)                                  # d logit_t / d pooled
        g_y = np.repeat(np.repeat(g_pool, bh, axis=1), bw, axis=2) / (bh * bw)    # average pool: every element of a cell, 1 / area
        if guided:
            g_y = np.where(g_y <= 0, 0.0, g_y)                                    # THE clamp: on the complete gradient of the ReLU's output
        g_z = np.where(z > 0, g_y, 0.0)                                           # the gate
        gp = np.zeros((C, H + 2, W + 2))
        for o in range(O):
            for i in range(H):
                for j in range(W):
                    gp[:, i:i + 3, j:j + 3] += w[o] * g_z[o, i, j]
        out[n] = gp[:, 1:-1, 1:-1]
    return out


def test_guided_backprop_restated_is_the_definition():
    net = _tiny64(0)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    t = torch.tensor([3, 8])
    got = R.guided_backprop(net, x, t).numpy()
    want = _manual_guided_backward(net, x, t)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    plain = _manual_guided_backward(net, x, t, guided=False)
    xr = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(net(xr).gather(1, t.view(-1, 1)).sum(), xr)
    assert np.abs(g.numpy() - plain).max() <= 1e-12 * np.abs(plain).max()        # the loops are a backward pass at all
    assert np.abs(want - plain).max() >= 0.1 * np.abs(plain).max()               # and the clamp is no detail
    assert not any(m._backward_pre_hooks for m in net.modules())                 # hooks removed


def test_guided_gradcam_restated_is_the_product_with_the_nearest_upsampled_cam():
    net = _tiny64(2)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    t = torch.tensor([1, 6])
    act, g = R.layer_act_and_grad(net, net.act, x, t)
    cam = np.zeros((2, 8, 8))
    for n in range(2):
        for c in range(8):
            cam[n] += g[n, c].numpy().mean() * act[n, c].numpy()
    cam = np.maximum(cam, 0.0)
    assert np.abs(R.gradcam(net, net.act, x, t)[:, 0].numpy() - cam).max() <= 1e-12 * cam.max()
    want = _manual_guided_backward(net, x, t) * cam[:, None]                     # the layer has the input's size: nearest is the identity
    got = R.guided_gradcam(net, net.act, x, t).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    m = R.harness_map(torch.from_numpy(want[0]))
    assert m.shape == (8, 8) and np.array_equal(m, np.abs((want[0][0] + want[0][1]) + want[0][2]))


@pytest.mark.parametrize("n_in,n_out", [(7, 224), (3, 80), (5, 37), (7, 100), (4, 53), (1, 12)])
def test_nearest_index_rule_is_interpolates(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1).expand(1, 1, n_in, n_in).contiguous()
    got = F.interpolate(src, size=(n_out, n_out), mode="nearest")[0, 0, :, 0].long().tolist()
    assert got == R.nearest_index(n_in, n_out)
    if (n_in, n_out) == (7, 100):                                                # not nearest-exact, which centres the samples
        exact = F.interpolate(src, size=(n_out, n_out), mode="nearest-exact")[0, 0, :, 0].long().tolist()
        assert exact != got


def test_both_torch_op_paths_equal_the_restatement_on_a_resnet_on_the_cpu():
    """Off the GPU a fused classifier's sites fall back to the PyTorch modules and take the guided rule from the small autograd
    function; an unfused classifier takes it from the gradient hooks of the compatibility path.  Both against the restatement's
    backward-pre-hooks on the same CPU kernels: bit for bit.  (The drivers themselves refuse CPU tensors; this drives their parts.)"""
    from xai_engine import guided, prepare
    from xai_engine.zoo import resnet50
    model = resnet50(seed=0, width=8, num_classes=10).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    t = torch.tensor([3, 7])
    want = R.guided_backprop(model, x, t)
    _, want_ga = R.layer_act_and_grad(model, model.layer4, x, t)

    def grads(m, ctx):
        kept = {}
        h = m.layer4.register_forward_hook(lambda mod, inp, out: kept.__setitem__("act", out))
        xr = x.clone().requires_grad_(True)
        with ctx:
            score = m(xr).gather(1, t.view(-1, 1)).sum()
        h.remove()
        return torch.autograd.grad(score, [xr, kept["act"]])                   # outside the context
    for fork in (False, True):
        gx, ga = grads(prepare.fuse_bn_relu(model, fork_residual=fork), prepare.guided_relu())
        assert torch.equal(gx, want) and torch.equal(ga, want_ga)              # the layer gradient is the PLAIN one: no ReLU behind layer4
    gx, ga = grads(model, guided._guided_modules(model))
    assert torch.equal(gx, want) and torch.equal(ga, want_ga)
    xr = x.clone().requires_grad_(True)
    (plain,) = torch.autograd.grad(model(xr).gather(1, t.view(-1, 1)).sum(), xr)
    assert float((plain - want).abs().max()) > 0.1 * float(want.abs().max())
    assert not any(m._forward_hooks for m in model.modules())
