"""Guided Backprop / Guided Grad-CAM on the device: the guided forms of the two fused backward kernels and K28 at tolerance 0
against torch expressions on the same device, and the whole classifier (fused, fused + forked, unfused) against the restatement
of captum's flow (tests/guided_restated.py) on the unfused model -- same convolutions under deterministic solvers (conftest), fused
sites bitwise PyTorch's, so the expected difference is 0 and the bar is the project's 1e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guided_restated as R
from conftest import BAR, check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPECIAL = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-40, -1e-40, 1.0, -1.0]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _equal_nan_aware(a, b):
    na, nb = a.isnan(), b.isnan()
    zero = torch.zeros((), device=a.device)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


def _clamp(g):
    return torch.where(g <= 0, torch.zeros((), device=g.device), g)


def _bn_params(Cc, gen):
    w = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    w[::3] *= -1                            # negative scales: the sign of a zero gradient is part of the bit pattern
    return (w, torch.randn(Cc, device=DEV, generator=gen), torch.randn(Cc, device=DEV, generator=gen),
            torch.rand(Cc, device=DEV, generator=gen) + 0.2, 1e-5)


def _sprinkle(t, gen, every=5):
    vals = torch.tensor(SPECIAL, device=DEV)
    pos = torch.randperm(t.numel(), device=DEV, generator=gen)[: t.numel() // every]
    t.view(-1)[pos] = vals[torch.arange(pos.numel(), device=DEV) % len(SPECIAL)]
    return t


# ------------------------------------------------------------------------------------------------ guided mask backward
@pytest.mark.parametrize("shape", [(2, 3, 7, 7),          # HW = 49: scalar path, n = 294
                                   (1, 5, 14, 14),        # HW = 196: vector path, a partial last wavefront
                                   (50, 16, 7, 7)])       # scalar path, channels changing inside a lane's four elements
@pytest.mark.parametrize("add", ["none", "identity", "bn2"])
@pytest.mark.parametrize("second", [False, True])
def test_guided_mask_backward_is_the_unguided_one_on_the_clamped_sum(shape, add, second):
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    gen = torch.Generator(device=DEV).manual_seed(41)
    Cc = shape[1]
    w, b, mean, var, eps = _bn_params(Cc, gen)
    x, idt = (torch.randn(shape, device=DEV, generator=gen) for _ in range(2))
    gy = _sprinkle(torch.randn(shape, device=DEV, generator=gen), gen)
    gy2 = _sprinkle(torch.randn(shape, device=DEV, generator=gen), gen, every=7) if second else None
    identity = None if add == "none" else idt
    bn2f = bn2b = None
    if add == "bn2":
        w2, b2, m2, v2, e2 = _bn_params(Cc, gen)
        bn2f, bn2b = (w2, b2, m2, v2, e2), (w2, v2, e2)
    y, mask = K.bn_relu_fwd_mask(x, identity, w, b, mean, var, eps, BN_VARIANT, bn2=bn2f)
    assert 0.2 < float((y > 0).float().mean()) < 0.8                           # open and closed gates both
    g = gy if gy2 is None else gy + gy2                                        # one fp32 add, as the kernel's
    assert bool((g < 0).any()) and bool(g.isnan().any()) and bool((g == 0).any())
    kw = dict(want_identity=identity is not None, bn2=bn2b)
    want_gx, want_gid = K.bn_relu_bwd_mask(_clamp(g), mask, w, var, eps, BN_VARIANT, gy2=None, **kw)
    gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, eps, BN_VARIANT, gy2=gy2, guided=True, **kw)
    assert _bits_equal(gx, want_gx)
    assert (gid is None and want_gid is None) or _bits_equal(gid, want_gid)
    # and unguided it is still what the y-reading kernel of the parent computes
    ref_gx, ref_gid = K.bn_relu_bwd(gy, y, w, var, eps, BN_VARIANT, gy2=gy2, **kw)
    gx0, gid0 = K.bn_relu_bwd_mask(gy, mask, w, var, eps, BN_VARIANT, gy2=gy2, guided=False, **kw)
    assert _bits_equal(gx0, ref_gx) and ((gid0 is None and ref_gid is None) or _bits_equal(gid0, ref_gid))
    assert not _bits_equal(gx, gx0)


# ------------------------------------------------------------------------------------------------ guided stem backward
@pytest.mark.parametrize("shape,geom", [((2, 3, 9, 10), (2, 1, 1)), ((3, 3, 20, 20), (2, 2, 0)), ((1, 3, 37, 53), (4, 2, 2)),
                                        ((2, 3, 113, 111), (3, 2, 1))])
@pytest.mark.parametrize("second", [False, True])
def test_guided_stem_backward_equals_the_pytorch_chain_with_the_clamp_on_the_relu_output(shape, geom, second):
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    k, s, p = geom
    gen = torch.Generator(device=DEV).manual_seed(43)
    N, Cc, H, W = shape
    w = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    w[1] *= -1
    b = torch.randn(Cc, device=DEV, generator=gen) * 0.1
    mean = torch.randn(Cc, device=DEV, generator=gen) * 0.1
    var = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    x = torch.randn(shape, device=DEV, generator=gen).round(decimals=1)        # ties on purpose
    xr = x.clone().requires_grad_(True)
    act = F.relu(F.batch_norm(xr, mean, var, w, b, False, 0.0, 1e-5))
    act.register_hook(_clamp)                                                   # the complete gradient of the ReLU's output
    y_ref, idx = F.max_pool2d(act, k, s, p, 1, False, True)
    g1 = _sprinkle(torch.randn_like(y_ref), gen, every=11)
    g2 = torch.randn_like(y_ref) if second else None
    if second:
        (want,) = torch.autograd.grad([y_ref, y_ref], xr, [g1, g2])
    else:
        (want,) = torch.autograd.grad(y_ref, xr, g1)
    y, code = K.bn_relu_maxpool_fwd_code(x, w, b, mean, var, 1e-5, BN_VARIANT, k, s, p)
    assert _equal_nan_aware(y, y_ref.detach())
    got = K.bn_relu_maxpool_bwd(g1, code, w, var, 1e-5, BN_VARIANT, H, W, k, s, p, gy2=g2, guided=True)
    assert _equal_nan_aware(got, want)
    plain = K.bn_relu_maxpool_bwd(g1, code, w, var, 1e-5, BN_VARIANT, H, W, k, s, p, gy2=g2)
    assert not _equal_nan_aware(got, plain)
    if k > s:
        # the case must not be passable by clamping per window: some open position was selected by several windows whose
        # gradients have both signs
        g = (g1 if g2 is None else g1 + g2).flatten(2)
        flat = idx.flatten(2)
        pos = torch.zeros(N, Cc, H * W, device=DEV).scatter_add_(2, flat, (g > 0).float())
        neg = torch.zeros(N, Cc, H * W, device=DEV).scatter_add_(2, flat, (g < 0).float())
        mixed = (pos > 0) & (neg > 0) & (act.detach().flatten(2) > 0)
        assert int(mixed.sum()) >= 3
        per_window = torch.zeros(N, Cc, H * W, device=DEV).scatter_add_(2, flat, torch.nan_to_num(_clamp(g), nan=0.0, posinf=0.0))
        whole = _clamp(torch.zeros(N, Cc, H * W, device=DEV).scatter_add_(2, flat, torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0)))
        assert bool((per_window[mixed] != whole[mixed]).any())


# ------------------------------------------------------------------------------------------------ K28
def _k28_want(grad, cam):
    a = grad if cam is None else grad * F.interpolate(cam[:, None], grad.shape[2:], mode="nearest")
    m = a[:, 0]
    for c in range(1, a.shape[1]):
        m = m + a[:, c]
    return a, m.abs()


@pytest.mark.parametrize("case", [(2, 3, 224, 224, 7, 7),         # vector path
                                  (1, 3, 80, 80, 3, 3),            # W % 4 == 0 and a non-integer factor
                                  (2, 3, 37, 53, 5, 4),            # scalar path, non-integer factors
                                  (1, 1, 8, 8, 2, 2), (1, 4, 16, 12, 1, 1)])
@pytest.mark.parametrize("with_cam", [False, True])
@pytest.mark.parametrize("outputs", ["attr", "map", "both"])
@pytest.mark.parametrize("misaligned", [False, True])
def test_k28_equals_the_torch_expression(case, with_cam, outputs, misaligned):
    from xai_engine import kernels as K
    B, Cc, H, W, h, w = case
    gen = torch.Generator(device=DEV).manual_seed(47)
    n = B * Cc * H * W
    store = torch.randn(n + 1, device=DEV, generator=gen)
    grad = store[1:].view(B, Cc, H, W) if misaligned else store[:n].view(B, Cc, H, W)      # 4-byte aligned only: the scalar path
    cam = torch.randn(B, h, w, device=DEV, generator=gen).relu() if with_cam else None
    want_attr, want_map = _k28_want(grad, cam)
    guard = 64
    poison = float("nan")
    attr_buf = torch.full((n + guard,), poison, device=DEV)
    map_buf = torch.full((B * H * W + guard,), poison, device=DEV)
    wa, wm = outputs in ("attr", "both"), outputs in ("map", "both")
    out = K.guided_map(grad, cam, want_attr=wa, want_map=wm, attr=attr_buf[:n].view(B, Cc, H, W) if wa else None,
                       map=map_buf[:B * H * W].view(B, H, W) if wm else None)
    got_attr, got_map = out if outputs == "both" else ((out, None) if wa else (None, out))
    if wa:
        assert _bits_equal(got_attr, want_attr) and got_attr.data_ptr() == attr_buf.data_ptr()
    else:
        assert bool(attr_buf.isnan().all())
    if wm:
        assert _bits_equal(got_map, want_map)
    else:
        assert bool(map_buf.isnan().all())
    assert bool(attr_buf[n:].isnan().all()) and bool(map_buf[B * H * W:].isnan().all())       # nothing past the end
    if not misaligned and outputs == "both" and with_cam:                          # allocating form
        a2, m2 = K.guided_map(grad.contiguous(), cam, want_attr=True, want_map=True)
        assert _bits_equal(a2, want_attr) and _bits_equal(m2, want_map)


def test_k28_nearest_indices_are_the_restated_rule():
    from xai_engine import kernels as K
    for n_in, n_out in ((7, 224), (3, 80), (5, 37), (7, 100)):
        cam = torch.arange(n_in * n_in, dtype=torch.float32, device=DEV).view(1, n_in, n_in)
        got = K.guided_map(torch.ones(1, 1, n_out, n_out, device=DEV), cam)[0, 0].cpu().long()
        idx = torch.tensor(R.nearest_index(n_in, n_out))
        assert torch.equal(got, idx[:, None] * n_in + idx[None, :])


# ------------------------------------------------------------------------------------------------ the whole classifier
_CACHE = {}


def _model(full=False):
    """the unfused classifier with BatchNorm statistics that are not the initial (0, 1, 1, 0)"""
    key = ("model", full)
    if key not in _CACHE:
        from xai_engine.zoo import resnet50
        model = resnet50(seed=0) if full else resnet50(seed=0, num_classes=10, width=8)
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for mod in model.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                    mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                    mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                    mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
        model = model.to(DEV).eval()
        for prm in model.parameters():
            prm.requires_grad_(False)
        _CACHE[key] = model
    return _CACHE[key]


def _variant(kind, full=False):
    key = ("variant", kind, full)
    if key not in _CACHE:
        from xai_engine.prepare import fuse_bn_relu
        base = _model(full)
        _CACHE[key] = base if kind == "unfused" else fuse_bn_relu(base, fork_residual=kind == "forked")
    return _CACHE[key]


def _inputs(B, hw):
    x = torch.randn(B, 3, hw, hw, generator=torch.Generator().manual_seed(5 + hw)).to(DEV)
    t = torch.tensor([3, 7][:B]).to(DEV)
    return x, t


def _restated(B, hw, full=False):
    """computed once per shape, shared, never written to"""
    key = ("restated", B, hw, full)
    if key not in _CACHE:
        model = _model(full)
        x, t = _inputs(B, hw)
        gbp = R.guided_backprop(model, x, t)
        ggc = R.guided_gradcam(model, model.layer4, x, t)
        _CACHE[key] = (gbp, ggc)
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["fused", "forked", "unfused"])
@pytest.mark.parametrize("B,hw", [(2, 64), (1, 80)])
def test_guided_backprop_and_gradcam_equal_the_restated_captum_flow(kind, B, hw):
    from xai_engine.guided import guided_backprop_batch
    assert torch.backends.cudnn.deterministic
    model = _variant(kind)
    x, t = _inputs(B, hw)
    want_gbp, want_ggc = _restated(B, hw)
    assert float(want_ggc.abs().max()) > 0
    # the restatement is not the plain gradient by as much as its own magnitude: the test cannot pass with the feature missing
    xr = x.clone().requires_grad_(True)
    (plain,) = torch.autograd.grad(_model()(xr).gather(1, t.view(-1, 1)).sum(), xr)
    assert float((plain - want_gbp).abs().max()) > 0.1 * float(want_gbp.abs().max())
    for graphs in (False, True):
        tag = f"{kind}/B{B}x{hw}/{'replay' if graphs else 'eager'}"
        attr, m = guided_backprop_batch(x, model, t, want_attr=True, want_map=True, graphs=graphs)
        check(f"guided/gbp/{tag}", attr.cpu().numpy(), want_gbp.cpu().numpy(), BAR, against="restated")
        check(f"guided/gbp_map/{tag}", m[0].cpu().numpy(), R.harness_map(want_gbp[0]), BAR, against="restated")
        attr, m = guided_backprop_batch(x, model, t, layer=model.layer4, want_attr=True, want_map=True, graphs=graphs)
        check(f"guided/ggc/{tag}", attr.cpu().numpy(), want_ggc.cpu().numpy(), BAR, against="restated")
        check(f"guided/ggc_map/{tag}", m[0].cpu().numpy(), R.harness_map(want_ggc[0]), BAR, against="restated")


@pytest.mark.parametrize("kind", ["fused", "forked", "unfused"])
def test_the_layer_gradient_is_the_same_in_guided_and_in_plain_mode(kind):
    """what the single backward of Guided Grad-CAM rests on: behind layer4 there is no ReLU"""
    from xai_engine.guided import guided_gradients
    model = _variant(kind)
    x, t = _inputs(2, 64)
    gx_g, act_g, ga_g = guided_gradients(x, model, t.view(-1, 1), model.layer4, guided=True)
    gx_p, act_p, ga_p = guided_gradients(x, model, t.view(-1, 1), model.layer4, guided=False)
    assert torch.equal(act_g, act_p) and torch.equal(ga_g, ga_p)
    assert not torch.equal(gx_g, gx_p)
    ref_act, ref_ga = R.layer_act_and_grad(_model(), _model().layer4, x, t)
    assert torch.equal(act_g, ref_act) and torch.equal(ga_g, ref_ga)


@pytest.mark.parametrize("kind", ["fused", "forked", "unfused"])
def test_a_guided_pass_leaves_plain_gradients_as_they_were(kind):
    from xai_engine.guided import guided_backprop_batch
    from xai_engine import prepare
    model = _variant(kind)
    x, t = _inputs(2, 64)

    def plain():
        xr = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(model(xr).gather(1, t.view(-1, 1)).sum(), xr)
        return g
    before = plain()
    guided_backprop_batch(x, model, t, graphs=False)
    guided_backprop_batch(x, model, t, layer=model.layer4)
    assert not prepare.guided_active()
    assert not any(m._forward_hooks or m._backward_pre_hooks for m in model.modules())
    assert torch.equal(plain(), before)
    # a forward built inside the context keeps its guided backward when the backward runs outside it
    if kind != "unfused":
        xr = x.clone().requires_grad_(True)
        with prepare.guided_relu():
            score = model(xr).gather(1, t.view(-1, 1)).sum()
        (g,) = torch.autograd.grad(score, xr)
        assert torch.equal(g, guided_backprop_batch(x, model, t, graphs=False))


def test_graph_replay_is_bitwise_the_eager_pass_and_is_captured_once():
    from xai_engine import guided
    model = _variant("forked")
    x, t = _inputs(2, 64)
    x2 = x.flip(0).contiguous()
    guided._PASSES.entries().clear()
    before = dict(guided.GUIDED_COUNTS)
    for layer in (None, model.layer4):
        eager = [guided.guided_backprop_batch(v, model, t, layer=layer, want_attr=True, want_map=True, graphs=False) for v in (x, x2)]
        replay = [guided.guided_backprop_batch(v, model, t, layer=layer, want_attr=True, want_map=True, graphs=True) for v in (x, x2, x)]
        for e, r in zip(eager + eager[:1], replay):
            assert _bits_equal(e[0], r[0]) and _bits_equal(e[1], r[1])
    d = {k: guided.GUIDED_COUNTS[k] - before[k] for k in before}
    assert d == {"captures": 2, "captures_refused": 0, "replayed": 6, "eager": 4}, d
    assert len(guided._PASSES.entries()) == 2


@pytest.mark.parametrize("attr_func", ["gbp", "ggc"])
def test_harness_rows_return_the_restated_map(attr_func):
    from xai_engine.sweep import get_CNN_attr
    model = _variant("forked")
    x, t = _inputs(1, 80)
    want = R.harness_map(_restated(1, 80)[0 if attr_func == "gbp" else 1][0])
    td = {"models": [_variant("unfused"), model], "batch_size": 50, "img_hw": 80, "device": DEV, "attr_func": attr_func}
    host = get_CNN_attr(x.cpu(), None, t[0], td)
    assert isinstance(host, np.ndarray) and host.shape == (80, 80) and host.dtype == np.float32
    check(f"guided/harness/{attr_func}/numpy", host, want, BAR, against="restated")
    dev_map = get_CNN_attr(x, None, t[0], dict(td, device_maps=True))
    assert torch.is_tensor(dev_map) and dev_map.is_cuda and tuple(dev_map.shape) == (80, 80)
    check(f"guided/harness/{attr_func}/device", dev_map.cpu().numpy(), want, BAR, against="restated")
    only = get_CNN_attr(x, None, t[0], dict(td, models=[_variant("unfused")]))          # models[0] when there is no second model
    check(f"guided/harness/{attr_func}/models0", only, want, BAR, against="restated")


def test_captum_shaped_classes_and_the_torch_op_modes():
    from xai_engine import guided
    model = _variant("fused")
    x, t = _inputs(2, 64)
    want_gbp, want_ggc = _restated(2, 64)
    check("guided/class/gbp", guided.GuidedBackprop(model).attribute(x, target=t).cpu().numpy(), want_gbp.cpu().numpy(), BAR, against="restated")
    ggc = guided.GuidedGradCam(model, model.layer4)
    check("guided/class/ggc", ggc.attribute(x, t).cpu().numpy(), want_ggc.cpu().numpy(), BAR, against="restated")
    base = _model()
    want = want_gbp * F.interpolate(R.gradcam(base, base.layer4, x, t), x.shape[2:], mode="bilinear")
    got = ggc.attribute(x, t, interpolate_mode="bilinear")
    assert got.is_cuda
    check("guided/class/ggc_bilinear", got.cpu().numpy(), want.cpu().numpy(), BAR, against="restated")


def test_resnet50_at_224_guided_gradcam_equals_the_restated_flow():
    from xai_engine.guided import guided_backprop_batch
    model = _variant("forked", full=True)
    x, t = _inputs(2, 224)
    _, want = _restated(2, 224, full=True)
    attr, m = guided_backprop_batch(x, model, t, layer=model.layer4, want_attr=True, want_map=True)
    check("guided/ggc/resnet50_224/forked/replay", attr.cpu().numpy(), want.cpu().numpy(), BAR, against="restated")
    check("guided/ggc_map/resnet50_224/forked/replay", m[1].cpu().numpy(), R.harness_map(want[1]), BAR, against="restated")
