"""The gradient-pass forms of the classifier fusion (csrc/bnrelu_kernels.hip): BN(+add)+ReLU with a 1-bit gate mask in place
of y in the backward, and the stem max_pool(relu(bn(x))) as one kernel per direction.  Everything is bitwise: the mask pair
against the y-reading pair it replaces (K.bn_act_fwd / K.bn_relu_bwd), the stem and the whole classifier against the PyTorch
kernels.  Tensors that may hold NaN or signed zeros are compared through their bit patterns, or as "NaN at the same positions
and torch.equal everywhere else" where the other side is a PyTorch kernel whose NaN payload is its own business."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _equal_nan_aware(a, b):
    na, nb = a.isnan(), b.isnan()
    zero = torch.zeros((), device=a.device)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


def _bn_params(Cc, gen, identityish=False):
    if identityish:                         # bn(x) = fma(x * rsqrt(1 + 0), 1, 0) = x: y takes exactly the values put into x
        one, zero = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        return one, zero, zero.clone(), one.clone(), 0.0
    w = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    w[::3] *= -1                            # negative scales: the sign of a zero gradient is part of the bit pattern
    return (w, torch.randn(Cc, device=DEV, generator=gen), torch.randn(Cc, device=DEV, generator=gen),
            torch.rand(Cc, device=DEV, generator=gen) + 0.2, 1e-5)


def _expected_mask(y, n_bytes):
    """The documented layout: the gate of flat element e is bit (e % 256) / 4 of 64-bit word (e / 256) * 4 + e % 4; every other
    bit of the xai_bn_gate_mask_bytes(n) bytes is 0."""
    e = torch.arange(y.numel(), device=y.device)
    word, bit = (e // 256) * 4 + e % 4, (e % 256) // 4
    byte = word * 8 + bit // 8
    want = torch.zeros(n_bytes, dtype=torch.int32, device=y.device)
    want.index_add_(0, byte, ((y.flatten() > 0).int() << (bit % 8)).int())
    return want.to(torch.uint8)


SPECIAL = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-40, -1e-40, 1.0, -1.0]


@pytest.mark.parametrize("shape", [(2, 3, 7, 7),          # HW = 49: scalar path, n = 294 (not a multiple of 4, 64 or 256)
                                   (1, 5, 14, 14),        # HW = 196: vector path, n = 980 (245 lanes: a partial last wavefront and group)
                                   (3, 8, 56, 56),        # HW = 3136
                                   (50, 16, 7, 7)])       # scalar path over many groups, channels changing inside a lane's four elements
@pytest.mark.parametrize("add", ["none", "identity", "bn2"])
def test_gate_mask_pair_equals_the_pair_that_reads_y(shape, add):
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    gen = torch.Generator(device=DEV).manual_seed(11)
    Cc = shape[1]
    for special in (False, True):
        w, b, mean, var, eps = _bn_params(Cc, gen, identityish=special)
        x, idt, gy, gy2 = (torch.randn(shape, device=DEV, generator=gen) for _ in range(4))
        if special:                                       # y in {+0, -0 -> relu, NaN, +inf, denormal, ...} at scattered positions
            vals = torch.tensor(SPECIAL, device=DEV)
            pos = torch.randperm(x.numel(), device=DEV, generator=gen)[: x.numel() // 3]
            x.view(-1)[pos] = vals[torch.arange(pos.numel(), device=DEV) % len(SPECIAL)]
            idt.view(-1)[pos] = 0.0
        identity = None if add == "none" else idt
        bn2f = bn2b = None
        if add == "bn2":
            w2, b2, m2, v2, e2 = _bn_params(Cc, gen, identityish=special)
            bn2f, bn2b = (w2, b2, m2, v2, e2), (w2, v2, e2)
        need = K.bn_gate_mask_bytes(x.numel())
        assert need == -(-x.numel() // 256) * 32
        poisoned = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        y_ref = K.bn_act_fwd(x, identity, w, b, mean, var, eps, BN_VARIANT, relu=True, bn2=bn2f)
        y, mask = K.bn_relu_fwd_mask(x, identity, w, b, mean, var, eps, BN_VARIANT, bn2=bn2f, mask=poisoned)
        assert _bits_equal(y, y_ref)
        assert torch.equal(mask[:need], _expected_mask(y_ref, need))          # every word written, the tail's spare bits 0
        assert bool((mask[need:] == 0xFF).all())                              # and nothing past the mask touched
        for second in (None, gy2):
            gx_ref, gid_ref = K.bn_relu_bwd(gy, y_ref, w, var, eps, BN_VARIANT, want_identity=identity is not None, gy2=second, bn2=bn2b)
            gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, eps, BN_VARIANT, want_identity=identity is not None, gy2=second, bn2=bn2b)
            assert _bits_equal(gx, gx_ref)
            assert (gid is None and gid_ref is None) or _bits_equal(gid, gid_ref)
        if not special:                                   # finite data: torch.equal as well, the suite's usual form
            assert torch.equal(y, y_ref) and torch.equal(gx, gx_ref)


def _stem_inputs(shape, gen, planes):
    """x and BN parameters with chosen planes made constant (ties), all-negative after BN (every gate closed) or holding NaN."""
    N, Cc, H, W = shape
    w = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    b = torch.randn(Cc, device=DEV, generator=gen) * 0.1
    mean = torch.randn(Cc, device=DEV, generator=gen) * 0.1
    var = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    x = torch.randn(shape, device=DEV, generator=gen).round(decimals=1)        # ties on purpose
    if planes:
        x[:, 0] = 0.75                                                          # constant plane: every window is one big tie
        x[:, 1] = mean[1] - 4.0 - x[:, 1].abs()                                 # bn < 0 everywhere (w > 0, |b| small): all gates closed
        x[0, 2, H // 2, W // 3] = float("nan")
        x[-1, 2, 0, 0] = float("nan")
        x[-1, 2, H - 1, W - 1] = float("nan")
    return x, w, b, mean, var


@pytest.mark.parametrize("shape,geom", [((2, 4, 112, 112), (3, 2, 1)), ((3, 3, 20, 20), (2, 2, 0)), ((2, 3, 113, 111), (3, 2, 1)),
                                        ((2, 3, 113, 111), (2, 2, 0)), ((1, 3, 37, 53), (4, 2, 2)), ((2, 3, 9, 10), (2, 1, 1))])
@pytest.mark.parametrize("planes", [False, True])
def test_fused_stem_equals_the_pytorch_chain(shape, geom, planes):
    import torch.nn.functional as F
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    k, s, p = geom
    gen = torch.Generator(device=DEV).manual_seed(23)
    x, w, b, mean, var = _stem_inputs(shape, gen, planes)
    xr = x.clone().requires_grad_(True)
    y_ref = F.max_pool2d(F.relu(F.batch_norm(xr, mean, var, w, b, False, 0.0, 1e-5)), k, s, p)
    g1, g2 = torch.randn_like(y_ref), torch.randn_like(y_ref)
    (gx1_ref,) = torch.autograd.grad(y_ref, xr, g1, retain_graph=True)
    (gx2_ref,) = torch.autograd.grad([y_ref, y_ref], xr, [g1, g2])
    y, code = K.bn_relu_maxpool_fwd_code(x, w, b, mean, var, 1e-5, BN_VARIANT, k, s, p)
    assert code.dtype == torch.uint8 and code.shape == y.shape
    assert _equal_nan_aware(y, y_ref.detach())
    if planes:
        assert bool((code[:, 1] == 255).all()) and bool(y.isnan().any())
    gx1 = K.bn_relu_maxpool_bwd(g1, code, w, var, 1e-5, BN_VARIANT, shape[2], shape[3], k, s, p)
    gx2 = K.bn_relu_maxpool_bwd(g1, code, w, var, 1e-5, BN_VARIANT, shape[2], shape[3], k, s, p, gy2=g2)
    assert torch.equal(gx1, gx1_ref) and torch.equal(gx2, gx2_ref)


def test_stem_autograd_function_forks_and_falls_back():
    import torch.nn as nn
    from xai_engine.prepare import stem_autograd, max_pool, bn_relu
    gen = torch.Generator(device=DEV).manual_seed(31)
    bn = nn.BatchNorm2d(6).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(6, generator=gen, device=DEV) * 0.1)
        bn.running_var.copy_(torch.rand(6, generator=gen, device=DEV) + 0.5)
        bn.weight.copy_(torch.rand(6, generator=gen, device=DEV) + 0.5)
        bn.bias.copy_(torch.randn(6, generator=gen, device=DEV) * 0.1)
    for prm in bn.parameters():
        prm.requires_grad_(False)
    pool = nn.MaxPool2d(3, 2, 1)
    x = torch.randn(3, 6, 33, 41, device=DEV, generator=gen).round(decimals=1)
    xa, xb, xc = (x.clone().requires_grad_(True) for _ in range(3))
    ya = pool(torch.relu(bn(xa)))
    yb = stem_autograd(xb, bn, pool, fork=True)
    yc = stem_autograd(xc, bn, pool, fork=False)
    assert yb is not None and hasattr(yb, "_xai_alias") and yc is not None and not hasattr(yc, "_xai_alias")
    assert yb._xai_alias.data_ptr() == yb.data_ptr()
    g1, g2 = torch.randn_like(ya), torch.randn_like(ya)
    (ga2,) = torch.autograd.grad([ya, ya], xa, [g1, g2], retain_graph=True)
    (ga1,) = torch.autograd.grad(ya, xa, g1)
    (gb,) = torch.autograd.grad([yb, yb._xai_alias], xb, [g1, g2])
    (gc,) = torch.autograd.grad(yc, xc, g1)
    assert torch.equal(ya, yb) and torch.equal(ya, yc) and torch.equal(ga2, gb) and torch.equal(ga1, gc)
    # only one of the two handles used: the gradient of the other never arrives, the kernel gets one
    xd = x.clone().requires_grad_(True)
    yd = stem_autograd(xd, bn, pool, fork=True)
    (gd,) = torch.autograd.grad(yd._xai_alias, xd, g1)
    assert torch.equal(gd, ga1)
    # nothing to differentiate, or a geometry the kernels do not cover: None, and the caller's chain is PyTorch's pool
    assert stem_autograd(x, bn, pool) is None
    with torch.no_grad():
        assert stem_autograd(x.clone().requires_grad_(True), bn, pool) is None
    for other in (nn.MaxPool2d(3, 1, 1), nn.MaxPool2d(5, 2, 2), nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 1, dilation=2),
                  nn.MaxPool2d((3, 2), 2, 0)):
        xe, xf = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        assert stem_autograd(xe, bn, other) is None
        ye, yf = other(torch.relu(bn(xe))), max_pool(bn_relu(xf, bn), other)
        ge = torch.randn_like(ye)
        assert torch.equal(ye, yf) and torch.equal(torch.autograd.grad(ye, xe, ge)[0], torch.autograd.grad(yf, xf, ge)[0])


def test_forward_only_calls_write_no_mask_and_gradient_calls_save_it_instead_of_y():
    import torch.nn as nn
    from xai_engine.prepare import bn_relu
    bn = nn.BatchNorm2d(4).to(DEV).eval()
    for prm in bn.parameters():
        prm.requires_grad_(False)
    x = torch.randn(2, 4, 14, 14, device=DEV)
    assert bn_relu(x, bn).grad_fn is None
    with torch.no_grad():
        assert bn_relu(x.clone().requires_grad_(True), bn).grad_fn is None
    y = bn_relu(x.clone().requires_grad_(True), bn)
    saved = y.grad_fn.saved_tensors
    assert saved[0].dtype == torch.uint8 and saved[0].numel() == -(-x.numel() // 256) * 32
    assert all(t.numel() < x.numel() for t in saved)                          # the activation itself is not kept for the backward


def test_resnet50_at_224_is_bit_identical_and_its_backward_has_no_add_kernel():
    """fuse_bn_relu(fork_residual=True) on ResNet-50 at 224 x 224 under deterministic MIOpen solvers (conftest): logits and input
    gradients equal the unfused classifier's bit for bit, every call site verified on the way; the kernel trace of one backward
    holds the gate-mask and stem kernels and no element-wise add (every residual join and the stem's two gradients are summed
    inside the fused backward kernels) and no PyTorch max-pool."""
    from torch.profiler import profile, ProfilerActivity
    from xai_engine.prepare import fuse_bn_relu
    from xai_engine.zoo import resnet50
    assert torch.backends.cudnn.deterministic
    model = resnet50(seed=0).to(DEV)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(DEV)
    fused = fuse_bn_relu(model, verify=x, fork_residual=True)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    oa, ob = model(xa), fused(xb)
    (ga,) = torch.autograd.grad(oa[:, 3].sum(), xa)
    (gb,) = torch.autograd.grad(ob[:, 3].sum(), xb)
    assert torch.equal(oa, ob)
    assert torch.equal(ga, gb)
    with torch.no_grad():
        assert torch.equal(fused(x), oa.detach())                             # the inference stem and the mask-less forward
    xc = x.clone().requires_grad_(True)
    score = fused(xc)[:, 3].sum()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        (gc_,) = torch.autograd.grad(score, xc)
        torch.cuda.synchronize()
    assert torch.equal(gc_, ga)
    names = [e.key for e in prof.key_averages() if getattr(e, "self_device_time_total", getattr(e, "self_cuda_time_total", 0)) > 0]   # kernels
    joined = "\n".join(names)
    assert "bn_relu_bwd_mask_kernel" in joined and "bn_relu_maxpool_bwd_kernel" in joined, joined
    assert "CUDAFunctor_add" not in joined and "max_pool" not in joined and "bn_relu_bwd_kernel" not in joined, joined


def test_an_unsupported_stem_geometry_takes_the_earlier_path_through_the_whole_model():
    from xai_engine.prepare import fuse_bn_relu
    from xai_engine.zoo import resnet50
    model = resnet50(seed=0, width=16, num_classes=20).to(DEV)
    model.maxpool = torch.nn.MaxPool2d(3, 1, 1)                                # ceil(3 / 1) = 3 windows per axis over a position
    x = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(9)).to(DEV)
    fused = fuse_bn_relu(model, verify=x, fork_residual=True)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    oa, ob = model(xa), fused(xb)
    (ga,), (gb,) = torch.autograd.grad(oa[:, 3].sum(), xa), torch.autograd.grad(ob[:, 3].sum(), xb)
    assert torch.equal(oa, ob) and torch.equal(ga, gb)
