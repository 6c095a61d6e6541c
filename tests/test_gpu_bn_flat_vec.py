"""The flat 16-byte path of the fused BN/ReLU kernels (csrc/bnrelu_kernels.hip: n % 4 == 0, HW % 4 != 0) and the stem pair with
its 3/2/1 pool geometry at compile time.  Everything is bitwise.  On finite data the reference is the PyTorch chain
relu(batch_norm(x) [+ identity | + batch_norm(identity)]) and its autograd.grad with one and with two incoming gradients, which
DESIGN 5a states is bit-identical and which shares nothing with the code under test; with NaN, infinities, signed zeros and
denormals scattered in, the mask pair and the y-reading pair are compared with each other through their bit patterns."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPECIAL = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-40, -1e-40, 1.0, -1.0]      # tests/test_gpu_bn_gates.py's

# n = 588: a partial last group, lanes straddling channels;  n = 72: lanes straddling an image boundary, so c wraps to 0;
# HW = 1: four channels in one lane;  many groups
FLAT_SHAPES = [(4, 3, 7, 7), (4, 2, 3, 3), (2, 4, 1, 1), (50, 16, 7, 7)]
ADDS = ["none", "identity", "bn2"]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _equal_nan_aware(a, b):
    na, nb = a.isnan(), b.isnan()
    zero = torch.zeros((), device=a.device)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


def _clamp(g):
    return torch.where(g <= 0, torch.zeros((), device=g.device), g)


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


def _off_by_one_float(t):
    """the same values in a view that starts one float into a larger buffer: contiguous, 4-byte but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _pytorch_chain(x, idt, bn, bn2, add, grads, guided=False):
    """-> y, gx, g_identity (None without an identity operand) of the PyTorch kernels; `grads`: one or two incoming gradients"""
    w, b, mean, var, eps = bn
    xr = x.clone().requires_grad_(True)
    ir = idt.clone().requires_grad_(True)
    a = F.batch_norm(xr, mean, var, w, b, False, 0.0, eps)
    if add == "identity":
        a = a + ir
    elif add == "bn2":
        w2, b2, m2, v2, e2 = bn2
        a = a + F.batch_norm(ir, m2, v2, w2, b2, False, 0.0, e2)
    y = F.relu(a)
    if guided:
        y.register_hook(_clamp)                                                 # the complete gradient of the ReLU's output
    got = torch.autograd.grad([y] * len(grads), [xr] if add == "none" else [xr, ir], list(grads))
    return y.detach(), got[0], (None if add == "none" else got[1])


def _inputs(shape, add, gen, identityish=False):
    Cc = shape[1]
    bn = _bn_params(Cc, gen, identityish)
    x, idt, gy, gy2 = (torch.randn(shape, device=DEV, generator=gen) for _ in range(4))
    bn2 = _bn_params(Cc, gen, identityish) if add == "bn2" else None
    return bn, bn2, x, idt, gy, gy2


def _kernel_args(bn, bn2):
    w, b, mean, var, eps = bn
    bn2f = bn2
    bn2b = None if bn2 is None else (bn2[0], bn2[3], bn2[4])
    return w, b, mean, var, eps, bn2f, bn2b


def _check_both_pairs_against_the_chain(shape, add, tensors=None):
    """both kernel pairs (and the guided mask backward) on `shape` against the PyTorch chain; `tensors` may replace inputs by
    views of the same values (misaligned ones)"""
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    gen = torch.Generator(device=DEV).manual_seed(17)
    bn, bn2, x, idt, gy, gy2 = _inputs(shape, add, gen)
    w, b, mean, var, eps, bn2f, bn2b = _kernel_args(bn, bn2)
    kx, kidt, kgy, kgy2 = (tensors or (lambda *t: t))(x, idt, gy, gy2)
    identity = None if add == "none" else kidt
    want_id = add != "none"
    need = K.bn_gate_mask_bytes(x.numel())
    assert need == -(-x.numel() // 256) * 32
    poisoned = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    y, mask = K.bn_relu_fwd_mask(kx, identity, w, b, mean, var, eps, BN_VARIANT, bn2=bn2f, mask=poisoned)
    y2 = K.bn_act_fwd(kx, identity, w, b, mean, var, eps, BN_VARIANT, relu=True, bn2=bn2f)
    for second in (None, kgy2):
        grads = (gy,) if second is None else (gy, gy2)
        y_ref, gx_ref, gid_ref = _pytorch_chain(x, idt, bn, bn2, add, grads)
        assert x.numel() < 64 or 0.1 < float((y_ref > 0).float().mean()) < 0.9  # open and closed gates both
        assert _bits_equal(y, y_ref) and _bits_equal(y2, y_ref)
        assert torch.equal(mask[:need], _expected_mask(y_ref, need))            # every word written, the tail's spare bits 0
        assert bool((mask[need:] == 0xFF).all())                                # and nothing past the mask touched
        for gx, gid in (K.bn_relu_bwd_mask(kgy, mask, w, var, eps, BN_VARIANT, want_identity=want_id, gy2=second, bn2=bn2b),
                        K.bn_relu_bwd(kgy, y2, w, var, eps, BN_VARIANT, want_identity=want_id, gy2=second, bn2=bn2b)):
            assert _bits_equal(gx, gx_ref)
            assert (gid is None and gid_ref is None) or _bits_equal(gid, gid_ref)
        _, gx_ref, gid_ref = _pytorch_chain(x, idt, bn, bn2, add, grads, guided=True)
        gx, gid = K.bn_relu_bwd_mask(kgy, mask, w, var, eps, BN_VARIANT, want_identity=want_id, gy2=second, bn2=bn2b, guided=True)
        assert _bits_equal(gx, gx_ref)
        assert (gid is None and gid_ref is None) or _bits_equal(gid, gid_ref)


@pytest.mark.parametrize("shape", FLAT_SHAPES)
@pytest.mark.parametrize("add", ADDS)
def test_flat_path_equals_the_pytorch_chain(shape, add):
    assert shape[0] * shape[1] * shape[2] * shape[3] % 4 == 0 and (shape[2] * shape[3]) % 4 != 0
    _check_both_pairs_against_the_chain(shape, add)


@pytest.mark.parametrize("shape", FLAT_SHAPES)
@pytest.mark.parametrize("add", ADDS)
def test_flat_path_with_special_values_mask_pair_equals_the_pair_that_reads_y(shape, add):
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    gen = torch.Generator(device=DEV).manual_seed(19)
    bn, bn2, x, idt, gy, gy2 = _inputs(shape, add, gen, identityish=True)
    w, b, mean, var, eps, bn2f, bn2b = _kernel_args(bn, bn2)
    vals = torch.tensor(SPECIAL, device=DEV)
    pos = torch.randperm(x.numel(), device=DEV, generator=gen)[: max(x.numel() // 3, len(SPECIAL))]
    x.view(-1)[pos] = vals[torch.arange(pos.numel(), device=DEV) % len(SPECIAL)]   # y in {+0, -0 -> relu, NaN, +inf, denormal, ...}
    idt.view(-1)[pos] = 0.0
    pos_g = torch.randperm(x.numel(), device=DEV, generator=gen)[: max(x.numel() // 5, len(SPECIAL))]
    gy.view(-1)[pos_g] = vals[torch.arange(pos_g.numel(), device=DEV) % len(SPECIAL)]
    identity = None if add == "none" else idt
    want_id = add != "none"
    need = K.bn_gate_mask_bytes(x.numel())
    poisoned = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    y_ref = K.bn_act_fwd(x, identity, w, b, mean, var, eps, BN_VARIANT, relu=True, bn2=bn2f)
    y, mask = K.bn_relu_fwd_mask(x, identity, w, b, mean, var, eps, BN_VARIANT, bn2=bn2f, mask=poisoned)
    assert _bits_equal(y, y_ref)
    at = y_ref.view(-1)[pos]                              # bn(x) = x and identity = 0 there: fmaxf turns NaN into 0, the rest stays
    assert bool(at.isinf().any()) and bool((at == 1.0).any()) and not bool(at.isnan().any())
    assert bool(gy.isnan().any()) and bool((gy == 0).any())
    assert torch.equal(mask[:need], _expected_mask(y_ref, need)) and bool((mask[need:] == 0xFF).all())
    for second in (None, gy2):
        gx_ref, gid_ref = K.bn_relu_bwd(gy, y_ref, w, var, eps, BN_VARIANT, want_identity=want_id, gy2=second, bn2=bn2b)
        for guided in (False, True):
            g_in = gy if second is None else gy + gy2      # one fp32 add, as the kernel's
            if guided:                                     # the guided form is the plain one on the clamped sum
                gx_ref, gid_ref = K.bn_relu_bwd(_clamp(g_in), y_ref, w, var, eps, BN_VARIANT, want_identity=want_id, bn2=bn2b)
            gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, eps, BN_VARIANT, want_identity=want_id, gy2=second, bn2=bn2b, guided=guided)
            assert _bits_equal(gx, gx_ref)
            assert (gid is None and gid_ref is None) or _bits_equal(gid, gid_ref)


@pytest.mark.parametrize("add", ADDS)
def test_n_not_a_multiple_of_four_still_takes_the_scalar_path_and_is_right(add):
    _check_both_pairs_against_the_chain((2, 3, 7, 7), add)


@pytest.mark.parametrize("which", ["x", "identity", "gy", "gy2"])
def test_a_misaligned_input_takes_the_scalar_path_and_is_right(which):
    def swap(x, idt, gy, gy2):
        t = dict(x=x, identity=idt, gy=gy, gy2=gy2)
        t[which] = _off_by_one_float(t[which])
        return t["x"], t["identity"], t["gy"], t["gy2"]
    for add in ("identity", "bn2"):
        _check_both_pairs_against_the_chain((4, 3, 7, 7), add, tensors=swap)


@pytest.mark.parametrize("which", ["y", "mask_y", "bwd_y", "gx", "gid", "mask_gx", "mask_gid"])
def test_a_misaligned_output_or_saved_activation_takes_the_scalar_path_and_is_right(which):
    """the outputs are allocated by the Python wrappers, always aligned: here the C entries get views of the test's own"""
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    shape, add = (4, 3, 7, 7), "identity"
    gen = torch.Generator(device=DEV).manual_seed(17)
    bn, bn2, x, idt, gy, gy2 = _inputs(shape, add, gen)
    w, b, mean, var, eps = bn
    N, Cc, HW = shape[0], shape[1], shape[2] * shape[3]
    y_ref, gx_ref, gid_ref = _pytorch_chain(x, idt, bn, bn2, add, (gy, gy2))

    def out(name):
        t = torch.full(shape, float("nan"), device=DEV)
        return _off_by_one_float(t) if which == name else t
    p = K._ptr
    mask = torch.empty(K.bn_gate_mask_bytes(x.numel()), dtype=torch.uint8, device=DEV)
    y, ym = out("y"), out("mask_y")
    K._call("xai_bn_act_fwd_f32", x.device, p(x), p(idt), p(w), p(b), p(mean), p(var), eps, None, None, None, None, 0.0, BN_VARIANT, 1, N, Cc, HW, p(y))
    K._call("xai_bn_relu_fwd_mask_f32", x.device, p(x), p(idt), p(w), p(b), p(mean), p(var), eps, None, None, None, None, 0.0, BN_VARIANT, N, Cc, HW,
            p(ym), p(mask))
    assert _bits_equal(y, y_ref) and _bits_equal(ym, y_ref)
    assert torch.equal(mask, _expected_mask(y_ref, mask.numel()))
    saved = _off_by_one_float(y_ref) if which == "bwd_y" else y_ref
    gx, gid, gxm, gidm = out("gx"), out("gid"), out("mask_gx"), out("mask_gid")
    K._call("xai_bn_relu_bwd_f32", x.device, p(gy), p(gy2), p(saved), p(w), p(var), eps, None, None, 0.0, BN_VARIANT, N, Cc, HW, p(gx), p(gid))
    K._call("xai_bn_relu_bwd_mask_f32", x.device, p(gy), p(gy2), p(mask), p(w), p(var), eps, None, None, 0.0, BN_VARIANT, N, Cc, HW, p(gxm), p(gidm))
    assert _bits_equal(gx, gx_ref) and _bits_equal(gid, gid_ref) and _bits_equal(gxm, gx_ref) and _bits_equal(gidm, gid_ref)


# ---------------------------------------------------------------------------------------------------------------- the stem
def _stem_inputs(shape, gen, planes):
    """x and BN parameters; ties everywhere, and with `planes` a constant plane (every window one big tie), a plane that is
    negative after BN (every gate closed) and NaNs in the middle and at two corners, as far as the channels go"""
    N, Cc, H, W = shape
    w = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    b = torch.randn(Cc, device=DEV, generator=gen) * 0.1
    mean = torch.randn(Cc, device=DEV, generator=gen) * 0.1
    var = torch.rand(Cc, device=DEV, generator=gen) + 0.5
    x = torch.randn(shape, device=DEV, generator=gen).round(decimals=1)        # ties on purpose
    if planes:
        if Cc >= 3:
            x[:, 0] = 0.75
        if Cc >= 2:
            x[:, 1] = mean[1] - 4.0 - x[:, 1].abs()                             # bn < 0 everywhere (w > 0, |b| small)
        x[0, Cc - 1, H // 2, W // 3] = float("nan")
        x[-1, Cc - 1, 0, 0] = float("nan")
        x[-1, Cc - 1, H - 1, W - 1] = float("nan")
    return x, w, b, mean, var


def _check_stem(shape, geom, planes, misaligned_gx=False):
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    k, s, p = geom
    N, Cc, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(23)
    x, w, b, mean, var = _stem_inputs(shape, gen, planes)
    y, code = K.bn_relu_maxpool_fwd_code(x, w, b, mean, var, 1e-5, BN_VARIANT, k, s, p)
    assert code.dtype == torch.uint8 and code.shape == y.shape
    g1, g2 = torch.randn(y.shape, device=DEV, generator=gen), torch.randn(y.shape, device=DEV, generator=gen)
    # the forward-only stem shares the 3/2/1 kernel; its fmaxf turns a NaN into 0, everything else is the same number
    y_fwd = K.bn_relu_maxpool_fwd(x, w, b, mean, var, 1e-5, BN_VARIANT, k, s, p)
    assert torch.equal(y_fwd, torch.where(y.isnan(), y_fwd, y)) and not bool(y_fwd.isnan().any())
    for guided in (False, True):
        xr = x.clone().requires_grad_(True)
        act = F.relu(F.batch_norm(xr, mean, var, w, b, False, 0.0, 1e-5))
        if guided:
            act.register_hook(_clamp)
        y_ref = F.max_pool2d(act, k, s, p)
        (gx1_ref,) = torch.autograd.grad(y_ref, xr, g1, retain_graph=True)
        (gx2_ref,) = torch.autograd.grad([y_ref, y_ref], xr, [g1, g2])
        assert _equal_nan_aware(y, y_ref.detach())
        if planes and Cc >= 2:
            closed = code[:, 1] == 255
            assert bool(closed.all()) if Cc > 2 else bool(closed.any())         # the NaNs of a two-channel case sit in that plane
        if planes:
            assert bool(y.isnan().any())
        if misaligned_gx:
            for second, want in ((None, gx1_ref), (g2, gx2_ref)):
                gx = _off_by_one_float(torch.full(shape, float("nan"), device=DEV))
                K._call("xai_bn_relu_maxpool_bwd_guided_f32" if guided else "xai_bn_relu_maxpool_bwd_f32", x.device, K._ptr(g1), K._ptr(second),
                        K._ptr(code), K._ptr(w), K._ptr(var), 1e-5, BN_VARIANT, N, Cc, H, W, y.shape[2], y.shape[3], k, s, p, K._ptr(gx))
                assert torch.equal(gx, want)
        else:
            gx1 = K.bn_relu_maxpool_bwd(g1, code, w, var, 1e-5, BN_VARIANT, H, W, k, s, p, guided=guided)
            gx2 = K.bn_relu_maxpool_bwd(g1, code, w, var, 1e-5, BN_VARIANT, H, W, k, s, p, gy2=g2, guided=guided)
            assert torch.equal(gx1, gx1_ref) and torch.equal(gx2, gx2_ref)


# The 3/2/1 kernels tile 16 input rows (forward: 8 pooled rows; backward: 256 / TX row pairs, TX = 16 | 32 | 64 lanes of four
# columns for W <= 64 | <= 128 | wider, i.e. 32, 16 or 8 rows) and the forward stages W + 2 columns over 64 | 128 | 256 lanes.
# H and W one below, at and one above each of those, W % 4 != 0 among them, a second column trip (W > 256), planes smaller
# than one tile, two images so that the plane is image * C + channel.
STEM_321 = [(1, 1, 3, 3), (1, 2, 5, 6), (2, 3, 15, 62), (1, 3, 16, 63), (1, 3, 17, 64), (1, 3, 31, 65), (1, 3, 32, 64), (2, 3, 33, 61),
            (1, 3, 7, 126), (1, 3, 8, 127), (1, 3, 9, 128), (1, 3, 15, 129), (1, 3, 16, 132), (1, 3, 17, 124),
            (1, 3, 7, 254), (1, 3, 8, 255), (1, 3, 9, 256), (1, 3, 5, 257), (1, 3, 3, 260), (2, 3, 2, 4), (1, 3, 1, 1)]


@pytest.mark.parametrize("shape", STEM_321)
@pytest.mark.parametrize("planes", [False, True])
def test_the_3_2_1_stem_equals_the_pytorch_chain(shape, planes):
    _check_stem(shape, (3, 2, 1), planes)


@pytest.mark.parametrize("shape", [(1, 3, 17, 64), (2, 3, 16, 132), (1, 3, 9, 256)])
def test_the_3_2_1_stem_backward_into_a_misaligned_gx(shape):
    assert shape[3] % 4 == 0
    _check_stem(shape, (3, 2, 1), True, misaligned_gx=True)


@pytest.mark.parametrize("planes", [False, True])
def test_another_geometry_still_reaches_the_runtime_kernels_and_is_right(planes):
    _check_stem((1, 3, 37, 53), (4, 2, 2), planes)
    _check_stem((2, 3, 9, 10), (2, 1, 1), planes)
