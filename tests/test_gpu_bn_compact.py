"""K62-K64 (include/xai_hip_compact.h) on the MI355X against the kernels they restate: the gather against torch's strided slice,
the CNHW-identity forward and the CNHW / compact / broadcast backward against xai_bn_relu_fwd_mask_f32 / xai_bn_relu_bwd_mask_f32
fed the same operands in the layout those take -- dense, permuted, zero-filled or expanded.  Everything is compared bit for bit.
Shapes: N in {1, 2, 3}, C in {3, 8}, H = W in {5, 6, 8, 14}: odd and even H, HW with and without % 4 == 0, n % 4 != 0, so the
vector path (HW % 4 == 0), the flat 16-byte path (n % 4 == 0 only) and the scalar path all run; plus one operand set moved off
16-byte alignment by an offset view."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 9                    # prepare.BN_VARIANT
SHAPES = [(N, C, H) for N in (1, 2, 3) for C in (3, 8) for H in (5, 6, 8, 14)]


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


def rand(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def off16(t):
    """the same values in storage that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def bn(C, seed):
    return rand(C, seed=seed), rand(C, seed=seed + 1), rand(C, seed=seed + 2), rand(C, seed=seed + 3).abs() + 0.5


def to_cnhw(t):
    return t.permute(1, 0, 2, 3).contiguous()


def paths_of(shapes):
    """which element path a dense launch of each shape takes: 'vec', 'flat' or 'scalar'"""
    return {"vec" if (H * H) % 4 == 0 else "flat" if (N * C * H * H) % 4 == 0 else "scalar" for N, C, H in shapes}


def test_the_shapes_reach_all_three_element_paths():
    assert paths_of(SHAPES) == {"vec", "flat", "scalar"}
    assert any(H % 2 for _, _, H in SHAPES) and any(N * C * H * H > 1024 for N, C, H in SHAPES)       # odd H; more than one block


@pytest.mark.parametrize("N,C,H", SHAPES)
@pytest.mark.parametrize("stride", [2, 3])
def test_k62_gather_is_the_strided_slice_channel_major(K, N, C, H, stride):
    side = rand(N, C, H, H, seed=N + C + H)
    want = side[:, :, ::stride, ::stride].permute(1, 0, 2, 3).contiguous()
    assert bits(K.stride_gather_cnhw(side, stride), want)
    assert bits(K.stride_gather_cnhw(off16(side), stride), want)


@pytest.mark.parametrize("N,C,H", SHAPES)
@pytest.mark.parametrize("with_bn2", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_k63_forward_with_a_cnhw_identity_is_the_nchw_forward(K, N, C, H, with_bn2, misaligned):
    x, idt = rand(N, C, H, H, seed=1), rand(N, C, H, H, seed=2)
    w, b, mean, var = bn(C, 10)
    bn2 = (*bn(C, 20), 1e-3) if with_bn2 else None
    y, mask = K.bn_relu_fwd_mask(x, idt, w, b, mean, var, 1e-5, V, bn2=bn2)
    xin, cin = (off16(x), off16(to_cnhw(idt))) if misaligned else (x, to_cnhw(idt))
    yc, maskc = K.bn_relu_fwd_cnhw(xin, cin, w, b, mean, var, 1e-5, V, bn2=bn2)
    assert bits(y, yc) and torch.equal(mask, maskc)
    y0, none = K.bn_relu_fwd_cnhw(xin, cin.view(1, C, N * H, H), w, b, mean, var, 1e-5, V, bn2=bn2, gated=False)
    assert none is None and bits(y0, y)
    assert (y > 0).any() and (y == 0).any()


def gated(K, N, C, H, seed=3):
    w, b, mean, var = bn(C, 30)
    _, mask = K.bn_relu_fwd_mask(rand(N, C, H, H, seed=seed), None, w, b, mean, var, 1e-5, V)
    return mask, w, var


@pytest.mark.parametrize("N,C,H", SHAPES)
@pytest.mark.parametrize("with_bn2", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_k64_g_identity_in_cnhw_order_is_todays_permuted(K, N, C, H, with_bn2, guided):
    mask, w, var = gated(K, N, C, H)
    gy, gy2 = rand(N, C, H, H, seed=4), rand(N, C, H, H, seed=5)
    bn2 = (rand(C, seed=6), rand(C, seed=7).abs() + 0.5, 1e-3) if with_bn2 else None
    gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, want_identity=True, gy2=gy2, bn2=bn2, guided=guided)
    gxc, gidc = K.bn_relu_bwd_compact(gy, mask, w, var, 1e-5, V, gy2=gy2, bn2=bn2, guided=guided, identity_cnhw=True)
    assert gidc.shape == (1, C, N * H, H) and bits(gx, gxc) and bits(to_cnhw(gid), gidc.view(C, N, H, H))
    gxm, gidm = K.bn_relu_bwd_compact(off16(gy), mask, w, var, 1e-5, V, gy2=gy2, bn2=bn2, guided=guided, identity_cnhw=True)
    assert bits(gx, gxm) and bits(gidc, gidm)
    # and with nothing special asked it is the plain entry
    gxp, gidp = K.bn_relu_bwd_compact(gy, mask, w, var, 1e-5, V, want_identity=True, gy2=gy2, bn2=bn2, guided=guided)
    assert bits(gx, gxp) and bits(gid, gidp)


@pytest.mark.parametrize("N,C,H", SHAPES)
@pytest.mark.parametrize("stride", [2, 3])
@pytest.mark.parametrize("want_identity", [False, True])
def test_k64_compact_gy2_is_the_dense_zero_filled_gy2(K, N, C, H, stride, want_identity):
    mask, w, var = gated(K, N, C, H)
    mask.fill_(0xFF)                                     # every gate open: g_identity is g itself, the sign of a zero included
    gy = rand(N, C, H, H, seed=8)
    gy.view(-1)[::3] = -0.0                              # negative zeros, at positions the compact tensor covers and at others
    Ho = (H - 1) // stride + 1
    compact = rand(C, N, Ho, Ho, seed=9)
    compact.view(-1)[::5] = -0.0
    dense = torch.zeros_like(gy)                         # +0 everywhere, as MIOpen's zero-fill leaves it
    dense[:, :, ::stride, ::stride] = compact.permute(1, 0, 2, 3)
    covered = torch.zeros_like(gy, dtype=torch.bool)
    covered[:, :, ::stride, ::stride] = True
    neg_zero = (gy == 0) & torch.signbit(gy)
    assert (neg_zero & ~covered).any() and (neg_zero & covered).any()
    gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, want_identity=want_identity, gy2=dense)
    gxc, gidc = K.bn_relu_bwd_compact(gy, mask, w, var, 1e-5, V, want_identity=want_identity, gy2_compact=compact, stride=stride)
    assert bits(gx, gxc) and (gid is None) == (gidc is None) and (gid is None or bits(gid, gidc))
    if want_identity:                                    # -0 + (+0) = +0 where nothing is covered: the add is not skipped
        assert not torch.signbit(gidc[neg_zero & ~covered]).any()
    gxm, _ = K.bn_relu_bwd_compact(off16(gy), mask, w, var, 1e-5, V, want_identity=want_identity, gy2_compact=off16(compact), stride=stride)
    assert bits(gx, gxm)


@pytest.mark.parametrize("N,C,H", SHAPES)
@pytest.mark.parametrize("with_gy2", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_k64_broadcast_gy_is_the_expanded_tensor(K, N, C, H, with_gy2, guided):
    mask, w, var = gated(K, N, C, H)
    classes = 5
    fc = rand(classes, C, seed=11)
    targets = torch.tensor([3, 3, 0][:N], dtype=torch.int64, device=DEV)             # repeated targets
    grad_out = torch.tensor([0.75, -1.5, 3.0][:N], dtype=torch.float32, device=DEV)  # not ones
    gy2 = rand(N, C, H, H, seed=12) if with_gy2 else None
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H * H), dtype=torch.float32)
    rows = grad_out[:, None] * fc[targets]                                            # one rounding
    for divisor, per_nc in ((0.0, rows * scale.to(DEV)), (float(H * H), rows / torch.full_like(rows, float(H * H)))):     # tensor / tensor: a true division
        gy = per_nc[:, :, None, None].expand(N, C, H, H).contiguous()
        gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, want_identity=True, gy2=gy2, guided=guided)
        gxb, gidb = K.bn_relu_bwd_bcast(grad_out, fc, targets, (N, C, H, H), mask, w, var, 1e-5, V, want_identity=True, gy2=gy2,
                                        guided=guided, divisor=divisor)
        assert bits(gx, gxb) and bits(gid, gidb)
    assert (gid != 0).any()


@pytest.mark.parametrize("N,C,H", SHAPES)
@pytest.mark.parametrize("with_bn2", [False, True])
def test_k64_compact_gy2_and_cnhw_g_identity_in_one_launch(K, N, C, H, with_bn2):
    """a strided block right behind another: the site takes a compact gy2 AND writes a channel-major g_identity"""
    mask, w, var = gated(K, N, C, H)
    gy = rand(N, C, H, H, seed=13)
    Ho = (H + 1) // 2
    compact = rand(C, N, Ho, Ho, seed=14)
    dense = torch.zeros_like(gy)
    dense[:, :, ::2, ::2] = compact.permute(1, 0, 2, 3)
    bn2 = (rand(C, seed=6), rand(C, seed=7).abs() + 0.5, 1e-3) if with_bn2 else None
    gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, want_identity=True, gy2=dense, bn2=bn2)
    gxc, gidc = K.bn_relu_bwd_compact(gy, mask, w, var, 1e-5, V, gy2_compact=compact, stride=2, bn2=bn2, identity_cnhw=True)
    assert bits(gx, gxc) and bits(to_cnhw(gid), gidc.view(C, N, H, H))


@pytest.mark.parametrize("N,C,H", SHAPES)
def test_k64_broadcast_gy_with_the_identity_operands_own_batchnorm(K, N, C, H):
    mask, w, var = gated(K, N, C, H)
    fc = rand(4, C, seed=15)
    targets = torch.tensor([2, 2, 1][:N], dtype=torch.int64, device=DEV)             # (N = 1 has one target: nothing to repeat)
    grad_out = torch.tensor([-0.5, 2.25, 1.5][:N], dtype=torch.float32, device=DEV)
    bn2 = (rand(C, seed=16), rand(C, seed=17).abs() + 0.5, 1e-3)
    scale = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H * H), dtype=torch.float32)).to(DEV)
    gy = ((grad_out[:, None] * fc[targets]) * scale)[:, :, None, None].expand(N, C, H, H).contiguous()
    gx, gid = K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, bn2=bn2)
    gxb, gidb = K.bn_relu_bwd_bcast(grad_out, fc, targets, (N, C, H, H), mask, w, var, 1e-5, V, bn2=bn2)
    assert gid is not None and bits(gx, gxb) and bits(gid, gidb) and not bits(gid, gx)


def test_the_wrappers_refuse_what_the_kernels_cannot_take(K):
    mask, w, var = gated(K, 2, 3, 6)
    gy = rand(2, 3, 6, 6)
    with pytest.raises(ValueError, match="gy2_compact must hold"):
        K.bn_relu_bwd_compact(gy, mask, w, var, 1e-5, V, gy2_compact=rand(3, 2, 3, 2))
    with pytest.raises(ValueError, match="gy2_compact must hold"):
        K.bn_relu_bwd_compact(gy, mask, w, var, 1e-5, V, gy2=gy, gy2_compact=rand(3, 2, 3, 3))
    with pytest.raises(ValueError, match="element count"):
        K.bn_relu_fwd_cnhw(gy, rand(3, 2, 6, 5), w, w, w, var, 1e-5, V)
    with pytest.raises(ValueError, match="fc_weight"):
        K.bn_relu_bwd_bcast(rand(2), rand(5, 4), torch.zeros(2, dtype=torch.int64, device=DEV), (2, 3, 6, 6), mask, w, var, 1e-5, V)
