"""Host side of the gradient-pass fusion entry points (gate-mask pair, one-kernel stem): sizes, and argument validation that
returns before any HIP call -- checkable without a GPU, with made-up non-null addresses that are never dereferenced."""
import os
import subprocess

from conftest import PKG


def _lib():
    from xai_engine import _lib, LIB_PATH
    if not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    return _lib.load()


def test_gate_mask_bytes():
    lib = _lib()
    assert lib.xai_bn_gate_mask_bytes(0) == 0 and lib.xai_bn_gate_mask_bytes(-5) == 0
    assert [lib.xai_bn_gate_mask_bytes(n) for n in (1, 255, 256, 257, 294, 980)] == [32, 32, 32, 64, 64, 128]
    n = 50 * 64 * 112 * 112                                   # one bit per element, 1/32 of the fp32 activation
    assert lib.xai_bn_gate_mask_bytes(n) == n // 8 == n * 4 // 32
    assert lib.xai_bn_gate_mask_bytes(3 * 2**32) == 3 * 2**29                  # 64-bit element counts


def test_gate_mask_pair_rejects_bad_arguments_before_any_hip_call():
    lib = _lib()
    p = 4096                                                  # non-null, 16-byte aligned, never dereferenced: every call below is refused
    fwd, bwd = lib.xai_bn_relu_fwd_mask_f32, lib.xai_bn_relu_bwd_mask_f32
    assert fwd(None, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 9, 1, 2, 4, p, p, None) == -1         # x
    assert fwd(p, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 9, 1, 2, 4, None, p, None) == -1         # y
    assert fwd(p, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 9, 1, 2, 4, p, None, None) == -1         # mask
    assert fwd(p, None, p, p, p, p, 1e-5, p, p, p, p, 1e-5, 9, 1, 2, 4, p, p, None) == -1                       # bn2 needs identity
    assert fwd(p, p, p, p, p, p, 1e-5, p, None, p, p, 1e-5, 9, 1, 2, 4, p, p, None) == -1                       # bn2 is a set
    assert fwd(p, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 16, 1, 2, 4, p, p, None) == -2           # variant
    assert fwd(p, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 9, 0, 2, 4, p, p, None) == -2            # N
    assert fwd(p, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 9, 1, 2, -4, p, p, None) == -2           # HW
    assert fwd(p, None, p, p, p, p, 1e-5, None, None, None, None, 0.0, 9, 1, 2, 4, p, p + 4, None) == -2        # mask not 8-byte aligned
    assert bwd(None, None, p, p, p, 1e-5, None, None, 0.0, 9, 1, 2, 4, p, None, None) == -1                     # gy
    assert bwd(p, None, None, p, p, 1e-5, None, None, 0.0, 9, 1, 2, 4, p, None, None) == -1                     # mask
    assert bwd(p, None, p, p, p, 1e-5, None, None, 0.0, 9, 1, 2, 4, None, None, None) == -1                     # gx
    assert bwd(p, None, p, p, p, 1e-5, p, p, 1e-5, 9, 1, 2, 4, p, None, None) == -1                             # bn2 needs g_identity
    assert bwd(p, None, p, p, p, 1e-5, None, None, 0.0, -1, 1, 2, 4, p, None, None) == -2                       # variant
    assert bwd(p, None, p, p, p, 1e-5, None, None, 0.0, 9, 1, 0, 4, p, None, None) == -2                        # C
    assert bwd(p, None, p + 2, p, p, 1e-5, None, None, 0.0, 9, 1, 2, 4, p, None, None) == -2                    # mask alignment


def test_stem_pair_rejects_bad_arguments_before_any_hip_call():
    lib = _lib()
    p = 4096
    fwd, bwd = lib.xai_bn_relu_maxpool_fwd_code_f32, lib.xai_bn_relu_maxpool_bwd_f32

    def f(N=1, C=1, H=8, W=8, PH=4, PW=4, k=3, s=2, pad=1, variant=9, x=p, y=p, code=p):
        return fwd(x, p, p, p, p, 1e-5, variant, N, C, H, W, PH, PW, k, s, pad, y, code, None)

    def g(N=1, C=1, H=8, W=8, PH=4, PW=4, k=3, s=2, pad=1, variant=9, gy=p, code=p, gx=p, var=p):
        return bwd(gy, None, code, p, var, 1e-5, variant, N, C, H, W, PH, PW, k, s, pad, gx, None)

    for fn in (f, g):
        assert fn(k=0) == -2 and fn(s=0) == -2 and fn(pad=-1) == -2 and fn(N=0) == -2 and fn(variant=16) == -2
        assert fn(PH=5) == -2 and fn(PW=3) == -2                          # not the pooled extents of H, W: the kernels index by them
        assert fn(pad=2) == -2                                            # 2 * pad > kernel: a window of padding only
        assert fn(H=1, W=1, PH=1, PW=1, k=3, pad=0) == -2                 # kernel larger than the padded input
        assert fn(N=70000) == -3                                          # planes ride on grid.y
        assert fn(k=3, s=1, PH=8, PW=8) == -3                             # ceil(kernel / stride) = 3 windows over one position
        assert fn(k=16, s=8, pad=8, H=32, W=32, PH=5, PW=5) == -3         # window positions must fit a byte next to "closed"
    assert f(x=None) == -1 and f(y=None) == -1 and f(code=None) == -1
    assert g(gy=None) == -1 and g(code=None) == -1 and g(gx=None) == -1 and g(var=None) == -1
    assert f(H=8, W=4000, PH=4, PW=2000) == -3                            # forward tile beyond 48 KiB of LDS
    assert g(H=8, W=4000, PH=4, PW=2000) == -3                            # backward tile beyond 48 KiB of LDS


def test_prepare_leaves_cpu_tensors_to_pytorch():
    """Off the GPU nothing is fused: the autograd stem declines like the inference stem does."""
    import torch
    from xai_engine.prepare import stem_autograd
    bn, pool = torch.nn.BatchNorm2d(3).eval(), torch.nn.MaxPool2d(3, 2, 1)
    for prm in bn.parameters():
        prm.requires_grad_(False)
    assert stem_autograd(torch.randn(1, 3, 8, 8, requires_grad=True), bn, pool) is None
