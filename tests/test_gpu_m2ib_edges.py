"""K88, K89 and K90 (libxai_cm2ib.so) on the device against their NumPy restatements (tests/m2ib_restated.py), at their edges.

expf is the first operation of all three kernels, so what is held bit for bit is every kernel GIVEN the device's lam, read out of K88
itself (x9 = 1, eps = 0: t = lam * 1 + sd * 0 = lam exactly); lam is held to the header's 8 u behind expf, K90's capacity to the
header's bound behind logf, and K90's sums GIVEN the capacity it wrote bit for bit again.  Every case runs in well under a second."""
import ctypes as C

import numpy as np
import pytest
import torch

import m2ib_restated as M
from clip_restated import same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# the smallest shapes where the indexing can go wrong: L = 2 (one patch), 3, 65 (K90: more tokens than a workgroup's four waves,
# K88 / K89: L * D past one workgroup of 256 lanes); D = 1, 63, 64, 65 (K90's lane loop around a wave), 130 (three rounds of it)
SHAPES = [(L, D) for L in (2, 3, 65) for D in (1, 63, 64, 65, 130)]
BATCHES = [(1, 1), (3, 10), (1, 10), (3, 1)]                                   # (B, R)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def operands(B, R, L, D, half, seed=0, spread=1.0):
    g = np.random.default_rng(1000 * L + D + 7 * B + R + seed)
    dt = np.float16 if half else np.float32
    alpha = (5 + spread * g.standard_normal((B, L, D))).astype(np.float32)
    x9 = (2 * g.standard_normal((B, L, D))).astype(dt)
    eps = g.standard_normal((B, R, L, D)).astype(np.float32)
    gt = (1e-3 * g.standard_normal((B, R, L, D))).astype(dt)
    return alpha, x9, eps, gt, dt


def device_lam(alpha):
    """the device's lam = 1 / (1 + expf(-alpha)): K88_f32 with x9 = 1 and eps = 0"""
    from xai_engine import kernels as K
    a = dev(alpha)
    return K.m2ib_sample(a, torch.ones_like(a), torch.zeros((a.shape[0], 1) + tuple(a.shape[1:]), device=DEV))[:, 0].cpu().numpy()


def check_lam(alpha, lam):
    """the header's bound behind expf; where the restated lam is 0 the device's is, where it is 1 the device's is within the bound"""
    want = M.lam32(alpha)
    assert lam.dtype == np.float32 and (np.abs(lam.astype(np.float64) - want) <= M.lam_bound(want)).all()
    assert ((lam >= 0) & (lam <= 1)).all()


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("L,D", SHAPES)
def test_sample_and_adam_step_equal_the_restatement_given_lam(L, D, half):
    from xai_engine import kernels as K
    for B, R in BATCHES:
        alpha, x9, eps, gt, dt = operands(B, R, L, D, half)
        lam = device_lam(alpha)
        check_lam(alpha, lam)
        t = K.m2ib_sample(dev(alpha), dev(x9), dev(eps))
        assert t.dtype == (torch.float16 if half else torch.float32) and tuple(t.shape) == (B, R, L, D)
        assert same(t.cpu().numpy(), M.k88(alpha, x9, eps, dt, lam)), (B, R)
        # step k = 1 from zero moments (m / sqrt(v) is +-1), then k = 9 from moments that have a history
        g = np.random.default_rng(L + D)
        for k, m, v in ((1, np.zeros_like(alpha), np.zeros_like(alpha)),
                        (9, (1e-3 * g.standard_normal(alpha.shape)).astype(np.float32), (1e-6 * g.random(alpha.shape)).astype(np.float32))):
            a_d, m_d, v_d = dev(alpha), dev(m), dev(v)
            out = K.m2ib_adam_step(dev(gt), dev(eps), dev(x9), a_d, m_d, v_d, M.BETA, *M.adam_scalars(k))
            assert out is a_d
            a_w, m_w, v_w, g_w = M.k89(gt, eps, x9, alpha, m, v, M.BETA, M.adam_scalars(k), lam)
            for name, got, want in (("alpha", a_d, a_w), ("m", m_d, m_w), ("v", v_d, v_w)):
                assert same(got.cpu().numpy(), want), (B, R, k, name)
            if k == 1:                                                           # sign(g) * lr, up to adam_eps: |g| / (|g| + 1e-8)
                size = np.abs(g_w.astype(np.float64))
                assert np.abs(np.abs(a_w - alpha) - size / (size + 1e-8)).max() <= 1e-5 and ((a_w < alpha) == (g_w > 0)).all()


@pytest.mark.parametrize("L,D", SHAPES)
def test_saliency_equals_the_restatement_given_lam_and_the_capacity_it_wrote(L, D):
    from xai_engine import kernels as K
    for B in (1, 3):
        alpha, x9, _, _, _ = operands(B, 1, L, D, False, seed=3, spread=3.0)
        alpha = np.minimum(alpha, np.float32(14))                                # lam < 1: the +Inf capacity is test_edge_values'
        lam = device_lam(alpha)
        out, cap = K.m2ib_saliency(dev(alpha), dev(x9), want_capacity=True)
        assert tuple(out.shape) == (B, L - 1) and tuple(cap.shape) == (B, L, D)
        cap, want = cap.cpu().numpy(), M.k90_cap(alpha, x9, lam)
        assert np.isfinite(want).all() and (np.abs(cap.astype(np.float64) - want) <= M.cap_bound(alpha, x9, lam)).all()
        assert same(out.cpu().numpy(), M.k90_sum(cap))
        assert same(K.m2ib_saliency(dev(alpha), dev(x9)).cpu().numpy(), out.cpu().numpy())          # without cap_out: the same bytes


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_edge_values(half):
    """alpha at 5 (the start); at +20, where lam rounds to 1 and the NaN rule holds; at -20 and -100, where lam is near 0 and 0; a NaN and
    an Inf in x9; a token whose every term is a NaN; dL/dt all zero (pure compression); fp16 x9 at +-65504"""
    from xai_engine import kernels as K
    B, R, L, D = 1, 10, 3, 65
    alpha, x9, eps, gt, dt = operands(B, R, L, D, half, seed=5)
    alpha[:] = 5
    alpha[0, 1, 0], alpha[0, 1, 1], alpha[0, 1, 2], alpha[0, 1, 3] = 20, -20, -100, 17
    x9[0, 1, 10], x9[0, 1, 11], x9[0, 1, 12] = np.nan, np.inf, -np.inf
    x9[0, 2, :] = np.nan                                                         # token 2: every term a NaN
    if half:
        x9[0, 1, 20], x9[0, 1, 21] = 65504, -65504
    lam = device_lam(alpha)
    check_lam(alpha, lam)
    assert lam[0, 1, 0] == 1 and lam[0, 1, 3] == 1 and 0 < lam[0, 1, 1] < 1e-8 and lam[0, 1, 2] == 0
    t = K.m2ib_sample(dev(alpha), dev(x9), dev(eps)).cpu().numpy()
    assert same(t, M.k88(alpha, x9, eps, dt, lam))
    if half:
        assert not np.isnan(t[0, :, 1, 20:22]).any() and (np.abs(t[0, :, 1, 20:22].astype(np.float32)) > 60000).all()
    for zero in (False, True):
        g = np.zeros_like(gt) if zero else gt
        a_d, m_d, v_d = dev(alpha), dev(np.zeros_like(alpha)), dev(np.zeros_like(alpha))
        K.m2ib_adam_step(dev(g), dev(eps), dev(x9), a_d, m_d, v_d, M.BETA, *M.adam_scalars(1))
        a_w, m_w, v_w, g_w = M.k89(g, eps, x9, alpha, np.zeros_like(alpha), np.zeros_like(alpha), M.BETA, M.adam_scalars(1), lam)
        for got, want in ((a_d, a_w), (m_d, m_w), (v_d, v_w)):
            got = got.cpu().numpy()
            assert same(got, want)
            assert np.isnan(got[0, 1, 0]) and np.isnan(got[0, 1, 3])             # THE NaN RULE: 0 * Inf where lam rounds to 1
            assert np.isfinite(got[0, 1, 1]) and np.isfinite(got[0, 1, 2]) and np.isfinite(got[0, 0]).all()
        if zero:                                                                 # pure compression: every finite x9 pulls alpha down
            assert (g_w[0, 0] > 0).all() and (a_d.cpu().numpy()[0, 0] < 5).all()
    x32 = x9.astype(np.float32)
    out, cap = K.m2ib_saliency(dev(alpha), dev(x32), want_capacity=True)
    out, cap = out.cpu().numpy(), cap.cpu().numpy()
    want = M.k90_cap(alpha, x32, lam)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(cap), np.isnan(want)) and np.array_equal(np.isposinf(cap), np.isposinf(want))
    assert (np.abs(cap[fin].astype(np.float64) - want[fin]) <= M.cap_bound(alpha, x32, lam)[fin]).all()
    assert np.isnan(cap[0, 1, 10]) and np.isposinf(cap[0, 1, 0]) and np.isnan(cap[0, 2]).all()
    assert same(out, M.k90_sum(cap)) and out[0, 1] == 0 and np.isposinf(out[0, 0])                    # an all-NaN token gives +0
    alpha[0, 1, 0] = alpha[0, 1, 3] = 5                                         # without the +Inf terms the NaN ones are skipped
    x32[0, 1, 11] = x32[0, 1, 12] = 1
    out = K.m2ib_saliency(dev(alpha), dev(x32)).cpu().numpy()
    assert np.isfinite(out).all() and out[0, 0] > 0


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_two_steps_in_place_equal_the_restatement_run_twice(half):
    from xai_engine import kernels as K
    B, R, L, D = 3, 10, 3, 65
    alpha, x9, eps, gt, _ = operands(B, R, L, D, half, seed=9)
    a_d, m_d, v_d = dev(alpha), dev(np.zeros_like(alpha)), dev(np.zeros_like(alpha))
    a_w, m_w, v_w = alpha, np.zeros_like(alpha), np.zeros_like(alpha)
    for k in (1, 2):
        lam = device_lam(a_w)
        K.m2ib_adam_step(dev(gt), dev(eps), dev(x9), a_d, m_d, v_d, M.BETA, *M.adam_scalars(k))
        a_w, m_w, v_w, _ = M.k89(gt, eps, x9, a_w, m_w, v_w, M.BETA, M.adam_scalars(k), lam)
        assert same(a_d.cpu().numpy(), a_w) and same(m_d.cpu().numpy(), m_w) and same(v_d.cpu().numpy(), v_w), k
    assert (a_w != alpha).all() and (m_w != 0).all() and (v_w > 0).all()


def test_argument_errors_return_codes_and_launch_nothing():
    from xai_engine import _lib
    lib = _lib.load("cm2ib")
    buf = torch.full((64,), 7.0, device=DEV)
    p, stream = buf.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream
    s = (C.c_float(0.1),) * 7
    assert lib.xai_cm2ib_sample_f32(None, p, p, 1, 1, 2, 2, p, stream) == -1
    assert lib.xai_cm2ib_sample_f16(p, p, p, 1, 0, 2, 2, p, stream) == -2
    assert lib.xai_cm2ib_sample_f32(p, p, p, 1, 1, 4097, 2, p, stream) == -3
    assert lib.xai_cm2ib_adam_step_f32(p, p, p, 1, 1, 2, 2, *s, p, p, None, stream) == -1
    assert lib.xai_cm2ib_adam_step_f16(p, p, p, 1, 1, 2, 0, *s, p, p, p, stream) == -2
    assert lib.xai_cm2ib_adam_step_f32(p, p, p, 1, 1025, 2, 2, *s, p, p, p, stream) == -3
    assert lib.xai_cm2ib_saliency_f32(p, None, 1, 2, 2, None, p, stream) == -1
    assert lib.xai_cm2ib_saliency_f32(p, p, 1, 1, 2, None, p, stream) == -2
    assert lib.xai_cm2ib_saliency_f32(p, p, 1, 2, 8193, None, p, stream) == -3
    torch.cuda.synchronize()
    assert (buf == 7).all()
