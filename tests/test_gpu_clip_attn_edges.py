"""K82-K85 (csrc/clip/clip_attn_kernels.hip) at their edges, both dtypes, bit for bit against the NumPy restatements of
tests/clip_attn_restated.py (a NaN by position): include/xai_cattn.h states every accumulation order and every rounding point, and the
kernels call no transcendental function, so there is no bound to derive.

Every launch here goes through the C entry with the caller's buffers: each output lies between guard elements that must stay
untouched, and a second run must give the same bytes.  Shapes: the smallest that reach each path of the kernels -- fewer columns than
waves, one wave of lanes and one past it (63, 64, 65), more than one round of the 16 waves (129, 197), one round of the 1024 lanes and
one past it (1024, 1025, with d small), head widths below, at and past a wave (1, 16, 64, 65), L * L a multiple of the 16-byte
vector and not."""
import numpy as np
import pytest
import torch

import clip_attn_restated as A
from clip_restated import same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 8
SENTINEL = 12288.0          # a value both dtypes hold exactly
DTYPES = [(np.float32, torch.float32, "f32"), (np.float16, torch.float16, "f16")]
DT_IDS = ["float32", "float16"]


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


def values(seed, shape, tdt, scale=1.0):
    """seeded randn cast to the dtype -> (fp32 NumPy values of that dtype, the same on the device)"""
    t = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(tdt)
    return t.float().numpy(), t.to(DEV)


def to_dev(a, tdt, off=0):
    """host fp32 values of the dtype -> a device tensor of it whose first element lies `off` elements past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
    buf = torch.empty(t.numel() + 16, dtype=tdt, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def guarded(shape, tdt, off=0):
    """-> (the whole buffer, the view of `shape` inside it, GUARD + off elements from its start), everything the sentinel"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, dtype=tdt, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n].view(shape)


def guards_intact(buf, view):
    n, start = view.numel(), (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    host = buf.float().cpu().numpy()
    return (host[:start] == SENTINEL).all() and (host[start + n:] == SENTINEL).all() and len(host[:start]) >= GUARD and len(host[start + n:]) >= GUARD


def strided_v(v, tdt):
    """v (L, B, D) as the V half of an (L, B, 2 D) in-projection buffer: ld_l = 2 B D > B D, ld_b = 2 D"""
    L, B, D = v.shape
    kv = torch.zeros((L, B, 2 * D), dtype=tdt, device=DEV)
    kv[:, :, D:] = torch.from_numpy(v).to(tdt).to(DEV)
    return kv[:, :, D:]


def game(K, sfx, g, v, a0, out):
    B, T, D = g.shape
    _, H, L = a0.shape
    K._call(f"xai_cattn_game_map_{sfx}", g.device, g.data_ptr(), v.data_ptr(), v.stride(0), v.stride(1), a0.data_ptr(), B, L, D, H, T,
            out.data_ptr(), lib="cattn")


def rollout(K, sfx, a0, T, out):
    B, H, L = a0.shape
    K._call(f"xai_cattn_rollout_row_{sfx}", a0.device, a0.data_ptr(), B, H, L, T, out.data_ptr(), lib="cattn")


def matrices(K, sfx, attn, grad, c):
    n, B, H, L, _ = attn.shape
    K._call(f"xai_cattn_lrp_matrices_{sfx}", attn.device, attn.data_ptr(), grad.data_ptr(), n, B, H, L, c.data_ptr(), lib="cattn")


def lrp_row(K, sfx, c, out):
    B, n, L, _ = c.shape
    K._call(f"xai_cattn_lrp_row_{sfx}", c.device, c.data_ptr(), n, B, L, out.data_ptr(), lib="cattn")


def twice(launch, buf, view):
    """run, read, wipe, run again -> the first result; asserts the guards and that both runs gave the same bytes"""
    launch()
    first = view.cpu().numpy().copy()
    assert guards_intact(buf, view)
    view.fill_(SENTINEL)
    launch()
    assert view.cpu().numpy().tobytes() == first.tobytes() and guards_intact(buf, view)
    return first


# ------------------------------------------------------------------------------------------------ K82
# (L, H, d, B, T)
K82_SHAPES = [(2, 1, 1, 1, 1), (5, 2, 16, 3, 2), (63, 3, 64, 1, 3), (64, 12, 16, 1, 1), (65, 2, 65, 3, 2), (129, 3, 1, 1, 3),
              (197, 12, 64, 3, 2), (1024, 2, 1, 1, 1), (1025, 1, 16, 3, 2)]


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("L,H,d,B,T", K82_SHAPES)
def test_k82_game_map_is_the_restatement_bit_for_bit(K, L, H, d, B, T, dt, tdt, sfx):
    D = H * d
    g, gd = values(1, (B, T, D), tdt, 0.1)
    v, _ = values(2, (L, B, D), tdt)
    a0, ad = values(3, (B, H, L), tdt)
    a0, ad = np.abs(a0), ad.abs()
    vd = strided_v(v, tdt)
    assert vd.stride(0) > B * D and vd.stride(2) == 1
    buf, out = guarded((B, L - 1), torch.float32)
    got = twice(lambda: game(K, sfx, gd, vd, ad, out), buf, out)
    want = A.k82(g, v, a0, dt)
    assert same(got, want) and (L == 2 or (want > 0).any())            # L = 2: one patch, and its one product is negative
    # the wrapper, on a dense V, and an image alone has its own bytes
    dense = K.clip_game_map(gd, vd.contiguous(), ad)
    assert dense.dtype == torch.float32 and same(dense.cpu().numpy(), want)
    if B > 1:
        one = K.clip_game_map(gd[1:2].contiguous(), vd[:, 1:2], ad[1:2].contiguous())
        assert same(one.cpu().numpy(), want[1:2])


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
def test_k82_special_values_and_the_all_negative_map(K, dt, tdt, sfx):
    """NaN, +-Inf, subnormals and -0 in every operand; then every product negative: the map is +0 everywhere"""
    L, H, d, B, T = 9, 3, 5, 2, 2
    D = H * d
    g, _ = values(4, (B, T, D), tdt)
    v, _ = values(5, (L, B, D), tdt)
    a0 = np.abs(values(6, (B, H, L), tdt)[0])
    tiny = np.float32(2.0 ** -24 if dt == np.float16 else 1e-40)
    v[1, 0, 0], v[2, 0, 1], v[3, 0, 2], v[4, 0, 3], v[5, 0, 4] = np.nan, np.inf, -np.inf, tiny, -0.0
    g[0, 1, 7], g[1, 0, 0], g[1, 1, 1] = tiny, np.inf, -0.0
    a0[0, 1, 6], a0[1, 2, 2], a0[1, 0, 3], a0[0, 0, 7] = tiny, np.inf, 0.0, np.nan
    buf, out = guarded((B, L - 1), torch.float32)
    got = twice(lambda: game(K, sfx, to_dev(g, tdt), to_dev(v, tdt), to_dev(a0, tdt), out), buf, out)
    want = A.k82(g, v, a0, dt)
    assert same(got, want) and np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    g, v = np.abs(values(7, (B, T, D), tdt)[0]), -np.abs(values(8, (L, B, D), tdt)[0])
    a0 = np.abs(values(9, (B, H, L), tdt)[0]) + np.float32(1)
    got = twice(lambda: game(K, sfx, to_dev(g, tdt), to_dev(v, tdt), to_dev(a0, tdt), out), buf, out)
    assert same(got, A.k82(g, v, a0, dt)) and same(got, np.zeros((B, L - 1), np.float32))          # +0, bit for bit


# ------------------------------------------------------------------------------------------------ K83
# (L, H, B, T)
K83_SHAPES = [(2, 1, 1, 1), (5, 2, 3, 2), (63, 3, 1, 3), (64, 12, 3, 1), (65, 1, 1, 2), (129, 2, 3, 3), (197, 12, 3, 1), (256, 2, 1, 1),
              (257, 3, 1, 1), (1024, 3, 1, 2), (1025, 12, 3, 1)]


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("L,H,B,T", K83_SHAPES)
def test_k83_rollout_row_is_the_restatement_bit_for_bit(K, L, H, B, T, dt, tdt, sfx):
    a0 = torch.softmax(torch.randn((B, H, L), generator=torch.Generator().manual_seed(10)) * 2, dim=-1).to(tdt)
    ad, a0 = a0.to(DEV), a0.float().numpy()
    buf, out = guarded((B, L - 1), torch.float32, off=1)
    got = twice(lambda: rollout(K, sfx, ad, T, out), buf, out)
    want = A.k83(a0, T, dt)
    assert same(got, want) and (want > 0).all() and want.sum(axis=1).max() < 1
    assert same(K.clip_rollout_row(ad, texts=T).cpu().numpy(), want)
    if B > 1:
        assert same(K.clip_rollout_row(ad[2:3].contiguous(), texts=T).cpu().numpy(), want[2:3])


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
def test_k83_special_values(K, dt, tdt, sfx):
    L, H, B = 70, 2, 4
    a0 = np.abs(values(11, (B, H, L), tdt)[0])
    tiny = np.float32(2.0 ** -24 if dt == np.float16 else 1e-40)
    a0[0, 0, 5], a0[1, 1, 7], a0[2, 0, 3], a0[2, 1, 3], a0[3, :, 1:] = np.nan, np.inf, tiny, -0.0, 0.0
    buf, out = guarded((B, L - 1), torch.float32)
    got = twice(lambda: rollout(K, sfx, to_dev(a0, tdt), 1, out), buf, out)
    want = A.k83(a0, 1, dt)
    assert same(got, want) and np.isnan(want[0]).all() and np.isnan(want[1]).any() and not np.isnan(want[2:]).any()
    assert same(got[3], np.zeros(L - 1, np.float32))


# ------------------------------------------------------------------------------------------------ K84
# (L, H, n, B): L * L is a multiple of 8 at 64 and 8 (both dtypes take 16 bytes), of 4 alone at 6 (float only), odd elsewhere
K84_SHAPES = [(2, 1, 1, 1), (5, 2, 2, 3), (6, 2, 1, 1), (8, 3, 2, 3), (63, 3, 3, 1), (64, 12, 1, 3), (65, 1, 12, 1), (129, 2, 3, 3),
              (197, 12, 12, 1)]


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("L,H,n,B", K84_SHAPES)
def test_k84_matrices_are_the_restatement_bit_for_bit_on_both_paths(K, L, H, n, B, dt, tdt, sfx):
    """operands on a 16-byte boundary (the 16-byte flavour where L * L allows) and one element past it (the scalar flavour): the same
    bytes, and the restatement's"""
    attn = torch.softmax(torch.randn((n, B, H, L, L), generator=torch.Generator().manual_seed(12)), dim=-1).to(tdt).float().numpy()
    grad, _ = values(13, (n, B, H, L, L), tdt)
    want = A.k84(attn, grad, dt)
    assert (want > 0).any() and (want == 0).any()
    for off in (0, 1):
        ad, gd = to_dev(attn, tdt, off), to_dev(grad, tdt, off)
        assert ad.data_ptr() % 16 == off * ad.element_size()
        buf, c = guarded((B, n, L, L), tdt, off=off)
        got = twice(lambda: matrices(K, sfx, ad, gd, c), buf, c)
        assert same(got.astype(np.float32), want), off
    ad, gd = to_dev(attn, tdt), to_dev(grad, tdt)
    assert same(K.clip_lrp_matrices(ad, gd).float().cpu().numpy(), want)
    if B > 1:
        assert same(K.clip_lrp_matrices(ad[:, 1:2].contiguous(), gd[:, 1:2].contiguous()).float().cpu().numpy(), want[1:2])
    mine = torch.empty((B, n, L, L), dtype=tdt, device=DEV)
    assert K.clip_lrp_matrices(ad, gd, out=mine).data_ptr() == mine.data_ptr() and same(mine.float().cpu().numpy(), want)


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
def test_k84_special_values_on_both_paths(K, dt, tdt, sfx):
    L, H, n, B = 8, 3, 2, 2
    attn = np.abs(values(14, (n, B, H, L, L), tdt)[0])
    grad, _ = values(15, (n, B, H, L, L), tdt)
    tiny = np.float32(2.0 ** -24 if dt == np.float16 else 1e-40)
    grad[0, 0, 0, 0, 0], grad[0, 0, 1, 0, 1], grad[0, 0, 2, 0, 2], grad[0, 1, 0, 0, 3] = np.nan, np.inf, -np.inf, tiny
    grad[1, 0, :, 3, 3], attn[1, 0, :, 3, 3] = -0.0, 1.0
    attn[1, 1, 0, 0, 0], grad[1, 1, 0, 0, 0] = np.inf, 0.0                       # inf * 0
    attn[0, 1, 1, 7, 7], grad[0, 1, 1, 7, 7] = tiny, tiny                        # underflows to +0
    grad[1, 1, :, 5, :] = -np.abs(grad[1, 1, :, 5, :])                          # a whole row negative in every head
    want = A.k84(attn, grad, dt)
    assert np.isnan(want).sum() >= 2 and np.isinf(want).any() and (want[1, 1, 5] == 0).all()
    assert not np.signbit(want[0, 1, 3, 3]) and want[0, 1, 3, 3] == 0           # -0 in every head: +0
    for off in (0, 1):
        buf, c = guarded((B, n, L, L), tdt, off=off)
        got = twice(lambda: matrices(K, sfx, to_dev(attn, tdt, off), to_dev(grad, tdt, off), c), buf, c)
        assert same(got.astype(np.float32), want), off


# ------------------------------------------------------------------------------------------------ K85
# (L, n, B)
K85_SHAPES = [(2, 1, 1), (5, 2, 3), (63, 3, 1), (64, 12, 3), (65, 1, 1), (129, 2, 3), (197, 12, 3), (1024, 2, 1), (1025, 3, 1)]


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("L,n,B", K85_SHAPES)
def test_k85_relevance_row_is_the_restatement_bit_for_bit(K, L, n, B, dt, tdt, sfx):
    c = (torch.rand((B, n, L, L), generator=torch.Generator().manual_seed(16)) * (2.0 / L)).to(tdt)
    cd, c = c.to(DEV), c.float().numpy()
    buf, out = guarded((B, L - 1), torch.float32, off=1)
    got = twice(lambda: lrp_row(K, sfx, cd, out), buf, out)
    want = A.k85(c, dt)
    assert same(got, want) and (want > 0).all()
    assert same(K.clip_lrp_row(cd).cpu().numpy(), want)
    if B > 1:
        assert same(K.clip_lrp_row(cd[1:2].contiguous()).cpu().numpy(), want[1:2])


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
def test_k85_special_values_and_the_unit_row(K, dt, tdt, sfx):
    """NaN, +-Inf, subnormals and -0 in c; then c = 0 (what K84 leaves when every product is negative): r stays e_0, the map is +0"""
    L, n, B = 9, 3, 3
    c = (torch.rand((B, n, L, L), generator=torch.Generator().manual_seed(17)) * 0.2).to(tdt).float().numpy()
    tiny = np.float32(2.0 ** -24 if dt == np.float16 else 1e-40)
    c[0, 2, 0, 4], c[1, 1, 3, 3], c[1, 0, 2, 5], c[2, 2, 0, 1], c[2, 1, 1, 2], c[2, 0, 6, 6] = np.nan, np.inf, -np.inf, tiny, tiny, -0.0
    buf, out = guarded((B, L - 1), torch.float32)
    got = twice(lambda: lrp_row(K, sfx, to_dev(c, tdt), out), buf, out)
    want = A.k85(c, dt)
    assert same(got, want) and np.isnan(want[0]).any() and np.isnan(want[1]).any() and np.isfinite(want[2]).all()
    zero = np.zeros((B, n, L, L), np.float32)
    got = twice(lambda: lrp_row(K, sfx, to_dev(zero, tdt), out), buf, out)
    assert same(got, np.zeros((B, L - 1), np.float32)) and same(A.k85(zero, dt), got)


@pytest.mark.parametrize("dt,tdt,sfx", DTYPES, ids=DT_IDS)
def test_all_negative_products_give_lrp_the_unit_row_through_both_kernels(K, dt, tdt, sfx):
    L, H, n, B = 12, 3, 3, 2
    attn = np.abs(values(18, (n, B, H, L, L), tdt)[0])
    grad = -np.abs(values(19, (n, B, H, L, L), tdt)[0])
    c = K.clip_lrp_matrices(to_dev(attn, tdt), to_dev(grad, tdt))
    assert same(c.float().cpu().numpy(), np.zeros((B, n, L, L), np.float32))
    assert same(K.clip_lrp_row(c).cpu().numpy(), np.zeros((B, L - 1), np.float32))


# ------------------------------------------------------------------------------------------------ the wrappers
def test_wrappers_refuse_wrong_operands_before_a_launch(K):
    from xai_engine import _lib
    h, f = torch.float16, torch.float32
    g, v, a0 = torch.zeros(2, 1, 8, dtype=h, device=DEV), torch.zeros(5, 2, 8, dtype=h, device=DEV), torch.zeros(2, 2, 5, dtype=h, device=DEV)
    c = torch.zeros(2, 3, 5, 5, dtype=h, device=DEV)
    a5 = torch.zeros(3, 2, 4, 5, 5, dtype=h, device=DEV)
    with pytest.raises(TypeError, match="g: expected torch.float16"):
        K.clip_game_map(g.float(), v, a0)
    with pytest.raises(TypeError, match="a0: expected torch.float16"):
        K.clip_game_map(g, v, a0.float())
    with pytest.raises(TypeError, match="expected torch.float32 or torch.float16"):
        K.clip_rollout_row(a0.double())
    with pytest.raises(ValueError, match=r"a0 must be \(2, H, 5\) with H dividing D = 8"):
        K.clip_game_map(g, v, torch.zeros(2, 3, 5, dtype=h, device=DEV))
    with pytest.raises(ValueError, match=r"a0 must be \(2, H, 5\)"):
        K.clip_game_map(g, v, a0[:, :, :4].contiguous())
    with pytest.raises(ValueError, match=r"g must be \(2, T, 8\)"):
        K.clip_game_map(g[:1], v, a0)
    with pytest.raises(ValueError, match="contiguous in its last axis"):
        K.clip_game_map(g, v.transpose(1, 2), a0)
    with pytest.raises(ValueError, match="a0 must be contiguous"):
        K.clip_rollout_row(a0.transpose(0, 1))
    with pytest.raises(ValueError, match=r"2 <= L <= 4096"):
        K.clip_rollout_row(torch.zeros(1, 1, 4097, device=DEV))
    with pytest.raises(ValueError, match=r"T = 0 texts"):
        K.clip_rollout_row(a0, texts=0)
    with pytest.raises(ValueError, match=r"T = 1025 texts"):
        K.clip_rollout_row(a0, texts=1025)
    with pytest.raises(TypeError, match="grad: expected torch.float16"):
        K.clip_lrp_matrices(a5, a5.float())
    with pytest.raises(ValueError, match="grad must have the shape and device of attn"):
        K.clip_lrp_matrices(a5, a5[:2].contiguous())
    with pytest.raises(ValueError, match=r"attn must be \(n, B, H, L, L\)"):
        K.clip_lrp_matrices(a5[..., :4], a5[..., :4])
    with pytest.raises(ValueError, match="out has the wrong size"):
        K.clip_lrp_matrices(a5, a5, out=torch.zeros(2, 3, 5, 4, dtype=h, device=DEV))
    with pytest.raises(TypeError, match="out: expected torch.float16"):
        K.clip_lrp_matrices(a5, a5, out=torch.zeros(2, 3, 5, 5, device=DEV))
    with pytest.raises(ValueError, match=r"c must be \(B, n, L, L\)"):
        K.clip_lrp_row(c[..., :4])
    with pytest.raises(ValueError, match="c must be contiguous"):
        K.clip_lrp_row(c.transpose(2, 3))
    with pytest.raises(TypeError, match="expected torch.float32 or torch.float16"):
        K.clip_lrp_row(c.to(torch.bfloat16))
    for call in (lambda: K.clip_game_map(g.cpu(), v, a0), lambda: K.clip_lrp_matrices(a5, a5.cpu()), lambda: K.clip_rollout_row(a0.cpu())):
        with pytest.raises((_lib.XaiHipError, ValueError)):
            call()
    assert f is torch.float32
