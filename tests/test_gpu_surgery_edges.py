"""K86 and K87 (libxai_csurg.so) on the device against their NumPy restatements (tests/surgery_restated.py), at their edges: bit for
bit up to the first expf (K86's scores; K87's map once the kernel's own w is fed back into the restatement), inside the bounds
include/xai_csurg.h derives after it (K86's output, K87's w).  Every case runs in well under a second."""
import numpy as np
import pytest
import torch

import surgery_restated as S
from clip_restated import same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def limits():
    from xai_engine import kernels as K
    return K.csurg_limits()


def operands(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


SENTINEL, PAD = 7e30, 64


def guarded(numel):
    """-> (a buffer of PAD sentinels, numel floats, PAD sentinels; the view of the numel floats)"""
    buf = torch.full((numel + 2 * PAD,), SENTINEL, device=DEV)
    return buf, buf[PAD:PAD + numel]


def intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def run_k86(v, H):
    """v (n, L, B, D) on the CPU -> (scores, out) of the kernel, v handed over as the strided last third of a (n, L, B, 3 D) buffer
    of sentinels.  The entry is also called directly with its outputs between sentinels: the same bytes, the sentinels intact."""
    from xai_engine import _lib
    from xai_engine import kernels as K
    n, L, B, D = v.shape
    qkv = torch.full((n, L, B, 3 * D), SENTINEL, device=DEV)
    third = qkv[..., 2 * D:]
    third.copy_(v.to(DEV))
    out, scores = K.clip_vv_attention(third, H, want_scores=True)
    assert tuple(out.shape) == (n, B, L, D) and tuple(scores.shape) == (n, B, H, L, L) and out.is_contiguous()
    alone = K.clip_vv_attention(third, H)                                      # without the optional output: the same bytes
    assert same(alone.cpu().numpy(), out.cpu().numpy())
    out_buf, out_view = guarded(out.numel())
    s_buf, s_view = guarded(scores.numel())
    code = _lib.load("csurg").xai_csurg_vv_attention_f32(third.data_ptr(), third.stride(0), third.stride(1), third.stride(2), n, B, L, D, H,
                                                        float(D // H) ** -0.5, s_view.data_ptr(), out_view.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0 and intact(out_buf) and intact(s_buf)
    assert same(out_view.cpu().numpy(), out.cpu().numpy().ravel()) and same(s_view.cpu().numpy(), scores.cpu().numpy().ravel())
    assert bool((qkv[..., :2 * D] == SENTINEL).all())                          # and nothing of the operand's buffer was written
    return scores.cpu().numpy(), out.cpu().numpy()


def check_k86(v, H):
    scores, out = run_k86(v, H)
    s_ref, p_ref, o_ref = S.k86(v.numpy(), H)
    assert same(scores, s_ref)
    assert same(scores, np.ascontiguousarray(np.swapaxes(scores, -1, -2)))     # s_ij == s_ji bit for bit
    nan = np.isnan(o_ref)
    assert np.array_equal(np.isnan(out), nan)
    bound = S.k86_bound(np.nan_to_num(p_ref), np.nan_to_num(v.numpy(), nan=0.0, posinf=0.0, neginf=0.0), H)
    err = np.abs(out.astype(np.float64) - o_ref.astype(np.float64))
    assert (err[~nan] <= bound[~nan]).all(), float((err[~nan] / np.maximum(bound[~nan], 1e-300)).max())
    return scores, out, p_ref


@pytest.mark.parametrize("L", [2, 5, 64, 65, 197])
def test_k86_token_counts_around_a_wave_and_a_tile(L):
    """L = 2 (the least), 5 (fewer keys than a wave, fewer rows than a tile), 64 / 65 (a wave, one past it: a second key round and a
    fifth tile), 197 (ViT-B/16: 13 tiles, the last of 5 rows)"""
    check_k86(operands((1, L, 1, 64), L), 1)


@pytest.mark.parametrize("d,H", [(1, 1), (1, 3), (16, 3), (64, 1), (65, 1), (65, 3)])
def test_k86_head_widths_and_head_counts(d, H):
    """d = 1, 16, 64 (one column round), 65 (a second column round; an even LDS row stride); H = 1 and 3"""
    check_k86(operands((1, 21, 1, d * H), 100 + d + H, scale=d ** -0.25), H)


@pytest.mark.parametrize("n,B", [(1, 2), (6, 1), (6, 2)])
def test_k86_blocks_and_images_in_one_launch(n, B):
    check_k86(operands((n, 19, B, 32), 10 * n + B), 2)


def test_k86_the_largest_l_the_lds_limit_allows_and_one_more_is_refused():
    from xai_engine import kernels as K
    _, _, _, lds, waves = limits()
    L = lds // (64 + 1 + waves)
    assert L == 237 and waves == 4
    check_k86(operands((1, L, 1, 64), 237, scale=0.5), 1)
    with pytest.raises(ValueError, match="over the limits of K86"):
        K.clip_vv_attention(torch.zeros(1, L + 1, 1, 64, device=DEV), 1)
    # the entry itself, behind the wrapper's own check: XAI_E_UNSUPPORTED (-3) before any launch
    from xai_engine import _lib
    z = torch.zeros(1, L + 1, 1, 64, device=DEV)
    code = _lib.load("csurg").xai_csurg_vv_attention_f32(z.data_ptr(), z.stride(0), z.stride(1), z.stride(2), 1, 1, L + 1, 64, 1, 0.125,
                                                        None, z.data_ptr(), None)
    assert code == -3


def test_k86_one_hot_rows_equal_rows_and_expf_down_to_zero():
    # rows of large norm: every off-diagonal score is far below the diagonal one, the softmax is one-hot and o_i = v_i exactly
    v = operands((1, 9, 1, 16), 1)
    v = v / v.norm(dim=-1, keepdim=True) * 40.0
    v[0, 3] = v[0, 2]                                                          # two equal rows share their mass
    scores, out, p = check_k86(v, 1)
    for i in (0, 1, 4, 5, 6, 7, 8):
        assert p[0, 0, 0, i, i] == 1.0 and same(out[0, 0, i], v[0, i, 0].numpy())
    assert p[0, 0, 0, 2, 2] == p[0, 0, 0, 2, 3] == 0.5 and same(scores[0, 0, 0, 2], scores[0, 0, 0, 3])
    # one axis: s_ij = a_i a_j, so s_ij - max_j runs from 0 down through expf's subnormal range (below -87.3) to 0 (below -103.3)
    a = torch.tensor([0.0, 1.0, 5.0, 8.0, 8.5, 8.7, 8.8, 9.0, 9.2, 9.3, 9.35, 9.4, 9.5, 9.8, 10.0, 10.2, 10.4, 12.0, 16.0])
    v = torch.zeros(1, len(a), 1, 4)
    v[0, :, 0, 1] = a
    scores, out, p = check_k86(v, 1)
    e_last = S.exp32(scores[0, 0, 0, -1] - scores[0, 0, 0, -1].max())
    tiny = np.finfo(np.float32).tiny
    assert ((e_last > 0) & (e_last < tiny)).any() and (e_last == 0).any() and (e_last >= tiny).sum() >= 2
    # the device's expf keeps subnormal results: the kernel's row sums to 1 and its output is inside the bound (checked above)
    assert np.isfinite(out).all()


def test_k86_a_nan_row_and_an_inf_row_propagate_as_torchs():
    v = operands((1, 7, 2, 8), 5)
    v[0, 2, 0, 3] = float("nan")
    v[0, 4, 1, 0] = float("inf")
    scores, out, _ = check_k86(v, 1)
    vh = v.permute(0, 2, 1, 3)                                                  # (n, B, L, d), one head
    want = ((vh @ vh.transpose(-2, -1)) * 8 ** -0.5).softmax(-1) @ vh
    assert np.array_equal(np.isnan(out), torch.isnan(want).numpy())
    assert np.isnan(out[0, 0]).all()                                           # every row has a key with a NaN score
    # a row whose score against the Inf row is -Inf gives that key e = 0 and stays finite, but for 0 * Inf in the Inf row's column
    assert np.isnan(out[0, 1, 4]).all() and np.isnan(out[0, 1, :, 0]).all() and np.isfinite(out[0, 1, :, 1:]).any()
    v = operands((1, 7, 1, 8), 6)
    v[0, 2, 0, 3] = float("-inf")
    v[0, :, 0, 3].clamp_(min=float("-inf"), max=-0.5)                           # the products with -Inf are +Inf: every row has one
    _, out, _ = check_k86(v, 1)
    assert np.isnan(out).all()


def run_k87(feats, txt, T_out):
    """-> (out, w) of the kernel; the entry is also called directly with its outputs between sentinels"""
    from xai_engine import _lib
    from xai_engine import kernels as K
    f, t = feats.to(DEV), txt.to(DEV)
    out, w = K.clip_surgery_similarity(f, t, texts_out=T_out, want_weights=True)
    alone = K.clip_surgery_similarity(f, t, texts_out=T_out)
    assert same(alone.cpu().numpy(), out.cpu().numpy())
    B, L, E = f.shape
    T = t.shape[-2]
    out_buf, out_view = guarded(out.numel())
    w_buf, w_view = guarded(w.numel())
    code = _lib.load("csurg").xai_csurg_similarity_map_f32(f.data_ptr(), t.data_ptr(), T * E if t.dim() == 3 else 0, B, L, E, T, T_out,
                                                          w_view.data_ptr(), out_view.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0 and intact(out_buf) and intact(w_buf)
    assert same(out_view.cpu().numpy(), out.cpu().numpy().ravel()) and same(w_view.cpu().numpy(), w.cpu().numpy().ravel())
    return out.cpu().numpy(), w.cpu().numpy()


def check_k87(feats, txt, T_out=1):
    out, w = run_k87(feats, txt, T_out)
    _, w_ref = S.k87(feats.numpy(), txt.numpy(), T_out)
    nan = np.isnan(w_ref)
    assert np.array_equal(np.isnan(w), nan)
    err = np.abs(w.astype(np.float64) - w_ref.astype(np.float64))
    assert (err[~nan] <= S.k87_w_bound(w_ref)[~nan]).all()
    fed, _ = S.k87(feats.numpy(), txt.numpy(), T_out, w=w)                      # behind w everything is exact arithmetic on it
    assert same(out, fed)
    return out, w


@pytest.mark.parametrize("E", [1, 63, 64, 65, 512])
def test_k87_embedding_widths_around_a_wave(E):
    """E = 1, 63, 64, 65: the lane loop of DOT at and around one round; 512: CLIP's"""
    out, _ = check_k87(operands((1, 11, E), E).abs() + 0.1 if E == 1 else operands((1, 11, E), E), operands((5, E), E + 1), T_out=2)
    assert out.shape == (1, 2, 10)
    if E > 1:
        assert np.nanmin(out) == 0 and np.nanmax(out) == 1


def test_k87_one_patch_one_text_and_texts_out_below_t():
    out, _ = check_k87(operands((1, 2, 16), 1), operands((4, 16), 2))           # L = 2: one patch, lo == hi, 0 / 0
    assert out.shape == (1, 1, 1) and np.isnan(out).all()
    out, w = check_k87(operands((1, 9, 16), 3), operands((1, 16), 4))           # T = 1: w = 1, feats - mean is zero, 0 / 0
    assert np.isnan(out).all() and w.tolist() == [[1.0]]
    feats, txt = operands((1, 23, 32), 5), operands((60, 32), 6)
    one, _ = check_k87(feats, txt, 1)
    seven, _ = check_k87(feats, txt, 7)
    all_, _ = check_k87(feats, txt, 60)
    assert same(seven[:, :1], one) and same(all_[:, :7], seven)


def test_k87_a_batch_with_shared_and_with_per_image_texts_and_texts_beyond_a_wave():
    feats = operands((2, 18, 24), 7)
    shared, own = operands((70, 24), 8), operands((2, 70, 24), 9)               # T = 70: a second round of the softmax's lane loop
    both, _ = check_k87(feats, shared, 3)
    for b in range(2):
        assert same(both[b:b + 1], check_k87(feats[b:b + 1], shared, 3)[0])
    both, _ = check_k87(feats, own, 3)
    for b in range(2):
        assert same(both[b:b + 1], check_k87(feats[b:b + 1], own[b], 3)[0])


def test_k87_a_zero_feature_column_and_a_constant_similarity_column():
    feats, txt = operands((1, 12, 8), 10), operands((3, 8), 11)
    feats[0, :, 5] = 0.0                                                        # 0 / 0 through the norm over the tokens
    out, w = check_k87(feats, txt, 2)
    assert np.isnan(out).all() and np.isnan(w).all()
    # every patch row the same: sim is constant over the patches, lo == hi
    feats = operands((1, 12, 8), 12)
    feats[0, 1:] = feats[0, 1]
    out, w = check_k87(feats, txt, 3)
    assert np.isnan(out).all() and np.isfinite(w).all()
    # sharp probabilities: 2 * prob drives expf down through its subnormal range to 0; the map of text 0 stays finite
    feats = operands((1, 12, 8), 13)
    col = feats[0].norm(dim=0)
    unit = feats[0, 0] / col
    per = 2.0 * float((unit * unit).sum())                                      # x_t = 2 prob_t = k * per for the text k * f_0
    txt = torch.stack([(60.0 - gap / per) * unit for gap in (0.0, 1.0, 60.0, 88.0, 95.0, 102.0, 120.0)])      # x_0 - x_t = gap
    out, w = check_k87(feats, txt, 6)
    tiny = np.finfo(np.float32).tiny
    assert w[0, 0] > 1 and w[0, 6] == 0 and ((w[0] > 0) & (w[0] < tiny)).any() and np.isfinite(out[0, 0]).all()


def test_the_same_bytes_on_two_runs():
    v = operands((6, 50, 2, 128), 20)
    a, b = run_k86(v, 2), run_k86(v, 2)
    assert same(a[0], b[0]) and same(a[1], b[1])
    feats, txt = operands((2, 50, 512), 21), operands((60, 512), 22)
    a, b = run_k87(feats, txt, 2), run_k87(feats, txt, 2)
    assert same(a[0], b[0]) and same(a[1], b[1])
