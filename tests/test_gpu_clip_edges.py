"""K75-K77 (csrc/clip/clip_kernels.hip) against tests/clip_restated.py at the kernels' own edges, in both dtypes: D below, at and
above a wave and a workgroup, L around the 16 wave rounds and the 1024-lane strides, the shipped models' shapes, many workgroups,
the documented limits, and the values at which the rule of include/xai_clip.h branches (the clamp of NORMALIZE, 0 / 0, NaN and
infinite scores, subnormal products, a sum of -0, exp results below the normal range).

Operands are seeded randn cast to T, kept as fp32 NumPy values of T and as device tensors of T.  K and V are the last two thirds of
one (L, B, 3 D) device buffer whose first third is NaN, k_out is a view into a NaN-padded (L, B, D + 3) buffer: a lane that reads
past D reads another operand or a NaN, and every comparison below would show it.

Comparisons are those of test_gpu_eclip.py.  K76, K77 and K75's scores: bytes (`same`, a NaN by position).  K75's attn and att_out:
the header's derived bound, with its absolute term for fp32 results below 2^-126 (SUBNORMAL); every measured max(err / bound) is
written to profiles/r22_clip_edges.json, and no other number in this file is a tolerance."""
import os

import numpy as np
import pytest
import torch

import clip_restated as R
from clip_restated import same
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
DTYPES = (np.float32, np.float16)
SUBNORMAL = 3 * 2.0 ** -149          # the header: two expf results below 2^-126 and the quotient's rounding, 2^-149 each
SENTINEL = -4096.0                  # what surrounds an output passed as a view; no kernel result in these tests equals it
GUARD = 5                            # elements of it on either side (an odd count: a half view is then 2-byte aligned only)
_LEDGER = []

SHAPES = R.EDGE_SHAPES
LIMITS = (4096, 8192, 1)
CASES = [(s, dt) for s in SHAPES for dt in DTYPES]
IDS = ["x".join(map(str, s)) + "-" + np.dtype(dt).name for s, dt in CASES]
BOTH = pytest.mark.parametrize("dt", DTYPES, ids=("float32", "float16"))


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _write_the_ledger():
    yield
    if _LEDGER:
        R.merge_ledger(os.path.join(ROOT, "profiles", "r22_clip_edges.json"), _LEDGER, device=torch.cuda.get_device_name(0),
                       torch=torch.__version__)


# ------------------------------------------------------------------------------------------------ operands
def tdt(dt):
    return torch.float16 if dt == np.float16 else torch.float32


host = R.edge_operands


def device(h, dt):
    """the values of `h` as device tensors of T in the layout of this file's docstring"""
    t = {n: torch.from_numpy(a).to(tdt(dt)) for n, a in h.items()}
    assert all((t[n].float().numpy() == h[n]).all() or np.isnan(h[n]).any() for n in h)         # h holds values of T
    d = {n: t[n].to(DEV) for n in t if n not in ("k", "v", "k_out")}
    if "v" in t:
        L, B, D = t["v"].shape
        qkv = torch.full((L, B, 3 * D), NAN, dtype=tdt(dt), device=DEV)
        qkv[:, :, 2 * D:] = t["v"].to(DEV)
        d["v"] = qkv[:, :, 2 * D:]
        if "k" in t:
            qkv[:, :, D:2 * D] = t["k"].to(DEV)
            d["k"] = qkv[:, :, D:2 * D]
        assert d["v"].stride() == (3 * B * D, 3 * D, 1) and bool(qkv[:, :, :D].isnan().all())
    if "k_out" in t:
        L, B, D = t["k_out"].shape
        padded = torch.full((L, B, D + 3), NAN, dtype=tdt(dt), device=DEV)
        padded[:, :, :D] = t["k_out"].to(DEV)
        d["k_out"] = padded[:, :, :D]
        assert d["k_out"].stride(0) == B * (D + 3)
    return d


def np_of(t):
    return t.float().cpu().numpy() if t.dtype == torch.float16 else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the three comparisons
def check_k75(name, h, dt, attn, att_out, scores, exact=()):
    """scores: bytes.  attn and att_out: a NaN by position, the rest within the header's bound; the images in `exact` bytes too"""
    torch.cuda.synchronize()
    L, B, D = h["k"].shape
    assert attn.dtype == att_out.dtype == scores.dtype == tdt(dt) and tuple(attn.shape) == tuple(scores.shape) == (B, L)
    assert tuple(att_out.shape) == (B, D)
    _qs, s_ref, p_ref, o_ref = R.k75(h["q0"], h["k"], h["v"], dt)
    assert same(np_of(scores), s_ref), name
    p, o = attn.double().cpu().numpy(), att_out.double().cpu().numpy()
    assert np.array_equal(np.isnan(p), np.isnan(p_ref)) and np.array_equal(np.isnan(o), np.isnan(o_ref)), name
    dp, do = R.k75_bound(p, p_ref, o, o_ref, h["v"], dt, subnormal=SUBNORMAL)
    for what, got, ref, bound in (("attn", p, p_ref, dp), ("att_out", o, o_ref, do)):
        ok = ~np.isnan(ref)
        ratio = float((np.abs(got - ref)[ok] / bound[ok]).max()) if ok.any() else 0.0
        _LEDGER.append({"name": f"gpu/k75/{what}/{name}/{np.dtype(dt).name}", "measured": ratio, "bound": 1.0})
        print(f"k75/{what}/{name}/{np.dtype(dt).name}: max(err / bound) = {ratio:.3e}")
        assert ratio <= 1.0, (name, what, ratio)
    for b in exact:
        assert same(np_of(attn)[b], p_ref[b]) and same(np_of(att_out)[b], o_ref[b]), (name, b)
    return s_ref, p_ref, o_ref


PAIRS = [(True, True), (True, False), (False, True), (False, False)]


def check_k76(K, h, d, dt, pairs=PAIRS):
    """every flag pair: bytes -> {pair: the restated map}"""
    T = h["grad"].shape[1]
    wants = {}
    for withksim, withgrad in pairs:
        got = K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], d["grad"] if withgrad else None, texts=T, withksim=withksim,
                               withgrad=withgrad)
        want, _ = R.k76(h["q_out0"], h["k_out"], h["v"], h["grad"], T, withksim, withgrad, dt)
        assert got.dtype == torch.float32 and same(got.cpu().numpy(), want), (withksim, withgrad)
        wants[withksim, withgrad] = want
    return wants


def check_k77(K, h, d, dt):
    """per-image texts and shared texts: bytes -> the restated map of the per-image texts"""
    got = K.clip_maskclip_map(d["v_final"], d["txt"], d["k_out"])
    want = R.k77(h["v_final"], h["txt"], h["k_out"], dt)
    assert got.dtype == torch.float32 and same(got.cpu().numpy(), want)
    shared = K.clip_maskclip_map(d["v_final"], d["txt"][-1], d["k_out"])                         # txt_ld_b = 0
    assert same(shared.cpu().numpy(), R.k77(h["v_final"], np.broadcast_to(h["txt"][-1:], h["txt"].shape), h["k_out"], dt))
    return want


def widths(D):
    """E of K77 at width D: around a wave, and never D itself"""
    return sorted({1, 63, 64, 65, D // 2 + 1} - {D}) + ([512] if D == 768 else [])


# ------------------------------------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_k75_at_every_edge_shape(K, shape, dt):
    L, D, B = shape
    h = host(L, D, B, dt, names=("q0", "k", "v"))
    d = device(h, dt)
    _s, p_ref, _o = check_k75("x".join(map(str, shape)), h, dt, *K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True))
    assert (p_ref > 0).any() and not np.isnan(p_ref).any()


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_k76_at_every_edge_shape_for_every_flag_pair(K, shape, dt):
    """L = 2 is one patch: max - min = 0, the min-max is 0 / 0 and the map is NaN on both sides whenever withksim is set"""
    L, D, B = shape
    h = host(L, D, B, dt, names=("q_out0", "k_out", "v", "grad"))
    wants = check_k76(K, h, device(h, dt), dt)
    for (withksim, _), want in wants.items():
        if L == 2 and withksim:
            assert np.isnan(want).all()
        else:
            assert not np.isnan(want).any()
    assert any((w != 0).any() for w in wants.values())


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_k77_at_every_edge_shape_and_embedding_width(K, shape, dt):
    L, D, B = shape
    for E in widths(D):
        h = host(L, D, B, dt, E=E, names=("k_out", "v_final", "txt"))
        want = check_k77(K, h, device(h, dt), dt)
        assert not np.isnan(want).any() and (want != 0).any(), E


@BOTH
def test_the_most_texts_the_header_allows(K, dt):
    T = K.clip_limits()[2]
    assert T == 1024
    h = host(5, 8, 1, dt, T=T)
    d = device(h, dt)
    check_k76(K, h, d, dt)
    check_k77(K, h, d, dt)


# ------------------------------------------------------------------------------------------------ the layout
@BOTH
@pytest.mark.parametrize("shape", [(18, 70, 3), (3, 65, 3), (1025, 9, 3)], ids=("18x70", "3x65", "1025x9"))
def test_one_image_sliced_out_of_a_batch_of_three_has_the_batch_runs_bytes(K, shape, dt):
    """ld_b != D, and with odd D in half every row of K and V starts at a 2-byte-aligned offset"""
    L, D, B = shape
    h = host(L, D, B, dt)
    d = device(h, dt)
    one = {n: (t[:, 1:2] if n in ("k", "v", "k_out") else t[1:2].contiguous()) for n, t in d.items()}
    assert one["k"].stride() == (3 * B * D, 3 * D, 1) and one["k_out"].stride(0) == B * (D + 3)
    whole, alone = K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True), K.clip_cls_attention(one["q0"], one["k"], one["v"], want_scores=True)
    for w, a in zip(whole, alone):
        assert same(np_of(a), np_of(w[1:2]))
    for withksim, withgrad in PAIRS:
        w = K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], d["grad"], texts=3, withksim=withksim, withgrad=withgrad)
        a = K.clip_eclip_map(one["q_out0"], one["k_out"], one["v"], one["grad"], texts=3, withksim=withksim, withgrad=withgrad)
        assert same(a.cpu().numpy(), w[1:2].cpu().numpy()) and (a != 0).any()
    w = K.clip_maskclip_map(d["v_final"], d["txt"], d["k_out"])
    a = K.clip_maskclip_map(one["v_final"], one["txt"], one["k_out"])
    assert same(a.cpu().numpy(), w[1:2].cpu().numpy()) and (a != 0).any()


def guarded(shape, dtype):
    """-> (a contiguous view of `shape` inside a larger buffer of SENTINEL, the buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(shape), whole


def untouched(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


@BOTH
@pytest.mark.parametrize("shape", [(2, 1, 1), (3, 65, 2), (18, 70, 1), (1025, 8, 2), (3, 1025, 2)], ids=lambda s: "x".join(map(str, s)))
def test_outputs_passed_as_views_leave_what_surrounds_them_untouched(K, shape, dt):
    """every output of the three entries as a view into a larger buffer: the bytes of the wrapper's own call inside, the sentinels
    in front and behind as they were"""
    L, D, B = shape
    h = host(L, D, B, dt)
    d = device(h, dt)
    p, sfx, T, E = K._ptr, K._suffix(d["v"]), h["grad"].shape[1], h["txt"].shape[2]
    (attn, attn_w), (att_out, out_w), (scores, scores_w) = guarded((B, L), tdt(dt)), guarded((B, D), tdt(dt)), guarded((B, L), tdt(dt))
    assert attn.data_ptr() % 4 == (2 if dt == np.float16 else 0)
    K._call(f"xai_clip_cls_attention_{sfx}", d["v"].device, p(d["q0"]), p(d["k"]), d["k"].stride(0), d["k"].stride(1), p(d["v"]), d["v"].stride(0),
            d["v"].stride(1), B, L, D, float(D) ** -0.5, p(scores), p(attn), p(att_out), lib="clip")
    want = K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True)
    for got, w, whole in ((attn, want[0], attn_w), (att_out, want[1], out_w), (scores, want[2], scores_w)):
        assert same(np_of(got), np_of(w)) and untouched(whole) and not bool((got == SENTINEL).any())
    for withksim, withgrad in PAIRS:
        out, whole = guarded((B, L - 1), torch.float32)
        K._call(f"xai_clip_eclip_map_{sfx}", d["v"].device, p(d["q_out0"]), p(d["k_out"]), d["k_out"].stride(0), d["k_out"].stride(1), p(d["v"]),
                d["v"].stride(0), d["v"].stride(1), p(d["grad"]), B, L, D, T, int(withksim), int(withgrad), p(out), lib="clip")
        want = K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], d["grad"], texts=T, withksim=withksim, withgrad=withgrad)
        assert same(out.cpu().numpy(), want.cpu().numpy()) and untouched(whole) and not bool((out == SENTINEL).any())
    for ld_b, txt in ((T * E, d["txt"]), (0, d["txt"][0])):
        out, whole = guarded((B, L - 1), torch.float32)
        K._call(f"xai_clip_maskclip_map_{sfx}", d["v"].device, p(d["v_final"]), p(txt), ld_b, p(d["k_out"]), d["k_out"].stride(0), d["k_out"].stride(1),
                B, L, D, E, T, p(out), lib="clip")
        assert same(out.cpu().numpy(), K.clip_maskclip_map(d["v_final"], txt, d["k_out"]).cpu().numpy()) and untouched(whole)
        assert not bool((out == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ the documented limits
def test_k75_at_the_documented_limits_in_half(K):
    """L = 4096, D = 8192: 48 KiB of dynamic LDS beside the static reduction scratch, four trips of the L loops, eight of the D loops"""
    L, D, B = LIMITS
    assert (L, D) == K.clip_limits()[:2]
    h = host(L, D, B, np.float16, names=("q0", "k", "v"))
    d = device(h, np.float16)
    check_k75("limits", h, np.float16, *K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True))


def test_k76_at_the_documented_limits_in_half(K):
    L, D, B = LIMITS
    h = host(L, D, B, np.float16, names=("q_out0", "k_out", "v", "grad"))
    want = check_k76(K, h, device(h, np.float16), np.float16, pairs=PAIRS[:1])[True, True]
    assert not np.isnan(want).any() and (want > 0).any()


def test_k77_at_the_documented_limits_in_half(K):
    L, D, B = LIMITS
    h = host(L, D, B, np.float16, E=K.clip_limits()[1], T=2, names=("k_out", "v_final", "txt"))
    d = device(h, np.float16)
    got = K.clip_maskclip_map(d["v_final"], d["txt"], d["k_out"])
    want = R.k77(h["v_final"], h["txt"], h["k_out"], np.float16)
    assert same(got.cpu().numpy(), want) and not np.isnan(want).any() and (want != 0).any()


# ------------------------------------------------------------------------------------------------ the values: K76 and K77
tiny_rows = R.tiny_rows


@BOTH
def test_k76_and_k77_where_normalize_clamps_or_divides_by_zero(K, dt):
    """(6, 70, 4), an image each.  1: a zero patch row of k_out; in float the clamp makes its cosine 0 and the image stays finite, in
    half the clamp is 0, the row is 0 / 0 and the NaN cosine takes K76's whole image and K77's one entry.  2: a zero q_out0 (K76:
    every cosine 0 or NaN, so 0 / 0 in both dtypes) and a zero class row k_out[0] (K77: float 0, half NaN).  3: patch rows of tiny
    norm: below the clamp in float, subnormal in half."""
    half = dt == np.float16
    h = host(6, 70, 4, dt)
    h["k_out"][2, 1] = 0
    h["q_out0"][2] = 0
    h["k_out"][0, 2] = 0
    h["k_out"][1:, 3] = tiny_rows(h["k_out"][1:, 3], dt)
    d = device(h, dt)
    w76 = check_k76(K, h, d, dt)
    for pair in PAIRS[:2]:                                         # withksim
        w = w76[pair]
        assert not np.isnan(w[0]).any() and np.isnan(w[1]).all() == half and np.isnan(w[1]).any() == half and np.isnan(w[2]).all()
        assert not np.isnan(w[3]).any()
    assert (w76[True, True][3] != 0).any() and not any(np.isnan(w76[p]).any() for p in PAIRS[2:])
    w77 = check_k77(K, h, d, dt)
    assert not np.isnan(w77[0]).any() and not np.isnan(w77[3]).any() and (w77[3] != 0).any()
    assert np.array_equal(np.isnan(w77[1]), np.arange(5) == 1 if half else np.zeros(5, bool)) and (half or w77[1, 1] == 0)
    assert np.isnan(w77[2]).all() if half else (w77[2] == 0).all()


@BOTH
def test_k77_with_a_zero_embedding_row_and_a_product_of_minus_zero(K, dt):
    """(70, 8, 1) would do; (6, 70, 4) keeps an untouched image beside each.  1: a zero row of v_final (float: the clamp, a = 0; half:
    0 / 0).  2: texts of zeros: a = +0 (a sum from +0), a * c = -0 wherever the cosine is negative, and the sum over the texts from
    +0 must come out +0.  3: embedding rows of tiny norm."""
    half = dt == np.float16
    h = host(6, 70, 4, dt)
    h["v_final"][1, 3] = 0
    h["txt"][2] = 0
    h["v_final"][3] = tiny_rows(h["v_final"][3], dt)
    d = device(h, dt)
    want = check_k77(K, h, d, dt)
    got = K.clip_maskclip_map(d["v_final"], d["txt"], d["k_out"]).cpu().numpy()
    assert np.array_equal(np.isnan(want[1]), np.arange(5) == 3 if half else np.zeros(5, bool)) and (half or want[1, 3] == 0)
    kn = R.normalize_rows(h["k_out"][:, 2], dt)
    cos = R.rT(R.wave_sum_rows(R.rT(kn[:1] * kn[1:], dt)), dt)
    assert (cos < 0).any() and np.signbit(R.rT(np.float32(0) * cos, dt)).any()                    # the -0 products are there
    assert (got[2] == 0).all() and not np.signbit(got[2]).any() and not np.signbit(want[2]).any()
    assert not np.isnan(want[3]).any() and (want[3] != 0).any() and not np.isnan(want[0]).any()


@BOTH
def test_k76_with_an_infinite_v_subnormal_products_and_a_sum_of_minus_zero(K, dt):
    """(6, 70, 4).  1: one +inf in v, and one -inf in another row.  2: grad * v in the subnormal range of T: fp32 denormals are kept
    and half subnormals are rounded to their spacing of 2^-24, neither is flushed.  3: every term of every per-text sum is -0.  SUM
    starts each lane from +0, so the sum itself is +0 (no per-text sum of K76 can be -0: a sum of terms of T is a multiple of T's
    least spacing, and x + (-x) = +0); the map must be +0.  K77's -0 is in the test above."""
    half = dt == np.float16
    h = host(6, 70, 4, dt)
    h["v"][2, 1, 5], h["v"][4, 1, 69] = INF, -INF
    if half:
        h["grad"][2], h["v"][1:, 2] = R.rT(h["grad"][2] * np.float32(2.0 ** -10), dt), R.rT(h["v"][1:, 2] * np.float32(2.0 ** -10), dt)
        low, high = 2.0 ** -24, 2.0 ** -14
    else:
        h["grad"][2], h["v"][1:, 2] = h["grad"][2] * np.float32(1e-25), h["v"][1:, 2] * np.float32(1e-15)
        low, high = 2.0 ** -149, 2.0 ** -126
    prod = np.abs(h["grad"][2][:, None, :].astype(np.float64) * h["v"][1:, 2][None].astype(np.float64))
    assert (prod < high).all() and (prod > low).mean() > 0.5
    h["grad"][3] = np.float32(-0.0)
    h["v"][1:, 3] = np.abs(h["v"][1:, 3])
    assert np.signbit(R.rT(h["grad"][3][:, None, :] * h["v"][1:, 3][None], dt)).all()
    d = device(h, dt)
    wants = check_k76(K, h, d, dt)
    for pair in PAIRS:
        assert not np.isnan(wants[pair][0]).any() and (wants[pair][0] != 0).any()
    assert wants[False, False][1, 1] == INF and wants[False, False][1, 3] == 0                    # the rows of the two infinities; relu(-inf) = 0
    assert not np.isfinite(wants[False, True][1, [1, 3]]).all()
    for pair in ((True, True), (False, True)):                                                    # withgrad
        assert (wants[pair][2] != 0).any(), pair                                                  # not flushed
        got = K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], d["grad"], withksim=pair[0], withgrad=True).cpu().numpy()
        assert (got[3] == 0).all() and not np.signbit(got[3]).any() and not np.signbit(wants[pair][3]).any()


# ------------------------------------------------------------------------------------------------ the values: K75
@BOTH
@pytest.mark.parametrize("shape", [(6, 70, 4), (70, 8, 1), (1025, 8, 1), (2049, 4, 2)], ids=lambda s: "x".join(map(str, s)))
def test_k75_with_all_scores_equal_is_exact(K, shape, dt):
    """every key row the same row: s_j equal, e_j = exp(0) = 1 on both sides, so attn = rT(1 / BLOCKSUM(L; 1)) and att_out are
    defined bit for bit"""
    L, D, B = shape
    h = host(L, D, B, dt, names=("q0", "k", "v"))
    h["k"][:] = h["k"][:1]
    d = device(h, dt)
    s_ref, p_ref, _o = check_k75("equal-" + "x".join(map(str, shape)), h, dt, *K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True),
                                 exact=range(B))
    assert (s_ref == s_ref[:, :1]).all() and (p_ref == R.rT(np.float32(1) / np.float32(L), dt)).all()


@BOTH
def test_k75_with_a_nan_an_infinite_and_only_minus_infinite_scores(K, dt):
    """(6, 70, 4), an image each.  1: one NaN score.  2: one +inf score (half: a query large enough that the scores overflow).
    3: every score -inf.  Each of these rows of attn and att_out is all NaN on both sides; image 0 stays finite."""
    half = dt == np.float16
    h = host(6, 70, 4, dt, names=("q0", "k", "v"))
    h["k"][3, 1, 7] = NAN
    if half:
        h["q0"][2], h["k"][2, 2] = np.float32(60000), np.float32(100)
    else:
        h["q0"][2, 9], h["k"][2, 2, 9] = np.float32(1.5), INF
    h["q0"][3, 0], h["k"][:, 3, 0] = np.float32(1), -INF
    d = device(h, dt)
    attn, att_out, scores = K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True)
    s_ref, p_ref, o_ref = check_k75("specials", h, dt, attn, att_out, scores)
    assert np.isnan(s_ref[1]).sum() == 1 and (s_ref[2] == INF).any() and not np.isnan(s_ref[2]).any() and (s_ref[3] == -INF).all()
    assert not np.isnan(p_ref[0]).any() and np.isnan(p_ref[1:]).all() and not np.isnan(o_ref[0]).any() and np.isnan(o_ref[1:]).all()
    assert bool(attn[1:].isnan().all()) and bool(att_out[1:].isnan().all()) and not bool(attn[0].isnan().any())


def test_k75_with_exp_results_in_the_normal_range_the_subnormal_range_and_at_zero(K):
    """fp32, (70, 8, 1): q = sqrt(8) everywhere, k[j][0] = -2 j, so the scores are 0, -2, ..., -138 and e_j = exp(-2 j) runs through
    the normal range (to j = 43), the subnormal range (j = 44 .. 51) and 0.  The relative bound means nothing below 2^-126, where one
    ulp is 2^-149 absolute: the header's SUBNORMAL term.  Had the device's expf returned 0 for subnormal results this test would fail
    by at most 2^-126; it does not."""
    dt = np.float32
    h = host(70, 8, 1, dt, names=("q0", "k", "v"))
    h["q0"][:] = np.sqrt(np.float32(8))
    h["k"][:] = 0
    h["k"][:, 0, 0] = -2 * np.arange(70, dtype=np.float32)
    d = device(h, dt)
    attn, att_out, scores = K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True)
    s_ref, p_ref, _o = check_k75("exp-range", h, dt, attn, att_out, scores)
    assert (np.abs(s_ref[0] + 2.0 * np.arange(70)) <= 2.0 * np.arange(70) * 2.0 ** -22).all()
    tiny = 2.0 ** -126
    assert (p_ref[0] >= tiny).sum() >= 40 and ((p_ref[0] > 0) & (p_ref[0] < tiny)).sum() >= 6 and (p_ref[0] == 0).sum() >= 15
    p = attn[0].cpu().numpy()
    assert ((p > 0) & (p < tiny)).sum() >= 6                                                      # the device keeps them too
