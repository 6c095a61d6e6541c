"""LIME on the MI355X: K31 bit for bit against a NumPy select, K32 against the reference's recorded runs (tests/golden/lime.npz)
and the fp64 restatement (tests/lime_restated.py), K33 against table[seg], the reference interface and the harness row.

What is exact and what is not.  K31 and K33 copy floats: every float is compared as its int32 bits.  The 0/1 matrix, the order of
an explanation and the masks are integers and must be equal.  K32's fp64 outputs are held to conftest.BAR.  An order can only be
compared where it does not hinge on rounding: every case whose order is compared is asserted (never skipped) to keep gaps between
neighbouring |coef| of at least 100 times the measured difference of the two arithmetics (lime_restated.conditioned).

Exact ties.  Two duplicated columns give coefficients that agree only to rounding, in any arithmetic, so their mutual order is
not a property of LIME; columns that are constant over the samples (a superpixel that is never switched off) are centred to exact
zeros, get coefficients that are exact zeros in K32 and in the restatement, and fall behind every other feature in the order of
the alpha = 0.01 fit and then of the lower index: that is the tie the duplicated-columns case pins."""
import functools

import numpy as np
import pytest
import torch

import lime_restated as R
from conftest import BAR, check, load_golden
from helpers import tiny_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from xai_engine import lime
    return lime


@pytest.fixture(scope="module")
def model():
    return tiny_from(load_golden("ig_small.npz"), DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rows(mats, words=None):
    """0/1 matrices of B images (one N) -> int64 (B * N, words) on the device, D (B,) int32."""
    words = max((m.shape[1] + 63) // 64 for m in mats) if words is None else words
    packed = np.concatenate([R.pack(m, words) for m in mats]).view(np.int64)
    return torch.from_numpy(packed).to(DEV), torch.tensor([m.shape[1] for m in mats], dtype=torch.int32).to(DEV)


# ------------------------------------------------------------------------------------------------------------- K31
N_ROWS = 6


@functools.lru_cache(maxsize=None)
def _compose_case(shape, dpair):
    """Two images with dpair superpixel counts: random ids in [0, D) plus three ids no row can switch off (-1, D, 10000), NaN / Inf
    / -0 planted in x, rows = all ones, all zeros, random.  -> x, seg, mats, fudged, hide."""
    C, H, W = shape
    rng = np.random.default_rng(hash((shape, dpair)) % 2 ** 32)
    x = rng.standard_normal((2, C, H, W)).astype(np.float32)
    fudged = rng.standard_normal((2, C, H, W)).astype(np.float32)
    hide = rng.standard_normal(C).astype(np.float32)
    seg = np.stack([rng.integers(0, D, (H, W)) for D in dpair]).astype(np.int32)
    for b, D in enumerate(dpair):
        seg[b, 0, 0], seg[b, H - 1, W - 1], seg[b, H // 2, W // 2] = -1, D, 10000
        x[b, 0, 0, 1], x[b, 0, H - 1, 0], x[b, C - 1, 1, 2], x[b, 0, 2, 3] = np.nan, np.inf, -np.inf, -0.0
    mats = []
    for D in dpair:
        m = rng.integers(0, 2, (N_ROWS, D))
        m[0], m[1] = 1, 0
        mats.append(m)
    return x, seg, mats, fudged, hide


def _composed(x, seg, mats, fill, first, n):
    out = []
    for r in range(first, first + n):
        b, s = divmod(r, N_ROWS)
        out.append(R.perturbed(x[b], seg[b], mats[b][s], fill[b] if fill.ndim == 4 else fill[:, None, None]))
    return np.stack(out)


@pytest.mark.parametrize("mode", ["hide", "fudged"])
@pytest.mark.parametrize("dpair", [(1, 130), (63, 65), (64, 64)])
@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 65, 63), (3, 40, 36)])
def test_k31_composes_bit_for_bit(shape, dpair, mode):
    """(3, 5, 7) and (1, 65, 63) have C*H*W % 4 != 0 (the scalar flavour), (3, 40, 36) takes 16-byte stores; D = 1, 63, 64, 65, 130
    cross the word boundaries; the images of a pass have different D; [4, 9) starts inside image 0 and ends inside image 1."""
    from xai_engine import kernels as K
    x, seg, mats, fudged, hide = _compose_case(shape, dpair)
    rows, D = _rows(mats)
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(seg).to(DEV)
    hd = torch.from_numpy(hide).to(DEV) if mode == "hide" else None
    fd = torch.from_numpy(fudged).to(DEV) if mode == "fudged" else None
    fill = hide if mode == "hide" else fudged
    chw = int(np.prod(shape))
    for first, n in ((0, 2 * N_ROWS), (4, 5), (7, 1)):
        guard = 64
        buf = torch.full((2 * guard + n * chw,), -7.5, dtype=torch.float32, device=DEV)
        out = buf[guard:guard + n * chw].view(n, *shape)
        K.lime_compose(xd, sd, rows, D, hd, first, n, fudged=fd, out=out)
        want = _composed(x, seg, mats, fill, first, n)
        host = buf.cpu().numpy()
        np.testing.assert_array_equal(_bits(host[guard:guard + n * chw]).reshape(want.shape), _bits(want))
        assert (host[:guard] == -7.5).all() and (host[guard + n * chw:] == -7.5).all()          # nothing written outside `out`
    # an all-ones row is the image itself, NaN and Inf included; in an all-zero row they are gone wherever an id can be switched off
    full = K.lime_compose(xd, sd, rows, D, hd, 0, 2 * N_ROWS, fudged=fd).cpu().numpy()
    for b in range(2):
        np.testing.assert_array_equal(_bits(full[b * N_ROWS]), _bits(x[b]))
        inside = (seg[b] >= 0) & (seg[b] < dpair[b])
        zero_row = full[b * N_ROWS + 1]
        fill_b = np.broadcast_to(fill[b] if fill.ndim == 4 else fill[:, None, None], x[b].shape)
        np.testing.assert_array_equal(_bits(zero_row[:, inside]), _bits(fill_b[:, inside]))
        np.testing.assert_array_equal(_bits(zero_row[:, ~inside]), _bits(x[b][:, ~inside]))      # ids outside [0, D) stay on
        assert np.isfinite(zero_row[:, inside]).all() and not np.isfinite(x[b][:, inside]).all()
    # fudged wins over hide when both are passed
    if mode == "fudged":
        both = K.lime_compose(xd, sd, rows, D, torch.from_numpy(hide).to(DEV), 0, 3, fudged=fd).cpu().numpy()
        np.testing.assert_array_equal(_bits(both), _bits(full[:3]))


HBM_ROWS = 1366          # rows of 3 x 64 x 64 floats (49 152 B): 1366 x 49 152 = 67 141 632 B >= 64 MiB > 1365 x 49 152 B


@functools.lru_cache(maxsize=None)
def _hbm_case():
    """Two images of 3 x 64 x 64 with 63 and 65 superpixels and HBM_ROWS / 2 rows each -> x, seg, mats, hide, the restated list."""
    rng = np.random.default_rng(31)
    x = rng.standard_normal((2, 3, 64, 64)).astype(np.float32)
    hide = rng.standard_normal(3).astype(np.float32)
    seg = np.stack([rng.integers(0, D, (64, 64)) for D in (63, 65)]).astype(np.int32)
    mats = [rng.integers(0, 2, (HBM_ROWS // 2, D)) for D in (63, 65)]
    want = np.stack([R.perturbed(x[b], seg[b], row, hide[:, None, None]) for b in range(2) for row in mats[b]])
    return x, seg, mats, hide, want


@pytest.mark.parametrize("n", [HBM_ROWS, HBM_ROWS - 1])
def test_k31_hbm_sized_pass_composes_bit_for_bit(n):
    """The smallest pass at or over the 64 MiB from which a lane writes two rows, and the largest under it."""
    from xai_engine import kernels as K
    x, seg, mats, hide, want = _hbm_case()
    rows, D = _rows(mats)
    got = K.lime_compose(torch.from_numpy(x).to(DEV), torch.from_numpy(seg).to(DEV), rows, D, torch.from_numpy(hide).to(DEV), 0, n)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want[:n]))


# ------------------------------------------------------------------------------------------------------------- K32
FP64 =("coef", "intercept", "score", "local_pred", "dist", "weight")


def _fit(mats, Ys, words=None, **kw):
    """K32 on B images -> dict of host arrays, the feature axis left at d_stride."""
    from xai_engine import kernels as K
    rows, D = _rows(mats, words)
    Y = torch.from_numpy(np.ascontiguousarray(np.stack(Ys), dtype=np.float32)).to(DEV)
    res = K.lime_fit(rows, D, Y, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _image(res, b, D):
    out = {k: res[k][b] for k in ("intercept", "score", "local_pred", "dist", "weight")}
    out["coef"], out["order"] = res["coef"][b][:, :D], res["order"][b][:, :D]
    assert not res["coef"][b][:, D:].any() and (res["order"][b][:, D:] == -1).all()
    return out


def _meets(name, got, want, against, skip=()):
    """fp64 outputs at BAR through the ledger; -> the largest |coef difference|, the `err` of `conditioned`."""
    for k in FP64:
        if k in skip or k not in want:
            continue
        check(f"{name}/{k}", got[k], want[k], BAR, against=against)
    return float(np.abs(got["coef"] - want["coef"]).max())


@pytest.mark.parametrize("tag", R.GOLDEN_CASES)
def test_k32_meets_the_references_recorded_fits(tag):
    g = load_golden("lime.npz")
    c = R.golden_case(g, tag)
    Y = c["labels"][:, c["top"]]
    got = _image(_fit([c["data"]], [Y]), 0, c["D"])
    ref = dict(coef=c["coef"], dist=g[f"{tag}_dist"], **{k: g[f"{tag}_{k}"] for k in ("intercept", "score", "local_pred")})
    err = _meets(f"lime_k32/{tag}", got, ref, "reference LIME")
    check(f"lime_k32/{tag}/weight", got["weight"], R.kernel_weights(g[f"{tag}_dist"]), BAR, against="reference LIME")
    assert R.conditioned(dict(coef=c["coef"], order=c["order"]), err), err
    np.testing.assert_array_equal(got["order"], c["order"])
    for l in range(len(c["top"])):
        assert R.chosen_features(got["order"][l], got["coef"][l]) == R.chosen_features(c["order"][l], c["coef"][l])
    np.testing.assert_array_equal(R.mask_of(c["seg"], got["order"][0], got["coef"][0]), g[f"{tag}_mask"])


@pytest.mark.parametrize("shape", [(1000, 60, 5), (1000, 128, 5), (50, 128, 1), (8, 3, 5), (2, 1, 1), (300, 65, 1)])
def test_k32_meets_the_restatement_on_seeded_cases(shape):
    """(50, 128): fewer samples than features, the Gram matrix is singular without the ridge; (8, 3) and (2, 1) hold an all-zero row
    (distance 1); 128 is the cap; 65 crosses the word and the lane boundary."""
    N, D, nl = shape
    data, Y = R.seeded_fit_case(N, D, nl, seed=N * 1000 + D, zero_rows=1 if N <= 8 else 0)
    assert N > 8 or not data[1].any()
    want = R.explain(data, Y)
    got = _image(_fit([data], [Y]), 0, D)
    err = _meets(f"lime_k32/seeded{shape}", got, want, "restated LIME")
    assert R.conditioned(want, err), err
    np.testing.assert_array_equal(got["order"], want["order"])
    if N <= 8:
        assert got["dist"][1] == 1.0 and got["dist"][0] == 0.0 and got["weight"][0] == 1.0


def test_k32_with_only_the_instance_itself():
    """N = 1: nothing varies, every coefficient is exactly 0, the stable order is 0 .. D - 1, nothing is chosen, the score is
    undefined (NaN, as sklearn's r2_score below two samples)."""
    data, Y = R.seeded_fit_case(1, 5, 2, seed=4)
    want = R.explain(data, Y)
    got = _image(_fit([data], [Y]), 0, 5)
    assert not got["coef"].any() and not want["coef"].any()
    assert got["order"].tolist() == want["order"].tolist() == [[0, 1, 2, 3, 4]] * 2
    assert np.isnan(got["score"]).all() and np.isnan(want["score"]).all()
    _meets("lime_k32/n1", got, want, "restated LIME", skip=("score", "coef"))
    assert R.conditioned(want, 0.0) and R.chosen_features(got["order"][0], got["coef"][0]) == []
    assert not R.mask_of(np.zeros((3, 3), int), got["order"][0], got["coef"][0]).any()


def test_k32_exact_ties_follow_the_selection_fit_and_then_the_lower_index():
    """Columns 3 and 7 are duplicates that never vary: exact zero coefficients in both fits, so they end the order as 3, 7."""
    data, Y = R.seeded_fit_case(400, 12, 5, seed=9)
    data[:, 3] = data[:, 7] = 1
    want = R.explain(data, Y)
    got = _image(_fit([data], [Y]), 0, 12)
    assert not got["coef"][:, [3, 7]].any() and not want["coef"][:, [3, 7]].any()
    err = _meets("lime_k32/ties", got, want, "restated LIME")
    assert R.conditioned(want, err), err
    np.testing.assert_array_equal(got["order"], want["order"])
    assert (got["order"][:, -2:] == [3, 7]).all()


def test_k32_batch_equals_the_images_alone_and_two_runs_bit_for_bit():
    """B = 3 with D = (24, 1, 70) in one launch: every image gets what it gets alone, to the bit; a second run repeats the first."""
    N, nl = 120, 5
    cases = [R.seeded_fit_case(N, D, nl, seed=D) for D in (24, 1, 70)]
    mats, Ys = [c[0] for c in cases], [c[1] for c in cases]
    both = _fit(mats, Ys)
    again = _fit(mats, Ys)
    for k in both:
        np.testing.assert_array_equal(both[k].view(np.int64 if both[k].dtype == np.float64 else np.int32),
                                      again[k].view(np.int64 if again[k].dtype == np.float64 else np.int32))
    for b, D in enumerate((24, 1, 70)):
        alone = _image(_fit([mats[b]], [Ys[b]]), 0, D)
        batch = _image(both, b, D)
        for k in alone:
            assert alone[k].tobytes() == batch[k].tobytes(), (b, k)
        want = R.explain(mats[b], Ys[b])
        err = _meets(f"lime_k32/batch{b}", batch, want, "restated LIME")
        assert R.conditioned(want, err), err
        np.testing.assert_array_equal(batch["order"], want["order"])


def test_an_image_above_the_cap_is_fitted_on_the_host(L, model):
    """D = cap + 1 through lime_batch: K32 skips the image, the driver's fp64 host fit fills it and LIME_COUNTS counts it."""
    from xai_engine import kernels as K
    D = K.lime_max_features() + 1
    H, W = 40, 36
    seg = (np.arange(H * W) * D // (H * W)).reshape(H, W)
    assert len(np.unique(seg)) == D
    _, image = R.seeded_case(H, W, 5, 3)
    x = torch.from_numpy(image.transpose(2, 0, 1).copy())[None].to(DEV)
    before = L.LIME_COUNTS["host_fits"]
    out, det = L.lime_batch(x, model, seg, num_samples=150, top_labels=2, random_state=5, pass_size=50, want="details")
    assert L.LIME_COUNTS["host_fits"] == before + 1
    data, Y = det.data[0], det.labels[0].cpu().numpy()
    want = R.explain(data, Y)
    got = dict(coef=det.coef[0, :, :D].cpu().numpy(), order=det.order[0, :, :D].cpu().numpy(), intercept=det.intercept[0].cpu().numpy(),
               score=det.score[0].cpu().numpy(), local_pred=det.local_pred[0].cpu().numpy(), dist=det.distances[0].cpu().numpy(),
               weight=det.weights[0].cpu().numpy())
    err = _meets("lime_batch/above_cap", got, want, "restated LIME")
    assert R.conditioned(want, err), err
    np.testing.assert_array_equal(got["order"], want["order"])
    np.testing.assert_array_equal(out[0].cpu().numpy(), 3.0 * R.mask_of(seg, want["order"][0], want["coef"][0]))


# ------------------------------------------------------------------------------------------------------------- K33
def test_k33_paints_table_of_seg_exactly():
    from xai_engine import kernels as K
    one = K.lime_paint(torch.tensor([[2.5], [-1.0]], device=DEV), torch.zeros((2, 3, 5), dtype=torch.int32, device=DEV)).cpu().numpy()
    assert (one[0] == 2.5).all() and (one[1] == -1.0).all()
    g = load_golden("lime.npz")
    rng = np.random.default_rng(0)
    seg = np.stack([g["in1_seg"].astype(np.int32), rng.integers(0, 70, (65, 63)).astype(np.int32)])
    table = rng.standard_normal((2, 70)).astype(np.float32)
    table[0, 5], table[1, 6] = np.nan, -0.0
    got = K.lime_paint(torch.from_numpy(table).to(DEV), torch.from_numpy(seg).to(DEV)).cpu().numpy()
    want = np.stack([table[b][seg[b]] for b in range(2)])
    np.testing.assert_array_equal(_bits(got), _bits(want))
    seg[1, 0, 0], seg[1, 64, 62] = -1, 70                                     # outside the table: 0
    got = K.lime_paint(torch.from_numpy(table).to(DEV), torch.from_numpy(seg).to(DEV)).cpu().numpy()
    assert got[1, 0, 0] == 0.0 and got[1, 64, 62] == 0.0
    want[1, 0, 0] = want[1, 64, 62] = 0.0
    np.testing.assert_array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------------- end to end
def _eager_probs(model, image, seg, data, fill, top):
    x = image.transpose(2, 0, 1)
    batch = np.stack([R.perturbed(x, seg, row, fill) for row in data])
    with torch.no_grad():
        p = torch.softmax(model(torch.from_numpy(batch).to(DEV)), dim=1)
    return p[:, torch.as_tensor(np.asarray(top)).to(DEV)].cpu().numpy()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_explainer_on_the_golden_case(L, model, tag):
    """The engine's LimeImageExplainer with the stored seed and segments (hide_color 0 and None): the reference's matrix, the
    probabilities of an eager forward of the restated perturbed images, the explanation the restatement gives for them."""
    from xai_engine.streams import LOGIT_RTOL
    g = load_golden("lime.npz")
    c = R.golden_case(g, tag)
    seg = c["seg"].astype(np.int64)
    exp = L.LimeImageExplainer(random_state=c["seed"]).explain_instance(c["image"], L.batch_predict, model, DEV, top_labels=5,
                                                                       hide_color=c["hide"], num_samples=c["N"], segmentation_fn=lambda im: seg)
    det = exp.details
    np.testing.assert_array_equal(det.data[0], c["data"])
    assert exp.top_labels == c["top"].tolist()
    fill = np.float32(c["hide"]) if c["hide"] is not None else R.segment_means(c["image"], seg).transpose(2, 0, 1)
    Y = det.labels[0].cpu().numpy()
    check(f"lime_e2e/{tag}/probabilities", Y, _eager_probs(model, c["image"], seg, c["data"], fill, exp.top_labels), LOGIT_RTOL,
          against="eager torch")
    check(f"lime_e2e/{tag}/probabilities_vs_reference", Y, c["labels"][:, c["top"]], LOGIT_RTOL, against="reference LIME")
    want = R.explain(c["data"], Y)
    got = dict(coef=np.array([[dict(exp.local_exp[l])[f] for f in range(c["D"])] for l in exp.top_labels]),
               intercept=np.array([exp.intercept[l] for l in exp.top_labels]))
    check(f"lime_e2e/{tag}/coef", got["coef"], want["coef"], BAR, against="restated LIME")
    check(f"lime_e2e/{tag}/intercept", got["intercept"], want["intercept"], BAR, against="restated LIME")
    check(f"lime_e2e/{tag}/score", exp.score, want["score"][0], BAR, against="restated LIME")
    check(f"lime_e2e/{tag}/local_pred", exp.local_pred, want["local_pred"][:1], BAR, against="restated LIME")
    check(f"lime_e2e/{tag}/distances", det.distances[0].cpu().numpy(), want["dist"], BAR, against="restated LIME")
    assert R.conditioned(want, float(np.abs(got["coef"] - want["coef"]).max()))
    assert [[f for f, _ in exp.local_exp[l]] for l in exp.top_labels] == want["order"].tolist()
    _, mask = exp.get_image_and_mask(exp.top_labels[0], positive_only=True, hide_rest=False)
    np.testing.assert_array_equal(mask, R.mask_of(seg, want["order"][0], want["coef"][0]))
    np.testing.assert_array_equal(mask, g[f"{tag}_mask"])                      # and, the case being well conditioned, the reference's own


def test_get_lime_attr_is_the_references_call(L, model, monkeypatch):
    """limeAttr.get_lime_attr: numpy's global RandomState (seed draw, then the matrix), 1000 samples, top 5, hide colour 0; the
    segmenter is replaced, skimage not being needed by any test."""
    c = R.golden_case(load_golden("lime.npz"), "a")
    seg = c["seg"].astype(np.int64)
    seen = []
    monkeypatch.setattr(L, "quickshift_segments", lambda image, random_seed: (seen.append(random_seed), seg)[1])
    np.random.seed(21)
    got = L.get_lime_attr(c["image"], model, DEV)
    np.random.seed(21)
    assert seen == [np.random.randint(0, high=1000)]
    np.random.seed(21)
    exp = L.LimeImageExplainer().explain_instance(c["image"], L.batch_predict, model, DEV, top_labels=5, hide_color=0, num_samples=1000,
                                                  segmentation_fn=lambda im: seg)
    _, mask = exp.get_image_and_mask(exp.top_labels[0], positive_only=True, hide_rest=False)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 40, 36) and not got.is_cuda
    np.testing.assert_array_equal(got.numpy(), np.broadcast_to(mask, (3, 40, 36)).astype(np.float32))
    assert exp.details.data[0].shape == (1000, c["D"]) and mask.sum() > 0


@functools.lru_cache(maxsize=None)
def _harness_inputs():
    rng = np.random.default_rng(60)
    seg = R.voronoi_labels(224, 224, 60, rng).astype(np.int64)
    yy, xx = np.mgrid[0:224, 0:224]
    img = np.stack([0.5 + 0.4 * np.sin(yy / 17.0 + c) * np.cos(xx / 23.0 - c) for c in range(3)]).astype(np.float32)
    img = np.clip(img + 0.1 * (rng.random(img.shape).astype(np.float32) - 0.5), 0, 1)
    return seg, torch.from_numpy(img)


def _testing_dict(model, seg, **extra):
    return dict(models=[model], batch_size=50, img_hw=224, device=DEV, attr_func="lime", lime_segments=lambda im: seg,
                lime_random_state=np.random.RandomState(7), **extra)


def test_harness_row(L, model):
    """get_CNN_attr(..., attr_func="lime") at 224 x 224 with N = 1000 and about 60 Voronoi superpixels: the host map and the device
    map are equal, {0, 3}-valued, and the restatement's mask x 3 for the probabilities the engine saw."""
    from xai_engine.sweep import get_CNN_attr
    seg, trans = _harness_inputs()
    D = int(seg.max()) + 1
    assert 50 <= D <= 60
    x = trans[None]                                          # the row perturbs trans_img; input_tensor only has to be there
    calls = []

    def segments(im):
        calls.append(im)
        return seg
    td = _testing_dict(model, seg)
    td["lime_segments"] = segments
    host = get_CNN_attr(x, trans, 0, td)
    dev = get_CNN_attr(x, trans, 0, _testing_dict(model, seg, device_maps=True))
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.shape == (224, 224)
    assert torch.is_tensor(dev) and dev.is_cuda
    np.testing.assert_array_equal(host, dev.cpu().numpy())
    assert set(np.unique(host).tolist()) == {0.0, 3.0}
    assert calls[0].shape == (224, 224, 3) and np.array_equal(calls[0], trans.permute(1, 2, 0).numpy())
    out, det = L.lime_batch(trans[None].to(DEV), model, lambda im, seed: seg, num_samples=1000, top_labels=5, hide_color=0,
                            random_state=np.random.RandomState(7), want="details")
    np.testing.assert_array_equal(out[0].cpu().numpy(), host)
    rs = np.random.RandomState(7)
    rs.randint(0, high=1000)
    np.testing.assert_array_equal(det.data[0], L.draw_data(rs, 1000, D))
    want = R.explain(det.data[0], det.labels[0].cpu().numpy())
    got_coef = det.coef[0, :, :D].cpu().numpy()
    check("lime_harness/coef", got_coef, want["coef"], BAR, against="restated LIME")
    assert R.conditioned(want, float(np.abs(got_coef - want["coef"]).max()))
    np.testing.assert_array_equal(det.order[0, :, :D].cpu().numpy(), want["order"])
    np.testing.assert_array_equal(host, 3.0 * R.mask_of(seg, want["order"][0], want["coef"][0]))
    weights = L.lime_batch(trans[None].to(DEV), model, seg, num_samples=1000, data=det.data, want="weights")
    np.testing.assert_array_equal(weights[0].cpu().numpy(), got_coef[0].astype(np.float32)[seg])


def test_harness_row_needs_trans_img(model):
    from xai_engine.sweep import get_CNN_attr
    seg, trans = _harness_inputs()
    with pytest.raises(ValueError, match="trans_img"):
        get_CNN_attr(trans[None], None, 0, _testing_dict(model, seg))


def test_second_call_replays_the_captured_pass(L, model):
    """With graphs on, the harness row's one pass size is captured once per thread and model: a further call only replays."""
    seg, trans = _harness_inputs()
    x = trans[None].to(DEV)
    kw = dict(num_samples=300, top_labels=5, hide_color=0, random_state=3)
    first = L.lime_batch(x, model, seg, **kw)
    before = dict(L.LIME_COUNTS)
    second = L.lime_batch(x, model, seg, **kw)
    assert L.LIME_COUNTS["captures"] == before["captures"] and L.LIME_COUNTS["captures_refused"] == before["captures_refused"] == 0
    assert L.LIME_COUNTS["replayed"] == before["replayed"] + 3 and L.LIME_COUNTS["eager"] == before["eager"]
    assert L.LIME_COUNTS["rows"] == before["rows"] + 300
    assert torch.equal(first, second)
    eager = L.lime_batch(x, model, seg, graphs=False, **kw)
    assert L.LIME_COUNTS["eager"] == before["eager"] + 3
    assert torch.equal(first, eager)
