"""The sanity-test kernels K39-K43 (csrc/sanity_kernels.hip) at their edges against tests/sanity_restated.py (NumPy and scipy
alone), the drivers get_sanity / get_sanity_batch, and evaluate_sanity end to end on a small CNN and a small ViT.

Bounds: K39, the S map of K40 and the Spearman values are compared bit for bit (a NaN by position).  K40's mean may differ from
the restatement's by two fp64 summation orders of the same fp32 values: 2 N 2^-53 mean|S| over the N interior pixels.  K43's
features are fp32 roundings of fp64 values whose last bits depend on libm against the device's atan2 / hypot and on the
summation order: two fp32 ulps of 1.0, 2.4e-7 absolute; a flipped bin shows at 1e-4 or more."""
import copy
import csv

import numpy as np
import pytest
import torch
from scipy.stats import rankdata

import sanity_restated as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HOG_TOL = 2.4e-7


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    """equal bit for bit, a NaN matching a NaN at the same place"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


# ------------------------------------------------------------------------------------------------ K39
def _normalize_inputs(count, rng):
    rand = rng.standard_normal(count).astype(np.float32)
    out = {"random": rand, "constant": np.full(count, 2.5, np.float32)}
    for name, v in (("plus_inf", np.inf), ("minus_inf", -np.inf), ("nan", np.nan)):
        x = rand.copy()
        x[count // 2] = v
        out[name] = x
    z = np.zeros(count, np.float32)                      # Inf values whose removal leaves a constant map
    z[::3] = np.inf
    z[count - 1] = -np.inf
    out["inf_over_constant"] = z
    return out


@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 50176])
def test_k39_normalize_is_the_references_bit_for_bit(K, count, guard):
    cases = _normalize_inputs(count, np.random.default_rng(count))
    x = np.stack(list(cases.values()))
    got = K.sanity_normalize(_dev(x), guard=guard).cpu().numpy()
    for i, name in enumerate(cases):
        want = R.normalize_image(x[i], guard=guard)
        assert _same_bits(got[i], want), (name, count, guard)
    if count % 4:                                        # one map alone
        assert _same_bits(K.sanity_normalize(_dev(x[:1]), guard=guard).cpu().numpy()[0], got[0])


# ------------------------------------------------------------------------------------------------ K40
def _ssim_shapes(K):
    T = K.ssim_tile()
    return [(11, 11), (12, 17), (T - 1, T), (T, T + 1), (T + 1, T - 1), (224, 224)]


def _ssim_pairs(H, W, rng):
    a, b = rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32)
    nan = a.copy()
    nan[H // 2, W // 3] = np.nan
    x = np.stack([a, a, np.full((H, W), 0.25, np.float32), nan])
    y = np.stack([b, a.copy(), b, b])
    return x, y                                          # random / equal maps / a constant map / a map with a NaN


def _check_ssim(K, x, y, tag):
    mean, S = K.ssim(_dev(x), _dev(y), data_range=2.0, want_map=True)
    mean2, S2 = K.ssim(_dev(x), _dev(y), data_range=2.0, want_map=True)
    assert torch.equal(mean.view(torch.int64), mean2.view(torch.int64)) and torch.equal(S.view(torch.int32), S2.view(torch.int32)), tag
    assert torch.equal(K.ssim(_dev(x), _dev(y)).view(torch.int64), mean.view(torch.int64)), tag       # without the map
    mean, S = mean.cpu().numpy(), S.cpu().numpy()
    for i in range(x.shape[0]):
        want_mean, want_S = R.ssim(x[i], y[i], 2.0)
        assert _same_bits(S[i], want_S), (tag, i)
        inner = want_S[5:-5, 5:-5].astype(np.float64)
        bound = 2 * inner.size * 2.0 ** -53 * np.abs(inner).mean()
        err = abs(mean[i] - want_mean)
        print(f"ssim {tag} pair {i}: mean {mean[i]!r} want {want_mean!r} err {err:.3e} bound {bound:.3e}")
        assert (np.isnan(want_mean) and np.isnan(mean[i])) or err <= bound, (tag, i, err, bound)


@pytest.mark.parametrize("shape_index", range(6))
def test_k40_ssim_map_is_skimages_bit_for_bit_and_the_mean_within_two_summation_orders(K, shape_index):
    H, W = _ssim_shapes(K)[shape_index]
    x, y = _ssim_pairs(H, W, np.random.default_rng(100 + shape_index))
    _check_ssim(K, x[:3], y[:3], f"{H}x{W} B=3")
    _check_ssim(K, x[3:], y[3:], f"{H}x{W} B=1 nan")
    assert np.isnan(K.ssim(_dev(x[3:]), _dev(y[3:])).cpu().numpy()).all()
    if (H, W) == (11, 11):
        _check_ssim(K, x[:1], y[:1], "11x11 B=1")
        assert abs(float(K.ssim(_dev(x[1:2]), _dev(y[1:2]))[0]) - 1.0) <= 1e-6       # equal maps


def test_k40_refuses_maps_below_the_window(K):
    from xai_engine import _lib
    x = torch.zeros(1, 10, 40, device=DEV)
    with pytest.raises(ValueError, match="11 x 11"):
        K.ssim(x, x)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    code = _lib.load("ext2").xai_ssim_f32(x.data_ptr(), x.data_ptr(), 1, 10, 40, *K.ssim_weights(), 1e-4, 1e-3, out.data_ptr(), None,
                                         ws.data_ptr(), 64, None)
    assert code == -2                                    # XAI_E_SHAPE, where skimage raises


# ------------------------------------------------------------------------------------------------ K41 + K42
def _rank_pairs(n, rng):
    """seven kinds of rows a, each against a row b of the same kind drawn again"""
    def kinds(r):
        cont = r.standard_normal(n).astype(np.float32)
        relu = np.maximum(r.standard_normal(n), 0).astype(np.float32)          # about half exact zeros
        halves = (np.round(r.standard_normal(n) * 4) / 2).astype(np.float32)
        zeros = cont.copy()
        zeros[::2] = 0.0
        zeros[1::4] = -0.0                                                      # -0 next to +0: one tie group
        infs = cont.copy()
        infs[0] = np.inf
        infs[n - 1] = -np.inf
        if n > 4:
            infs[n // 2] = np.inf
        nan = cont.copy()
        nan[n // 2] = np.nan
        return [cont, relu, halves, zeros, infs, nan]
    a, b = kinds(rng), kinds(rng)
    a.append(np.full(n, 1.5, np.float32))                # all equal: one tie group over the whole row, a NaN correlation
    b.append(rng.standard_normal(n).astype(np.float32))
    return np.stack(a), np.stack(b)


def _spearman_device(K, a, b):
    both = _dev(np.concatenate([a, b]))
    order, _ = K.rank(both)
    r2 = K.tie_ranks(both, order)
    B = a.shape[0]
    return K.rank_corr(r2[:B], r2[B:], both[:B], both[B:]).cpu().numpy(), r2.cpu().numpy()


def _rank_sizes(K):
    T = K.tie_ranks_chunk()
    return [2, 3, 63, 64, 65, T - 1, T + 1, 11664, 50176]


@pytest.mark.parametrize("size_index", range(9))
def test_k41_k42_spearman_is_scipys_bit_for_bit(K, size_index):
    n = _rank_sizes(K)[size_index]
    a, b = _rank_pairs(n, np.random.default_rng(n))
    got, r2 = _spearman_device(K, a, b)
    rows = np.concatenate([a, b])
    for i in range(rows.shape[0]):
        if not np.isnan(rows[i]).any():
            assert np.array_equal(r2[i], (2 * rankdata(rows[i])).astype(np.int64)), (n, i)       # exact integers
    want = np.array([R.spearman(a[i], b[i]) for i in range(a.shape[0])])
    assert np.isnan(want[5]) and np.isnan(want[6])       # the NaN row and the constant row
    assert _same_bits(got, want), (n, got, want)
    got1, _ = _spearman_device(K, a[:1], b[:1])          # one pair alone
    assert _same_bits(got1, want[:1])


@pytest.mark.parametrize("n_off", [1, 50176])
def test_k41_tie_groups_that_straddle_a_chunk_and_cover_the_row(K, n_off):
    T = K.tie_ranks_chunk()
    n = T + 1 if n_off == 1 else n_off
    rng = np.random.default_rng(7)
    a = rng.permutation(n).astype(np.float32)
    a[(a >= T - 3) & (a <= T + 3)] = T                   # sorted positions T-3 .. T+3 (or to the row's end) hold one value
    big = rng.permutation(n).astype(np.float32)
    big[(big >= 5) & (big < n - 5)] = 7.0                # one group over nearly the whole row, across every chunk
    whole = np.full(n, -2.0, np.float32)
    rows = np.stack([a, big, whole])
    t = _dev(rows)
    order, _ = K.rank(t)
    r2 = K.tie_ranks(t, order).cpu().numpy()
    for i in range(3):
        assert np.array_equal(r2[i], (2 * rankdata(rows[i])).astype(np.int64)), i
    assert (r2[2] == n + 1).all()
    b = rng.standard_normal((3, n)).astype(np.float32)
    got, _ = _spearman_device(K, rows, b)
    assert _same_bits(got, np.array([R.spearman(rows[i], b[i]) for i in range(3)]))


def test_k42_refuses_rows_above_its_limit_and_the_driver_still_answers_as_scipy(K):
    from xai_engine import _lib, sanity
    n = K.rank_corr_max_n() + 1
    assert n == 131073
    r = torch.zeros(1, n, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.XaiHipError, match="code -3"):
        K.rank_corr(r, r)
    rng = np.random.default_rng(11)
    a = np.maximum(rng.standard_normal((1, n)), 0).astype(np.float32)
    b = rng.standard_normal((1, n)).astype(np.float32)
    got = sanity.spearman_batch(_dev(a), _dev(b))
    assert got.is_cuda and got.dtype == torch.float64
    assert _same_bits(got.cpu().numpy(), np.array([R.spearman(a[0], b[0])]))


# ------------------------------------------------------------------------------------------------ K43
def _step_image(H, W):
    """axis-aligned steps: orientations exactly 0 and 90 degrees (and 180 -> 0 on the falling edges), cells without a gradient"""
    img = np.zeros((H, W), np.float32)
    img[: H // 3, W // 2:] = 1.0
    img[2 * H // 3:, : W // 4] = 0.5
    return img


HOG_CASES = [(48, 48, (16, 16)), (50, 70, (16, 16)), (24, 40, (8, 8)), (224, 224, (16, 16))]


@pytest.mark.parametrize("H,W,cell", HOG_CASES)
def test_k43_hog_features_and_their_correlation(K, H, W, cell):
    from xai_engine import sanity
    rng = np.random.default_rng(H * W)
    imgs = np.stack([rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32), _step_image(H, W)])
    for img in imgs[:2]:                                 # the comparison cannot hide a bin flip behind the input
        mag, ori = R.hog_gradients(img)
        # the border rows and columns have one gradient component exactly 0, so their orientation is exactly 0 or 90 on both
        # sides (atan2 of an exact zero; the step image below is made of these); every other orientation stays clear of the edges
        free = ori[(mag > 0) & (ori != 0.0) & (ori != 90.0)]
        assert free.size > 0.9 * (H - 2) * (W - 2)
        to_edge = np.abs(free[:, None] - 20.0 * np.arange(10)[None, :]).min()
        assert to_edge >= 1e-9, to_edge
    mag, ori = R.hog_gradients(imgs[2])
    assert set(np.unique(ori[mag > 0])) >= {0.0, 90.0} and (mag == 0).mean() > 0.5
    feat = K.hog(_dev(imgs), cell)
    assert torch.equal(feat, K.hog(_dev(imgs), cell))    # bit-identical repeats
    got = feat.cpu().numpy()
    assert got.shape == (3, R.hog_length(H, W, cell))
    for i in range(3):
        want = R.hog(imgs[i], cell)
        err = np.abs(got[i].astype(np.float64) - want).max()
        print(f"hog {H}x{W} cell {cell} image {i}: max abs err {err:.3e}")
        assert err <= HOG_TOL, (i, err)
    # the correlation of the device's own vectors: scipy's, bit for bit
    corr = sanity.spearman_batch(feat[:2].contiguous(), feat[1:].contiguous()).cpu().numpy()
    assert _same_bits(corr, np.array([R.spearman(got[0], got[1]), R.spearman(got[1], got[2])]))


def test_k43_refuses_fewer_than_three_cells(K):
    with pytest.raises(ValueError, match="fewer than 3 cells"):
        K.hog(torch.zeros(1, 47, 64, device=DEV))


# ------------------------------------------------------------------------------------------------ the drivers
def _compare_with_restatement(vals, a, b, tag, guard=True):
    """vals = (SSIM, SPR, HOG) of the maps a, b (host fp32, (H, W)): SSIM within K40's bound, SPR exactly, HOG exactly scipy's on
    the device's own features, which are within K43's bound of the restated ones"""
    from xai_engine import kernels as Kk
    an, bn = R.normalize_image(a, guard), R.normalize_image(b, guard)
    want_ssim, S = R.ssim(an, bn, 2.0)
    inner = S[5:-5, 5:-5].astype(np.float64)
    bound = 2 * inner.size * 2.0 ** -53 * np.abs(inner).mean()
    assert (np.isnan(want_ssim) and np.isnan(vals[0])) or abs(vals[0] - want_ssim) <= bound, (tag, vals[0], want_ssim, bound)
    assert _same_bits(np.float64(vals[1]), np.float64(R.spearman(a, b))), (tag, vals[1])
    feat = Kk.hog(_dev(np.stack([an, bn]))).cpu().numpy()
    for f, m in zip(feat, (an, bn)):
        assert np.array_equal(np.isnan(f), np.isnan(R.hog(m))) and np.nanmax(np.abs(f - R.hog(m)), initial=0.0) <= HOG_TOL, tag
    assert _same_bits(np.float64(vals[2]), np.float64(R.spearman(feat[0], feat[1]))), (tag, vals[2])
    print(f"sanity {tag}: {vals} restated HOG {R.spearman(R.hog(an), R.hog(bn))!r}")


def test_get_sanity_takes_device_tensors_and_numpy_arrays_alike():
    from xai_engine import sanity
    rng = np.random.default_rng(21)
    a = np.abs(rng.standard_normal((64, 64, 1))).astype(np.float32)
    b = np.maximum(rng.standard_normal((64, 64, 1)), 0).astype(np.float32)
    host = sanity.get_sanity(a, b)
    assert list(host) == ["SSIM", "SPR", "HOG"] and all(isinstance(v, float) for v in host.values())
    dev = sanity.get_sanity(_dev(a), _dev(b))
    flat = sanity.get_sanity(a[:, :, 0], b[:, :, 0], abs=True)
    assert host == dev == flat
    _compare_with_restatement([host[k] for k in sanity.KEYS], a[:, :, 0], b[:, :, 0], "get_sanity 64x64")
    batch = sanity.get_sanity_batch(_dev(np.stack([a[:, :, 0], b[:, :, 0]])), _dev(np.stack([b[:, :, 0], a[:, :, 0]])))
    assert all(t.is_cuda and t.dtype == torch.float64 and t.shape == (2,) for t in batch)
    assert [float(t[0]) for t in batch] == [host[k] for k in sanity.KEYS]
    # float64 maps whose values float32 cannot hold: SPR is scipy's on the dtype given
    a64 = a.astype(np.float64) + rng.standard_normal(a.shape) * 1e-12
    assert sanity.get_sanity(a64, b)["SPR"] == R.spearman(a64, b)
    # the mirrored module: K39 without the guard
    from util.test_methods import sanityForMethods as M
    assert M.evaluate(a, b) == (host["SSIM"], host["SPR"], host["HOG"])
    assert _same_bits(M.normalize_image(a), R.normalize_image(a, guard=False))
    assert np.isnan(M.normalize_image(np.full((4, 4), 2.0))).all()


def test_get_sanity_names_the_limit_for_several_channels():
    from xai_engine import sanity
    rng = np.random.default_rng(22)
    a, b = rng.random((48, 48, 3), dtype=np.float32), rng.random((48, 48, 3), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="3-channel"):
        sanity.get_sanity(a, b)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        sanity.get_sanity(a, b, abs=True)
    # the channels' SSIMs as separate pairs, averaged: normalize_image over the whole array, skimage's channel_axis=2
    an, bn = R.normalize_image(a), R.normalize_image(b)
    want = np.mean([R.ssim(np.ascontiguousarray(an[:, :, c]), np.ascontiguousarray(bn[:, :, c]), 2.0)[0] for c in range(3)])
    assert abs(sanity.get_ssim(a, b) - want) <= 2 * 38 * 38 * 2.0 ** -53


# ------------------------------------------------------------------------------------------------ end to end
def _write_images(tmp_path, count, hw, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i in range(count):
        name = f"ILSVRC2012_val_{i + 1:08d}.png"
        Image.fromarray((rng.random((hw + 6, hw + 10, 3)) * 255).astype(np.uint8)).save(tmp_path / name)
        names.append(name)
    return names


def _frozen(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(DEV).eval()


@pytest.mark.parametrize("model_name,attr_func", [("R50", "grad"), ("R50", "gc"), ("VIT16", "attn")])
def test_evaluate_sanity_end_to_end(tmp_path, monkeypatch, model_name, attr_func):
    from xai_engine import harness, sanity
    from xai_engine.zoo import VisionTransformer, resnet50
    hw = 64
    if model_name == "R50":
        base = resnet50(seed=0, width=8, num_classes=10)
        torch.manual_seed(5)
        rand = sanity.randomize_CNN_model(copy.deepcopy(base))
        norm = (harness.CNN_MEAN, harness.CNN_STD)
    else:
        torch.manual_seed(0)
        base = VisionTransformer(img=hw, patch=16, dim=32, depth=2, heads=4, num_classes=10)
        torch.manual_seed(5)
        rand = sanity.randomize_VIT_model(copy.deepcopy(base))
        norm = (harness.VIT_MEAN, harness.VIT_STD)
    base, rand = _frozen(base), _frozen(rand)
    names = _write_images(tmp_path, 3, hw, 9)
    monkeypatch.setattr(harness, "select_images", lambda td, cc, rank=0, world=1, lazy=False:
                        (names, harness.SelectedImages(str(tmp_path), names, hw, *norm), [0, 0, 0]))
    td = {"models": [base, base, rand, rand], "img_hw": hw, "batch_size": 25, "device": DEV, "attr_func": attr_func, "normalize": norm,
          "imagenet_dataset": str(tmp_path), "model_name": model_name, "image_count": 3, "num_patches": 4, "sanity_batch": 2}
    maps = []
    total, used, got_names = sanity.evaluate_sanity(td, out_dir=str(tmp_path / "out"), keep_maps=maps)
    assert used == 3 and got_names == names and list(total) == ["SSIM", "SPR", "HOG"] and len(maps) == 3
    rows = list(csv.reader(open(tmp_path / "out" / model_name / f"{attr_func}_3_images.csv")))
    assert [r[0] for r in rows] == ["SSIM", "SPR", "HOG", "Total Runtime"] and float(rows[3][1]) > 0
    assert [r[1] for r in rows[:3]] == [str(total[k] / 3) for k in sanity.KEYS]
    # every image's three values against the restated comparison of the maps the engine returned
    per_image = []
    for name, a, b in maps:
        assert a.is_cuda and a.shape == (hw, hw) and a.dtype == torch.float32
        vals = [float(t[0]) for t in sanity.get_sanity_batch(a[None], b[None])]
        _compare_with_restatement(vals, a.cpu().numpy(), b.cpu().numpy(), f"{model_name}/{attr_func}/{name}")
        per_image.append(vals)
    for j, k in enumerate(sanity.KEYS):                  # the sums are the plain sums of exactly these values
        assert _same_bits(np.float64(total[k]), np.float64(np.sum(np.asarray(per_image, np.float64)[:, j]))), k
    # the reference's fold over the same rows
    folded, used2, _ = sanity.evaluate_sanity(td, out_dir=str(tmp_path / "out2"), reference_counter=True)
    want = sanity.fold_reference_counter(per_image)
    assert used2 == 3 and list(folded) == list(want) and all(_same_bits(np.float64(folded[k]), np.float64(want[k])) for k in want)
