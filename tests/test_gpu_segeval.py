"""The segmentation-evaluation kernels K44-K45 (csrc/seg_kernels.hip) at their edges against tests/seg_restated.py and torch's CPU
expressions, the drivers of xai_engine/segeval.py against the reference-made golden file, and evaluate_imagenet_seg end to end on a
small CNN and a small ViT.

Bounds: everything is compared exactly.  K44's map is torch's CPU expression by == (a NaN by position); its threshold is
fp32(math.fsum(out) / hw) bit for bit: the kernel's fp64 tree and the exactly rounded sum differ by a few fp64 ulps, which moves the
fp32 rounding only on a double-rounding boundary (about one seed in 2^27); none of the fixed seeds below lands on one.  K45's table
is integers."""
import math

import numpy as np
import pytest
import torch

import seg_restated as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


def _offset(a, by):
    """the array on the device, its first element `by` elements past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[by:by + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * by) % 16
    return view


def _nan_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and bool((got[~gn] == want[~wn]).all())


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------------------------------------ K44
KINDS = ("random", "nan", "plus_inf", "minus_inf", "constant", "zeros")


def _k44_map(kind, hw, rng):
    x = rng.standard_normal(hw).astype(np.float32)
    at = hw // 2
    if kind == "nan":
        x[at] = np.nan
    elif kind == "plus_inf":
        x[at] = np.inf
    elif kind == "minus_inf":
        x[at] = -np.inf
    elif kind == "constant":
        x[:] = 2.5
    elif kind == "zeros":                                # -0 and +0 are the minimum; either may come back
        x = np.abs(x)
        x[::2] = 0.0
        x[1::4] = -0.0
    return x


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 63, 64, 65, 255, 257, 50176])
def test_k44_normalize_and_stated_mean(K, hw, n):
    rng = np.random.default_rng(1000 * n + hw)
    for j, kind in enumerate(KINDS):
        x = np.stack([_k44_map(KINDS[(j + m) % len(KINDS)] if m else kind, hw, rng) for m in range(n)])
        t = torch.from_numpy(x)
        want = torch.stack([(r - r.min()) / (r.max() - r.min()) for r in t]).numpy()       # torch's CPU expression, per map
        want_stats = np.stack([[r.min().item(), r.max().item()] for r in t]).astype(np.float32)
        want_thr = np.array([np.float32(math.fsum(r.astype(np.float64)) / hw) for r in want], np.float32)
        for by in (0, 1):                                # 16-byte aligned, and one element past (scalar accesses)
            xd = _offset(x, by)
            out, thr, stats = K.seg_normalize(xd)
            torch.cuda.synchronize()
            assert _nan_equal(out.cpu().numpy(), want), (kind, hw, n, by)
            assert _nan_equal(stats.cpu().numpy(), want_stats), (kind, by)
            got_thr = thr.cpu().numpy()
            print(f"K44 {kind} hw={hw} n={n} offset={by}: thr {got_thr.tolist()} want {want_thr.tolist()}")
            assert np.array_equal(np.isnan(got_thr), np.isnan(want_thr))
            assert _bits(got_thr[~np.isnan(got_thr)]) == _bits(want_thr[~np.isnan(want_thr)]), (kind, hw, n, by)
            assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True)                   # the input is untouched
        # the tree of the header, restated: the same bits before the fp32 rounding could hide a difference
        stated = np.array([R.stated_mean(r) for r in want], np.float32)
        assert np.array_equal(np.isnan(stated), np.isnan(got_thr)) and _bits(stated[~np.isnan(stated)]) == _bits(got_thr[~np.isnan(got_thr)])
    xd = _offset(x, 0)                                   # in place: out may be x
    out, thr2, _ = K.seg_normalize(xd, out=xd)
    assert out.data_ptr() == xd.data_ptr() and _nan_equal(xd.cpu().numpy(), want) and _nan_equal(thr2.cpu().numpy(), got_thr)


def test_k44_wrapper_checks(K):
    with pytest.raises(ValueError):
        K.seg_normalize(torch.zeros(4, device=DEV))
    with pytest.raises(TypeError):
        K.seg_normalize(torch.zeros((2, 4), device=DEV, dtype=torch.float64))
    from xai_engine._lib import XaiHipError
    with pytest.raises(XaiHipError):
        K.seg_normalize(torch.zeros((2, 4)))


# ------------------------------------------------------------------------------------------------ K45
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 12, 16])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 64), (3, 63), (2, 65), (5, 257), (224, 224)])
def test_k45_counts_equal_the_restatement(K, H, W, T, n):
    rng = np.random.default_rng(H * 100000 + W * 100 + T * 3 + n)
    size = H * W
    res = rng.random((n, H, W), dtype=np.float32)
    labels = (rng.random((n, H, W)) < 0.4).astype(np.int32)
    thr = rng.random((n, T), dtype=np.float32)
    if size >= 7:
        res.reshape(n, -1)[:, 3::7] = np.nan             # NaN pixels: state 2
    eq = size // 3 + (1 if size >= 7 and (size // 3 - 3) % 7 == 0 else 0)
    thr[0, 0] = res[0].flat[eq]                          # a pixel exactly equal to a threshold: state 0 (<=)
    if T >= 12:
        thr[:, 3], thr[:, 4], thr[:, 5] = np.nan, np.inf, -np.inf
    elif n == 3:
        thr[1, 0], thr[2, 0] = np.nan, np.inf
    if n == 3 or size > 1:                               # labels that are neither 0 nor 1, in the last map
        labels[-1].flat[size // 2] = 2
        labels[-1].flat[size - 1] = -1
    rd, ld, td = _offset(res, 1), _offset(labels, 3), _offset(thr, 1)                    # unaligned slices
    counts, other = K.seg_counts(rd, ld, td)
    counts2, other2 = K.seg_counts(rd, ld, td)
    torch.cuda.synchronize()
    got, got_other = counts.cpu().numpy(), other.cpu().numpy()
    assert got.shape == (n, T, H, 2, 3) and got.dtype == np.int32
    assert _bits(got) == _bits(counts2.cpu().numpy()) and _bits(got_other) == _bits(other2.cpu().numpy())
    for m in range(n):
        want, want_other = R.count_table(res[m], labels[m], thr[m])
        assert np.array_equal(got[m], want), (m, np.argwhere(got[m] != want)[:4])
        assert got_other[m] == want_other
        row_other = ((labels[m] != 0) & (labels[m] != 1)).sum(1)
        assert (got[m].sum((2, 3)) == (W - row_other)[None, :]).all()
    if size > 1:
        assert got_other[-1] == (1 if size // 2 == size - 1 else 2)
    r, c = divmod(eq, W)                                 # the pixel equal to its threshold sits in the <= column
    assert res[0, r, c] == thr[0, 0]
    if labels[0, r, c] in (0, 1):
        alone = R.count_table(res[0, r:r + 1, c:c + 1], labels[0, r:r + 1, c:c + 1], thr[0, :1])[0]
        assert alone[0, 0, labels[0, r, c], 0] == 1 and got[0, 0, r, labels[0, r, c], 0] >= 1


def test_k45_wrapper_checks(K):
    res = torch.zeros((2, 4, 4), device=DEV)
    lab = torch.zeros((2, 4, 4), device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError):
        K.seg_counts(res, lab, torch.zeros((3, 1), device=DEV))
    with pytest.raises(ValueError):
        K.seg_counts(res, lab[:1], torch.zeros((2, 1), device=DEV))
    with pytest.raises(TypeError):
        K.seg_counts(res, lab.long(), torch.zeros((2, 1), device=DEV))
    from xai_engine._lib import XaiHipError
    with pytest.raises(XaiHipError, match="-3"):
        K.seg_counts(res, lab, torch.zeros((2, 17), device=DEV))


# ------------------------------------------------------------------------------------------------ the drivers and the golden file
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def golden_cases():
    return [(f"{kind}{seed}",) + R.seeded_case(kind, seed) for kind, seed in R.CASES]


def test_eval_batch_device_equals_the_golden_bit_for_bit(golden_cases):
    from xai_engine import segeval
    g = load_golden("seg.npz")
    maps = torch.from_numpy(np.stack([x for _, x, _ in golden_cases])).to(DEV)
    labels = np.stack([l for _, _, l in golden_cases])
    scores, res, thr = segeval.eval_batch_device(maps, labels, want_maps=True)
    thr = thr.cpu().numpy()
    for i, (tag, x, _) in enumerate(golden_cases):
        assert _nan_equal(res[i].cpu().numpy(), R.normalize(x))
        # the stated mean may differ from torch's own by the golden's `cond`; the stored cases are cut identically by both
        assert np.isnan(thr[i, 0]) == np.isnan(g[f"{tag}_ret"]) and not abs(np.float64(thr[i, 0]) - np.float64(g[f"{tag}_ret"])) > g["cond"]
        for name in ("correct", "labeled", "inter", "union", "ap", "f1"):
            assert _same(getattr(scores[i], name), g[f"{tag}_{name}"]), (tag, name)
    fold = segeval.SegFold()
    for s in scores:
        fold.add(s)
    assert _same(np.array(fold.numbers(), np.float64), g["fold_numbers"]) and fold.lines() == [l.decode() for l in g["fold_lines"]]
    bad = labels.copy()
    bad[2, 5, 5] = 2
    with pytest.raises(ValueError, match="map 2 has 1 pixels"):
        segeval.eval_batch_device(maps, bad)


def test_eval_batch_keeps_the_references_signature_and_tuple(golden_cases):
    from xai_engine import segeval
    g = load_golden("seg.npz")
    for tag, x, labels in golden_cases[:1] + golden_cases[3:4]:          # a smooth map, and the constant one (all NaN)
        Res = torch.from_numpy(R.normalize(x)).reshape(1, 1, R.HW, R.HW).to(DEV)
        ret = torch.tensor(g[f"{tag}_ret"])
        lab = torch.from_numpy(labels)[None]
        out = segeval.eval_batch(Res, ret, lab)
        assert len(out) == 8
        correct, labeled, inter, union, ap, f1, pred, target = out
        for got, name in zip(out[:6], ("correct", "labeled", "inter", "union", "ap", "f1")):
            assert _same(got, g[f"{tag}_{name}"]), (tag, name)
        assert isinstance(correct, np.int64) and inter.shape == (2,) and ap.shape == (1,) and f1.shape == (R.HW,)
        assert pred.shape == (R.HW * R.HW,) and pred.dtype == np.float32 and target.shape == (R.HW * R.HW,) and target.dtype == np.int64
        assert not torch.isnan(Res).any()                                # zeroed in place, after the masks were taken
        host = torch.from_numpy(R.normalize(x)).reshape(1, 1, R.HW, R.HW)
        host[host != host] = 0
        assert _nan_equal(pred, (host.clamp(min=0) / host.max()).view(-1).numpy())


def test_best_threshold_sweeps_twelve_thresholds_in_one_launch(golden_cases):
    from xai_engine import segeval
    _, x, labels = golden_cases[0]
    Res = torch.from_numpy(R.normalize(x)).reshape(1, 1, R.HW, R.HW).to(DEV)
    scaled, best, iou = segeval.best_threshold(Res, labels[None])
    host = scaled.cpu().numpy().reshape(R.HW, R.HW)
    table, _ = R.count_table(host, labels, segeval.fp32_thresholds(segeval.MAG_VALS))
    want = []
    for t in range(12):
        s = segeval.scores_from_counts(table[t])
        want.append(np.mean(np.float64(1.0) * s.inter / (np.spacing(1, dtype=np.float64) + s.union)))
    assert _same(iou, np.array(want)) and best == segeval.MAG_VALS[int(np.argmax(want))]
    assert torch.equal(scaled, Res / Res.mean() * 0.5)


# ------------------------------------------------------------------------------------------------ end to end
def _frozen(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(DEV).eval()


def _loader(count, hw, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hw, 0:hw] / hw
    for _ in range(count):
        image = torch.from_numpy(rng.random((1, 3, hw, hw), dtype=np.float32))
        cy, cx, rad = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.15, 0.3)
        yield image, torch.from_numpy((((yy - cy) ** 2 + (xx - cx) ** 2) < rad ** 2).astype(np.int64))[None]


@pytest.mark.parametrize("model_name,attr_func", [("R50", "grad"), ("R50", "gc"), ("VIT16", "attn")])
def test_evaluate_imagenet_seg_end_to_end(tmp_path, model_name, attr_func):
    pytest.importorskip("sklearn")
    from xai_engine import harness, segeval
    from xai_engine.zoo import VisionTransformer, resnet50
    hw = 64
    if model_name == "R50":
        model, norm = resnet50(seed=0, width=8, num_classes=10), (harness.CNN_MEAN, harness.CNN_STD)
    else:
        torch.manual_seed(0)
        model, norm = VisionTransformer(img=hw, patch=16, dim=32, depth=2, heads=4, num_classes=10), (harness.VIT_MEAN, harness.VIT_STD)
    model = _frozen(model)
    td = {"models": [model, model], "img_hw": hw, "batch_size": 25, "device": DEV, "attr_func": attr_func, "normalize": norm,
          "model_name": model_name, "image_count": 3, "num_patches": 4}
    files, maps = [], []
    for batch, keep in ((1, None), (32, maps)):
        out = tmp_path / f"out{batch}"
        numbers = segeval.evaluate_imagenet_seg(dict(td, segmentation_dataloader=_loader(3, hw, 9)), out_dir=str(out), batch=batch,
                                                keep_maps=keep)
        files.append(open(out / model_name / f"{attr_func}_3_images").read())
    assert files[0] == files[1] and len(maps) == 3 and len(numbers) == 4
    # the restated host flow (sklearn) on the very maps that were scored
    rows = []
    for m, lab in maps:
        assert m.is_cuda and m.shape == (hw, hw) and m.dtype == torch.float32
        res = R.normalize(m.cpu().numpy())
        rows.append(R.host_scores(res, R.stated_mean(res), lab.cpu().numpy()))
    want_numbers, want_lines = R.fold(rows)
    assert files[1].splitlines(keepends=True) == want_lines
    assert _same(np.array(numbers, np.float64), np.array(want_numbers, np.float64))
    with pytest.raises(NotImplementedError, match="t_attr"):
        segeval.evaluate_imagenet_seg(dict(td, model_name="VIT16", attr_func="t_attr", segmentation_dataloader=[]))


def test_vit_maps_take_no_abs_after_the_resize(K):
    """the seg script resizes the patch map and normalises it as it is; the sweep's get_VIT_attr fuses an abs into its resize"""
    from xai_engine import segeval, sweep
    from xai_engine.zoo import VisionTransformer
    hw = 64
    torch.manual_seed(0)
    model = _frozen(VisionTransformer(img=hw, patch=16, dim=32, depth=2, heads=4, num_classes=10))
    td = {"models": [model, model], "img_hw": hw, "device": DEV, "attr_func": "grad", "num_patches": 4}
    x = torch.randn(1, 3, hw, hw)
    patch = sweep.vit_patch_map(x, torch.tensor(1), td)
    got = segeval._attribution_map(x, None, torch.tensor(1), td, True, torch.device(DEV))
    assert torch.equal(got, K.bilinear_up(patch, hw, hw, scale=1.0, take_abs=False)[0].reshape(hw, hw))
    assert np.array_equal(sweep.get_VIT_attr(x, None, torch.tensor(1), td), got.abs().cpu().numpy())
    assert sweep.vit_patch_map(x, torch.tensor(1), dict(td, attr_func="VIT_CX")) is None
