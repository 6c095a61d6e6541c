"""The segmentation evaluation without a GPU: the third extension header (include/xai_hip_ext3.h) and its library, the argument
checks K44 and K45 make before any HIP call, the host arithmetic of xai_engine/segeval.py against sklearn and against the
reference-made golden file (tests/golden/seg.npz), the fp32 thresholds of the MDA_dense sweep, the fold and the dataset readers."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import seg_restated as R
from abi_libs import PINNED, built, declared, exported, exported_elsewhere
from conftest import ROOT, load_golden

EXT3_HEADER = os.path.join(ROOT, "include", "xai_hip_ext3.h")
ENTRIES = ["xai_seg_counts_i32", "xai_seg_max_hw", "xai_seg_max_thresholds", "xai_seg_normalize_f32"]
_p, _i, _l = C.c_void_p, C.c_int, C.c_int64


# ------------------------------------------------------------------------------------------------ header and library
def test_ext3_header_parses_at_1_0_and_cites_the_reference():
    from xai_engine import _lib
    text = open(EXT3_HEADER).read()
    args, ret, version = _lib.parse_header(text, _lib.LIBRARIES["ext3"].defines)
    assert version == (1, 0) and (_lib.LIBRARIES["ext3"].version, _lib.LIBRARIES["ext3"].minor) == PINNED["ext3"] == (1, 0)
    assert sorted(args) == declared(EXT3_HEADER) == sorted(ENTRIES + ["xai_ext3_version", "xai_ext3_version_minor"])
    assert args["xai_seg_normalize_f32"] == [_p, _i, _l, _p, _p, _p, _p]
    assert args["xai_seg_counts_i32"] == [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p]
    assert all(t is _i for t in ret.values())
    listed = text[text.index(" *   0 = "):text.index("#define XAI_EXT3_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    for name in ENTRIES:
        if name.endswith(("_f32", "_f64", "_i32")):
            at = text.index(name + "(")
            comment = text[text.rfind("/*", 0, at):at]
            assert re.search(r"replaces\s+evaluateImageNetSeg\.py:\d+", comment), name
    assert re.search(r"metrices\.py:\d+", text[text.index("K45"):])


def test_ext3_library_exports_exactly_its_header_and_the_others_gained_nothing():
    from xai_engine import _lib
    assert exported(built("ext3")) == declared(EXT3_HEADER) == sorted(_lib.LIBRARIES["ext3"].signatures)
    lib = _lib.load("ext3")
    assert (lib.xai_ext3_version(), lib.xai_ext3_version_minor()) == (1, 0)
    assert lib.xai_seg_max_thresholds() == 16 and lib.xai_seg_max_hw() == 1 << 30
    # no other library carries an entry of this feature.  (`xai_seg_`, not a bare "seg": XRAI's xai_segment_sums_f32 and MDA's
    # xai_mda_max_segments have been in libxai_hip.so and libxai_ext2.so all along, and those libraries may not change.)
    elsewhere = exported_elsewhere("ext3")
    assert not [(o, n) for o, n in elsewhere if n.startswith("xai_seg_") or "ext3" in n]
    assert [(o, n) for o, n in elsewhere if "seg" in n] == [("hip", "xai_segment_sums_f32"), ("ext2", "xai_mda_max_segments")]


def test_k44_and_k45_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext3")
    lib = _lib.load("ext3")
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def norm(x=p, out=p, thr=p, stats=p, n=1, hw=64):
        return lib.xai_seg_normalize_f32(x, n, hw, out, thr, stats, None)
    assert [norm(**{k: None}) for k in ("x", "out", "thr", "stats")] == [-1] * 4
    assert [norm(n=0), norm(n=-1), norm(hw=0), norm(hw=(1 << 30) + 1)] == [-2, -2, -2, -3]

    def counts(res=p, labels=p, thr=p, out=p, other=p, n=1, H=4, W=4, T=1):
        return lib.xai_seg_counts_i32(res, labels, thr, n, H, W, T, out, other, None)
    assert [counts(**{k: None}) for k in ("res", "labels", "thr", "out", "other")] == [-1] * 5
    assert [counts(n=0), counts(H=0), counts(W=0), counts(T=0)] == [-2] * 4
    assert [counts(T=17), counts(n=65536), counts(H=1 << 16, W=1 << 15)] == [-3] * 3


# ------------------------------------------------------------------------------------------------ the host arithmetic
def _small_cases():
    """seeded 12 x 12 cases: NaN pixels, labels that are all 0 or all 1, thresholds outside [0, 1], a NaN threshold"""
    rng = np.random.default_rng(7)
    for i in range(40):
        res = rng.random((12, 12), dtype=np.float32)
        labels = (rng.random((12, 12)) < rng.choice([0.2, 0.5, 0.8])).astype(np.int64)
        thr = np.float32(rng.choice([0.5, res[3, 4], -0.25, 1.5, rng.random()]))
        if i % 5 == 1:
            res[rng.random((12, 12)) < 0.1] = np.nan
        if i % 8 == 2:
            labels[:] = 0
        if i % 8 == 5:
            labels[:] = 1
        if i == 13:
            thr = np.float32(np.nan)
        if i == 14:
            res[:] = np.nan
        if i % 10 == 7:
            labels[::2] = 0                  # rows without a positive: F1's 0 / 0
            res[::2] = 0.0
        yield res, labels, thr


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_scores_from_counts_equals_sklearn_on_the_expanded_arrays():
    pytest.importorskip("sklearn")
    from xai_engine import segeval
    seen_ap = set()
    for res, labels, thr in _small_cases():
        table, other = R.count_table(res, labels, [thr])
        assert other == 0 and (table[0].sum((1, 2)) == 12).all()
        got = segeval.scores_from_counts(table[0])
        correct, labeled, inter, union, ap, f1 = R.host_scores(res, thr, labels)
        assert got.correct == correct and got.labeled == labeled
        assert _same(got.inter, inter) and _same(got.union, union)
        assert _same(got.ap, np.array([ap])), (got.ap, ap)
        assert _same(got.f1, f1)
        seen_ap.add(float(ap))
    assert 0.5 in seen_ap and len(seen_ap) > 20


def test_scores_from_counts_equals_the_golden_cases():
    from xai_engine import segeval
    g = load_golden("seg.npz")
    for kind, seed in R.CASES:
        tag = f"{kind}{seed}"
        x, labels = R.seeded_case(kind, seed)
        res = R.normalize(x)
        stated = R.stated_mean(res)
        # the generator's condition: the stated mean cuts the map exactly where the reference's own mean does
        assert np.isnan(stated) == np.isnan(g[f"{tag}_ret"]) and not abs(np.float64(stated) - np.float64(g[f"{tag}_ret"])) > g["cond"]
        table, other = R.count_table(res, labels, [stated])
        got = segeval.scores_from_counts(table[0])
        assert other == 0
        for name in ("correct", "labeled", "inter", "union", "ap", "f1"):
            assert _same(getattr(got, name), g[f"{tag}_{name}"]), (tag, name)
    assert segeval.scores_from_counts(table[0]).f1.shape == (R.HW,)
    with pytest.raises(ValueError):
        segeval.scores_from_counts(np.zeros((4, 3, 2)))


def test_fold_reproduces_the_goldens_numbers_and_lines():
    from xai_engine import segeval
    g = load_golden("seg.npz")
    fold, rows = segeval.SegFold(), []
    for tag in (t.decode() for t in g["tags"]):
        s = segeval.SegScores(*(g[f"{tag}_{n}"] for n in ("correct", "labeled", "inter", "union", "ap", "f1")))
        fold.add(s)
        rows.append(tuple(s))
    assert _same(np.array(fold.numbers(), np.float64), g["fold_numbers"])
    assert fold.lines() == [l.decode() for l in g["fold_lines"]]
    numbers, lines = R.fold(rows)                                         # and the yardstick's own fold says the same
    assert _same(np.array(numbers, np.float64), g["fold_numbers"]) and lines == fold.lines()


def test_mag_thresholds_are_compared_in_fp32_as_torch_does():
    from xai_engine import segeval
    thr = segeval.fp32_thresholds(segeval.MAG_VALS)
    assert thr.dtype == np.float32 and len(thr) == 12
    rng = np.random.default_rng(3)
    res = rng.random((16, 16), dtype=np.float32)
    res.ravel()[:12] = thr                                               # a pixel equal to every fp32(v)
    res.ravel()[12:24] = np.nextafter(thr, np.float32(2))
    res[5, 5] = np.nan
    t = torch.from_numpy(res)
    for v, th in zip(segeval.MAG_VALS, thr):
        with np.errstate(invalid="ignore"):
            assert np.array_equal((res > th), t.gt(np.float64(v)).numpy()) and np.array_equal((res <= th), t.le(np.float64(v)).numpy())
        table, _ = R.count_table(res, np.ones((16, 16), np.int64), [th])
        assert table[0, :, 1, 1].sum() == int(t.gt(np.float64(v)).sum()) and table[0, :, 1, 2].sum() == 1
    assert not t.gt(np.float64(0.55))[0, 3] and np.float64(res[0, 3]) > 0.55      # fp32(0.55) > 0.55 in fp64, yet gt says False


# ------------------------------------------------------------------------------------------------ the dataset readers and the CLI
def test_npz_segmentation_round_trips(tmp_path):
    from PIL import Image
    from xai_engine import segeval
    rng = np.random.default_rng(5)
    data = {}
    for i, (h, w) in enumerate(((224, 224), (150, 301), (333, 250))):
        data[f"img_{i}"] = (rng.random((h, w, 3)) * 255).astype(np.uint8)
        data[f"gt_{i}"] = (rng.random((h, w)) < 0.4).astype(np.uint8)
    np.savez(tmp_path / "seg.npz", **data)
    ds = segeval.NpzSegmentation(str(tmp_path / "seg.npz"))
    assert len(ds) == 3
    image, labels = ds[0]                                                # already 224 x 224: both pass through unchanged
    assert image.dtype == torch.float32 and labels.dtype == torch.int64
    assert np.array_equal((image * 255).round().byte().permute(1, 2, 0).numpy(), data["img_0"]) and np.array_equal(labels.numpy(), data["gt_0"])
    for i in (1, 2):
        image, labels = ds[i]
        assert image.shape == (3, 224, 224) and labels.shape == (224, 224) and set(np.unique(labels)) <= {0, 1}
        want = torch.nn.functional.interpolate(torch.from_numpy(data[f"gt_{i}"])[None, None].float(), size=(224, 224), mode="nearest-exact")
        assert np.array_equal(labels.numpy(), want[0, 0].numpy().astype(np.int64))
        want = np.array(Image.fromarray(data[f"img_{i}"]).resize((224, 224), Image.BILINEAR))
        assert np.array_equal((image * 255).round().byte().permute(1, 2, 0).numpy(), want)
    batches = list(ds.loader(2))
    assert len(batches) == 2 and batches[0][0].shape == (1, 3, 224, 224) and batches[0][1].shape == (1, 224, 224)
    with pytest.raises(IndexError):
        ds[3]


def test_mat_segmentation_without_h5py_names_it(tmp_path, monkeypatch):
    from xai_engine import segeval
    monkeypatch.setitem(sys.modules, "h5py", None)                       # import h5py -> ImportError, installed or not
    with pytest.raises(ImportError, match="h5py"):
        segeval.MatSegmentation(str(tmp_path / "gtsegs_ijcv.mat"))


def test_cli_has_the_references_flags_and_refuses_by_name():
    from xai_engine import evaluate_imagenet_seg as cli, segeval
    opts = {a.dest for a in cli.build_parser()._actions}
    assert {"model", "image_count", "attr_func", "cuda_num", "dataset_path", "weights", "out_dir", "batch"} <= opts
    with pytest.raises(SystemExit, match="unknown --model CLIP16"):
        cli.main(["--model", "CLIP16"])
    for attr, word in (("t_attr", "relprop"), ("MDA_dense", "MASCalibrate")):
        with pytest.raises(NotImplementedError, match=attr):
            segeval.evaluate_imagenet_seg({"model_name": "VIT16", "attr_func": attr})
        assert word in segeval.REFUSED[attr]
    with pytest.raises(NotImplementedError, match="CLIP"):
        segeval.evaluate_imagenet_seg({"model_name": "CLIP16", "attr_func": "eclip"})
