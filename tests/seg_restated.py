"""The yardstick of the segmentation evaluation (xai_engine/segeval.py, K44-K45), written from the definitions: NumPy for the
normalisation, the stated mean tree and the count table; sklearn, called the way the evaluated script calls it, for the host flow.

A case is a (224, 224) raw attribution map and a label mask, rebuilt from a seed.  The host flow scores ONE image:
  masks      hi = res > thr, lo = res <= thr, both compared in fp32; a pixel in neither mask (NaN) has hi = lo = 0
  pixel acc  predicted class = argmax over (lo, hi) with the first index on a tie; correct = label-1 pixels predicted 1,
             labeled = label-1 pixels
  IoU        per class k: |pred == k and label == k| and |pred == k| + |label == k| - that
  AP         sklearn.metrics.average_precision_score on the 2 HW samples (label == 0, lo), (label == 1, hi)
  F1         sklearn.metrics.f1_score of every image ROW of hi against the row's labels (the evaluated script hands the H x W mask
             to a function that treats the first axis as a batch), NaN -> 0
and the fold adds the integers, keeps the AP and F1 arrays, and prints four lines.
"""
import warnings

import numpy as np

HW = 224
CASES = (("smooth", 11), ("smooth", 12), ("two", 21), ("const", 31), ("lab0", 41), ("lab1", 51))


def seeded_case(kind, seed, hw=HW):
    """-> (raw map float32 (hw, hw), labels int64 (hw, hw))"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hw, 0:hw].astype(np.float64) / hw
    smooth = np.zeros((hw, hw))
    for _ in range(6):
        fy, fx, ph = rng.uniform(0.5, 4.0), rng.uniform(0.5, 4.0), rng.uniform(0, 2 * np.pi)
        smooth += rng.uniform(0.2, 1.0) * np.cos(2 * np.pi * (fy * yy + fx * xx) + ph)
    smooth = (smooth + 0.05 * rng.standard_normal((hw, hw))).astype(np.float32)
    blobs = np.zeros((hw, hw), np.int64)
    for _ in range(3):
        cy, cx, rad = rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.08, 0.25)
        blobs[(yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2] = 1
    if kind == "smooth":
        return smooth, blobs
    if kind == "two":
        return np.where(smooth > np.median(smooth), np.float32(3.5), np.float32(-1.25)), blobs
    if kind == "const":
        return np.full((hw, hw), 0.75, np.float32), blobs
    if kind == "lab0":
        return smooth, np.zeros((hw, hw), np.int64)
    if kind == "lab1":
        return smooth, np.ones((hw, hw), np.int64)
    raise ValueError(kind)


def normalize(x):
    """(x - min) / (max - min) in fp32; min and max are NaN when a NaN is present; Inf stays"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mn, mx = np.min(x), np.max(x)
        return ((x - mn) / (mx - mn)).astype(np.float32)


def stated_sum(values):
    """The fp64 sum of fp32 values in K44's stated tree: lane t of 1024 owns the elements i with (i // 4) % 1024 == t and adds them
    in ascending i from +0.0; the 64 lanes of a wave by an xor butterfly (32, 16, ..., 1); the 16 waves in ascending order from +0.0."""
    v = np.asarray(values, np.float32).ravel().astype(np.float64)
    pad = (-v.size) % 4096
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, 1024, 4)          # + 0.0 changes no partial sum
    lanes = np.zeros(1024)
    with np.errstate(invalid="ignore", over="ignore"):
        for chunk in v:
            for k in range(4):
                lanes = lanes + chunk[:, k]
        lanes = lanes.reshape(16, 64)
        idx = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ off]
        s = np.float64(0.0)
        for w in range(16):
            s = s + lanes[w, 0]
    return s


def stated_mean(values):
    with np.errstate(invalid="ignore"):
        return np.float32(stated_sum(values) / np.float64(np.asarray(values).size))


def count_table(res, labels, thr):
    """res (H, W) float32, labels (H, W) integers, thr (T,) -> (counts int32 (T, H, 2, 3), other): pixels of a row by label and by
    state (0: res <= thr, 1: res > thr, 2: neither); other = pixels whose label is not 0 or 1 (in no cell)"""
    res = np.asarray(res, np.float32)
    labels = np.asarray(labels)
    thr = np.asarray(thr, np.float32).reshape(-1)
    out = np.zeros((thr.size, res.shape[0], 2, 3), np.int32)
    with np.errstate(invalid="ignore"):
        for t, th in enumerate(thr):
            le, gt = res <= th, res > th
            state = np.where(le, 0, np.where(gt, 1, 2))
            for l in (0, 1):
                for s in (0, 1, 2):
                    out[t, :, l, s] = ((labels == l) & (state == s)).sum(1)
    return out, int(((labels != 0) & (labels != 1)).sum())


def host_scores(res, thr, labels):
    """The host flow on one image -> (correct, labeled, inter (2,), union (2,), ap, f1 (H,)); needs sklearn."""
    from sklearn.metrics import average_precision_score, f1_score
    res = np.asarray(res, np.float32)
    labels = np.asarray(labels).astype(np.int64)
    with np.errstate(invalid="ignore"):
        hi, lo = res > np.float32(thr), res <= np.float32(thr)
    pred = np.where(hi & ~lo, 1, 0)                                       # argmax over (lo, hi), the first index on a tie
    correct = np.int64(((pred == 1) & (labels == 1)).sum())
    labeled = np.int64((labels == 1).sum())
    inter = np.array([((pred == k) & (labels == k)).sum() for k in (0, 1)], np.int64)
    union = np.array([(pred == k).sum() + (labels == k).sum() for k in (0, 1)], np.int64) - inter
    y_true = np.concatenate([(labels == 0).ravel(), (labels == 1).ravel()]).astype(np.int64)
    y_score = np.concatenate([lo.ravel(), hi.ravel()]).astype(np.float32)
    ap = np.nan_to_num(average_precision_score(y_true, y_score))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f1 = np.array([np.nan_to_num(f1_score(t, p.astype(np.int8))) for p, t in zip(hi, labels)], np.float64)
    return correct, labeled, inter, union, np.float64(ap), f1


def fold(scores):
    """scores: (correct, labeled, inter, union, ap, f1) per image -> (mIoU, pixAcc, mAP, mF1) and the four lines"""
    eps = np.spacing(np.float64(1.0))
    correct = sum(np.int64(s[0]) for s in scores)
    labeled = sum(np.int64(s[1]) for s in scores)
    inter = sum(np.asarray(s[2], np.int64) for s in scores)
    union = sum(np.asarray(s[3], np.int64) for s in scores)
    pix = np.float64(correct) / (eps + labeled)
    miou = (inter.astype(np.float64) / (eps + union)).mean()
    m_ap = np.mean([np.reshape(s[4], (1,)) for s in scores])
    m_f1 = np.mean([s[5] for s in scores])
    lines = [f"Mean IoU over 2 classes: {miou:.4f}\n", f"Pixel-wise Accuracy: {pix * 100:2.2f}%\n",
             f"Mean AP over 2 classes: {m_ap:.4f}\n", f"Mean F1 over 2 classes: {m_f1:.4f}\n"]
    return (miou, pix, m_ap, m_f1), lines
