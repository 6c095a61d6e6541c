"""The ImageNet-segmentation evaluation (reference XAI_Survey/evaluations/evaluateImageNetSeg.py with utils/metrices.py): every
attribution map is min-max normalised, cut at its mean and scored against a ground-truth object mask by pixel accuracy, mIoU, mAP
and mF1.

The reference scores on the host, one image at a time, through sklearn.  All four numbers are functions of a small integer table:
per image row r, label l (0 / 1) and prediction state s (0: res <= thr, 1: res > thr, 2: neither -- a NaN pixel or a NaN threshold),
the number of pixels.  Here a group of maps stays on the device: K44 (kernels.seg_normalize) normalises them and takes each one's
mean in a stated fp64 order, K45 (kernels.seg_counts) fills the table, one read-back per group brings it to the host and
`scores_from_counts` does the reference's arithmetic on it, about 230 fp64 divisions per image.

What the reference computes, kept as it is:
  * the masks are Res.gt(ret) and Res.le(ret); a pixel that is in neither (NaN) is predicted as class 0 by torch.max's first index;
  * pixel accuracy counts label-1 pixels only (batch_pix_accuracy's `target > 0`);
  * AP is sklearn's average_precision_score on the 2 x HW one-hot / mask arrays, whose scores are 0 or 1;
  * "F1" is get_f1_scores(output[0, 1], labels[0]), which takes the image height as its batch size: one F1 per image ROW, and mF1 is
    the mean over all rows of all images.
Refused by name: the rows that need timm's relprop layers (t_attr), MASCalibrate (MDA_dense) and CLIP.
"""
import os
from collections import namedtuple

import numpy as np
import torch

from . import kernels as K
from .ig import hip_device

MAG_VALS = (0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)        # evaluateImageNetSeg.py:339
REFUSED = {"t_attr": "it needs timm's relprop (LRP) layers", "MDA_dense": "it needs MASCalibrate"}

SegScores = namedtuple("SegScores", "correct labeled inter union ap f1")


# ---------------------------------------------------------------------------------------------- the host arithmetic
def average_precision_from_counts(c):
    """sklearn's average_precision_score of eval_batch's arrays from the image's (2, 3) table, in sklearn's operation sequence.
    The 2 HW samples are (label == 0, res <= thr) and (label == 1, res > thr) per pixel, so the scores are 0 or 1 and the curve has
    at most two thresholds: precision_recall_curve gives precision [tp / n_pred, HW / 2HW], recall [tp / HW, 1], reversed and
    closed with (1, 0); AP = max(0, -sum(diff(recall) * precision[:-1])).  With no score of 1 (every pixel in state 2) only the
    threshold 0 is left and AP is 0.5."""
    c = np.asarray(c, np.int64)
    hw = int(c.sum())
    tp = np.float64(c[0, 0] + c[1, 1])                   # samples with score 1 that are positives
    n_pred = np.float64(c[:, 0].sum() + c[:, 1].sum())   # samples with score 1
    if n_pred == 0:
        tps, fps = np.array([np.float64(hw)]), np.array([np.float64(hw)])
    else:
        tps, fps = np.array([tp, np.float64(hw)]), np.array([n_pred - tp, np.float64(hw)])
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    recall = tps / tps[-1]
    precision, recall = np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0))
    return float(max(0.0, -np.sum(np.diff(recall) * np.array(precision)[:-1])))


def scores_from_counts(counts):
    """counts: integer (H, 2, 3) table of one image and one threshold (K45's counts[m][t]) -> SegScores with the reference's values
    and types: correct, labeled np.int64 (batch_pix_accuracy: label-1 pixels only), inter, union int64 (2,) per class
    (batch_intersection_union), ap float64 (1,) (get_ap_scores), f1 float64 (H,) (get_f1_scores: one value per image row,
    2 tp / (2 tp + fp + fn), 0 where that denominator is 0)."""
    rows = np.asarray(counts).astype(np.int64)
    if rows.ndim != 3 or rows.shape[1:] != (2, 3):
        raise ValueError(f"scores_from_counts: expected an (H, 2, 3) table, got {rows.shape}")
    c = rows.sum(0)
    pred0 = c[:, 0] + c[:, 2]                            # torch.max picks index 0 where both masks are 0
    pred1 = c[:, 1]
    correct, labeled = c[1, 1], c[1].sum()
    inter = np.array([pred0[0], pred1[1]], np.int64)
    union = np.array([pred0.sum(), pred1.sum()], np.int64) + c.sum(1) - inter
    ap = np.array([average_precision_from_counts(c)], np.float64)
    tp, fp, fn = rows[:, 1, 1], rows[:, 0, 1], rows[:, 1, 0] + rows[:, 1, 2]
    num, den = (2 * tp).astype(np.float64), (2 * tp + fp + fn).astype(np.float64)
    f1 = np.zeros_like(num)
    np.divide(num, den, out=f1, where=(den != 0))
    return SegScores(np.int64(correct), np.int64(labeled), inter, union, ap, f1)


def fp32_thresholds(values):
    """The thresholds as torch compares them: a float32 tensor against a Python or NumPy scalar is compared in fp32, so
    Res.gt(np.float64(0.55)) is Res > fp32(0.55)."""
    return np.asarray(values, np.float64).astype(np.float32)


class SegFold:
    """The running totals of evaluate_imagenet_seg (:513-555), in the reference's arithmetic."""

    def __init__(self):
        self.correct = self.label = np.int64(0)
        self.inter = self.union = np.int64(0)
        self.ap, self.f1 = [], []

    def add(self, s):
        self.correct = self.correct + s.correct.astype("int64")
        self.label = self.label + s.labeled.astype("int64")
        self.inter = self.inter + s.inter.astype("int64")
        self.union = self.union + s.union.astype("int64")
        self.ap += [s.ap]
        self.f1 += [s.f1]

    def numbers(self):
        """-> (mIoU, pixAcc, mAP, mF1)"""
        pix_acc = np.float64(1.0) * self.correct / (np.spacing(1, dtype=np.float64) + self.label)
        iou = np.float64(1.0) * self.inter / (np.spacing(1, dtype=np.float64) + self.union)
        return iou.mean(), pix_acc, np.mean(self.ap), np.mean(self.f1)

    def lines(self):
        miou, pix_acc, m_ap, m_f1 = self.numbers()
        return ["Mean IoU over %d classes: %.4f\n" % (2, miou), "Pixel-wise Accuracy: %2.2f%%\n" % (pix_acc * 100),
                "Mean AP over %d classes: %.4f\n" % (2, m_ap), "Mean F1 over %d classes: %.4f\n" % (2, m_f1)]


# ---------------------------------------------------------------------------------------------- the device scoring
def _labels_i32(labels, dev, shape):
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
    lab = lab.detach().to(dev).reshape(shape)
    return lab.to(torch.int32).contiguous()


def eval_batch_device(maps, labels, thr=None, want_maps=False):
    """maps: (B, H, W) float32 device tensor; labels: (B, H, W) integers (0 / 1), tensor or array.
    thr None: every map is normalised by K44 and cut at its own stated mean (the reference's Res and ret); else thr is (B,) or
    (B, T) thresholds, taken in fp32, for the maps as given.  K45 counts, then ONE read-back of the table for the whole batch.
    -> a list of B SegScores (T == 1) or of B lists of T SegScores; with want_maps also the maps that were scored and the (B, T)
    threshold tensor.  A label other than 0 / 1 raises (the reference fails in scatter_)."""
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3:
        raise ValueError("eval_batch_device: maps must be a (B, H, W) device tensor")
    maps = maps.detach().contiguous()
    B, H, W = maps.shape
    lab = _labels_i32(labels, maps.device, (B, H, W))
    if thr is None:
        res, mean, _ = K.seg_normalize(maps)
        thr_dev = mean.view(B, 1)
    else:
        res = maps
        t = thr if isinstance(thr, torch.Tensor) else torch.from_numpy(np.asarray(thr, np.float64).astype(np.float32))
        thr_dev = t.detach().to(maps.device, torch.float32).reshape(B, -1).contiguous()
    T = thr_dev.shape[1]
    counts, other = K.seg_counts(res, lab, thr_dev)
    host = torch.cat([counts.view(-1), other]).cpu().numpy()                         # the one read-back
    table, others = host[:-B].reshape(B, T, H, 2, 3), host[-B:]
    if others.any():
        bad = int(np.flatnonzero(others)[0])
        raise ValueError(f"eval_batch_device: map {bad} has {int(others[bad])} pixels whose label is neither 0 nor 1 "
                         "(the reference fails in scatter_)")
    scores = [[scores_from_counts(table[b, t]) for t in range(T)] for b in range(B)]
    if T == 1:
        scores = [s[0] for s in scores]
    return (scores, res, thr_dev) if want_maps else scores


def eval_batch(Res, ret, labels):
    """evaluateImageNetSeg.py:470-507 with its signature and its 8-tuple: Res (1, 1, H, W) float32, ret the threshold (a 0-d tensor
    or a number, compared in fp32), labels (1, H, W) -> (correct, labeled, inter, union, ap, f1, pred, target).  The masks are taken
    from Res as given; only then are its NaN zeroed IN PLACE (:474, :479: Res_1_AP is Res itself), and pred = Res.clamp(min=0) /
    Res.max() is computed from the zeroed map with plain torch ops (:483-485)."""
    if not isinstance(Res, torch.Tensor) or Res.dim() != 4 or Res.shape[:2] != (1, 1):
        raise ValueError("eval_batch: Res must be a (1, 1, H, W) tensor")
    H, W = Res.shape[2:]
    dev_map = Res if Res.is_cuda else Res.to(hip_device("cuda"))
    ret32 = float(ret.detach().float().cpu()) if isinstance(ret, torch.Tensor) else float(np.float32(ret))
    s = eval_batch_device(dev_map.detach().reshape(1, H, W).float(), labels, thr=np.array([ret32]))[0]
    Res[Res != Res] = 0
    pred = Res.clamp(min=0) / Res.max()
    pred = pred.view(-1).data.cpu().numpy()
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels))
    target = lab.reshape(-1).data.cpu().numpy()
    return 0 + s.correct, 0 + s.labeled, 0 + s.inter, 0 + s.union, 0 + s.ap, 0 + s.f1, pred, target


def best_threshold(Res, labels, mag_vals=MAG_VALS):
    """The MDA_dense sweep of :337-363 on a normalised map Res (1, 1, H, W): Res / Res.mean() * 0.5, the len(mag_vals) thresholds
    (fp32_thresholds) in one K45 launch, the argmax of the per-image IoU.  -> (the rescaled Res, mag_vals[best], the IoU array)"""
    if len(mag_vals) > 16:
        raise ValueError("best_threshold: at most 16 thresholds go into one launch")
    Res = Res / Res.mean() * 0.5
    H, W = Res.shape[-2:]
    thr = fp32_thresholds(mag_vals)[None]
    per_t = eval_batch_device(Res.detach().reshape(1, H, W).float(), labels, thr=thr)[0]
    per_t = per_t if isinstance(per_t, list) else [per_t]
    iou = np.array([np.mean(np.float64(1.0) * s.inter / (np.spacing(1, dtype=np.float64) + s.union)) for s in per_t])
    return Res, np.asarray(mag_vals)[int(np.argmax(iou))], iou


# ---------------------------------------------------------------------------------------------- the harness
def _normalized_input(image, norm):
    if callable(norm):
        return norm(image)
    from .harness import normalize
    mean, std = (norm.mean, norm.std) if hasattr(norm, "mean") else norm
    return normalize(image, mean, std)


def _attribution_map(x, trans_img, target, testing_dict, is_vit, dev):
    """The (H, W) device map the reference normalises: |sum over channels| for the CNN rows (:214); the bilinear up-sample of the
    patch map WITHOUT abs for the ViT patch rows (:235-268 take none); VIT_CX and MDA keep theirs (:259-261, :290)."""
    from . import sweep
    hw = testing_dict["img_hw"]
    if not is_vit:
        m = sweep.get_CNN_attr(x, trans_img, target, dict(testing_dict, device_maps=True))
    else:
        sal = sweep.vit_patch_map(x, target, testing_dict)
        m = (K.bilinear_up(sal, hw, hw, scale=1.0, take_abs=False)[0] if sal is not None else
             sweep.get_VIT_attr(x, trans_img, target, testing_dict))
    m = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
    return m.detach().to(dev, torch.float32).reshape(hw, hw)


def evaluate_imagenet_seg(testing_dict, out_dir="seg_test_results", batch=32, keep_maps=None):
    """evaluateImageNetSeg.py:509-573 for the R* and VIT* models.  testing_dict has the reference's keys (:660-672);
    "segmentation_dataloader" is any iterable of (image (1, 3, H, W) in [0, 1], labels (1, H, W)).  Per image the class is
    model_utils.getClass's and the map comes from the sweep's attribution table; the maps collect in a (batch, H, W) device buffer and
    every group is scored by one K44, one K45 and one read-back.  The fold and the four-line file
    <out_dir>/<model>/<attr>_<count>_images are the reference's.  keep_maps: a list that receives every (map, labels) pair as scored.
    -> (mIoU, pixAcc, mAP, mF1)"""
    from util import model_utils
    from . import sweep
    name, attr = testing_dict["model_name"], testing_dict["attr_func"]
    if attr in REFUSED:
        raise NotImplementedError(f"evaluate_imagenet_seg: the row {attr!r} is not served: {REFUSED[attr]}")
    if "CLIP" in name or not ("R" in name or "VIT" in name):
        raise NotImplementedError(f"evaluate_imagenet_seg: model {name!r} is not served (R* and VIT* models only; the CLIP rows need CLIP)")
    is_vit = "VIT" in name
    table = sweep.VIT_ATTR_FUNCS + sweep.VIT_TRANS_ATTR_FUNCS if is_vit else sweep.CNN_ATTR_FUNCS
    if attr not in table:
        raise ValueError(f"evaluate_imagenet_seg: {attr!r} is not an attribution of {name} (choose from {', '.join(table)})")
    dev = hip_device(testing_dict["device"])
    model = testing_dict["models"][0]
    hw = testing_dict["img_hw"]
    needs_trans = attr in (sweep.VIT_TRANS_ATTR_FUNCS if is_vit else sweep.TRANS_ATTR_FUNCS)
    batch = max(1, int(batch))
    buf = torch.empty((batch, hw, hw), dtype=torch.float32, device=dev)
    lab = torch.empty((batch, hw, hw), dtype=torch.int32, device=dev)
    fold, fill = SegFold(), 0

    def flush():
        nonlocal fill
        if fill:
            for s in eval_batch_device(buf[:fill], lab[:fill]):
                fold.add(s)
            fill = 0

    for image, labels in testing_dict["segmentation_dataloader"]:
        trans_img = torch.as_tensor(image).squeeze(0).float()
        x = _normalized_input(trans_img, testing_dict["normalize"]).unsqueeze(0)
        with torch.no_grad():
            target = model_utils.getClass(x, model, dev)
        m = _attribution_map(x, trans_img if needs_trans else None, target, testing_dict, is_vit, dev)
        buf[fill].copy_(m)
        lab[fill].copy_(torch.as_tensor(labels).reshape(hw, hw).to(dev))
        if keep_maps is not None:
            keep_maps.append((m.clone(), lab[fill].clone()))
        fill += 1
        if fill == batch:
            flush()
    flush()
    if not fold.ap:
        raise ValueError("evaluate_imagenet_seg: the data source gave no image")
    folder = os.path.join(out_dir, name)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, f'{attr}_{testing_dict["image_count"]}_images'), "w") as fh:
        fh.writelines(fold.lines())
    return fold.numbers()


# ---------------------------------------------------------------------------------------------- the dataset readers
def _resized_pair(img, gt, size):
    """(image uint8 HWC, mask uint8 HW) -> (float32 (3, size, size) in [0, 1], int64 (size, size)): Resize((size, size)) then
    ToTensor for the image (:643-646, PIL's bilinear), Resize(..., NEAREST_EXACT) for the mask (:647-649; on a PIL image torchvision
    maps NEAREST_EXACT to Image.NEAREST, which picks the pixel under each output centre, as F.interpolate's nearest-exact does)."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(img)).convert("RGB").resize((size, size), Image.BILINEAR)
    mask = Image.fromarray(np.ascontiguousarray(gt)).resize((size, size), Image.NEAREST)
    image = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
    return image, torch.from_numpy(np.array(mask)).long()


class NpzSegmentation:
    """An .npz file with the keys img_<i> (uint8 HWC) and gt_<i> (uint8 HW), i = 0, 1, ...; item i is (image (3, size, size) float32
    in [0, 1], labels (size, size) int64).  `loader(count)` yields the (1, ...) batches evaluate_imagenet_seg takes."""

    def __init__(self, path, size=224):
        self.data = np.load(path, allow_pickle=False)
        self.size = size
        self.n = sum(1 for k in self.data.files if k.startswith("img_"))

    def __len__(self):
        return self.n

    def _raw(self, i):
        return self.data[f"img_{i}"], self.data[f"gt_{i}"]

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return _resized_pair(*self._raw(i), self.size)

    def loader(self, count=-1):
        for i in range(len(self) if count in (-1, None) else min(count, len(self))):
            image, labels = self[i]
            yield image[None], labels[None]


class MatSegmentation(NpzSegmentation):
    """gtsegs_ijcv.mat, the reference's Imagenet_Segmentation source (an HDF5 file: value/img and value/gt hold references, stored
    transposed).  It needs h5py, imported here and named in the error when it is missing."""

    def __init__(self, path, size=224):
        try:
            import h5py
        except ImportError as e:
            raise ImportError("MatSegmentation: reading gtsegs_ijcv.mat needs the h5py package, which is not installed; convert the "
                              "file to .npz (keys img_<i>, gt_<i>) and use NpzSegmentation") from e
        self.h5 = h5py.File(path, "r")
        self.size = size
        self.n = self.h5["/value/img"].shape[0]

    def _raw(self, i):
        # MATLAB v7.3 cell arrays: a table of object references per field; the arrays come back with their axes reversed
        image_ref = self.h5["/value/img"][i, 0]
        gt_cell = self.h5[self.h5["/value/gt"][i, 0]]
        return np.asarray(self.h5[image_ref]).T, np.asarray(self.h5[gt_cell[0, 0]]).T
