"""The model-randomisation sanity test (Adebayo et al., "Sanity Checks for Saliency Maps"): counterpart of
XAI_Survey/evaluations/evaluateSanity.py.

The reference computes one attribution on the trained classifier and one on a randomised copy, reads both maps back and compares
them on the host: skimage's SSIM with Gaussian weights, scipy's spearmanr over all pixels, and spearmanr over the two skimage HOG
vectors (:82-106).  Here the maps stay where the attribution left them and a batch of pairs is compared by K8 (the argsort) and
K39-K43 (csrc/sanity_kernels.hip): `get_sanity_batch` launches them back to back on the caller's stream and reads nothing back;
`evaluate_sanity` reads the three numbers of a batch of images once.  No skimage is needed.

`data_range`: the reference passes none to structural_similarity.  The skimage releases that accept that for float images take
the range of the dtype, (-1, 1), i.e. R = 2; later releases raise instead, and the reference pins no release.  The engine therefore
takes data_range=2.0 as a documented default.
"""
import csv
import os
import time
from collections import Counter

import numpy as np
import torch

from . import kernels as K
from .ig import hip_device, _logits_of

KEYS = ("SSIM", "SPR", "HOG")
HOG_CELL = (16, 16)                                  # evaluateSanity.py:90-95 pixels_per_cell


# ---------------------------------------------------------------------------------------------- the comparison
def _host_spearman(a, b):
    import warnings
    from scipy.stats import spearmanr
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(spearmanr(a, b)[0])


def spearman_batch(a, b):
    """a, b (B, n) float32 device tensors -> float64 (B,) device tensor: scipy.stats.spearmanr(a[i], b[i]).statistic bit for bit,
    by K8 + K41 + K42.  Rows longer than K42 takes (kernels.rank_corr_max_n()) go to scipy on the host."""
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"spearman_batch: a and b must be (B, n) of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, n = a.shape
    if n > K.rank_corr_max_n():
        ah, bh = a.cpu().numpy(), b.cpu().numpy()
        return torch.tensor([_host_spearman(ah[i], bh[i]) for i in range(B)], dtype=torch.float64, device=a.device)
    both = torch.cat([a, b]).contiguous()
    order, _ = K.rank(both)
    r2 = K.tie_ranks(both, order)
    return K.rank_corr(r2[:B], r2[B:], both[:B], both[B:])


def get_sanity_batch(normal, random, data_range=2.0, guard=True, cell=HOG_CELL):
    """normal, random (B, H, W) float32 device tensors -> (SSIM, SPR, HOG), three float64 (B,) device tensors: get_sanity of every
    pair (evaluateSanity.py:82-106).  SPR ranks the maps as given (:97); SSIM and HOG take the K39-normalised maps (:83-95).
    Everything is launched on the current stream; nothing is read back.  guard=False: sanityForMethods.py's normalize_image."""
    K._maps(normal, "normal")
    K._shaped_like(random, normal, "random", "normal")
    B = normal.shape[0]
    both = torch.cat([normal, random]).contiguous()
    flat = both.view(2 * B, -1)
    spr = spearman_batch(flat[:B], flat[B:])
    norm = K.sanity_normalize(both, guard=guard)
    ssim = K.ssim(norm[:B], norm[B:], data_range=data_range)
    feat = K.hog(norm, cell)
    hog = spearman_batch(feat[:B], feat[B:])
    return ssim, spr, hog


def _as_host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _fp32_exact(x):
    """is x float32, or does a cast to float32 keep every value (then ranks and ties are those of the dtype given)"""
    if x.dtype == np.float32:
        return True
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.array_equal(x.astype(np.float32).astype(x.dtype), x, equal_nan=True))


def _device_of(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return hip_device("cuda")


def _pair_on_device(normal_attr, random_layer_attr, abs):
    """-> (a, b as given: float32 device tensors or host arrays; (2, H * W * C) float32 device tensor; H, W, C)"""
    dev = _device_of(normal_attr, random_layer_attr)
    a, b = (t if _is_f32_device(t) else _as_host(t) for t in (normal_attr, random_layer_attr))
    if a.ndim != (2 if abs else 3) or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"get_sanity(abs={abs}): both maps must be {'(H, W)' if abs else '(H, W, C)'} of one shape, got "
                         f"{tuple(a.shape)} and {tuple(b.shape)}")
    pair = torch.cat([_to_device_f32(t, dev).reshape(1, -1) for t in (a, b)])      # the reference's element order
    return a, b, pair, a.shape[0], a.shape[1], (1 if abs else a.shape[2])


def _normalized_channels(pair, H, W, Cc, guard=True):
    """normalize_image over each whole array (:83-84), then channel by channel: (2, C, H, W)"""
    return K.sanity_normalize(pair, guard=guard).view(2, H, W, Cc).permute(0, 3, 1, 2).contiguous()


def get_ssim(normal_attr, random_layer_attr, abs=False, data_range=2.0):
    """The SSIM of get_sanity alone; with C > 1 channels they are submitted as separate pairs and averaged as np.mean does."""
    _, _, pair, H, W, Cc = _pair_on_device(normal_attr, random_layer_attr, abs)
    norm = _normalized_channels(pair, H, W, Cc)
    return float(np.mean(K.ssim(norm[0], norm[1], data_range=data_range).cpu().numpy()))


def get_sanity(normal_attr, random_layer_attr, abs=False, data_range=2.0, guard=True):
    """evaluateSanity.py:82-106: Counter({"SSIM", "SPR", "HOG"}) of one pair of maps, NumPy arrays or device tensors.
    abs=False: (H, W, C) maps, the channel last, as the harness produces them with C = 1; abs=True: (H, W) maps.
    The harness never produces C > 1: HOG of several channels is not built (get_ssim has their SSIM).
    guard=False: sanityForMethods.py's normalize_image, without the constant-map test."""
    a, b, pair, H, W, Cc = _pair_on_device(normal_attr, random_layer_attr, abs)
    if Cc > 1:
        raise NotImplementedError(f"get_sanity: HOG of a {Cc}-channel map is not built (skimage picks, per pixel, the channel "
                                  "with the largest gradient): one channel only, as the harness produces")
    # SPR on the maps as given (:97): on the device when float32 holds every value, else scipy on the dtype given
    host_rank = any(not isinstance(t, torch.Tensor) and not _fp32_exact(t) for t in (a, b))
    norm = _normalized_channels(pair, H, W, Cc, guard)
    ssim = K.ssim(norm[0], norm[1], data_range=data_range)
    feat = K.hog(norm[:, 0].contiguous(), HOG_CELL)
    hog = spearman_batch(feat[:1], feat[1:])
    spr = [] if host_rank else [spearman_batch(pair[:1], pair[1:])]
    vals = torch.cat([ssim, hog] + spr).cpu().numpy()                              # one read-back
    return Counter({"SSIM": float(vals[0]), "SPR": _host_spearman(a.ravel(), b.ravel()) if host_rank else float(vals[2]),
                    "HOG": float(vals[1])})


def _is_f32_device(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


def _to_device_f32(t, dev):
    if isinstance(t, torch.Tensor):
        return t.detach().contiguous()
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev)


# ---------------------------------------------------------------------------------------------- the randomised copies
def randomize_CNN_model(model):
    """evaluateSanity.py:108-120: every module that holds parameters is visited in named_modules() order; a Conv2d gets a fresh
    Kaiming-uniform weight (ReLU gain), a Linear a fresh Xavier-uniform one, nothing else changes (biases and BatchNorm stay).
    A seeded run draws what the reference draws.  Apply it before prepare.fuse_bn_relu."""
    with torch.no_grad():
        for module in model.modules():
            if next(module.parameters(), None) is None:
                continue
            if isinstance(module, torch.nn.Conv2d):
                torch.nn.init.kaiming_uniform_(module.weight, nonlinearity="relu")
            elif isinstance(module, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(module.weight)
    return model


def randomize_VIT_model(model, randomization_fn=torch.nn.init.normal_):
    """evaluateSanity.py:122-130: every module that holds parameters redraws ALL parameters below it, so a parameter is drawn once
    for each of its ancestor modules (itself included) and the last draw -- its own module's -- stays.  The draws are kept, not
    skipped: a seeded run consumes the generator exactly like the reference's."""
    with torch.no_grad():
        for module in model.modules():
            for param in module.parameters():
                randomization_fn(param)
    return model


# ---------------------------------------------------------------------------------------------- the harness
def fold_reference_counter(rows):
    """The reference's running Counter over the images' results in file order (:485-488): the first Counter as it is, every later
    one folded in with `+=`, which drops a key whose running sum is not > 0 (a negative Spearman sum, a NaN).  The standard
    library's Counter itself, as sweep.replay_reference_counter."""
    total = None
    for r in rows:
        c = Counter({k: float(v) for k, v in zip(KEYS, r)})
        if total is None:
            total = c
        else:
            total += c
    return total if total is not None else Counter()


def write_csv(path, total, images_used, total_time):
    """rows `key,sum / images_used` in the Counter's order, then `Total Runtime` (:502-509)"""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        w = csv.writer(f)
        for k in total:
            w.writerow([k, str(total[k] / images_used)])
        w.writerow(["Total Runtime", str(total_time)])


def evaluate_sanity(testing_dict, out_dir="sanity_test_results", reference_counter=False, keep_maps=None):
    """evaluateSanity.py:425-511 for the R* and VIT* models.  testing_dict has the reference's keys (:616-629); "models" is
    [model, modified_model, model_rand, modified_model_rand] (:526, :543).  Images come from harness.select_images; the target of
    the trained attribution is the trained model's class, the one of the randomised attribution the randomised model's (:467-469).
    The maps stay on the device where the row supports it and are compared by get_sanity_batch, "sanity_batch" (default 16) images
    at a time; the host reads the three numbers once per batch.  Default: plain sums, always three rows; reference_counter=True:
    the reference's `+=` fold (fold_reference_counter).  keep_maps: a list that receives (name, map, random map) per image.
    -> (Counter of the sums, images used, file names)"""
    from . import harness, sweep
    t_start = time.time()
    name = testing_dict["model_name"]
    if "CLIP" in name or not ("R" in name or "VIT" in name):
        raise ValueError(f"evaluate_sanity: model {name!r} has no attribution table here (R* and VIT* models only)")
    models = testing_dict["models"]
    if len(models) < 4:
        raise ValueError("evaluate_sanity: testing_dict['models'] is [model, modified_model, model_rand, modified_model_rand]")
    cc = None
    if testing_dict.get("class_map_path"):
        cc = np.loadtxt(testing_dict["class_map_path"]).astype(np.int64)
    names, images, _ = harness.select_images(testing_dict, cc, lazy=True)
    dev = hip_device(testing_dict["device"])
    is_vit = "VIT" in name
    get_attr = sweep.get_VIT_attr if is_vit else sweep.get_CNN_attr
    td = dict(testing_dict, models=list(models[:2]))
    td_rand = dict(testing_dict, models=list(models[2:4]))
    if not is_vit:
        td["device_maps"] = td_rand["device_maps"] = True
    needs_trans = testing_dict["attr_func"] in (sweep.VIT_TRANS_ATTR_FUNCS if is_vit else sweep.TRANS_ATTR_FUNCS)
    batch = max(1, int(testing_dict.get("sanity_batch", 16)))
    rows, pend_a, pend_b = [], [], []

    def as_map(m):
        m = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
        return m.detach().to(dev, torch.float32).reshape(testing_dict["img_hw"], testing_dict["img_hw"])

    def flush():
        if pend_a:
            vals = torch.stack(get_sanity_batch(torch.stack(pend_a), torch.stack(pend_b),
                                                data_range=testing_dict.get("data_range", 2.0)), 1).cpu().numpy()
            rows.extend(vals)
            pend_a.clear(); pend_b.clear()

    for i, fname in enumerate(names):
        x, trans = images.load(i)
        with torch.no_grad():
            target = _logits_of(models[0](x.to(dev))).argmax(1)[0]
            target_rand = _logits_of(models[2](x.to(dev))).argmax(1)[0]
        a = as_map(get_attr(x, trans if needs_trans else None, target, td))
        b = as_map(get_attr(x, trans if needs_trans else None, target_rand, td_rand))
        pend_a.append(a); pend_b.append(b)
        if keep_maps is not None:
            keep_maps.append((fname, a, b))
        if len(pend_a) == batch:
            flush()
    flush()
    used = len(rows)
    if reference_counter:
        total = fold_reference_counter(rows)
    else:
        total = Counter()
        for k, col in zip(KEYS, np.asarray(rows, np.float64).reshape(-1, 3).T):
            total[k] = float(np.sum(col))
    if used:
        path = os.path.join(out_dir, name, f'{testing_dict["attr_func"]}_{testing_dict["image_count"]}_images.csv')
        write_csv(path, total, used, time.time() - t_start)
    return total, used, names
