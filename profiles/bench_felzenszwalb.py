#!/usr/bin/env python3
"""Device Felzenszwalb segmentation (K69-K74) for XRAI at 224 x 224, three channels, sigma 0.8, min_size 150, XRAI's six scales, B = 1
and B = 32: each kernel alone, K73 with its time per edge that reached the test of the two thresholds, and the whole
`felzenszwalb_batch`.  (profiles/r20_felzenszwalb.txt was written while K73 still had its second forest placement, int32 parents in
global memory beside the 16-bit parents in LDS that stayed: the file has both timings, this script now prints the one.)  With --xrai_row also the harness row
get_CNN_attr(..., "xrai") on ResNet-50 (seeded random weights) with the device segmenter and with finished label maps (no segmentation
at all), and where scikit-image is importable skimage's own six calls for comparison.
    python profiles/bench_felzenszwalb.py [--out profiles/r20_felzenszwalb.txt] [--xrai_row]
Kernel times are device events around `REPS` back-to-back launches after a warm-up, the median of `ROUNDS` such windows and their
spread, the candidates alternating inside a round.  The sort leaves its pairs sorted, so every timed sort after the first sorts sorted
pairs: a radix sort's passes do the same work whatever the order.  Whole calls that end in a host read are a host clock around calls
that end in a device synchronise, median of `ROUNDS`.  There is no CPU fallback: no device, no numbers."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import torch  # noqa: E402
from xai_engine import felzenszwalb as F  # noqa: E402
from xai_engine import kernels as K  # noqa: E402
from xai_engine import xrai  # noqa: E402

DEV = "cuda:0"
REPS, ROUNDS = 5, 7
SCALES, SIGMA, MIN_SIZE = xrai.FELZENSZWALB_SCALE_VALUES, 0.8, xrai.FELZENSZWALB_MIN_SEGMENT_SIZE


def smoothed(seed, H, W, blur):
    """tests/golden/make_golden_felzenszwalb.py's image: random, box-filtered, stretched to [-1, 1], float32"""
    img = np.random.RandomState(seed).rand(H, W, 3)
    for _ in range(blur):
        p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
        img = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    img = (img - img.min()) / (img.max() - img.min()) * 2.0 - 1.0
    return img.astype(np.float32)


def event_ms(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def windows(fns):
    """{name: fn} -> {name: (median ms, min ms, max ms)} over ROUNDS rounds, the functions alternating inside a round"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            got[k].append(event_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def wall(fn, reps=ROUNDS, sync=True):
    fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_felzenszwalb.txt"))
    ap.add_argument("--xrai_row", action="store_true", help="also the xrai harness row on ResNet-50, with and without the device segmenter")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_felzenszwalb.py: no HIP device; nothing is measured without one")
    H = W = 224
    E = K.felz_edges(H, W)
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {os.cpu_count()} host CPUs visible",
             f"kernel times: device events around {REPS} back-to-back launches, median [min .. max] of {ROUNDS} windows, the candidates alternating",
             f"whole calls: host clock around calls that end in a device synchronise, median [min .. max] of {ROUNDS}",
             f"224 x 224 x 3 float64, sigma {SIGMA} (radius 3), min_size {MIN_SIZE}, scales {SCALES}: {E} edges, {len(SCALES)} chains per image"]
    images = np.stack([smoothed(3 + b, H, W, 2) for b in range(32)]).astype(np.float64)
    w_dev = torch.from_numpy(F.gaussian_weights(SIGMA)).to(DEV)
    scales_dev = torch.from_numpy(np.array([s / 255. for s in SCALES])).to(DEV)
    S = len(SCALES)
    for B in (1, 32):
        x = torch.from_numpy(images[:B]).to(DEV)
        sm, keys, order, roots, stats, labels, counts, status = F._stages(x, SCALES, SIGMA, MIN_SIZE, None)
        F.raise_for_status(status)
        ws = K.felz_workspace(DEV, B, H, W, S)
        half = K.felz_smooth(x, w_dev, 0)
        st = stats.cpu().numpy()
        tested = int(st[..., 0].sum())
        fns = {"K69 smooth, axis 0": lambda: K.felz_smooth(x, w_dev, 0),
               "K69 smooth, axis 1": lambda: K.felz_smooth(half, w_dev, 1),
               "K70 costs": lambda: K.felz_costs(sm, status),
               "K71 / K72 sort (8 passes: count, scan, place)": lambda: K.felz_sort(keys, order, H, W, S, ws),
               "K73 merge, 16-bit forest in LDS": lambda: K.felz_merge(keys, order, scales_dev, H, W, MIN_SIZE, status, ws),
               "K74 labels": lambda: K.felz_labels(roots, status),
               "felzenszwalb_batch, whole (one status read)": lambda: F.felzenszwalb_batch(x, SCALES, SIGMA, MIN_SIZE)}
        lines.append(f"B = {B}:")
        got = windows(fns)
        for name, (med, lo, hi) in got.items():
            lines.append(f"  {name:52s} {med:9.4f} ms [{lo:.4f} .. {hi:.4f}]")
        lines.append(f"  image 0, per scale: edges tested {st[0, :, 0].tolist()}, merged {st[0, :, 1].tolist()}, segments {counts[0].tolist()}")
        slowest = int(st[..., 0].reshape(-1).max())
        for name in ("K73 merge, 16-bit forest in LDS",):
            lines.append(f"  {name}: {got[name][0] * 1e3 / slowest:.3f} us per tested edge of the longest chain ({slowest} tested); "
                         f"{got[name][0] * 1e3 * B * S / tested:.3f} us x chains per tested edge over all {B * S} chains ({tested} tested)")
        F.raise_for_status(status)
    img = images[0]
    got = F.felzenszwalb_batch(img[None], SCALES, SIGMA, MIN_SIZE)[0][0].cpu().numpy()
    med, lo, hi = wall(lambda: F.felzenszwalb_batch(img[None], SCALES, SIGMA, MIN_SIZE)[0].cpu())
    lines.append(f"  {'six maps of one host image, copies in and out':52s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]")
    try:
        import warnings
        warnings.filterwarnings("ignore")
        import skimage
        from skimage.segmentation import felzenszwalb as sk

        def six():
            return np.stack([sk(img, scale=s, sigma=SIGMA, min_size=MIN_SIZE) for s in SCALES])
        want = six()
        med, lo, hi = wall(six, sync=False)
        lines.append(f"  skimage {skimage.__version__} felzenszwalb, six calls on this machine's host, single-threaded: {med:9.3f} ms "
                     f"[{lo:.3f} .. {hi:.3f}]; labels equal the device's: {bool((want == got).all())}")
    except ImportError:
        lines.append("  scikit-image is not importable on this machine: no host figure here.  On the CPU-only development machine skimage "
                     "0.18.3 takes 41-53 ms per call at 224 x 224, about 270 ms for the six, single-threaded")

    if args.xrai_row:
        from xai_engine.sweep import get_CNN_attr
        from xai_engine.zoo import resnet50
        torch.backends.cudnn.benchmark = False
        torch.backends.cudnn.deterministic = True
        model = resnet50().to(DEV).eval()
        for p in model.parameters():
            p.requires_grad_(False)
        x = torch.from_numpy(img.astype(np.float32).transpose(2, 0, 1)[None].copy())
        with torch.no_grad():
            t = model(x.to(DEV)).argmax(1)[0].cpu()
        maps = xrai.device_felzenszwalb_label_maps(x[0].permute(1, 2, 0), device=DEV)
        td = {"models": [model, model], "img_hw": 224, "batch_size": 25, "device": DEV, "attr_func": "xrai"}
        given = dict(td, xrai_label_maps=lambda x_hwc: maps)
        device = dict(td, xrai_felzenszwalb="device")
        a = get_CNN_attr(x.clone(), None, t, given)
        b = get_CNN_attr(x.clone(), None, t, device)
        lines.append(f"xrai harness row on ResNet-50 (seeded random weights), {int(sum(int(m.amax()) + 1 for m in maps))} segments; "
                     f"the two maps are equal: {bool(np.array_equal(a, b))}")
        for name, d in (("xrai_label_maps given (no segmentation)", given), ("xrai_felzenszwalb = device", device)):
            med, lo, hi = wall(lambda d=d: get_CNN_attr(x.clone(), None, t, d))
            lines.append(f"  {name:52s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
