#!/usr/bin/env python3
"""Device quickshift (K53-K55) at 224^2 with LIME's arguments (kernel_size 4, max_dist 200, ratio 0.2): each kernel and the whole
call at B = 1 and B = 32, and the `lime` harness row on ResNet-50 (seed 0, 1000 samples) with the device
segmenter against the same row fed finished labels (what the segmentation adds to the row) and, when scikit-image is importable in
this process, against the row with skimage's segmenter on the host.
    python profiles/bench_quickshift.py [--out profiles/r16_quickshift.txt]
Kernel times are device events around `REPS` back-to-back launches after a warm-up, the median of `ROUNDS` such windows and their
spread (profiles/r16_quickshift_tiles.txt keeps the one comparison of 16 x 16 against 8 x 8 tiles, made before the slower
8 x 8 instantiation was removed).  Row times are a host clock around calls that end in a device synchronise.
Without scikit-image the host side is not timed here; the figure quoted then was taken on a CPU-only development machine
(skimage 0.18.3, single thread) and says nothing about the host of a GPU machine.  There is no CPU fallback: no device, no numbers."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import torch  # noqa: E402
from xai_engine import kernels as K  # noqa: E402
from xai_engine import lime  # noqa: E402
from xai_engine import quickshift as Q  # noqa: E402

DEV = "cuda:0"
HW, N = 224, 1000
ARGS = lime.QUICKSHIFT_ARGS
REPS, ROUNDS = 20, 7
HOST_FIGURE = "0.44-0.58 s per image (skimage 0.18.3, one thread, a CPU-only development machine; not a figure of this machine)"


def images(B, seed=0):
    """B seeded (3, HW, HW) float32 images in [0, 1]: smooth colour fields plus texture, so that quickshift finds tens of superpixels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HW, 0:HW] / HW
    out = []
    for _ in range(B):
        a, b, c = rng.uniform(2, 9, 3)
        img = np.stack([0.5 + 0.4 * np.sin(a * yy + k) * np.cos(b * xx - k) + 0.1 * np.sin(c * (xx + yy) * 4 + k) for k in range(3)])
        out.append((img + 0.05 * rng.random(img.shape)).clip(0, 1))
    return np.stack(out).astype(np.float32)


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


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_quickshift.txt"))
    ap.add_argument("--no_row", action="store_true", help="kernels only, no ResNet-50 rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_quickshift.py: no HIP device; nothing is measured without one")
    ks, md, ratio = ARGS["kernel_size"], ARGS["max_dist"], ARGS["ratio"]
    kw = int(np.ceil(3 * ks))
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"{HW} x {HW} x 3 fp64 features, kernel_size {ks} (window {2 * kw + 1}^2 = {(2 * kw + 1) ** 2} terms), max_dist {md}, ratio {ratio}",
             f"kernel times: device events around {REPS} back-to-back launches, median [min .. max] of {ROUNDS} windows, the kernels alternating"]
    imgs = images(32)
    feats = np.stack([Q.quickshift_features(im.transpose(1, 2, 0), ratio) for im in imgs])
    noise = np.stack([Q.tie_noise(s, HW, HW) for s in range(32)])
    exps = HW * HW * (2 * kw + 1) ** 2                                   # an upper count: border windows are clipped
    for B in (1, 32):
        f, n = torch.from_numpy(feats[:B]).to(DEV), torch.from_numpy(noise[:B]).to(DEV)
        dens = K.quickshift_density(f, n, ks)
        parent = K.quickshift_parent(f, dens, ks, md)[0]
        labels, D = K.quickshift_labels(parent)
        got = windows({"K53 density": lambda: K.quickshift_density(f, n, ks, out=dens),
                       "K54 parent": lambda: K.quickshift_parent(f, dens, ks, md),
                       "K55 labels (3 launches)": lambda: K.quickshift_labels(parent, labels=labels),
                       "quickshift_batch (K53-K55)": lambda: Q.quickshift_batch(f, n, ks, md)})
        lines.append(f"B = {B}: superpixels per image {D.tolist()[:8]}{' ...' if B > 8 else ''}; "
                     f"{B * 14 * 14} workgroups of 16 x 16 pixels")
        for k, (med, lo, hi) in got.items():
            rate = f", {B * exps / (med * 1e-3) / 1e9:6.1f} G exp/s (unclipped count)" if k.startswith("K53") else ""
            lines.append(f"  {k:28s} {med:9.4f} ms [{lo:.4f} .. {hi:.4f}]  {med / B:8.4f} ms per image{rate}   [incl. the allocation of outputs not passed in]")

    # the host half of one image, on this machine's CPU
    t0 = time.perf_counter()
    for i in range(8):
        Q.quickshift_features(imgs[i].transpose(1, 2, 0), ratio), Q.tie_noise(i, HW, HW)
    lines.append(f"host half (Lab features + tie noise, NumPy fp64): {(time.perf_counter() - t0) / 8 * 1e3:.2f} ms per image on this machine's CPU")

    try:
        from skimage.segmentation import quickshift as sk_quickshift
        import skimage
    except ImportError:
        sk_quickshift = None
    if sk_quickshift is not None:
        t0 = time.perf_counter()
        want = [sk_quickshift(imgs[i].transpose(1, 2, 0).astype(np.float64), random_seed=i, **ARGS) for i in range(3)]
        t_host = (time.perf_counter() - t0) / 3
        got = [Q.quickshift(imgs[i].transpose(1, 2, 0), random_seed=i, device=DEV, **ARGS) for i in range(3)]
        lines.append(f"skimage {skimage.__version__} quickshift on this machine's CPU: {t_host:.3f} s per image; labels equal to the device's: "
                     f"{[bool(np.array_equal(a, b)) for a, b in zip(want, got)]}")
    else:
        lines.append(f"scikit-image is not importable in this process: the host segmenter is not timed here.  Quoted, not measured here: {HOST_FIGURE}")

    if not args.no_row:
        from xai_engine.zoo import resnet50
        torch.backends.cudnn.benchmark = False
        torch.backends.cudnn.deterministic = True
        model = resnet50(seed=0).to(DEV).eval()
        for p in model.parameters():
            p.requires_grad_(False)
        x = torch.from_numpy(imgs[:1]).to(DEV)
        kwargs = dict(num_samples=N, top_labels=5, hide_color=0)
        seed = lime.draw_seed(np.random.RandomState(1))
        done = Q.quickshift(imgs[0].transpose(1, 2, 0), random_seed=seed, device=DEV, **ARGS).astype(np.int32)
        rows = {"device segmenter (lime.device_quickshift_segments)": lambda: lime.lime_batch(x, model, lime.device_quickshift_segments, random_state=1, **kwargs),
                "finished labels (no segmentation in the row)": lambda: lime.lime_batch(x, model, done, random_state=1, **kwargs)}
        if sk_quickshift is not None:
            rows["skimage on the host (lime.quickshift_segments)"] = lambda: lime.lime_batch(x, model, lime.quickshift_segments, random_state=1, **kwargs)
        maps = {k: fn() for k, fn in rows.items()}                       # warm: capture and proof of the pass's hipGraph
        lines.append(f"lime row, resnet50 seed 0, one image, {N} samples, {int(done.max()) + 1} superpixels, pass_size {lime.PASS_SIZE}; "
                     f"wall time of lime_batch, median [min .. max] of 5 calls; maps equal: {all(torch.equal(m, maps[next(iter(maps))]) for m in maps.values())}")
        for k, fn in rows.items():
            med, lo, hi = wall(fn, 5)
            lines.append(f"  {k:52s} {med * 1e3:9.1f} ms [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
