#!/usr/bin/env python3
"""The sanity test's map comparison (K8 + K39-K43) on ResNet-50 at 224^2; writes profiles/r13_sanity.txt.

    timeout -k 10 500 python profiles/bench_sanity.py --out profiles/r13_sanity.txt

rows     the harness rows `gc` and `grad` (sweep.get_CNN_attr with device maps) on the trained and the randomised classifier, per
         image: both attributions followed by the device comparison (sanity.get_sanity_batch, one read-back of three numbers)
         against both attributions followed by the reference's host comparison restated in the same process
         (tests/sanity_restated.py: the two maps read back, scipy's gaussian_filter and spearmanr, HOG in NumPy -- skimage is
         not installed, and the NumPy HOG loops over cells in Python, so the host figure is an upper bound on skimage's Cython).
         A host clock around work that ends in a synchronise, warmed, the median of REPS.
kernels  each kernel at B = 1 and B = 32 pairs of 224 x 224 maps: device events around LAUNCHES launches, warmed.
Parity configuration: cudnn.deterministic, benchmark off.  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
REPS = 15
LAUNCHES = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_sanity.txt"))
    args = ap.parse_args()
    import copy
    import numpy as np
    import torch
    import sanity_restated as R
    from xai_engine import kernels as K
    from xai_engine import sanity
    from xai_engine.sweep import get_CNN_attr
    from xai_engine.zoo import resnet50
    if not torch.cuda.is_available():
        raise SystemExit("bench_sanity: no GPU")
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    base = resnet50(seed=0)
    torch.manual_seed(1)
    rand = sanity.randomize_CNN_model(copy.deepcopy(base))
    models = []
    for m in (base, rand):
        for p in m.parameters():
            p.requires_grad_(False)
        models.append(m.to(DEV).eval())
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        targets = [m(x.to(DEV)).argmax(1)[0] for m in models]
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; resnet50, seeded random weights; 224 x 224; "
             f"deterministic; median of {REPS} (rows), mean of {LAUNCHES} launches (kernels)", ""]

    def median_ms(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    lines.append("rows: ms per image (median, min, max)")
    for row in ("gc", "grad"):
        tds = [{"models": [m, m], "img_hw": 224, "batch_size": 50, "device": DEV, "attr_func": row, "device_maps": True} for m in models]

        def maps():
            return [get_CNN_attr(x, None, t, td).detach().reshape(1, 224, 224) for t, td in zip(targets, tds)]

        def device_flow():
            a, b = maps()
            return torch.stack(sanity.get_sanity_batch(a, b)).cpu()

        def host_flow():
            a, b = (m.cpu().numpy().reshape(224, 224, 1) for m in maps())
            return R.get_sanity(a, b)

        a, b = maps()

        def device_compare():
            return torch.stack(sanity.get_sanity_batch(a, b)).cpu()

        ah, bh = a.cpu().numpy()[0], b.cpu().numpy()[0]
        got, want = device_compare()[:, 0].numpy(), R.get_sanity(ah, bh)
        lines.append(f"  {row}: values device {got.tolist()} host {[want[k] for k in sanity.KEYS]}")
        for name, fn in (("two attributions alone", maps), ("two attributions + device comparison + read-back", device_flow),
                         ("two attributions + read-back + host comparison", host_flow),
                         ("device comparison + read-back alone", device_compare), ("host comparison alone", lambda: R.get_sanity(ah, bh))):
            lines.append(f"  {row}: {name:52s} {'%9.3f %9.3f %9.3f' % median_ms(fn)}")
    lines += ["", "kernels: us per launch"]
    gen = torch.Generator(device=DEV).manual_seed(0)
    for B in (1, 32):
        both = torch.rand(2 * B, 224, 224, device=DEV, generator=gen).clamp_min(0.3)          # ties, like a ReLU map
        flat = both.view(2 * B, -1)
        norm = K.sanity_normalize(both)
        order, _ = K.rank(flat)
        r2 = K.tie_ranks(flat, order)
        feat = K.hog(norm)
        forder, _ = K.rank(feat)
        fr2 = K.tie_ranks(feat, forder)
        cases = [("K8 rank, 2B x 50176", lambda: K.rank(flat)), ("K39 normalize, 2B maps", lambda: K.sanity_normalize(both)),
                 ("K40 ssim, B pairs", lambda: K.ssim(norm[:B], norm[B:])), ("K41 tie ranks, 2B x 50176", lambda: K.tie_ranks(flat, order)),
                 ("K42 rank corr, B x 50176", lambda: K.rank_corr(r2[:B], r2[B:], flat[:B], flat[B:])), ("K43 hog, 2B maps", lambda: K.hog(norm)),
                 ("K8 rank, 2B x 11664", lambda: K.rank(feat)), ("K41 tie ranks, 2B x 11664", lambda: K.tie_ranks(feat, forder)),
                 ("K42 rank corr, B x 11664", lambda: K.rank_corr(fr2[:B], fr2[B:], feat[:B], feat[B:])),
                 ("get_sanity_batch, B pairs", lambda: sanity.get_sanity_batch(both[:B], both[B:]))]
        for name, fn in cases:
            for _ in range(5):
                fn()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(LAUNCHES):
                fn()
            stop.record()
            torch.cuda.synchronize()
            lines.append(f"  B = {B:2d}: {name:28s} {start.elapsed_time(stop) * 1e3 / LAUNCHES:10.1f}   (includes the wrapper's allocations)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
