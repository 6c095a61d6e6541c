#!/usr/bin/env python3
"""Guided IG on ResNet-50 at 224^2 (harness arguments: 50 steps, fraction 0.5, max_dist 1.0, zero baseline).
    python profiles/bench_gig.py [--json out.json]          # attributions/s: harness one-image call, guided_ig_batch B = 32,
                                                            # and the reference's flow (classifier on the GPU, inner loop on the host)
    python profiles/bench_gig.py --k22-only                 # a few calls only, for a rocprofv3 --kernel-trace --stats run
The reference's flow is restated below (GIGBuilder.py:228-292 as torch ops on CPU tensors, the gradient of the softmax
probability computed on the GPU and copied back every step), so that both run in the same process on the same classifier."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import torch  # noqa: E402
from xai_engine.guided_ig import guided_ig_batch  # noqa: E402
from xai_engine.zoo import resnet50  # noqa: E402

DEV = "cuda:0"
STEPS, FRACTION, MAX_DIST = 50, 0.5, 1.0


def host_flow(x_input, model, target):
    """The reference's loop: x on the host, one batch-1 classifier pass on the GPU per step."""
    x_baseline = torch.zeros_like(x_input)
    x = x_baseline.clone()
    l1_total = (x_input - x_baseline).abs().sum()
    attr = torch.zeros_like(x_input)
    for step in range(STEPS):
        xs = x.to(DEV).requires_grad_(True)
        p = torch.softmax(model(xs), dim=1)[:, target]
        grad_actual = torch.autograd.grad(p, xs, grad_outputs=torch.ones_like(p))[0].cpu()
        grad = grad_actual.clone()
        alpha = (step + 1.0) / STEPS
        alpha_min, alpha_max = max(alpha - MAX_DIST, 0.0), min(alpha + MAX_DIST, 1.0)
        x_min = x_baseline + (x_input - x_baseline) * alpha_min
        x_max = x_baseline + (x_input - x_baseline) * alpha_max
        l1_target = l1_total * (1 - (step + 1) / STEPS)
        gamma = float("inf")
        while gamma > 1.0:
            x_old = x.clone()
            x_alpha = torch.where(x_input - x_baseline != 0, (x - x_baseline) / (x_input - x_baseline), torch.nan)
            x_alpha[torch.isnan(x_alpha)] = alpha_max
            x[x_alpha < alpha_min] = x_min[x_alpha < alpha_min]
            l1_current = (x - x_input).abs().sum()
            if math.isclose(l1_target, l1_current, rel_tol=1e-9, abs_tol=1e-9):
                attr += (x - x_old) * grad_actual
                break
            grad[x == x_max] = float("inf")
            threshold = torch.quantile(torch.abs(grad), FRACTION, interpolation="lower")
            s = torch.logical_and(torch.abs(grad) <= threshold, grad != float("inf"))
            l1_s = ((x - x_max).abs() * s).sum()
            gamma = (l1_current - l1_target) / l1_s if l1_s > 0 else float("inf")
            if gamma > 1.0:
                x[s] = x_max[s]
            else:
                x[s] = (x + (x_max - x) * gamma)[s]
            attr += (x - x_old) * grad_actual
    return attr


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--k22-only", action="store_true")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    model = resnet50(seed=0).to(DEV).eval()
    xs = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        ts = model(xs).argmax(1)
    kw = dict(steps=STEPS, fraction=FRACTION, max_dist=MAX_DIST, baseline=0)
    if args.k22_only:
        for _ in range(2):
            guided_ig_batch(xs[:1], model, ts[:1], **kw)
        guided_ig_batch(xs[:8], model, ts[:8], **kw)
        print("k22-only done")
        return
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model": "resnet50 seed 0", "steps": STEPS,
           "fraction": FRACTION, "max_dist": MAX_DIST}
    guided_ig_batch(xs[:1], model, ts[:1], **kw)                       # first call: eager + capture + proof
    s1 = timed(lambda: guided_ig_batch(xs[:1], model, ts[:1], **kw), 5)
    res["harness_one_image_s"] = s1
    res["harness_one_image_attr_per_s"] = 1.0 / s1
    guided_ig_batch(xs, model, ts, **kw)
    s32 = timed(lambda: guided_ig_batch(xs, model, ts, **kw), 2)
    res["batch32_s"] = s32
    res["batch32_attr_per_s"] = 32.0 / s32
    torch.set_num_threads(16)
    host_flow(xs[0].cpu()[None], model, int(ts[0]))                   # warm
    sh = timed(lambda: host_flow(xs[1].cpu()[None], model, int(ts[1])), 2)
    res["reference_flow_s"] = sh
    res["reference_flow_attr_per_s"] = 1.0 / sh
    ref = host_flow(xs[2].cpu()[None], model, int(ts[2]))
    dev = guided_ig_batch(xs[2:3], model, ts[2:3], **kw).cpu()
    res["reference_flow_vs_device_rel_err"] = float((ref - dev).abs().max() / ref.abs().max())
    for k, v in res.items():
        print(f"{k:40s} {v}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
