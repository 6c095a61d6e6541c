#!/usr/bin/env python3
"""AGI on ResNet-50 at 224^2 (harness arguments: epsilon 0.05, max_iter 20, the ImageNet Normalize in front of the classifier,
the [0, 1] image divided by 255 once more as AGI.test does).
    python profiles/bench_agi.py [--json out.json]     # attributions/s: the harness's one-image call (topk 1), agi_batch at B = 32
                                                       # (topk 1), and the reference's flow restated (one image, one class, a host
                                                       # sync per iteration); plus the share of pair-iterations the replays waste
    python profiles/bench_agi.py --kernels-only        # a few calls only, for a rocprofv3 --kernel-trace --stats run
Parity configuration: cudnn.deterministic, benchmark off."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from xai_engine import agi  # noqa: E402
from xai_engine.harness import CNN_MEAN, CNN_STD  # noqa: E402
from xai_engine.zoo import resnet50  # noqa: E402

DEV = "cuda:0"
EPS, MAX_ITER = 0.05, 20
CLASSES = list(range(0, 999, 1000))                  # topk 1: [0]


def reference_flow(data, model, classes):
    """AGI.test restated with torch ops on the device: one image, the classes one after the other, `.item()` every iteration."""
    mean = torch.tensor(CNN_MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(CNN_STD, device=DEV).view(1, 3, 1, 1)
    net = lambda x: model((x - mean) / std)                           # noqa: E731
    init_pred = net(data).max(1, keepdim=True)[1]
    step_grad = 0
    for c in classes:
        if c == init_pred.item():
            continue
        x, c_delta = data.clone(), 0
        for _ in range(MAX_ITER):
            x.requires_grad_(True)
            out = net(x)
            if out.max(1, keepdim=True)[1].item() == c:
                break
            p = torch.softmax(out, dim=1)
            (g_adv,) = torch.autograd.grad(p[0, c], x, retain_graph=True)
            (g_lab,) = torch.autograd.grad(p[0, init_pred.item()], x)
            x = torch.clamp(data + EPS * g_adv.sign(), 0, 1)
            c_delta = c_delta + (-g_lab * (x - data))
        step_grad = step_grad + c_delta
    return step_grad


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
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    model = resnet50(seed=0).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    imgs = torch.rand(32, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    data = torch.from_numpy(imgs.numpy() / 255).to(DEV)               # the reference's data: the [0, 1] image / 255
    kw = dict(epsilon=EPS, max_iter=MAX_ITER, normalize=(CNN_MEAN, CNN_STD), want_map=True)
    if args.kernels_only:
        for _ in range(2):
            agi.agi_batch(data[:1], model, CLASSES, **kw)
        agi.agi_batch(data[:8], model, CLASSES, **kw)
        print("kernels-only done")
        return
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model": "resnet50 seed 0", "epsilon": EPS,
           "max_iter": MAX_ITER, "classes": CLASSES, "deterministic": True}
    agi.agi_batch(data[:1], model, CLASSES, **kw)                     # first call: eager + capture + proof
    s1 = timed(lambda: agi.agi_batch(data[:1], model, CLASSES, **kw), 5)
    res["harness_one_image_s"] = s1
    res["harness_one_image_attr_per_s"] = 1.0 / s1
    agi.agi_batch(data, model, CLASSES, **kw)
    before = dict(agi.AGI_COUNTS)
    s32 = timed(lambda: agi.agi_batch(data, model, CLASSES, **kw), 3)
    res["batch32_s"] = s32
    res["batch32_attr_per_s"] = 32.0 / s32
    ran = agi.AGI_COUNTS["pair_iterations"] - before["pair_iterations"]
    used = agi.AGI_COUNTS["pair_iterations_used"] - before["pair_iterations_used"]
    res["batch32_pair_iterations_run"] = ran
    res["batch32_pair_iterations_needed"] = used
    res["batch32_wasted_share"] = 1.0 - used / ran
    res["graph_counts"] = {k: agi.AGI_COUNTS[k] for k in ("captures", "captures_refused", "replayed", "eager")}
    reference_flow(data[:1], model, CLASSES)                          # warm
    sh = timed(lambda: reference_flow(data[1:2], model, CLASSES), 3)
    res["reference_flow_s"] = sh
    res["reference_flow_attr_per_s"] = 1.0 / sh
    ref = reference_flow(data[2:3], model, CLASSES)
    got = agi.agi_batch(data[2:3], model, CLASSES, **kw)[0]
    res["reference_flow_vs_device_rel_err"] = float((ref - got).abs().max() / ref.abs().max()) if torch.is_tensor(ref) else None
    for k, v in res.items():
        print(f"{k:40s} {v}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
