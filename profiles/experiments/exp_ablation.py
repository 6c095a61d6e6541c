#!/usr/bin/env python3
"""Feature Ablation (`fa`) and Occlusion (`occ`) on ResNet-50 at 224^2 with the harness's arguments (14 x 14 patch mask; window
(3, 64, 64), stride 32).
    python profiles/experiments/exp_ablation.py [--json out.json]
        attributions/s of the restated captum flow in this process (one altered image per forward, four torch ops per image, the score
        read back each time), of the harness's one-image call and of the *_batch entries at B = 32; the batching floor of the
        reference flow (restated batch 1 vs restated at the engine's pass size) next to the engine's error against batch 1
    python profiles/experiments/exp_ablation.py --kernels-only
        K26 on 4 images x 196 copies (472 MB out, past the 256 MiB Infinity Cache) next to xai_perturb_batch_f32 writing the same
        bytes, a few times each, for a `rocprofv3 --kernel-trace --stats` run (no counters in that run)
Parity configuration: cudnn.deterministic, benchmark off."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import torch  # noqa: E402
from xai_engine import ablation  # noqa: E402
from xai_engine import kernels as K  # noqa: E402
from xai_engine.sweep import get_CNN_attr  # noqa: E402
from xai_engine.zoo import resnet50  # noqa: E402

DEV = "cuda:0"
WINDOW, STRIDE = (3, 64, 64), 32


def captum_flow(x, model, target, masks, weighted):
    """captum's loop restated with torch ops on the device: one altered image per classifier call, `.item()`-style read-back of
    every score (captum moves each evaluation's difference into its running totals before it builds the next image)."""
    with torch.no_grad():
        s0 = model(x)[0, target]
        total = torch.zeros_like(x[0])
        weights = torch.zeros_like(x[0])
        for m in masks:
            xj = x[0] * (1 - m) + 0 * m
            d = float(s0 - model(xj[None])[0, target])            # the read-back
            total += d * m
            if weighted:
                weights += m
    return total / weights if weighted else total


def fa_masks():
    ids = ablation.harness_patch_mask(224).to(DEV)
    return [(ids == j).expand(3, 224, 224).float() for j in range(196)]


def occ_masks():
    out = []
    for k in range(36):
        m = torch.zeros(3, 224, 224, device=DEV)
        r0, c0 = (k % 6) * 32, (k // 6) * 32
        m[:, r0:r0 + 64, c0:c0 + 64] = 1.0
        out.append(m)
    return out


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def rel_inf(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def kernels_only():
    x = torch.randn(4, 3, 224, 224, device=DEV)
    pm = ablation.prepare_mask(ablation.harness_patch_mask(224), x.shape, DEV)
    out = torch.empty((4 * 196, 3, 224, 224), device=DEV)
    flip = torch.randint(0, 4 * 196, (224 * 224,), device=DEV, dtype=torch.int32)
    for _ in range(5):
        K.ablate_features(x, pm.ids, 0, 196, 0, 0, 4 * 196, out=out)
        K.perturb_batch(x[0], x[1], flip, 0, 4 * 196, out=out)
    for _ in range(5):
        K.ablate_windows(x, (64, 64), (32, 32), 0, 0, 4 * 36, out=out[:4 * 36])
    torch.cuda.synchronize()
    print(f"kernels-only done: {out.numel() * 4 / 1e6:.0f} MB per K26 / K6 launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    if args.kernels_only:
        kernels_only()
        return
    model = resnet50(seed=0).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        t = model(x).argmax(1)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model": "resnet50 seed 0", "pass_size": ablation.PASS_SIZE,
           "deterministic": True}
    td = {"models": [model, model], "img_hw": 224, "batch_size": 50, "device": DEV, "device_maps": True}
    batch = {"fa": lambda xs, ts, **kw: ablation.feature_ablation_batch(xs, model, ts, ablation.harness_patch_mask(224), **kw),
             "occ": lambda xs, ts, **kw: ablation.occlusion_batch(xs, model, ts, WINDOW, STRIDE, **kw)}
    for name, masks, weighted in (("fa", fa_masks(), False), ("occ", occ_masks(), True)):
        row = dict(td, attr_func=name)
        get_CNN_attr(x[:1], None, t[0], row)                          # first call: eager passes, capture, proof
        s1 = timed(lambda: get_CNN_attr(x[:1], None, t[0], row), 5)
        batch[name](x, t, want_map=14, attribution=False)
        s32 = timed(lambda: batch[name](x, t, want_map=14, attribution=False), 2)
        captum_flow(x[:1], model, int(t[0]), masks, weighted)        # warm
        sc = timed(lambda: captum_flow(x[1:2], model, int(t[1]), masks, weighted), 2)
        one = captum_flow(x[2:3], model, int(t[2]), masks, weighted)
        got = batch[name](x[2:3], t[2:3])
        res[name] = {"captum_flow_s": sc, "captum_flow_attr_per_s": 1 / sc, "harness_one_image_s": s1, "harness_one_image_attr_per_s": 1 / s1,
                     "batch32_s": s32, "batch32_attr_per_s": 32 / s32, "one_image_over_captum_flow": sc / s1,
                     "batch32_over_captum_flow": sc * 32 / s32, "engine_vs_captum_flow_rel_inf": rel_inf(got[0], one)}
    res["graph_counts"] = dict(ablation.ABLATION_COUNTS)
    for k, v in res.items():
        print(f"{k:20s} {json.dumps(v) if isinstance(v, dict) else v}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
