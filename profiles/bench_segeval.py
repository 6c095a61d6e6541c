#!/usr/bin/env python3
"""The per-image scoring of the segmentation evaluation (K44 + K45, xai_engine/segeval.py) at 224^2; writes profiles/r14_segeval.txt.

    timeout -k 10 500 python profiles/bench_segeval.py --out profiles/r14_segeval.txt

scoring  per image: the device scoring (K44 + K45 + one read-back of the count table + scores_from_counts on the host) at B = 1 and
         B = 32 maps per call, against the host flow restated in the same process (tests/seg_restated.py: the map read back, NumPy
         masks, sklearn's average_precision_score on 2 x 50176 samples and f1_score once per image row).  A host clock around work
         that ends in a read-back, warmed, the median of REPS.
rows     the harness rows `gc` and `grad` on ResNet-50 (sweep.get_CNN_attr with device maps), per image: the attribution alone, then
         followed by either scoring path.
kernels  K44 and K45 alone at B = 1 and B = 32: device events around LAUNCHES launches after a warm-up; the bytes each must move
         (K44: two reads and a write of the map; K45: the map and the labels once) over that time.
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
HOST_REPS = 3
LAUNCHES = 200
HW = 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_segeval.txt"))
    args = ap.parse_args()
    import numpy as np
    import sklearn
    import torch
    import seg_restated as R
    from xai_engine import kernels as K
    from xai_engine import segeval
    from xai_engine.sweep import get_CNN_attr
    from xai_engine.zoo import resnet50
    if not torch.cuda.is_available():
        raise SystemExit("bench_segeval: no GPU")
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; sklearn {sklearn.__version__}; {HW} x {HW}; "
             f"median of {REPS} (device paths) / {HOST_REPS} (host flow), mean of {LAUNCHES} launches (kernels)", ""]

    def median_ms(fn, reps=REPS, warm=3):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    cases = [R.seeded_case("smooth", 100 + i) for i in range(32)]
    maps = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)
    labels = torch.from_numpy(np.stack([c[1] for c in cases])).to(DEV, torch.int32)

    def host_flow(m, lab):
        res = R.normalize(m.cpu().numpy())
        return R.host_scores(res, R.stated_mean(res), lab.cpu().numpy())

    got, want = segeval.eval_batch_device(maps[:1], labels[:1])[0], host_flow(maps[0], labels[0])
    same = all(np.array_equal(np.asarray(a).ravel(), np.asarray(b).ravel()) for a, b in zip(got, want))
    lines.append(f"scoring: ms per image (median, min, max); device and host scores of the first map equal: {same}")
    for B in (1, 32):
        med, lo, hi = median_ms(lambda: segeval.eval_batch_device(maps[:B], labels[:B]))
        lines.append(f"  device scoring, B = {B:2d} (K44 + K45 + read-back + scores_from_counts)  {med / B:9.3f} {lo / B:9.3f} {hi / B:9.3f}")
    lines.append(f"  host flow restated (read-back, NumPy masks, sklearn AP and 224 F1s)      "
                 f"{'%9.3f %9.3f %9.3f' % median_ms(lambda: host_flow(maps[0], labels[0]), HOST_REPS, 1)}")

    model = resnet50(seed=0)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(DEV).eval()
    x = torch.randn(1, 3, HW, HW, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        target = model(x.to(DEV)).argmax(1)[0]
    lines += ["", "rows: ms per image on ResNet-50 (median, min, max)"]
    for row in ("gc", "grad"):
        td = {"models": [model, model], "img_hw": HW, "batch_size": 50, "device": DEV, "attr_func": row, "device_maps": True}

        def attribution():
            return get_CNN_attr(x, None, target, td).detach().reshape(1, HW, HW)

        lines.append(f"  {row}: {'attribution alone':44s} {'%9.3f %9.3f %9.3f' % median_ms(attribution)}")
        lines.append(f"  {row}: {'attribution + device scoring (B = 1)':44s} "
                     f"{'%9.3f %9.3f %9.3f' % median_ms(lambda: segeval.eval_batch_device(attribution(), labels[:1]))}")

        def batch_of_32():
            buf = torch.empty((32, HW, HW), dtype=torch.float32, device=DEV)
            for i in range(32):
                buf[i].copy_(attribution()[0])
            return segeval.eval_batch_device(buf, labels)

        med, lo, hi = median_ms(batch_of_32, 5, 1)
        lines.append(f"  {row}: {'attribution + device scoring (B = 32)':44s} {med / 32:9.3f} {lo / 32:9.3f} {hi / 32:9.3f}")
        lines.append(f"  {row}: {'attribution + read-back + host flow':44s} "
                     f"{'%9.3f %9.3f %9.3f' % median_ms(lambda: host_flow(attribution()[0], labels[0]), HOST_REPS, 1)}")

    lines += ["", "kernels: us per launch (includes the wrapper's allocations), GB/s of the bytes the kernel must move"]
    for B in (1, 32):
        m, lab = maps[:B].contiguous(), labels[:B].contiguous()
        res, thr, _ = K.seg_normalize(m)
        thr1, thr12 = thr.view(B, 1), thr.view(B, 1).repeat(1, 12).contiguous()
        px = B * HW * HW
        for name, fn, nbytes in (("K44 normalize + mean", lambda: K.seg_normalize(m), 12 * px),
                                 ("K45 counts, T = 1", lambda: K.seg_counts(res, lab, thr1), 8 * px),
                                 ("K45 counts, T = 12", lambda: K.seg_counts(res, lab, thr12), 8 * px)):
            for _ in range(10):
                fn()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(LAUNCHES):
                fn()
            stop.record()
            torch.cuda.synchronize()
            us = start.elapsed_time(stop) * 1e3 / LAUNCHES
            lines.append(f"  B = {B:2d}: {name:24s} {us:10.1f} us {nbytes / us / 1e3:10.1f} GB/s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
