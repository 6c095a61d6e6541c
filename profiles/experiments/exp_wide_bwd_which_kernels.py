"""MIOpen's backward-data of the stride-1 1x1 convolutions of layer1 and layer2 of ResNet-50 (gy channels K -> gx channels C on H x W),
one distinct site shape after the other, under deterministic solvers in immediate mode, batch 50 (backward five times) and batch 2
(seven times), and nothing else.  Between two shapes one launch of K79 on a 16 x 16 problem marks the border, so that a kernel trace
sorted by time says which rocBLAS kernel served which shape; run with MIOpen's logging it shows the solver.
usage: rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python3 profiles/experiments/exp_wide_bwd_which_kernels.py [--all]
       python3 profiles/experiments/exp_wide_bwd_which_kernels.py --summarize[-all] DIR/.../trace_kernel_trace.csv [output file]
(--all: layer3's and layer4's shapes after layer1's and layer2's; the summary keeps the GEMM library's kernels only)
       MIOPEN_ENABLE_LOGGING=1 MIOPEN_LOG_LEVEL=6 python3 profiles/experiments/exp_wide_bwd_which_kernels.py 2>&1 | grep -i solver"""
import os
import sys

# (label, gy channels K, gx channels C, H, W, batch folded into H: the compact shortcut view of DESIGN 5a (vii) runs at batch 1)
SHAPES = [("layer1 conv1 of block 0", 64, 64, 56, 56, False),
          ("layer1 conv1 of blocks 1-2", 64, 256, 56, 56, False),
          ("layer1 conv3, downsample.0", 256, 64, 56, 56, False),
          ("layer2 conv1 of block 0", 128, 256, 56, 56, False),
          ("layer2 conv3", 512, 128, 28, 28, False),
          ("layer2 conv1 of blocks 1-3", 128, 512, 28, 28, False),
          ("layer2 downsample.0, compact view", 512, 256, 28, 28, True)]
# the other stride-1 1x1 backward-data shapes of ResNet-50 (--all): whose launches the two slow rows of the trace really are
MORE_SHAPES = [("layer3 conv1 of block 0", 256, 512, 28, 28, False),
               ("layer3 conv3", 1024, 256, 14, 14, False),
               ("layer3 conv1 of blocks 1-5", 256, 1024, 14, 14, False),
               ("layer3 downsample.0, compact view", 1024, 512, 14, 14, True),
               ("layer4 conv1 of block 0", 512, 1024, 14, 14, False),
               ("layer4 conv1 of blocks 1-2", 512, 2048, 7, 7, False),
               ("layer4 downsample.0, compact view", 2048, 1024, 7, 7, True)]
BATCHES = ((50, 5), (2, 7))
MARK = "conv1x1_bwd_simple_kernel"


def operands(torch, g, K, C, H, W, folded, N, dev="cuda"):
    """x (requires grad), y = conv(x), gy and the weight, at batch N or on the (1, C, N*H, W) view"""
    import torch.nn.functional as F
    weight = torch.randn(K, C, 1, 1, device=dev, generator=g) * 0.05
    shape = (1, C, N * H, W) if folded else (N, C, H, W)
    x = torch.randn(shape, device=dev, generator=g).relu_().requires_grad_(True)
    y = F.conv2d(x, weight)
    return x, y, torch.randn(y.shape, device=dev, generator=g), weight


def run(shapes):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                    "image-classification-xai_amd"))
    import torch
    from xai_engine import kernels as Kn
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    g = torch.Generator(device="cuda").manual_seed(1)
    mg, mw = torch.randn(1, 16, 4, 4, device="cuda"), torch.randn(16, 16, device="cuda")
    for _, K, C, H, W, folded in shapes:
        for N, reps in BATCHES:
            x, y, gy, _ = operands(torch, g, K, C, H, W, folded, N)
            torch.cuda.synchronize()
            Kn.conv1x1_bwd_data(mg, mw, (1, 0, 0, 0, 0), simple=True)
            for _ in range(reps):
                torch.autograd.grad(y, x, gy, retain_graph=True)
            torch.cuda.synchronize()
    Kn.conv1x1_bwd_data(mg, mw, (1, 0, 0, 0, 0), simple=True)
    torch.cuda.synchronize()
    print("DONE")


def summarize(path, out, shapes):
    import collections
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    segments, cur = [], None
    for r in rows:
        if MARK in r["Kernel_Name"]:
            cur = collections.OrderedDict()
            segments.append(cur)
        elif cur is not None and r["Kernel_Name"].startswith("Cijk_") and "_Bjlk_" in r["Kernel_Name"]:
            a = cur.setdefault(r["Kernel_Name"], [0, 0])
            a[0] += 1
            a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    cases = [(s, N, reps) for s in shapes for N, reps in BATCHES]
    with open(out, "w") as f:
        for (s, N, reps), seg in zip(cases, segments):
            label, K, C, H, W, folded = s
            shape = f"(1, {K}->{C}, {N}*{H}, {W})" if folded else f"({N}, {K}->{C}, {H}, {W})"
            f.write(f"{label}: gy -> gx {shape}, {reps} backward calls (the first of them after MIOpen's trials of the shape)\n")
            for name, (n, t) in seg.items():
                f.write(f"  calls {n:3d}  avg {t / n / 1e3:8.1f} us  {name}\n")
            f.write("\n")
    print(open(out).read())


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1].startswith("--summarize"):
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "wide_bwd_rocblas_kernels.txt",
                  SHAPES + (MORE_SHAPES if sys.argv[1].endswith("-all") else []))
    else:
        run(SHAPES + (MORE_SHAPES if "--all" in sys.argv[1:] else []))
