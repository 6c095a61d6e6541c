"""Which K-walk reproduces MIOpen's backward-data of layer4.0.conv3 (1x1, 512 <- 2048 channels on 7x7) bit for bit under deterministic
solvers in immediate mode, at batch 50 and at the verify batch 2.  MIOpen hands the call to rocBLAS, which
answers with a global split-K GEMM and a reduction kernel (profiles/conv3_bwd_rocblas_kernels.txt has their names); the simple kernel
K79 (one wave per 16x16 outputs, operands from global memory, v_mfma_f32_16x16x4_f32) restates the sum with the walk as data: split
membership, k grouping, partial-sum order.  Every walk of 1, 2, 3, 4 and 19 partial sums is tried; a row says whether it is MIOpen's
bits and, if not, how many elements differ.  (A first run without 19 matched nothing, and MIOpen's result was ten times closer to the
fp64 sum than any of its walks: more, shorter partial sums.  The GEMM kernel's own name says GSU19.)  Also: K79 against an fp64 sum
(the operand layout), K78 against K79 on a few walks and both tile heights, and a first timing of K78 next to MIOpen.
Output: profiles/conv3_bwd_walk_probe.txt.
usage: python profiles/experiments/exp_conv3_bwd_walk.py [output file]"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import torch
import torch.nn.functional as F
from xai_engine import kernels as K

out = open(sys.argv[1] if len(sys.argv) > 1 else "conv3_bwd_walk_probe.txt", "w")


def say(*a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


torch.backends.cudnn.deterministic = True
torch.backends.cudnn.benchmark = False
dev = "cuda"
MEMBERSHIP = {0: "contiguous", 1: "round-robin"}
GROUPING = {0: "consecutive", 1: "stride-4"}
ORDER = {0: "ascending", 1: "descending"}
# 3: the reduction kernel is called PostGSU3; 19: the GEMM kernel's own name says GSU19 (its full name is in the kernel trace)
SPLITS = (1, 2, 3, 4, 19)


def name(walk):
    s, m, g, o, z = walk
    return f"S={s} {MEMBERSHIP[m]:11s} k {GROUPING[g]:11s} {ORDER[o]:10s} from {'+0' if z else 'first'}"


def differing(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def timed(f, reps=20):
    for _ in range(3):
        f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


g = torch.Generator(device=dev).manual_seed(1)
Cin, Cout, H = 512, 2048, 7
W = torch.randn(Cout, Cin, 1, 1, device=dev, generator=g) * 0.05
accepted = {}
for N in (50, 2):
    x = torch.randn(N, Cin, H, H, device=dev, generator=g).relu_().requires_grad_(True)
    y = F.conv2d(x, W)
    gy = torch.randn(y.shape, device=dev, generator=g)
    (ref,) = torch.autograd.grad(y, x, gy, retain_graph=True)
    (again,) = torch.autograd.grad(y, x, gy, retain_graph=True)
    say(f"N={N}: MIOpen backward-data twice, differing elements {differing(ref, again)} of {ref.numel()}")
    exact = torch.einsum("nkp,kc->ncp", gy.double().view(N, Cout, H * H), W.double().view(Cout, Cin)).view_as(ref)
    scale = float(exact.abs().max())
    say(f"N={N}: MIOpen against the fp64 sum: max |diff| / max |gx| = {float((ref.double() - exact).abs().max()) / scale:.3e}")
    first = K.conv1x1_bwd_data(gy, W, (1, 0, 0, 0, 0), simple=True)
    say(f"N={N}: K79 (S=1) against the fp64 sum: max |diff| / max |gx| = {float((first.double() - exact).abs().max()) / scale:.3e}")
    hits = []
    for s in SPLITS:
        for m, gr, o, z in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
            if s == 1 and (m or o):
                continue                      # one partial sum: membership and order say nothing
            walk = (s, m, gr, o, z)
            got = K.conv1x1_bwd_data(gy, W, walk, simple=True)
            d = differing(got, ref)
            say(f"N={N}: {name(walk)}  {'MATCH' if d == 0 else f'{d} differ'}")
            if d == 0:
                hits.append(walk)
    accepted[N] = hits
    say(f"N={N}: matching walks: {[name(w) for w in hits] or 'none'}")
    # K78 against K79, bit for bit, on the walks that matter and both tile heights
    for walk in (hits[:2] or [(19, 1, 0, 0, 0)]) + [(3, 0, 1, 1, 1), (1, 0, 0, 0, 0)]:
        want = K.conv1x1_bwd_data(gy, W, walk, simple=True)
        for tm in (32, 64):
            say(f"N={N}: K78 tile_rows={tm} {name(walk)}: {differing(K.conv1x1_bwd_data(gy, W, walk, tile_rows=tm), want)} differ from K79")
    walk = (hits or [(19, 1, 0, 0, 0)])[0]
    buf = torch.empty_like(ref)
    say(f"N={N}: MIOpen backward-data {timed(lambda: torch.autograd.grad(y, x, gy, retain_graph=True)):.1f} us per call (with autograd's overhead)")
    for tm in (32, 64):
        say(f"N={N}: K78 tile_rows={tm} {name(walk)}: {timed(lambda: K.conv1x1_bwd_data(gy, W, walk, tile_rows=tm, out=buf)):.1f} us per call")
    say(f"N={N}: K79 {timed(lambda: K.conv1x1_bwd_data(gy, W, walk, simple=True, out=buf)):.1f} us per call")
    del x, y, gy, ref
say("DONE")
