"""Three questions about MIOpen's backward-data of the stride-1 1x1 convolutions of ResNet-50 on planes of more than 64 positions (the
shapes of exp_wide_bwd_which_kernels.py), under deterministic solvers in immediate mode.
 1. Which K-walk is it?  K79 (`conv1x1_bwd_data(..., simple=True)`) over the walks of one partial sum against MIOpen's bits, at batch
    50 and batch 2; a row says MATCH or how many elements differ.  Where none matches: the GEMM kernels that serve those shapes are
    the ones whose names say SU32_SUS256, a K loop that starts at another iteration per output tile, so K81
    (`conv1x1_bwd_data_wide(..., simple=True)`) tries the staggered starts: loop depth 32 | 64, tiles of 32 | 64 | 128 along hw or
    along c, SU 2 .. 32, stride 256 bytes.  The matching ones are listed, and the closest of the others.
 2. Does K80 return K81's bits on the walk that matched, and what does it cost next to MIOpen's launch?
 3. What do MIOpen's launch and K80 cost while two other streams run classifier passes (ResNet-50, batch 50, forward and input
    gradient, each on its own host thread as xai_engine/streams.py has it)?  Timed with events around 20 calls on a third worker's
    stream once both others have finished two passes; autograd's host overhead is inside MIOpen's figures, alone and beside alike.
Output: profiles/wide_bwd_walk_probe.txt.
usage: python profiles/experiments/exp_wide_bwd_walk.py [output file]"""
import itertools
import os
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "image-classification-xai_amd"))
sys.path.insert(0, HERE)
import torch
from exp_wide_bwd_which_kernels import MORE_SHAPES, SHAPES, operands
from xai_engine import kernels as K
from xai_engine import streams, zoo

out = open(sys.argv[1] if len(sys.argv) > 1 else "wide_bwd_walk_probe.txt", "w")


def say(*a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


torch.backends.cudnn.deterministic = True
torch.backends.cudnn.benchmark = False
dev = torch.device("cuda", 0)
GROUPING = {0: "consecutive", 1: "stride-4"}
WALKS = [(1, 0, gr, 0, z) for gr, z in itertools.product((0, 1), (0, 1))]
# (grouping, from_zero, depth, tile, axis, stagger, stride)
STAGGERS = [(0, 0, d, t, ax, su, 256) for d, t, ax, su in itertools.product((64, 32), (32, 64, 128), (0, 1), (32, 16, 8, 4, 2))]


def name(walk):
    return f"S={walk[0]} k {GROUPING[walk[2]]:11s} from {'+0' if walk[4] else 'first'}"


def stagger_name(w):
    return f"depth {w[2]} tile {w[3]} along {'c' if w[4] else 'hw'} SU{w[5]} SUS{w[6]}"


def differing(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def timed(f, reps=20):
    for _ in range(3):
        f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.current_stream().synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.current_stream().synchronize()
    return a.elapsed_time(b) / reps * 1e3


g = torch.Generator(device="cuda").manual_seed(1)
held = []
for label, Kc, Cc, H, W, folded in SHAPES + MORE_SHAPES:
    found = {}
    for N in (50, 2):
        x, y, gy, weight = operands(torch, g, Kc, Cc, H, W, folded, N)
        (ref,) = torch.autograd.grad(y, x, gy, retain_graph=True)
        (again,) = torch.autograd.grad(y, x, gy, retain_graph=True)
        tag = f"{label} K={Kc} C={Cc} gy{tuple(gy.shape)}"
        say(f"{tag}: MIOpen backward-data twice, differing elements {differing(ref, again)} of {ref.numel()}")
        hits = []
        for walk in WALKS:
            d = differing(K.conv1x1_bwd_data(gy, weight, walk, simple=True), ref)
            say(f"{tag}: {name(walk)}  {'MATCH' if d == 0 else f'{d} differ'}")
            if d == 0:
                hits.append((walk[2], walk[4], 64, 64, 0, 0, 0))
        plain = K.conv1x1_bwd_data(gy, weight, WALKS[0], simple=True)
        say(f"{tag}: K81 without stagger against K79: {differing(K.conv1x1_bwd_data_wide(gy, weight, (0, 0, 64, 64, 0, 0, 0), simple=True), plain)} differ")
        if not hits:
            tried = []
            for w in STAGGERS:
                if Kc % w[2] == 0:
                    tried.append((differing(K.conv1x1_bwd_data_wide(gy, weight, w, simple=True), ref), w))
            for d, w in tried:
                if d == 0:
                    say(f"{tag}: {stagger_name(w)}  MATCH")
                    hits.append(w)
            d, w = min(tried, key=lambda t: (t[0] == 0, t[0]))
            say(f"{tag}: closest of the {len(tried) - len(hits)} others: {stagger_name(w)}  {d} differ")
        say(f"{tag}: matching walks: {len(hits)}")
        found[N] = hits
        if hits:
            w = hits[0]
            want = K.conv1x1_bwd_data_wide(gy, weight, w, simple=True)
            try:
                got = K.conv1x1_bwd_data_wide(gy, weight, w)
                say(f"{tag}: K80 on {stagger_name(w)}: {differing(got, want)} differ from K81, {differing(got, ref)} from MIOpen")
                buf = torch.empty_like(ref)
                flop = 2.0 * ref.numel() * Kc
                t_m = timed(lambda: torch.autograd.grad(y, x, gy, retain_graph=True))
                t_k = timed(lambda: K.conv1x1_bwd_data_wide(gy, weight, w, out=buf))
                say(f"{tag}: MIOpen {t_m:7.1f} us per call (with autograd's overhead), K80 {t_k:7.1f} us = {flop / t_k / 1e6:5.1f} TFLOP/s, "
                    f"{(gy.numel() + ref.numel()) * 4 / t_k / 1e3:6.0f} GB/s of gy + gx")
                if N == 50:
                    held.append((tag, (Kc, Cc, H, W, folded, N), w))
            except Exception as e:                                  # a walk K80 refuses (tiles along c)
                say(f"{tag}: K80 refuses {stagger_name(w)}: {e}")
        del x, y, gy, ref, again
    say(f"{label}: the same walk at batch 50 and batch 2: {bool(found[50]) and found[50][:1] == found[2][:1]}")

# ---- the premise: the launch alone, and beside two streams of classifier passes
model = zoo.resnet50().to(dev).eval()
ws = streams.workers(dev, 3)
stop = threading.Event()
passes = [0, 0]


def classifier_passes(i):
    xin = torch.randn(50, 3, 224, 224, device=dev).requires_grad_(True)
    last = None
    while not stop.is_set():
        torch.autograd.grad(model(xin).sum(), xin)
        ev = torch.cuda.Event()
        ev.record()
        if last is not None:                                        # the host stays one pass ahead of the device
            last.synchronize()
            passes[i] += 1
        last = ev
    torch.cuda.current_stream().synchronize()
    return passes[i]


def measure():
    # the operands are made on the measuring worker's own stream: autograd runs a backward node on its forward's stream
    res, gen = [], torch.Generator(device="cuda").manual_seed(2)
    for _, spec, w in held:
        x, y, gy, weight = operands(torch, gen, *spec)
        buf = torch.empty_like(x)
        res.append((timed(lambda: torch.autograd.grad(y, x, gy, retain_graph=True)),
                    timed(lambda: K.conv1x1_bwd_data_wide(gy, weight, w, out=buf))))
    return res


alone = ws[2].submit(measure).result()
busy = [ws[i].submit(lambda i=i: classifier_passes(i)) for i in (0, 1)]
while min(passes) < 2 and not any(f.done() for f in busy):
    time.sleep(0.05)
before = list(passes)
contended = ws[2].submit(measure).result()
during = [b - a for a, b in zip(before, passes)]
stop.set()
for f in busy:
    f.result()
say(f"classifier passes finished by the two other streams during the contended measurement: {during}")
for (tag, _, w), a, c in zip(held, alone, contended):
    say(f"{tag}: alone MIOpen {a[0]:7.1f} us, K80 {a[1]:7.1f} us; beside two streams of classifier passes MIOpen {c[0]:7.1f} us "
        f"(x{c[0] / a[0]:.2f}), K80 {c[1]:7.1f} us (x{c[1] / a[1]:.2f})")
say("DONE")
