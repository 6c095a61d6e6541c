#!/usr/bin/env python3
"""Transformer Attribution (xai_engine/lrp.py, K46-K52) on ViT-B/16 at 224^2; writes profiles/r15_lrp.txt.

    timeout -k 10 560 python profiles/bench_lrp.py --out profiles/r15_lrp.txt

calls    in one process, ms per image (median, min, max of REPS after a warm-up; a host clock around work that ends in a
         synchronisation): the one-image generate_LRP eager and replayed from its hipGraph, transformer_attribution_batch at B = 32
         replayed, and the reference's flow restated below as torch ops on the device -- the same forward and backward, then every
         relprop with torch.autograd.grad inside it and the inhibitor term of Linear.relprop computed, as the reference does.
launches per transformer block, for both flows: the aten operators a torch dispatch mode sees (each is at least one kernel launch)
         plus the engine's own HIP launches, counted over one eager relevance pass and divided by the depth.
kernels  K46-K52 alone at the shapes of one ViT-B/16 image: LAUNCHES launches captured as one hipGraph, device events around a
         replay (the fastest of 5), so that the host's launch rate is not what is measured.
GEMMs    every GEMM shape of the pass, timed alone the same way, times how often the pass calls it: the GEMM share of the replayed
         one-image call.
The claim to confirm or refute: the restated flow is bound by its launches, the replayed pass by its GEMMs.  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
REPS = 15
LAUNCHES = 100
BATCH = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_lrp.txt"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from torch.utils._python_dispatch import TorchDispatchMode
    from xai_engine import kernels as K
    from xai_engine import lrp
    from xai_engine.zoo import vit_base_patch16_224
    if not torch.cuda.is_available():
        raise SystemExit("bench_lrp: no GPU")
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ViT-B/16 (random weights), 224 x 224; median, min, max "
             f"of {REPS} calls after a warm-up; kernels and GEMMs: mean of {LAUNCHES} launches inside one hipGraph replay, fastest of 5", ""]

    def stats_ms(fn, reps=REPS, warm=3, per=1):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / per)
        return "%9.3f %9.3f %9.3f" % (statistics.median(ts), min(ts), max(ts)), statistics.median(ts)

    def event_us(fn, launches=LAUNCHES):
        """device time per launch: `launches` launches captured as one hipGraph (no host in between), the fastest of 5 replays"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(launches):
                fn()
        graph.replay()
        best = float("inf")
        for _ in range(5):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            graph.replay()
            stop.record()
            torch.cuda.synchronize()
            best = min(best, start.elapsed_time(stop) * 1e3 / launches)
        return best

    model = vit_base_patch16_224(seed=0).to(DEV)
    depth, heads = len(model.blocks), model.blocks[0].attn.heads
    gen = torch.Generator().manual_seed(1)
    xs = torch.randn(BATCH, 3, 224, 224, generator=gen).to(DEV)
    x = xs[:1].contiguous()
    with torch.no_grad():
        target = int(model(x).argmax(1)[0])

    # ---- the reference's flow restated as torch ops: autograd inside every relprop, the inhibitor computed
    sd = lrp.safe_divide

    def leaf(t):
        return t.detach().requires_grad_(True)

    def ref_linear(R, X, W):
        pw, nw, px, nx = W.clamp(min=0), W.clamp(max=0), X.clamp(min=0), X.clamp(max=0)

        def f(w1, w2):
            x1, x2 = leaf(px), leaf(nx)
            z1, z2 = F.linear(x1, w1), F.linear(x2, w2)
            s1, s2 = sd(R, z1 + z2), sd(R, z1 + z2)
            return x1 * torch.autograd.grad(z1, x1, s1)[0] + x2 * torch.autograd.grad(z2, x2, s2)[0]
        return 1 * f(pw, nw) - 0 * f(nw, pw)

    def ref_pair(R, a, b, op):
        a, b = leaf(a), leaf(b)
        z = op(a, b)
        ca, cb = torch.autograd.grad(z, (a, b), sd(R, z))
        return a * ca, b * cb

    def ref_add(R, a, b):
        a, b = ref_pair(R, a, b, torch.add)
        sa, sb = a.sum(), b.sum()
        fa = sd(sa.abs(), sa.abs() + sb.abs()) * R.sum()
        fb = sd(sb.abs(), sa.abs() + sb.abs()) * R.sum()
        return a * sd(fa, a.sum()), b * sd(fb, b.sum())

    def ref_clone(X, r1, r2):
        X = leaf(X)
        return X * torch.autograd.grad((X, X), X, (sd(r1, X), sd(r2, X)))[0]

    def ref_pass(tape, tgt, attns, grads):
        one_hot = torch.zeros_like(tape.logits).scatter_(1, tgt.view(-1, 1), 1.0)
        cam = ref_linear(one_hot, tape.top["head_in"], model.head.weight)
        x0 = tape.top["norm_out"][:, :1]
        R = torch.zeros_like(tape.top["norm_out"])
        R[:, :1] = x0 * sd(cam[:, None], x0)
        cams = []
        for i in range(depth - 1, -1, -1):
            blk, rec = model.blocks[i], tape.blocks[i]
            c1, c2 = ref_add(R, rec["x_mid"], rec["mlp_out"])
            c2 = ref_linear(ref_linear(c2, rec["g"], blk.mlp.fc2.weight), rec["n2"], blk.mlp.fc1.weight)
            R = ref_clone(rec["x_mid"], c1, c2)
            c1, c2 = ref_add(R, rec["x_in"], rec["attn_out"])
            c = ref_linear(c2, rec["pv"], blk.attn.proj.weight)
            B, N, D = c.shape
            c = c.reshape(B, N, heads, D // heads).permute(0, 2, 1, 3)
            q, k, v = lrp.split_heads(rec["qkv"], heads)
            camA, camv = ref_pair(c, attns[i], v, lambda a, b: torch.einsum("bhij,bhjd->bhid", a, b))
            camA, camv = camA / 2, camv / 2
            cams.append(camA)
            camq, camk = ref_pair(camA, q, k, lambda a, b: torch.einsum("bhid,bhjd->bhij", a, b))
            cam_qkv = torch.stack([camq / 2, camk / 2, camv]).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * D)
            R = ref_clone(rec["x_in"], c1, ref_linear(cam_qkv, rec["n1"], blk.attn.qkv.weight))
        mats = [(grads[i][0] * cam[0]).clamp(min=0).mean(dim=0)[None] for i, cam in zip(range(depth), reversed(cams))]
        aug = torch.stack(mats) + torch.eye(mats[0].shape[-1], device=DEV)
        aug = aug / aug.sum(dim=-1, keepdim=True)
        joint = aug[0]
        for i in range(1, depth):
            joint = aug[i].bmm(joint)
        return joint[:, 0, 1:]

    def ref_flow():
        tape, tgt, attns, grads = lrp.record(model, x, torch.tensor([target], device=DEV), True)
        return ref_pass(tape, tgt, attns, grads)

    eager = lrp.LRP(model)
    replayed = lrp.LRP(model, graphs=True)
    got = eager.generate_LRP(x, target, device=DEV)
    ref = ref_flow().detach().reshape(1, 14, 14)
    lines.append(f"engine against the restated reference flow on this input: max|a - b| / max|b| = "
                 f"{float((got - ref).abs().max() / ref.abs().max()):.2e}")
    lines += ["", "calls: ms per image (median, min, max)"]
    txt, _ = stats_ms(lambda: eager.generate_LRP(x, target, device=DEV))
    lines.append(f"  generate_LRP, eager                                   {txt}")
    txt, t_replayed = stats_ms(lambda: replayed.generate_LRP(x, target, device=DEV))
    lines.append(f"  generate_LRP, replayed (one hipGraph)                 {txt}")
    targets = torch.full((BATCH,), target)
    txt, _ = stats_ms(lambda: lrp.transformer_attribution_batch(xs, model, targets), reps=5, warm=1, per=BATCH)
    lines.append(f"  transformer_attribution_batch, B = {BATCH}, replayed        {txt}")
    txt, _ = stats_ms(ref_flow)
    lines.append(f"  the reference's flow restated as torch ops            {txt}")
    lines.append(f"  graph counters: {dict(lrp.LRP_COUNTS)}")

    # ---- launches per block
    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.overloadpacket.__name__
            if name not in ("detach", "view", "_unsafe_view", "reshape", "permute", "transpose", "t", "expand", "slice", "select", "alias",
                            "unsqueeze", "squeeze", "as_strided", "_reshape_alias", "empty", "empty_like", "empty_strided"):
                self.n += 1
            return func(*args, **(kwargs or {}))

    tape, tgt, attns, grads = lrp.record(model, x, torch.tensor([target], device=DEV), True)
    hip = [0]
    call = K._call

    def counted(*a, lib="hip"):
        hip[0] += lib == "ext4"                      # K46-K52 are the launches of libxai_ext4.so
        return call(*a, lib=lib)
    K._call = counted
    with Count() as c:
        lrp.relevance_pass(model, tape, tgt, attns, list(range(depth)))
    K._call = call
    lines += ["", "launches per transformer block over one eager relevance pass (aten operators that are not views, plus HIP launches)",
              f"  engine:            {c.n / depth:7.1f} aten operators + {hip[0] / depth:5.1f} launches of K46-K51"]
    with Count() as c:
        ref_pass(tape, tgt, attns, grads)
    lines.append(f"  restated reference: {c.n / depth:7.1f} aten operators")

    # ---- kernels at the shapes of one image
    N, D = tape.blocks[0]["x_in"].shape[1:]
    r = lambda *s: torch.randn(*s, device=DEV)                                  # noqa: E731
    a3, b3, c3, wide = r(1, N, D), r(1, N, D), r(1, N, D), r(1, N, 4 * D)
    a4, b4 = r(1, heads, N, N), r(1, heads, N, N)
    q4, c4 = r(1, heads, N, D // heads), r(1, heads, N, D // heads)
    qkv = torch.empty(1, N, 3 * D, device=DEV)
    cam5, grad5 = r(depth, 1, heads, N, N), r(depth, 1, heads, N, N)
    ws = torch.empty(K._lib.load("ext4").xai_lrp_add_workspace_bytes(1, N * D), dtype=torch.uint8, device=DEV)
    o1, o2 = torch.empty_like(a3), torch.empty_like(a3)
    ow1, ow2 = torch.empty_like(wide), torch.empty_like(wide)
    o4 = torch.empty_like(a4)
    lines += ["", "kernels: device us per launch at one ViT-B/16 image (N = %d, D = %d, h = %d)" % (N, D, heads)]
    for name, fn in (("K46 split (N x D)", lambda: K.lrp_split(a3, o1, o2)), ("K46 split (N x 4D)", lambda: K.lrp_split(wide, ow1, ow2)),
                     ("K47 ratio (N x D, z1 + z2)", lambda: K.lrp_ratio(a3, b3, c3, out=o1)),
                     ("K47 ratio (h x N x N)", lambda: K.lrp_ratio(a4, b4, out=o4)),
                     ("K48 gather (N x 4D)", lambda: K.lrp_gather(wide, ow1, ow2, out=ow1)),
                     ("K49 half product (h x N x N)", lambda: K.lrp_half_product(a4, b4, out=o4)),
                     ("K49 half product into cam_qkv", lambda: K.lrp_half_product(q4, c4, out=qkv, slot=1)),
                     ("K50 add (two launches)", lambda: K.lrp_add(a3, b3, c3, a=o1, b=o2, ws=ws)),
                     ("K51 clone (N x D)", lambda: K.lrp_clone(a3, b3, c3, out=o1)),
                     ("K52 matrices, 12 blocks, rollout", lambda: K.lrp_attn_matrices(cam5, grad5, K.LRP_ROLLOUT))):
        lines.append(f"  {name:36s} {event_us(fn):9.1f} us")

    # ---- the GEMMs of one image's pass
    hd = D // heads
    w1, w4 = r(D, D), r(4 * D, D)
    w3, wh = r(3 * D, D), r(model.head.weight.shape[0], D)
    s3, s4, sq = r(1, N, D), r(1, N, 4 * D), r(1, N, 3 * D)
    shapes = [("X W^T, W (D, D): proj", lambda: torch.matmul(a3, w1.t()), 2 * depth), ("S W, W (D, D): proj", lambda: torch.matmul(s3, w1), 2 * depth),
              ("X W^T, W (4D, D): fc1", lambda: torch.matmul(a3, w4.t()), 2 * depth), ("S W, W (4D, D): fc1", lambda: torch.matmul(s4, w4), 2 * depth),
              ("X W^T, W (D, 4D): fc2", lambda: torch.matmul(wide, w4), 2 * depth), ("S W, W (D, 4D): fc2", lambda: torch.matmul(s3, w4.t()), 2 * depth),
              ("X W^T, W (3D, D): qkv", lambda: torch.matmul(a3, w3.t()), 2 * (depth - 1)), ("S W, W (3D, D): qkv", lambda: torch.matmul(sq, w3), 2 * (depth - 1)),
              ("A V", lambda: torch.matmul(a4, q4), depth), ("S V^T", lambda: torch.matmul(q4, c4.transpose(-1, -2)), depth),
              ("A^T S", lambda: torch.matmul(a4.transpose(-1, -2), q4), depth - 1), ("Q K^T", lambda: torch.matmul(q4, c4.transpose(-1, -2)), depth - 1),
              ("S K, S^T Q", lambda: torch.matmul(a4, q4), 2 * (depth - 1))]
    lines += ["", "GEMMs of one image's relevance pass: device us per call, calls per pass"]
    total = 0.0
    for name, fn, calls in shapes:
        us = event_us(fn)
        total += us * calls
        lines.append(f"  {name:28s} {us:9.1f} us x {calls}")
    lines.append(f"  all GEMMs of the pass: {total / 1e3:.3f} ms = {100 * total / 1e3 / t_replayed:.0f}% of the replayed one-image call "
                 f"({t_replayed:.3f} ms, which also holds the classifier's forward and backward)")
    lrp.clear_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
