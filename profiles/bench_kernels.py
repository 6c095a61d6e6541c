#!/usr/bin/env python3
"""Per-kernel micro-benchmark at BASELINE shapes (HIP events around bursts of back-to-back launches): achieved
algorithmic GB/s of every C-ABI kernel against the 8 TB/s HBM peak.  Run on the GPU box:
    python profiles/bench_kernels.py [--json out.json]
Working sets are sized past the 256 MiB Infinity Cache where the shape allows it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from xai_engine import kernels as K  # noqa: E402

DEV = "cuda:0"
PEAK = 8000.0


def timeit(fn, iters=9, warm=2, burst=None):
    """ms per launch: HIP events around a back-to-back BURST of launches (amortises the ~10 us of host
    launch latency that a single event-bracketed call would include), median over `iters` bursts."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    one = max(a.elapsed_time(b), 1e-3)
    burst = burst or int(min(50, max(4, round(2.0 / one))))          # ~2 ms of work per burst
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / burst)
    return float(np.median(ts))


def conv1x1_rows(rep):
    """K78 at layer4's conv3 backward-data, 50 x 2048 -> 512 x 7 x 7, next to MIOpen's launch (a rocBLAS GSU19 GEMM and its
    reduction kernel) on the same tensors under deterministic solvers, and K79 for scale.  The bytes are the algorithmic ones: gy and
    the weight read once, gx written once; the kernel is a 5.14 GFLOP GEMM, so `note` carries TFLOP/s."""
    import torch.nn.functional as F
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    g = torch.Generator(device=DEV).manual_seed(1)
    w = torch.randn(2048, 512, 1, 1, device=DEV, generator=g) * 0.05
    x = torch.randn(50, 512, 7, 7, device=DEV, generator=g).requires_grad_(True)
    y = F.conv2d(x, w)
    gy = torch.randn(y.shape, device=DEV, generator=g)
    nbytes = (gy.numel() + w.numel() + x.numel()) * 4
    flop = 2.0 * 2048 * x.numel()
    walk = (19, K.WALK_ROUND_ROBIN, K.WALK_K_CONSECUTIVE, K.WALK_ASCENDING, 0)
    out = torch.empty_like(x)
    (ref,) = torch.autograd.grad(y, x, gy, retain_graph=True)
    same = bool((K.conv1x1_bwd_data(gy, w, walk).view(torch.int32) == ref.view(torch.int32)).all())
    ms = timeit(lambda: torch.ops.aten.convolution_backward(gy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, (True, False, False)))
    rep("MIOpen conv3 bwd-data 50x2048->512x7x7", nbytes, ms, f"{flop / ms / 1e9:.1f} TFLOP/s; GEMM + reduction kernel")
    for tile in (64, 32):
        ms = timeit(lambda: K.conv1x1_bwd_data(gy, w, walk, tile_rows=tile, out=out))
        rep(f"conv1x1_bwd_data tile_rows={tile}", nbytes, ms, f"{flop / ms / 1e9:.1f} TFLOP/s; MIOpen's bits: {same}")
    ms = timeit(lambda: K.conv1x1_bwd_data(gy, w, walk, simple=True, out=out))
    rep("conv1x1_bwd_data simple (K79)", nbytes, ms, f"{flop / ms / 1e9:.1f} TFLOP/s")
    torch.backends.cudnn.deterministic = det


def conv1x1_wide_rows(rep):
    """K80 at the enabled large-plane shapes of ResNet-50's backward-data, batch 50, next to MIOpen's launch (a
    rocBLAS MT32x32x64 or MT32x64x64 GEMM per image) on the same tensors under deterministic solvers, and K79 for scale.  The bytes are
    the algorithmic ones: gy and the weight read once, gx written once; every row is a 5.14 GFLOP GEMM, so `note` carries TFLOP/s and
    the share of the launch's lower bound, the larger of 33 us (155 TFLOP/s) and bytes / 6.29 TB/s."""
    import torch.nn.functional as F
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    g = torch.Generator(device=DEV).manual_seed(1)
    walk = (0, 0, 64, 32, 0, 32, 256)
    for name, Kc, Cc, H in (("layer2 conv3", 512, 128, 28), ("layer3 conv3", 1024, 256, 14), ("layer3 conv1", 256, 1024, 14),
                            ("layer4.0 conv1", 512, 1024, 14)):
        w = torch.randn(Kc, Cc, 1, 1, device=DEV, generator=g) * 0.05
        x = torch.randn(50, Cc, H, H, device=DEV, generator=g).requires_grad_(True)
        y = F.conv2d(x, w)
        gy = torch.randn(y.shape, device=DEV, generator=g)
        nbytes = (gy.numel() + w.numel() + x.numel()) * 4
        flop = 2.0 * Kc * x.numel()
        floor_ms = max(flop / 155e9, nbytes / 6.29e9)
        out = torch.empty_like(x)
        (ref,) = torch.autograd.grad(y, x, gy, retain_graph=True)
        same = bool((K.conv1x1_bwd_data_wide(gy, w, walk).view(torch.int32) == ref.view(torch.int32)).all())
        shape = f"50x{Kc}->{Cc}x{H}x{H}"
        ms = timeit(lambda: torch.ops.aten.convolution_backward(gy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, (True, False, False)))
        rep(f"MIOpen {name} bwd-data {shape}", nbytes, ms, f"{flop / ms / 1e9:.1f} TFLOP/s; {floor_ms / ms:.2f} of the bound")
        ms = timeit(lambda: K.conv1x1_bwd_data_wide(gy, w, walk, out=out))
        rep(f"conv1x1_bwd_data_wide (K80) {shape}", nbytes, ms, f"{flop / ms / 1e9:.1f} TFLOP/s; {floor_ms / ms:.2f} of the bound; MIOpen's bits: {same}")
        ms = timeit(lambda: K.conv1x1_bwd_data(gy, w, (1, 0, 0, 0, 0), simple=True, out=out))
        rep(f"conv1x1_bwd_data simple (K79) {shape}", nbytes, ms, f"{flop / ms / 1e9:.1f} TFLOP/s")
    torch.backends.cudnn.deterministic = det


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--json")
    ap.add_argument("--only", choices=["conv1x1", "conv1x1_wide"], help="run one group of rows only")
    args = ap.parse_args()
    res = []

    def rep(name, nbytes, ms, note=""):
        gbs = nbytes / ms / 1e6
        res.append(dict(kernel=name, bytes=nbytes, us=ms * 1e3, gbs=gbs, frac=gbs / PEAK, note=note))
        print(f"{name:34s} {nbytes / 1e6:10.1f} MB {ms * 1e3:9.1f} us {gbs:8.1f} GB/s  frac={gbs / PEAK:.3f}  {note}")

    if args.only in ("conv1x1", "conv1x1_wide"):
        (conv1x1_rows if args.only == "conv1x1" else conv1x1_wide_rows)(rep)
        if args.json:
            json.dump(res, open(args.json, "w"), indent=1)
        return
    C, H, W = 3, 224, 224
    N = C * H * W
    B, S = 32, 50
    g = torch.randn(B, S, C, H, W, device=DEV)
    x = torch.randn(B, C, H, W, device=DEV)
    al = torch.linspace(0, 1, S).to(DEV)
    # K2
    ms = timeit(lambda: K.ig_accum(g, x, 0.0, want_abs=True))
    rep("ig_accum  32img x 50 steps (+abs)", B * (S + 2) * 4 * N + B * H * W * 4, ms)
    nu = torch.full((B,), 37, dtype=torch.int32, device=DEV)
    ms = timeit(lambda: K.ig_accum(g, x, 0.0, n_use=nu))
    rep("ig_accum  Left-IG n_use=37", B * (37 + 2) * 4 * N, ms)
    ms = timeit(lambda: K.ig_accum(g[:1], x[:1], 0.0, want_abs=True))
    rep("ig_accum  1 image (cache-resident)", (S + 2) * 4 * N + H * W * 4, ms, "30 MB: Infinity-Cache resident")
    # K1
    out = torch.empty(B, S, C, H, W, device=DEV)
    ms = timeit(lambda: K.ig_interp(x, 0.0, al, out=out))
    rep("ig_interp 32img x 50 steps", B * (S + 1) * 4 * N, ms)
    ms = timeit(lambda: K.ig_interp(x[:2], 0.0, al, out=out[:2]))
    rep("ig_interp 2img x 50 steps", 2 * (S + 1) * 4 * N, ms, "60 MB")
    # streaming add
    acc = torch.zeros(C, H, W, device=DEV)
    ms = timeit(lambda: K.ig_accum_add(g[0], acc))
    rep("ig_accum_add 50 rows", (S + 2) * 4 * N, ms, "30 MB")
    # K6
    start, finish = x[0].contiguous(), torch.zeros_like(x[0])
    sal = torch.rand(1, H * W, device=DEV)
    ms = timeit(lambda: K.rank(sal))
    rep("rank 50176 keys", 4 * H * W * 8 * 2, ms, "4 passes x (key+idx) r+w, L2-resident; zero-fill kernel + 9 launches")
    order, rk = K.rank(sal)
    flip = K.flip_steps(rk[0], True, 224)
    buf = torch.empty(224, C, H, W, device=DEV)
    ms = timeit(lambda: K.perturb_batch(start, finish, flip, 0, 50, out=buf[:50]))
    rep("perturb_batch 50 steps", 50 * 4 * N + 2 * 4 * N + 4 * H * W, ms, "30 MB")
    ms = timeit(lambda: K.perturb_batch(start, finish, flip, 0, 224, out=buf))
    rep("perturb_batch 224 steps", 224 * 4 * N + 2 * 4 * N + 4 * H * W, ms, "135 MB")
    # K7
    k1d = torch.ones(31, device=DEV) / 31
    xb = torch.randn(32, C, H, W, device=DEV)
    ms = timeit(lambda: K.blur_sep(xb, k1d))
    rep("blur_sep 31 taps, 32 images", 2 * 32 * 4 * N, ms)
    ms = timeit(lambda: K.blur_sep(xb[:1], k1d))
    rep("blur_sep 31 taps, 1 image", 2 * 4 * N, ms)
    # K3
    act = torch.randn(32, 2048, 7, 7, device=DEV); grad = torch.randn(32, 2048, 7, 7, device=DEV)
    ms = timeit(lambda: K.gradcam(act, grad))
    rep("gradcam 32 x 2048x7x7", 2 * act.numel() * 4 + 32 * 49 * 4, ms)
    ms = timeit(lambda: K.gradcam(act[:1], grad[:1]))
    rep("gradcam 1 x 2048x7x7", 2 * 2048 * 49 * 4 + 49 * 4, ms, "latency-bound")
    cam = K.gradcam(act, grad)
    ms = timeit(lambda: K.bilinear_up(cam, 224, 224, 3.0, True))
    rep("bilinear_up 32 x 7x7->224x224", 32 * (49 + H * W) * 4, ms)
    # K4 / K5
    n = 1000
    grid = (torch.rand(n, 8, 8, device=DEV) < 0.5).to(torch.uint8)
    sh = torch.randint(0, 28, (n, 2), device=DEV, dtype=torch.int32)
    mbuf = torch.empty(n, C, H, W, device=DEV)
    ms = timeit(lambda: K.rise_apply(grid, sh, (28, 28), x[0].contiguous(), out=mbuf))
    rep("rise_apply 1000 masks", n * 4 * N + 4 * N, ms, "602 MB written")
    ms = timeit(lambda: K.rise_apply(grid[:50], sh[:50], (28, 28), x[0].contiguous(), out=mbuf[:50]))
    rep("rise_apply 50 masks", 50 * 4 * N + 4 * N, ms, "30 MB")
    sc = torch.rand(n, device=DEV)
    ms = timeit(lambda: K.rise_accum(grid, sh, sc, (28, 28), H, W, 1.0))
    rep("rise_accum 1000 masks (regen)", n * (64 + 8 + 4) + H * W * 8, ms, f"{n * H * W / ms / 1e6:.1f} G mask-pixels/s (compute-bound)")
    # K11-K14 (ViT-CX maskers): ViT-B/16 feature maps 768 x 14x14 -> 224x224, 64 clusters
    fm = torch.randn(768, 14, 14, device=DEV)
    ms = timeit(lambda: K.up_rownorm(fm, 224, 224))
    rep("up_rownorm 768 x 14x14->224x224", 768 * (196 + H * W) * 4, ms, "154 MB written once")
    rows = K.up_rownorm(fm, 224, 224)
    from xai_engine.vit_cx import cluster_members
    lab = np.random.default_rng(0).integers(0, 64, 768); lab[:64] = np.arange(64)
    mem, offs = (torch.from_numpy(a).to(DEV) for a in cluster_members(lab))
    ms = timeit(lambda: K.cluster_sum(rows, mem, offs))
    rep("cluster_sum 768 rows -> 64", (768 + 64) * H * W * 4, ms)
    cs = K.cluster_sum(rows, mem, offs)
    ms = timeit(lambda: K.rownorm(cs))
    rep("rownorm 64 x 50176", 64 * H * W * 4 * 3, ms, "2 reads (2nd from L2) + 1 write")
    noise = torch.randn(64, C, H, W, device=DEV)
    cm = K.rownorm(cs)
    ms = timeit(lambda: K.causal_apply(x[0].contiguous(), cm, noise, 0.1))
    rep("causal_apply 64 masks", 64 * (3 * N + H * W) * 4 + 4 * N, ms, "read noise+masks, write 2N images")
    # K16 (score-weighted mask sums of TIS / ViT-CX): one read of the stack; before round 3 two K2 launches read it twice
    pf = torch.rand(64, device=DEV)
    ms = timeit(lambda: K.masked_sums(cm, pf))
    rep("masked_sums 64 x 50176 (ViT-CX)", (64 + 2) * H * W * 4, ms, "one pass; stack cache-resident")
    ones_p = torch.ones((1, 1, H * W), device=DEV)
    ms = timeit(lambda: (K.ig_accum(cm.view(1, 64, 1, H * W), ones_p, 0.0, w1=pf.view(1, 64)), K.ig_accum(cm.view(1, 64, 1, H * W), ones_p, 0.0)))
    rep("  (same via two K2 launches)", 2 * (64 + 2) * H * W * 4, ms, "round 2's form")
    tm = (torch.rand(1024, 196, device=DEV) < 0.5).float(); ts = torch.rand(1024, device=DEV)
    ms = timeit(lambda: K.masked_sums(tm, ts))
    rep("masked_sums 1024 x 196 (TIS)", (1024 + 2) * 196 * 4, ms, "49 lanes walk 1024 rows: latency-bound")
    # K15 (classifier-side fusion): layer1 activation of the benchmark's pass, 100 x 256 x 56 x 56
    from xai_engine.prepare import BN_VARIANT
    act = torch.randn(100, 256, 56, 56, device=DEV); idt = torch.randn_like(act); gy = torch.randn_like(act)
    wv, bv, mv, vv = (torch.rand(256, device=DEV) + 0.5 for _ in range(4))
    nb = act.numel() * 4
    ms = timeit(lambda: K.bn_act_fwd(act, None, wv, bv, mv, vv, 1e-5, BN_VARIANT))
    rep("bn_act_fwd  relu(bn(x)) 321 MB", 2 * nb, ms)
    ms = timeit(lambda: K.bn_act_fwd(act, idt, wv, bv, mv, vv, 1e-5, BN_VARIANT))
    rep("bn_act_fwd  relu(bn(x)+id)", 3 * nb, ms)
    yv = K.bn_act_fwd(act, idt, wv, bv, mv, vv, 1e-5, BN_VARIANT)
    ms = timeit(lambda: K.bn_relu_bwd(gy, yv, wv, vv, 1e-5, BN_VARIANT))
    rep("bn_relu_bwd", 3 * nb, ms)
    ms = timeit(lambda: K.bn_relu_bwd(gy, yv, wv, vv, 1e-5, BN_VARIANT, want_identity=True))
    rep("bn_relu_bwd + g_identity", 4 * nb, ms)
    # the gradient-pass forms: the forward also writes 1 gate bit per element, the backward reads those bits instead of y
    ym, gate = K.bn_relu_fwd_mask(act, idt, wv, bv, mv, vv, 1e-5, BN_VARIANT)
    ms = timeit(lambda: K.bn_relu_fwd_mask(act, None, wv, bv, mv, vv, 1e-5, BN_VARIANT, mask=gate))
    rep("bn_relu_fwd_mask  relu(bn(x))", 2 * nb + nb // 32, ms)
    ms = timeit(lambda: K.bn_relu_fwd_mask(act, idt, wv, bv, mv, vv, 1e-5, BN_VARIANT, mask=gate))
    rep("bn_relu_fwd_mask  relu(bn(x)+id)", 3 * nb + nb // 32, ms)
    ms = timeit(lambda: K.bn_relu_bwd_mask(gy, gate, wv, vv, 1e-5, BN_VARIANT))
    rep("bn_relu_bwd_mask", 2 * nb + nb // 32, ms)
    ms = timeit(lambda: K.bn_relu_bwd_mask(gy, gate, wv, vv, 1e-5, BN_VARIANT, want_identity=True))
    rep("bn_relu_bwd_mask + g_identity", 3 * nb + nb // 32, ms)
    del act, idt, gy, yv, ym, gate
    # layer4 of the benchmark's pass (HW = 49: the flat 16-byte path): residual forms at 50 x 2048 x 7 x 7, plain forms at
    # 50 x 512 x 7 x 7.  Yardstick: the float4 kernels on the SAME buffers viewed with HW = 196 (same n, same bytes).
    for tag, shape, twin, residual in (("50x2048x7x7", (50, 2048, 7, 7), (50, 512, 14, 14), True), ("50x512x7x7", (50, 512, 7, 7), (50, 128, 14, 14), False)):
        a4, i4, g4, h4 = (torch.randn(shape, device=DEV) for _ in range(4))
        nb = a4.numel() * 4
        for view, note in ((shape, "HW=49"), (twin, "HW=196 twin")):
            Cv = view[1]
            wv, bv, mv, vv = (torch.rand(Cv, device=DEV) + 0.5 for _ in range(4))
            w2, b2, m2, v2 = (torch.rand(Cv, device=DEV) + 0.5 for _ in range(4))
            av, iv, gv, hv = (t.view(view) for t in (a4, i4, g4, h4))
            idv = iv if residual else None
            ops = 3 if residual else 2
            ms = timeit(lambda: K.bn_act_fwd(av, idv, wv, bv, mv, vv, 1e-5, BN_VARIANT))
            rep(f"bn_act_fwd {tag}", ops * nb, ms, note)
            yv, gate = K.bn_relu_fwd_mask(av, idv, wv, bv, mv, vv, 1e-5, BN_VARIANT)
            ms = timeit(lambda: K.bn_relu_fwd_mask(av, idv, wv, bv, mv, vv, 1e-5, BN_VARIANT, mask=gate))
            rep(f"bn_relu_fwd_mask {tag}", ops * nb + nb // 32, ms, note)
            ms = timeit(lambda: K.bn_relu_bwd(gv, yv, wv, vv, 1e-5, BN_VARIANT, want_identity=residual, gy2=hv))
            rep(f"bn_relu_bwd 2 grads {tag}", (ops + 2) * nb, ms, note)
            ms = timeit(lambda: K.bn_relu_bwd_mask(gv, gate, wv, vv, 1e-5, BN_VARIANT, want_identity=residual, gy2=hv))
            rep(f"bn_relu_bwd_mask 2 grads {tag}", (ops + 1) * nb + nb // 32, ms, note)
            ms = timeit(lambda: K.bn_relu_bwd_mask(gv, gate, wv, vv, 1e-5, BN_VARIANT, want_identity=residual, gy2=hv, guided=True))
            rep(f"bn_relu_bwd_mask guided {tag}", (ops + 1) * nb + nb // 32, ms, note)
            if residual:                                  # the down-sample block: the identity operand has a BatchNorm of its own
                ms = timeit(lambda: K.bn_relu_fwd_mask(av, iv, wv, bv, mv, vv, 1e-5, BN_VARIANT, bn2=(w2, b2, m2, v2, 1e-5), mask=gate))
                rep(f"bn_relu_fwd_mask +bn2 {tag}", 3 * nb + nb // 32, ms, note)
                ms = timeit(lambda: K.bn_relu_bwd_mask(gv, gate, wv, vv, 1e-5, BN_VARIANT, gy2=hv, bn2=(w2, v2, 1e-5)))
                rep(f"bn_relu_bwd_mask +bn2 {tag}", 4 * nb + nb // 32, ms, note)
        del a4, i4, g4, h4, av, iv, gv, hv, yv, gate
    # the stem of one benchmark pass (50 x 64 x 112 x 112 -> 56 x 56) with autograd, and the five-kernel chain it replaces
    sx = torch.randn(50, 64, 112, 112, device=DEV)
    sw, sb, sm, sv = (torch.rand(64, device=DEV) + 0.5 for _ in range(4))
    sn = sx.numel() * 4
    ms = timeit(lambda: K.bn_relu_maxpool_fwd_code(sx, sw, sb, sm, sv, 1e-5, BN_VARIANT, 3, 2, 1))
    rep("bn_relu_maxpool_fwd_code 3/2/1", sn + sn // 4 + sn // 16, ms)
    sy, scode = K.bn_relu_maxpool_fwd_code(sx, sw, sb, sm, sv, 1e-5, BN_VARIANT, 3, 2, 1)
    sg1, sg2 = torch.randn_like(sy), torch.randn_like(sy)
    ms = timeit(lambda: K.bn_relu_maxpool_bwd(sg1, scode, sw, sv, 1e-5, BN_VARIANT, 112, 112, 3, 2, 1, gy2=sg2))
    rep("bn_relu_maxpool_bwd (2 grads)", 2 * (sn // 4) + sn // 16 + sn, ms)

    def stem_chain_fwd():
        return torch.nn.functional.max_pool2d(K.bn_act_fwd(sx, None, sw, sb, sm, sv, 1e-5, BN_VARIANT), 3, 2, 1, 1, False, True)
    ms = timeit(stem_chain_fwd)
    rep("stem chain fwd (bn_act_fwd, torch max_pool)", 2 * sn + sn + sn // 4 + sn // 2, ms, "two kernels, int64 indices")
    sya = K.bn_act_fwd(sx, None, sw, sb, sm, sv, 1e-5, BN_VARIANT)
    _, sidx = stem_chain_fwd()
    ms = timeit(lambda: K.bn_relu_bwd(K.maxpool_bwd(sg1 + sg2, sidx, 112, 112, 3, 2, 1), sya, sw, sv, 1e-5, BN_VARIANT))
    rep("stem chain bwd (add, maxpool_bwd, bn_relu_bwd)", 3 * (sn // 4) + sn // 4 + sn // 2 + sn + 3 * sn, ms, "three kernels")
    del sx, sy, scode, sg1, sg2, sya, sidx
    # K78 / K79
    conv1x1_rows(rep)
    conv1x1_wide_rows(rep)
    # K9
    lg = torch.randn(50, 1000, device=DEV)
    ms = timeit(lambda: K.softmax_stats(lg, 3))
    rep("softmax_stats 50x1000", 50 * 1000 * 4, ms, "latency-bound")
    if args.json:
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
