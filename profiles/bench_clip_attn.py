#!/usr/bin/env python3
"""CLIP's game, rollout and lrp rows (xai_engine/clip_attn.py, K82-K85) at ViT-B/16 and ViT-B/32 shapes; one model and dtype per run,
appended to profiles/clip_attn_bench.txt, so that every step has a time limit of its own:

    for m in b16 b32; do for d in fp16 fp32; do
        timeout -k 10 300 python profiles/bench_clip_attn.py --model $m --dtype $d --out profiles/clip_attn_bench.txt || break
    done; done

Random weights, 224 x 224, one text, B = 1.
rows     ms per image of `attention_rows_batch(..., img_hw=224)`: a window is --calls calls after a warm-up, a host clock around work
         that ends in a synchronisation; the median of 7 windows, with their min and max.
kernels  K82-K85 alone on the operands of that pass, by device events around LAUNCHES back-to-back launches (the fastest of 5), us per
         launch; for K84 also the bytes it moves per second (2 n H L^2 values read, n L^2 written).
torch    lrp's maps from the same attention probabilities and gradients in plain torch operations, the reference's five per block
         (grad * cam, clamp(min=0), mean over the heads, bmm, add; generate_emap.py:231-238), the same way: the figure K84 + K85 stand
         against.
Nothing is gated on these numbers.  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
WINDOWS = 7
LAUNCHES = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_attn_bench.txt"))
    ap.add_argument("--model", choices=("b16", "b32"), default="b16")
    ap.add_argument("--dtype", choices=("fp16", "fp32"), default="fp16")
    ap.add_argument("--calls", type=int, default=3, help="calls per window")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from xai_engine import clip_attn, zoo
    from xai_engine import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_attn: no GPU")

    def windows_ms(fn):
        fn()
        ts = []
        for _ in range(WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / args.calls)
        return statistics.median(ts), min(ts), max(ts)

    def event_us(fn):
        for _ in range(3):
            fn()
        best = float("inf")
        for _ in range(5):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(LAUNCHES):
                fn()
            stop.record()
            torch.cuda.synchronize()
            best = min(best, start.elapsed_time(stop) * 1e3 / LAUNCHES)
        return best

    def torch_lrp(attn, grad):
        """clip_lrp's loop on stored operands (n, 1, H, L, L) -> R[:, 0, 1:]"""
        n, _, H, L, _ = attn.shape
        rel = torch.eye(L, dtype=attn.dtype, device=attn.device).unsqueeze(0)
        for i in range(n):
            cam = (grad[i, 0] * attn[i, 0]).reshape(1, H, L, L).clamp(min=0).mean(dim=1)
            rel = rel + torch.bmm(cam, rel)
        return rel[:, 0, 1:]

    name, ctor = {"b16": ("ViT-B/16", zoo.clip_vit_b16), "b32": ("ViT-B/32", zoo.clip_vit_b32)}[args.model]
    model = ctor()
    if args.dtype == "fp16":
        zoo.convert_weights_fp16(model)
    model = model.to(DEV).eval()
    dt = model.dtype
    txt = F.normalize(torch.randn(1, 512, generator=torch.Generator().manual_seed(1)), dim=-1).to(DEV).to(dt)
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    lines = []
    if not os.path.exists(args.out) or os.path.getsize(args.out) == 0:
        lines += [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; CLIP ViT-B (random weights), 224 x 224, one text, B = 1; "
                  f"rows: ms per image, median, min, max of {WINDOWS} windows of {args.calls} calls; kernels and torch: us per launch, {LAUNCHES} "
                  "launches between two device events, fastest of 5", ""]
    lines.append(f"{name} {args.dtype}: rows, ms per image")
    for row in clip_attn.METHODS:
        lines.append(f"  {row:8s} %9.3f %9.3f %9.3f" % windows_ms(lambda: clip_attn.attention_rows_batch(model, x, txt, row, img_hw=224)))
    visual, blocks, H = clip_attn.check_layout(model, every_block=True)
    attn, grad = clip_attn.lrp_operands(model, visual, blocks, H, x, txt.unsqueeze(0))
    n, _, _, L, _ = attn.shape
    p = clip_attn.cls_rows(model, x)
    g = (torch.randn(1, 1, p.v.shape[2], device=DEV) * 0.01).to(dt)
    c = K.clip_lrp_matrices(attn, grad)
    moved = (2 * n * H + n) * L * L * attn.element_size()
    lines.append(f"{name} {args.dtype}: kernels at n = {n}, H = {H}, L = {L}, D = {p.v.shape[2]}, T = 1, us per launch")
    sfx = "f16" if args.dtype == "fp16" else "f32"
    t84 = event_us(lambda: K.clip_lrp_matrices(attn, grad, out=c))
    t85 = event_us(lambda: K.clip_lrp_row(c))
    for label, t in ((f"K82 xai_cattn_game_map_{sfx}", event_us(lambda: K.clip_game_map(g, p.v, p.a0))),
                     (f"K83 xai_cattn_rollout_row_{sfx}", event_us(lambda: K.clip_rollout_row(p.a0))),
                     (f"K84 xai_cattn_lrp_matrices_{sfx}", t84), (f"K85 xai_cattn_lrp_row_{sfx}", t85)):
        lines.append(f"  {label:34s} %12.2f" % t)
    per_load = 16 // attn.element_size()
    flavour = "the 16-byte flavour" if (L * L) % per_load == 0 else f"the scalar flavour: L * L = {L * L} is no multiple of {per_load}"
    lines.append(f"  K84 moves {moved / 1e6:.2f} MB per image: {moved / t84 / 1e3:.1f} GB/s ({flavour})")
    t_torch = event_us(lambda: torch_lrp(attn, grad))
    same = torch.equal(torch_lrp(attn, grad).float(), K.clip_lrp_row(c))
    lines.append(f"  lrp in plain torch operations      %12.2f      K84 + K85 %12.2f      x %.2f      (the two maps {'are' if same else 'are not'} "
                 "bit-identical: the row form associates differently)" % (t_torch, t84 + t85, t_torch / (t84 + t85)))
    lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
