#!/usr/bin/env python3
"""The Grad-ECLIP rows of CLIP (xai_engine/eclip.py, K75-K77) at ViT-B/16 and ViT-B/32 shapes; writes profiles/r21_eclip.txt.

    timeout -k 10 560 python profiles/bench_eclip.py --out profiles/r21_eclip.txt

Random weights, OpenAI's mixed fp16, 224 x 224, one text, B = 1 and B = 32.
calls    in one process, ms per image: `eclip_batch` (the one-row flow) against the full-row flow (`eclip.clip_encode_dense` per
         image, then `grad_eclip` / `mask_clip` and the same resize), alternating.  A window is --calls calls (one at B = 32) after a warm-up, a host
         clock around work that ends in a synchronisation; the figure is the median of 7 windows, with their min and max.
kernels  K75-K77 alone at the same shapes, by device events around LAUNCHES back-to-back launches (the fastest of 5), us per launch.
A run without a GPU fails."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_eclip.txt"))
    ap.add_argument("--calls", type=int, default=3, help="calls per window")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from xai_engine import eclip, zoo
    from xai_engine import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("bench_eclip: no GPU")
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; CLIP ViT-B (random weights, mixed fp16), 224 x 224, one "
             f"text; ms per image: median, min, max of {WINDOWS} windows of {args.calls} calls (B = 1) or one call (B = 32); kernels: us per launch, {LAUNCHES} "
             "launches between two device events, fastest of 5", ""]

    def windows_ms(fn, images):
        calls = args.calls if images == 1 else 1               # a window is at least `calls` images
        fn()
        ts = []
        for _ in range(WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / (calls * images))
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

    def full_rows(model, x, txt, method):
        """the reference's flow, image by image as get_CLIP_attr runs it"""
        out = []
        for b in range(x.shape[0]):
            outputs, v_final, _x_in, v, q_out, k_out, attn, att_output, size = eclip.clip_encode_dense(x[b:b + 1], model)
            if method == "maskclip":
                emap = eclip.mask_clip(txt.T, v_final, k_out, size).sum(0)
            elif method == "selfattn":
                emap = attn[0, :1, 1:].detach().reshape(*size)
            else:
                cosines = (F.normalize(outputs[:, 0], dim=-1) @ txt.T)[0]
                emap = torch.stack([eclip.grad_eclip(c, q_out, k_out, v, att_output, size) for c in cosines]).sum(0)
            out.append(emap.float())
        return K.resize_bilinear(torch.stack(out).contiguous(), 224, 224, take_abs=True)

    for name, ctor in (("ViT-B/16", zoo.clip_vit_b16), ("ViT-B/32", zoo.clip_vit_b32)):
        model = zoo.convert_weights_fp16(ctor()).to(DEV).eval()
        txt = F.normalize(torch.randn(1, 512, generator=torch.Generator().manual_seed(1)), dim=-1).to(DEV).half()
        lines.append(f"{name}: ms per image           one-row flow (eclip_batch)        full-row flow (clip_encode_dense + grad_eclip)")
        for B in (1, 32):
            x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(DEV)
            for method in ("eclip", "maskclip", "selfattn"):
                one = windows_ms(lambda: eclip.eclip_batch(model, x, txt, method, img_hw=224), B)
                full = windows_ms(lambda: full_rows(model, x, txt, method), B)
                lines.append(f"  B = {B:2d} {method:9s}  %9.3f %9.3f %9.3f       %9.3f %9.3f %9.3f      x %.2f" % (one + full + (full[0] / one[0],)))
        with torch.no_grad():
            p = eclip.cls_pass(model, torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV), want_grad=False)
        L, B, D = p.k.shape
        q0 = p.q_out0
        grad = (torch.randn(B, 1, D, device=DEV) * 0.01).half()
        v_final = torch.randn(B, L - 1, 512, device=DEV).half()
        lines.append(f"{name}: kernels at L = {L}, D = {D}, E = 512, T = 1, us per launch        B = 1        B = 32")
        for label, fn in (("K75 xai_clip_cls_attention_f16", lambda n: K.clip_cls_attention(q0[:n], p.k[:, :n], p.v[:, :n])),
                          ("K76 xai_clip_eclip_map_f16", lambda n: K.clip_eclip_map(q0[:n], p.k_out[:, :n], p.v[:, :n], grad[:n])),
                          ("K77 xai_clip_maskclip_map_f16", lambda n: K.clip_maskclip_map(v_final[:n], txt, p.k_out[:, :n]))):
            lines.append(f"  {label:34s} %12.2f %12.2f" % (event_us(lambda: fn(1)), event_us(lambda: fn(32))))
        lines.append("")
        del model
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
