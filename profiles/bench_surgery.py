#!/usr/bin/env python3
"""The CLIP Surgery row (xai_engine/surgery.py, K86-K87) at ViT-B/16 and ViT-B/32 shapes; one model per run, appended to
profiles/surgery_bench.txt, so that every step has a time limit of its own:

    for m in b16 b32; do
        timeout -k 10 300 python profiles/bench_surgery.py --model $m --out profiles/surgery_bench.txt || break
    done

Random weights in OpenAI's mixed fp16 (the row computes on its fp32 copy of the visual tower), 224 x 224, T = 60 texts.
Every figure is taken by device events around a window of calls after a warm-up: the median of 7 windows, with their min and max.
row      ms per image of `surgery_batch(..., img_hw=224)` at B = 1 and B = 32, and of the reference's dual-path flow written as torch
         operators on the device in this process (clip_surgery_model.py:71-103, :253-280; clip.py:271-308), one image per call as
         the reference's harness runs it, on the same fp32 tower.
kernels  K86 and K87 alone on the operands of that pass, us per launch; K86 against its own torch expression (two bmm, the scale,
         the softmax and the transpose copy, for the six blocks), K87 against clip_feature_surgery and the min-max as torch operators.
--alt    a second build of the library with another workgroup size for K86 (-DXAI_CSURG_ALT_WAVES=<n>), timed on the same operands.
Nothing is gated on these numbers.  A run without a GPU fails."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
WINDOWS = 7
TEXTS = 60


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surgery_bench.txt"))
    ap.add_argument("--model", choices=("b16", "b32"), default="b16")
    ap.add_argument("--calls", type=int, default=3, help="calls of the row per window")
    ap.add_argument("--launches", type=int, default=100, help="launches of a kernel per window")
    ap.add_argument("--alt", default=None, help="path of a libxai_csurg.so built with -DXAI_CSURG_ALT_WAVES=<n>")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from xai_engine import clip_tower, surgery, zoo
    from xai_engine import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("bench_surgery: no GPU")

    def windows(fn, calls, unit):
        """(median, min, max) over WINDOWS windows of `calls` calls between two device events, in ms * unit per call"""
        fn()
        ts = []
        for _ in range(WINDOWS):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            torch.cuda.synchronize()
            ts.append(start.elapsed_time(stop) * unit / calls)
        return statistics.median(ts), min(ts), max(ts)

    def torch_vv(v, H):
        """K86 as torch operators: v (n, L, B, D) -> (n, B, L, D)"""
        n, L, B, D = v.shape
        vh = v.reshape(n, L, B, H, D // H).permute(0, 2, 3, 1, 4).reshape(n * B * H, L, D // H)
        attn = (torch.bmm(vh, vh.transpose(1, 2)) * (D // H) ** -0.5).softmax(dim=-1)
        return torch.bmm(attn, vh).reshape(n, B, H, L, D // H).transpose(2, 3).reshape(n, B, L, D)

    def torch_similarity(feats, txt):
        """clip_surgery_map's normalisation, clip_feature_surgery and the min-max of get_similarity_map: (1, L, E), (T, E) -> (1, L - 1, T)"""
        f = feats / feats.norm(dim=1, keepdim=True)
        prob = f[:, :1, :] @ txt.t()
        prob = (prob * 2).softmax(-1)
        w = prob / prob.mean(-1, keepdim=True)
        b, n_t, n_i, c = f.shape[0], txt.shape[0], f.shape[1], f.shape[2]
        prod = f.reshape(b, n_i, 1, c) * txt.reshape(1, 1, n_t, c)
        prod *= w.reshape(1, 1, n_t, 1)
        prod = prod - prod.mean(2, keepdim=True)
        sm = prod.sum(-1)[:, 1:, :]
        return (sm - sm.min(1, keepdim=True)[0]) / (sm.max(1, keepdim=True)[0] - sm.min(1, keepdim=True)[0])

    def torch_row(tower, H, x, txt, res):
        """the reference's flow for one image as torch operators -> (res, res), text 0"""
        with torch.no_grad():
            blocks = list(tower.transformer.resblocks)
            tok = clip_tower.native_tokens(tower, x)
            for blk in blocks[:-surgery.DUAL_BLOCKS]:
                tok = blk(tok)
            new = ori = tok
            for blk in blocks[-surgery.DUAL_BLOCKS:]:
                y = blk.ln_1(ori).transpose(0, 1)
                B, N, C = y.shape
                qkv = F.linear(y, blk.attn.in_proj_weight, blk.attn.in_proj_bias).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
                q, k, v = qkv[0], qkv[1], qkv[2]
                scale = (C // H) ** -0.5
                attn_ori = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
                attn = ((v @ v.transpose(-2, -1)) * scale).softmax(dim=-1)
                x_ori = (attn_ori @ v).transpose(1, 2).reshape(B, N, C)
                x_new = (attn @ v).transpose(1, 2).reshape(B, N, C)
                x_new = F.linear(x_new, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
                x_ori = F.linear(x_ori, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
                ori = ori + x_ori.transpose(0, 1)
                ori = ori + blk.mlp(blk.ln_2(ori))
                new = new + x_new.transpose(0, 1)
            new = torch.cat([ori[:1], new[1:]], dim=0).permute(1, 0, 2)
            sm = torch_similarity(tower.ln_post(new) @ tower.proj, txt)
            side = int(sm.shape[1] ** 0.5)
            sm = sm.reshape(sm.shape[0], side, side, -1).permute(0, 3, 1, 2)
            return F.interpolate(sm, (res, res), mode="bilinear").permute(0, 2, 3, 1)[0, :, :, 0].abs()

    name, ctor = {"b16": ("ViT-B/16", zoo.clip_vit_b16), "b32": ("ViT-B/32", zoo.clip_vit_b32)}[args.model]
    model = zoo.convert_weights_fp16(ctor()).to(DEV).eval()
    visual, _, H = surgery.check_model(model)
    txt = F.normalize(torch.randn(TEXTS, 512, generator=torch.Generator().manual_seed(1)), dim=-1).to(DEV)
    x32 = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    x1 = x32[:1]
    lines = []
    if not os.path.exists(args.out) or os.path.getsize(args.out) == 0:
        lines += [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; CLIP ViT-B (random weights, mixed fp16; the row on its "
                  f"fp32 tower), 224 x 224, T = {TEXTS}; device events around a window of calls, median, min, max of {WINDOWS} windows", ""]
    got = surgery.surgery_batch(model, x1, txt, img_hw=224)[0]
    tower = surgery.fp32_tower(model, visual)
    want = torch_row(tower, H, x1, txt, 224)
    err = float((got - want).abs().max() / want.abs().max())
    lines.append(f"{name}: the row, ms per image (surgery_batch against the dual-path flow as torch operators: max|diff| / max = {err:.2e})")
    lines.append("  surgery_batch, B = 1               %9.3f %9.3f %9.3f" % windows(lambda: surgery.surgery_batch(model, x1, txt, img_hw=224), args.calls, 1.0))
    lines.append("  surgery_batch, B = 32              %9.3f %9.3f %9.3f" % windows(lambda: surgery.surgery_batch(model, x32, txt, img_hw=224), 1, 1.0 / 32))
    lines.append("  torch operators, one image         %9.3f %9.3f %9.3f" % windows(lambda: torch_row(tower, H, x1, txt, 224), args.calls, 1.0))
    feats = surgery.image_features(model, x32)
    L, D = feats.shape[1], int(tower.transformer.width)
    lines.append(f"{name}: kernels at n = 6, H = {H}, L = {L}, D = {D}, E = 512, T = {TEXTS}, us per launch")
    for B in (1, 32):
        qkv = torch.randn(6, L, B, 3 * D, generator=torch.Generator().manual_seed(B)).to(DEV) * 0.5
        v = qkv[..., 2 * D:]
        t86 = windows(lambda: K.clip_vv_attention(v, H), args.launches, 1e3)
        t86t = windows(lambda: torch_vv(v, H), args.launches, 1e3)
        d86 = float((K.clip_vv_attention(v, H) - torch_vv(v, H)).abs().max())
        lines.append(f"  K86 xai_csurg_vv_attention_f32, B = {B:<2d}          %10.2f %10.2f %10.2f" % t86)
        lines.append(f"  its torch expression, B = {B:<2d}                    %10.2f %10.2f %10.2f      x %.2f   (max|diff| {d86:.1e})" % (*t86t, t86t[0] / t86[0]))
        if args.alt:
            alt = ctypes.CDLL(args.alt)
            alt.xai_csurg_vv_attention_f32.argtypes = [ctypes.c_void_p] + [ctypes.c_int64] * 3 + [ctypes.c_int] * 5 + [ctypes.c_float] + [ctypes.c_void_p] * 3
            alt.xai_csurg_vv_waves.restype = ctypes.c_int
            out = torch.empty((6, B, L, D), device=DEV)
            stream = torch.cuda.current_stream().cuda_stream

            def alt_call():
                code = alt.xai_csurg_vv_attention_f32(v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), 6, B, L, D, H, float(D // H) ** -0.5,
                                                      None, out.data_ptr(), stream)
                assert code == 0, code
            t_alt = windows(alt_call, args.launches, 1e3)
            same = torch.equal(out, K.clip_vv_attention(v, H))
            lines.append(f"  K86 with {alt.xai_csurg_vv_waves()} waves, {4 * alt.xai_csurg_vv_waves()} rows a workgroup, B = {B:<2d}    %10.2f %10.2f %10.2f      "
                         f"(the same bytes: {same})" % t_alt)
        f = feats[:B].contiguous()
        t87 = windows(lambda: K.clip_surgery_similarity(f, txt), args.launches, 1e3)
        lines.append(f"  K87 xai_csurg_similarity_map_f32, B = {B:<2d}        %10.2f %10.2f %10.2f" % t87)
        if B == 1:
            t87t = windows(lambda: torch_similarity(f, txt), args.launches, 1e3)
            lines.append("  its torch operators (all 60 texts), B = 1       %10.2f %10.2f %10.2f      x %.2f" % (*t87t, t87t[0] / t87[0]))
    lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
