#!/usr/bin/env python3
"""One SHA-256 per result of the CLIP rows' host plumbing and of the ten rows of get_CLIP_attr, on the mini CLIP of the M2IB
fixtures (tests/golden/m2ib_w_seventeen.npz: 12 blocks of width 64, input_resolution 32, L = 17), in fp32 and in mixed fp16: run it
on two trees and compare the lists line by line.
    python profiles/experiments/exp_clip_rows_same_bytes.py host   > host.txt        (no GPU needed)
    python profiles/experiments/exp_clip_rows_same_bytes.py device > device.txt      (an MI355X)
A tolerance would let a changed order of operations through; equal bytes do not.  The helpers are looked up under the names they
have in xai_engine/clip_tower.py and, failing that, under the private names they had in the row modules before that file existed,
so the same script runs on both sides of the move.  m2ib runs with noise="host" and a seed.  The whole run takes seconds."""
import hashlib
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from xai_engine import clip_attn, eclip, m2ib, surgery, sweep, zoo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = dict(embed_dim=16, image_resolution=32, vision_layers=12, vision_width=64, vision_patch_size=8, vision_heads=2,
             context_length=4, vocab_size=8, transformer_width=16, transformer_heads=1, transformer_layers=1)
ROWS = ("eclip", "eclip_wo", "eclip_nograd", "maskclip", "selfattn", "game", "rollout", "lrp", "surgery", "m2ib")
ONE_TEXT = ("lrp", "m2ib")
PLAIN = {"clip_attention_rows": "plain", "clip_surgery": "plain", "clip_m2ib": "plain", "m2ib_noise": "host", "m2ib_seed": 11}


def either(*names):
    """The first of "module.attribute" that exists in this tree"""
    for name in names:
        module, attr = name.rsplit(".", 1)
        try:
            return getattr(importlib.import_module(f"xai_engine.{module}"), attr)
        except (ImportError, AttributeError):
            continue
    raise AttributeError(f"none of {names}")


def emit(name, *outs):
    for i, t in enumerate(outs):
        if isinstance(t, torch.Tensor):
            a = np.ascontiguousarray(t.detach().cpu().numpy())
            print(f"{name}[{i}] {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}")
        else:
            print(f"{name}[{i}] {t!r}")


def model(fp16):
    z = np.load(os.path.join(GOLDEN, "m2ib_w_seventeen.npz"), allow_pickle=False)
    m = zoo.clip_vit(0, **SIZES)
    m.load_state_dict({k: torch.from_numpy(z[k]).float() for k in z.files}, strict=True)
    for p in m.parameters():
        p.requires_grad_(False)
    return (zoo.convert_weights_fp16(m) if fp16 else m).eval()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def texts(seed, *shape):
    return F.normalize(randn(seed, *shape), dim=-1)


def host():
    interpolated = either("clip_tower.interpolated_tokens", "eclip._tokens")
    native = either("clip_tower.native_tokens", "clip_attn._native_tokens")
    block = either("clip_tower.written_out_block", "clip_attn._block")
    ids = torch.randint(0, SIZES["vocab_size"], (3, SIZES["context_length"]), generator=torch.Generator().manual_seed(5))
    for fp16 in (False, True):
        m, tag = model(fp16), "fp16" if fp16 else "fp32"
        dtype = m.visual.conv1.weight.dtype
        with torch.no_grad():
            for hw in ((32, 32), (40, 24)):
                emit(f"interpolated_tokens {tag} {hw}", *interpolated(m.visual, randn(1, 2, 3, *hw)))
            tok = native(m.visual, randn(2, 2, 3, 32, 32))
            emit(f"native_tokens {tag}", tok)
            emit(f"written_out_block visual {tag}", *block(m.visual.transformer.resblocks[3], tok, SIZES["vision_heads"]))
            words = randn(3, SIZES["context_length"], 3, SIZES["transformer_width"]).to(dtype)
            emit(f"written_out_block text {tag}", *block(m.transformer.resblocks[0], words, SIZES["transformer_heads"]))
            emit(f"m2ib._text_block {tag}", m2ib._text_block(m.transformer.resblocks[0], words))
        emit(f"wrapper_text_features {tag}", m2ib.wrapper_text_features(m, ids))
        for hw in ((32, 32), (40, 24)):
            dense = eclip.clip_encode_dense(randn(4, 2, 3, *hw), m)
            emit(f"clip_encode_dense {tag} {hw}", *dense)
            outputs, v_final, _, v, q_out, k_out, _, attn_output, grid = dense
            txt = texts(6, 2, SIZES["embed_dim"]).to(dtype)
            for t, c in enumerate((F.normalize(outputs[:, 0], dim=-1) @ txt.t())[0]):
                for ksim, grad in ((True, True), (False, True), (True, False)):
                    emit(f"grad_eclip {tag} {hw} text {t} {ksim} {grad}", eclip.grad_eclip(c, q_out, k_out, v, attn_output, grid, ksim, grad))
            emit(f"mask_clip {tag} {hw}", eclip.mask_clip(txt.t(), v_final, k_out, grid))


def batch_call(m, row, x, txt, table):
    if row in eclip.METHODS:
        return eclip.eclip_batch(m, x, txt, row)
    if row in clip_attn.METHODS:
        return clip_attn.attention_rows_batch(m, x, txt, row)
    if row == "surgery":
        return surgery.surgery_batch(m, x, txt)
    return m2ib.m2ib_batch(m, x, table[1], noise="host", seed=11)


def device():
    dev = "cuda:0"
    ids = torch.randint(0, SIZES["vocab_size"], (3, SIZES["context_length"]), generator=torch.Generator().manual_seed(5))
    for fp16 in (False, True):
        m, tag = model(fp16).to(dev), "fp16" if fp16 else "fp32"
        table = m2ib.wrapper_text_features(m, ids.to(dev))
        emit(f"m2ib text table {tag}", table)
        for row in ROWS:
            for B in (1, 3):
                x = randn(20 + B, B, 3, 32, 32)
                for T in ((1,) if row in ONE_TEXT else (1, 3)):
                    emit(f"{row} {tag} B={B} T={T} shared", batch_call(m, row, x, texts(30 + T, T, 16), table))
                    if B > 1 and row not in ONE_TEXT:
                        emit(f"{row} {tag} B={B} T={T} per image", batch_call(m, row, x, texts(40 + T, B, T, 16), table))
            img = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(7))
            td = dict(PLAIN, attr_func=row, models=[m], img_hw=48, device=dev, embeddings=3.0 * texts(50, 4, 16).to(dev),
                      surgery_text_features=0.5 * texts(51, 5, 16), m2ib_text_features=table)
            emit(f"get_CLIP_attr {row} {tag}", torch.from_numpy(sweep.get_CLIP_attr(img, 2, td)),
                 sweep.get_CLIP_attr(img, 2, dict(td, device_maps=True)))
        surgery.clear_cache()
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] not in (["host"], ["device"]):
        raise SystemExit(__doc__)
    {"host": host, "device": device}[sys.argv[1]]()
