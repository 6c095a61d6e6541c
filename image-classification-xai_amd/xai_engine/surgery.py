"""The row surgery of the reference's get_CLIP_attr (XAI_Survey/evaluations/evaluatePerturbation.py:425-429), CLIP Surgery, in closed
form on the plain CLIP model.

The reference computes this row on a third model object, surgery_clip.load("CS-ViT-B/16") (testing_dict["models"][2]): plain CLIP's
state dict loaded into the CLIPSurgery class of CLIP_Surgery/clip/clip_surgery_model.py, whose forward differs.  Everything that
forward adds is a function of the plain model's own activations, so the row is served here on testing_dict["models"][0], with no
second copy of the model in memory; the harness does so only when asked to (sweep.get_CLIP_attr, `clip_surgery="plain"`).

  dual path    The last six visual blocks (`resblocks[-6:]`, clip_surgery_model.py:318-327) run two paths.  The original path x_ori is
               the plain block with its attention written out as softmax((q @ k^T) * scale) @ v.  The new path never feeds back:
               it accumulates x += proj(softmax((v @ v^T) * scale) @ v), v from ln_1(x_ori) of each of the six blocks, and has no
               MLP.  At the end x[0] = x_ori[0], then ln_post and `@ proj` on ALL L rows.  So
                   x_new = x_in + sum_i (S_i W_i^T + b_i),
               x_in the input of block n - 6, S_i block i's v-v attention output, W_i and b_i its out_proj: one launch of K86 over
               (block, image, head) and one GEMM with K = 6 D, where the reference runs about eight operators per block.
  fp32         The reference's build_model.py leaves convert_weights commented out and clip.load only calls .float() on the CPU, so
               on a GPU the Surgery model computes in fp32 on OpenAI's fp16-valued weights.  So does this row, always: a model in
               mixed fp16 gets a cached fp32 copy of its VISUAL TOWER, keyed by the model object (about 350 MB for ViT-B/16, against
               the 600 MB second model of the reference); clear_cache() frees it.  A model that is fp32 already (evaluate_clip's
               --clip_fp32) needs no copy.
  dim=1        clip_surgery_map (generate_emap.py:121) divides the (1, L, E) features by `image_features.norm(dim=1, keepdim=True)`:
               the norm over the TOKENS, per embedding channel, not over the embedding.  It is observable behaviour and is kept.
  surgery      clip_feature_surgery (clip.py:287-308) builds a (1, L, T, E) tensor, 24 MB at L = 197, T = 60, E = 512, and touches it
               four times.  In closed form sim[i][t] = sum_c f_ic (w_t t_tc - r_c), r_c = mean_t w_t t_tc: K87, which also does the
               normalisation above and the min-max of get_similarity_map (clip.py:274).  The harness reads text 0 only.
  resize       get_similarity_map's F.interpolate(..., mode="bilinear") to the image size, by torch's operator on the device.

With one text (T = 1) feats - mean over the texts is zero and the min-max is 0 / 0: the reference returns an all-NaN map, and so
does this.

The row takes the reference's `preprocess(img)` and the positional embedding as it is: the input is input_resolution-square,
anything else is refused (the Surgery tower's interpolation of the positional embedding is not built), and so are a ResNet visual
tower and a tower of fewer than six blocks (the reference's `resblocks[-i]` raises there).

The checks, the tokens, the per-image loop in front of the dual blocks and the epilogue are xai_engine/clip_tower.py's.  The
model's HIP device is required; there is no CPU path.
"""
import copy
import weakref

import torch
import torch.nn.functional as F

from . import clip_tower as T
from . import kernels as K
from .ig import hip_device

DUAL_BLOCKS = 6                     # clip_surgery_model.py:321, `for i in range(1, 7)`
_FP32_TOWERS = weakref.WeakKeyDictionary()      # model object -> the fp32 copy of its visual tower
resize_maps = T.resize_maps         # get_similarity_map's last step, under the name it has always had here


def clear_cache():
    """Free the fp32 copies of the visual towers of mixed-fp16 models"""
    _FP32_TOWERS.clear()


def cached_towers():
    """How many fp32 copies are held"""
    return len(_FP32_TOWERS)


def fp32_tower(clipmodel, visual):
    """The tower the row runs on: `visual` itself when it is fp32, else its cached fp32 copy"""
    if all(p.dtype == torch.float32 for p in visual.parameters()):
        return visual
    tower = _FP32_TOWERS.get(clipmodel)
    if tower is None or tower.conv1.weight.device != visual.conv1.weight.device:
        tower = copy.deepcopy(visual).float().eval()
        for p in tower.parameters():
            p.requires_grad_(False)
        _FP32_TOWERS[clipmodel] = tower
    return tower


def check_model(clipmodel):
    """The layout surgery_batch reads, or an error naming what is missing -> (visual, blocks, H)"""
    visual, blocks, H = T.check_layout(clipmodel, "surgery", every_block=True, heads=True)
    if len(blocks) < DUAL_BLOCKS:
        raise ValueError(f"surgery: the visual tower has {len(blocks)} blocks; the dual path takes the last {DUAL_BLOCKS} "
                         "(the reference's `resblocks[-i]` raises an IndexError there)")
    return visual, blocks, H


def _original_block(blk, x, H, qkv_out):
    """The original path of one dual block on (1, L, D) tokens in the reference's sequence (clip_surgery_model.py:71-79, :98, :102,
    :253-274): (q @ k^T) * scale, not q * scale first.  The block's in-projection (L, 3 D) is left in qkv_out."""
    _, L, D = x.shape
    d = D // H
    qkv = F.linear(blk.ln_1(x), blk.attn.in_proj_weight, blk.attn.in_proj_bias)
    qkv_out.copy_(qkv[0])
    q, k, v = qkv.reshape(1, L, 3, H, d).permute(2, 0, 3, 1, 4)
    attn = ((q @ k.transpose(-2, -1)) * (d ** -0.5)).softmax(dim=-1)
    x = x + F.linear((attn @ v).transpose(1, 2).reshape(1, L, D), blk.attn.out_proj.weight, blk.attn.out_proj.bias)
    return x + blk.mlp(blk.ln_2(x))


def image_features(clipmodel, x):
    """encode_image of the Surgery model for x (B, 3, R, R) on the model's HIP device -> (B, L, E) fp32, not normalised"""
    visual, blocks, H = check_model(clipmodel)
    T.native_input(visual, x, "surgery")
    hip_device(visual.conv1.weight.device)                  # a model that is refused gets no fp32 copy
    tower = fp32_tower(clipmodel, visual)
    blocks = list(tower.transformer.resblocks)
    head, dual = blocks[:-DUAL_BLOCKS], blocks[-DUAL_BLOCKS:]
    B, D = x.shape[0], int(tower.transformer.width)
    with torch.no_grad():
        w_cat = torch.cat([blk.attn.out_proj.weight for blk in dual], dim=1)              # (D, 6 D)
        bias = dual[0].attn.out_proj.bias
        for blk in dual[1:]:
            bias = bias + blk.attn.out_proj.bias
        qkv = x_in = cls = None
        for b, tok in T.per_image(tower, x, head, T.native_tokens):
            tok = tok.permute(1, 0, 2)                                                      # (1, L, D), as Attention.forward takes it
            if qkv is None:
                L, dev = tok.shape[1], tok.device
                qkv = torch.empty((DUAL_BLOCKS, L, B, 3 * D), dtype=torch.float32, device=dev)
                x_in = torch.empty((B, L, D), dtype=torch.float32, device=dev)
                cls = torch.empty((B, D), dtype=torch.float32, device=dev)
            x_in[b] = tok[0]
            for i, blk in enumerate(dual):
                tok = _original_block(blk, tok, H, qkv[i, :, b])
            cls[b] = tok[0, 0]
        s = K.clip_vv_attention(qkv[..., 2 * D:], H)                                        # (6, B, L, D)
        feats = torch.empty((B, L, tower.proj.shape[1]), dtype=torch.float32, device=dev)
        for b in range(B):
            new = x_in[b] + (s[:, b].permute(1, 0, 2).reshape(L, DUAL_BLOCKS * D) @ w_cat.t() + bias)
            new[0] = cls[b]
            feats[b] = tower.ln_post(new) @ tower.proj
    return feats


def surgery_batch(clipmodel, x, text_features, img_hw=None, texts_out=1):
    """The row surgery of get_CLIP_attr for x (B, 3, R, R), R the model's input_resolution, and normalised text features (T, E),
    shared, or (B, T, E), text 0 the one the harness reads and the others its context classes: (B, R, R) fp32 maps on the device,
    clip_surgery_map(...)[0, :, :, 0] per image; texts_out > 1: (B, texts_out, R, R), the maps of the first texts_out texts.  With
    img_hw the harness's map, resized to (img_hw, img_hw) and absolute (evaluatePerturbation.py:443-445).

    The row runs in fp32 whatever the model's dtype, as the reference's does: a model in mixed fp16 gets a cached fp32 copy of its
    visual tower, keyed by the model object, about 350 MB for ViT-B/16 (the reference holds a second whole model, 600 MB);
    clear_cache() frees it, and a model loaded in fp32 needs none."""
    visual, _, _ = check_model(clipmodel)
    res, grid = T.native_input(visual, x, "surgery")
    B = x.shape[0]
    T.texts(text_features, B, visual.proj.shape[1], "text_features")
    K._int(texts_out, "texts_out", least=1)
    if texts_out > text_features.shape[-2]:
        raise ValueError(f"texts_out = {texts_out} of T = {text_features.shape[-2]} texts")
    feats = image_features(clipmodel, x)
    txt = text_features.to(device=feats.device, dtype=torch.float32).contiguous()
    sim = K.clip_surgery_similarity(feats, txt, texts_out=texts_out)                        # (B, texts_out, L - 1)
    maps = T.finish(resize_maps(sim.reshape(B * texts_out, *grid), res, res), B * texts_out, (res, res), img_hw)
    return maps.reshape(B, *maps.shape[1:]) if texts_out == 1 else maps.reshape(B, texts_out, *maps.shape[1:])
