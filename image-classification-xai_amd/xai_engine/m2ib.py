"""The row m2ib of the reference's get_CLIP_attr (XAI_Survey/evaluations/evaluatePerturbation.py:430-433), M2IB's vision heatmap, in
closed form on the plain CLIP model.

The reference computes this row on a fourth model object, ClipWrapper(clipmodel) (testing_dict["models"][3], M2IB/scripts/
clip_wrapper.py): a deep copy of the plain model with plain CLIP's weights and dtype.  vision_heatmap_iba (methods.py:46-51,
iba.py:89-194) puts an information bottleneck behind visual block `vlayer` = 9 and takes ten Adam steps on its alpha (1, L, D),
each of them a forward of all twelve blocks and of the text tower on ten copies of the image.  The blocks in front of the
bottleneck never see it, so the row is served here on testing_dict["models"][0]; the harness does so only when asked to
(sweep.get_CLIP_attr, `clip_m2ib="plain"`).

  head         Blocks [0 .. layer] run once per image on one row: x9 = hidden_states[layer + 1] is a constant of the image, and the
               wrapper's text features are a constant of the caption (wrapper_text_features, once per caption).
  step         K88 samples t = mu + sqrt(var) * eps for the `copies` rows; the blocks behind the bottleneck, ln_post, proj and
               F.cosine_similarity(text, image, eps=1e-6).mean() run as the reference's torch operators under autograd with t as the
               leaf; K89 turns dL/dt into alpha's gradient (the fitting part and the compression part, beta * mean(capacity)) and
               takes torch's Adam step.  alpha, Adam's moments and the capacity are fp32, x9, t and dL/dt the model's dtype.
  steps - 1    The map is the capacity of the last forward, which uses alpha after steps - 1 updates; the reference's last
               optimizer.step is computed and never read, and is not computed here.
  finish       K90 (the capacity and its nansum over D per patch token), torch's F.interpolate(size=224, mode="bilinear") as the
               reference has it hard-coded (iba.py:157), whatever the input resolution, then the min-max on the 224 x 224 map.  The
               reference normalises twice (iba.py:159, utils.normalize inside and outside); the second pass subtracts 0 and
               divides by 1 - 0, which is exact, so it is done once.  max == min gives the reference's 0 / 0 = NaN map.
  dtype        The row runs in the model's dtype, because the wrapper copies model.dtype: no fp32 copy of the tower is made
               (unlike xai_engine/surgery.py).
  noise        "device": one (B, copies, L, D) normal draw per step from a torch.Generator on the model's device seeded by `seed`;
               the reference draws on its device too, so between runs it offers no more than statistical agreement either.
               "host": torch.empty(copies, L, D).normal_() per forward from torch's CPU generator (a fresh one seeded by `seed`, or
               the global one), image after image, `steps` draws per image as the reference makes them (the last one feeds the step
               that is never read): a CPU-seeded reference run is reproduced draw for draw.  A tensor (steps - 1, copies, L, D), or
               that with a leading B, is taken as given.

Every image of a batch gets the bytes of its own one-image call when it gets the same noise (the rule and the shared checks,
tokens, head loop and epilogue are xai_engine/clip_tower.py's).  Eager only: the step is static-shaped, but
its middle is torch.autograd.grad through torch's own blocks, whose graph and buffers are made anew in every step; it is not on the
shared capture-and-proof path, so no `graphs=True` is offered.  The model's HIP device is required; there is no CPU path
(wrapper_text_features alone is plain torch and runs on the CPU too).
"""
import math

import torch
import torch.nn.functional as F

from . import clip_tower as T
from . import kernels as K

MAP_SIZE = 224                      # iba.py:157, `interpolate(saliency, size=224, mode='bilinear')`
INITIAL_ALPHA = 5.0                 # iba.py:93
ADAM = (0.9, 0.999, 1e-8)           # torch.optim.Adam's defaults, which iba.py:175 takes


def check_model(clipmodel, layer=9):
    """The layout m2ib_batch reads, or an error naming what is missing -> (visual, blocks, H)"""
    visual, blocks, H = T.check_layout(clipmodel, "m2ib", every_block=True, heads=True)
    K._int(layer, "layer")
    if not 0 <= layer <= len(blocks) - 2:
        raise ValueError(f"m2ib: layer = {layer} is outside 0 .. {len(blocks) - 2}: the bottleneck sits behind visual block `layer` "
                         f"and needs at least one of the {len(blocks)} blocks behind it")
    return visual, blocks, H


def _checked_texts(text_features, B, E):
    T.tensor(text_features, "text_features")
    if text_features.dim() not in (1, 2) or (text_features.dim() == 2 and text_features.shape[0] not in (1, B)):
        raise ValueError(f"text_features must be (E,), (1, E) or ({B}, E), got {tuple(text_features.shape)}")
    return T.embeds_into(text_features, E, "text_features").reshape(-1, E)


def _checked_noise(noise, B, steps, R, L, D):
    if isinstance(noise, str):
        if noise not in ("device", "host"):
            raise ValueError(f"noise must be 'device', 'host' or a tensor, got {noise!r}")
        return noise
    if not isinstance(noise, torch.Tensor):
        raise TypeError(f"noise: expected 'device', 'host' or a torch.Tensor, got {type(noise).__name__}")
    if tuple(noise.shape) not in ((steps - 1, R, L, D), (B, steps - 1, R, L, D)):
        raise ValueError(f"noise must be ({steps - 1}, {R}, {L}, {D}) or that with a leading {B}, got {tuple(noise.shape)}")
    return noise


def _text_block(blk, x):
    """One block of the text tower on (L, N, D) tokens WITHOUT the causal mask (clip_wrapper.py:86, `layer.attn_mask = None`), in the
    sequence of nn.MultiheadAttention; the model's own block is not touched (the reference changes a deep copy)."""
    return T.written_out_block(blk, x, int(blk.attn.num_heads))[0]


def wrapper_text_features(clipmodel, token_ids):
    """The text features the reference's row uses, text_encoder_wrapper.forward (clip_wrapper.py:77-108) for token_ids (N, n) int64
    -> (N, E) in the model's dtype.  They are not encode_text's: the wrapper drops the causal mask, takes the LAST position and not
    the end-of-text token's, and multiplies by text_projection twice.  All three are observable behaviour and are kept; the second
    product needs transformer_width == embed_dim (the reference raises there): ValueError.  Plain torch operators, on the device of
    the model, CPU included; no tokenizer is involved, the caller brings the ids."""
    for name in ("token_embedding", "positional_embedding", "transformer", "ln_final", "text_projection"):
        if not hasattr(clipmodel, name):
            raise TypeError(f"wrapper_text_features needs a CLIP of OpenAI's layout: {type(clipmodel).__name__} has no `{name}`")
    if not isinstance(token_ids, torch.Tensor) or token_ids.dtype not in (torch.int64, torch.int32) or token_ids.dim() != 2 \
            or token_ids.numel() == 0:
        raise ValueError("token_ids must be a (N, n) integer tensor with at least one token")
    proj = clipmodel.text_projection
    if proj.shape[0] != proj.shape[1]:
        raise ValueError(f"wrapper_text_features: text_projection is {tuple(proj.shape)}; the wrapper multiplies by it a second time "
                         "(clip_wrapper.py:104), which needs transformer_width == embed_dim (the reference raises there)")
    n = token_ids.shape[1]
    if n > clipmodel.positional_embedding.shape[0]:
        raise ValueError(f"token_ids has {n} positions, the model's context length is {clipmodel.positional_embedding.shape[0]}")
    dtype = clipmodel.visual.conv1.weight.dtype
    with torch.no_grad():
        x = clipmodel.token_embedding(token_ids.to(proj.device)).to(dtype)
        x = (x + clipmodel.positional_embedding.to(dtype)[:n]).permute(1, 0, 2)
        for blk in clipmodel.transformer.resblocks:
            x = _text_block(blk, x.to(dtype))
        x = clipmodel.ln_final(x.permute(1, 0, 2)).to(dtype)
        x = x @ proj
        return x[torch.arange(x.shape[0]), -1] @ proj


def adam_scalars(k, lr=1.0):
    """The host-made scalars of Adam's step k = 1, 2, ... as include/xai_hip_cm2ib.h takes them: (w1, b2, w2, bc2s, step_size, eps)"""
    b1, b2, eps = ADAM
    return 1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** k), lr / (1 - b1 ** k), eps


def _tail_grad(visual, tail, t, txt):
    """t (R, L, D) in the model's dtype -> d(-cos(text, image).mean()) / dt, through the blocks behind the bottleneck as the
    reference's image_encoder_wrapper.forward runs them (clip_wrapper.py:52-59) and calc_loss's fitting term (iba.py:192)"""
    t = t.detach().requires_grad_(True)
    with torch.enable_grad():
        x = t.permute(1, 0, 2)
        for blk in tail:
            x = blk(x)
        x = x.permute(1, 0, 2)
        feats = visual.ln_post(x[:, 0, :]).to(t.dtype) @ visual.proj
        loss = -F.cosine_similarity(txt.expand(feats.shape[0], -1), feats, eps=1e-6).mean()
    return torch.autograd.grad(loss, t)[0]


def m2ib_batch(clipmodel, x, text_features, img_hw=None, layer=9, beta=0.1, steps=10, lr=1.0, copies=10, noise="device", seed=None):
    """The row m2ib of get_CLIP_attr for x (B, 3, R, R), R the model's input_resolution, and the wrapper's text features (E,), (1, E)
    or (B, E) (wrapper_text_features): (B, 224, 224) fp32 maps on the device, vision_heatmap_iba(...) per image; the 224 is the
    reference's (iba.py:157) whatever R is.  With img_hw the harness's map, resized to (img_hw, img_hw) and absolute
    (evaluatePerturbation.py:443-445).  layer, beta, steps, lr, copies: the reference's vlayer = 9, vbeta = 0.1, train_steps = 10,
    lr = 1, batch_size = 10.  noise, seed: see the module's docstring."""
    visual, blocks, _ = check_model(clipmodel, layer)
    _, grid = T.native_input(visual, x, "m2ib")
    B = x.shape[0]
    E, D = int(visual.proj.shape[1]), int(visual.transformer.width)
    L = grid[0] * grid[1] + 1
    txt = _checked_texts(text_features, B, E)
    K._int(steps, "steps", least=1)
    R = K._int(copies, "copies", least=1)
    if seed is not None:
        K._int(seed, "seed")
    noise = _checked_noise(noise, B, steps, R, L, D)
    if grid[0] != grid[1]:
        raise ValueError(f"m2ib: the patch grid {grid} is not square")
    dtype = visual.conv1.weight.dtype
    head, tail = blocks[:layer + 1], blocks[layer + 1:]
    with torch.no_grad():
        for b, tok in T.per_image(visual, x, head, T.native_tokens):
            if b == 0:
                dev = tok.device
                x9 = torch.empty((B, L, D), dtype=dtype, device=dev)
            x9[b] = tok[:, 0]
        txt = txt.to(device=dev, dtype=dtype)
        alpha = torch.full((B, L, D), INITIAL_ALPHA, dtype=torch.float32, device=dev)
        m, v = torch.zeros_like(alpha), torch.zeros_like(alpha)
        draw = _noise_source(noise, seed, B, steps, R, L, D, dev)
        gt = torch.empty((B, R, L, D), dtype=dtype, device=dev)
        for k in range(1, steps):
            eps = draw(k)
            t = K.m2ib_sample(alpha, x9, eps)
            for b in range(B):
                gt[b] = _tail_grad(visual, tail, t[b], txt[b if txt.shape[0] > 1 else 0][None])
            K.m2ib_adam_step(gt, eps, x9, alpha, m, v, beta, *adam_scalars(k, lr))
        sal = K.m2ib_saliency(alpha, x9.float())                                             # (B, L - 1)
        maps = T.resize_maps(sal.reshape(B, *grid), MAP_SIZE, MAP_SIZE)
        lo, hi = maps.amin(dim=(1, 2), keepdim=True), maps.amax(dim=(1, 2), keepdim=True)
        return T.finish((maps - lo) / (hi - lo), B, (MAP_SIZE, MAP_SIZE), img_hw)


def _noise_source(noise, seed, B, steps, R, L, D, dev):
    """-> draw(k): the (B, R, L, D) fp32 noise of step k = 1 .. steps - 1 on the device"""
    if isinstance(noise, torch.Tensor):
        given = noise.to(device=dev, dtype=torch.float32)
        if given.dim() == 4:
            return lambda k: given[k - 1].expand(B, R, L, D).contiguous()
        return lambda k: given[:, k - 1].contiguous()
    if noise == "device":
        gen = torch.Generator(device=dev)
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(seed)
        return lambda k: torch.randn((B, R, L, D), generator=gen, device=dev, dtype=torch.float32)
    gen = None if seed is None else torch.Generator().manual_seed(seed)
    host = torch.empty((B, steps, R, L, D), dtype=torch.float32)
    for b in range(B):                  # the reference's order: image after image, `steps` forwards each
        for k in range(steps):
            host[b, k] = torch.empty(R, L, D).normal_(generator=gen)
    given = host.to(dev)
    return lambda k: given[:, k - 1].contiguous()
