"""The rows game, rollout and lrp of the reference's get_CLIP_attr (XAI_Survey/evaluations/evaluatePerturbation.py:410-437), in closed
form on the plain CLIP model.

The reference computes these rows on a second model object, the CLIP of Game_MM_CLIP/clip/model.py (testing_dict["models"][1]).
That model has the weights and the forward of plain CLIP; its one modification is a hook that keeps each visual block's attention
probabilities `attn_probs` and lets autograd differentiate with respect to them (auxilary.py:243-252, model.py:167-198), and
mm_interpret, clip_lrp and compute_rollout_attention (generate_emap.py:133-285) read nothing else.  So the three rows are functions of
the plain model's multi-head attention probabilities A_i,h and of G_i,h = d logit / d A_i,h, logit = logit_scale.exp() * cos(image,
text) as model.forward (model.py:364-378) forms it.  Both are produced here on testing_dict["models"][0].  The engine has only that
model, so the harness serves these rows only when asked to (sweep.get_CLIP_attr, `clip_attention_rows="plain"`).

  game     mm_interpret with its default start_layer = -1 reads only the last block, and of R = I + mean_h clamp(G_h * A_h, min=0) only
           R[:, 0, 1:].  Behind the last attention every operation is token-wise and visual.forward reads token 0 only, so G is zero
           outside row 0 and G_h[0, j] = <g_h, V_h[j]>, g = d logit / d (attention output, row 0): the one-row flow of eclip.cls_pass
           with the last block in its H heads, a one-row backward, K82.
  rollout  mm_interpret(rollout=True) returns one matrix, the last block's A averaged over its T * H leading entries, and
           compute_rollout_attention adds an fp32 eye, divides by the row sum and reads row 0: no gradient, no text.  K83.
  lrp      clip_lrp walks all n blocks: C_i = mean_h clamp(G_i,h * A_i,h, min=0), R <- R + C_i @ R.  Every block's attention is
           written out below in torch operations in the reference's sequence (auxilary.py:153-255), so that A_i is an autograd node
           and rounds where the reference rounds; one autograd.grad gives all G_i; K84 reduces the 2 n H L^2 values to n L^2 and K85
           runs the chain for row 0 of R, the only row that is read.

The class-token row of the last block is K75's arithmetic per head: for one image K75 runs with the heads as its batch axis (K and V
of head h at column offset h * d, so ld_b = d, B = H, D = d); the softmax is not written a second time.

These rows take the reference's `preprocess(img)` and visual.forward, which adds the positional embedding without interpolating it:
the input is input_resolution-square, anything else is refused.

Every image of a batch gets the bytes of its own one-image call: the GEMMs and the autograd pass run image by image, the kernels take
the batch -- the rule of xai_engine/eclip.py and lrp.py.  Eager only: nothing here is captured into a hipGraph.  The model's HIP device is
required; there is no CPU path.
"""
import torch
import torch.nn.functional as F

from . import eclip
from . import kernels as K
from .ig import hip_device

METHODS = ("game", "rollout", "lrp")


def check_layout(clipmodel, every_block=False):
    """eclip.check_layout plus `attn.num_heads` (of every block for lrp) -> (visual, blocks, H)"""
    visual, last = eclip.check_layout(clipmodel)
    blocks = list(visual.transformer.resblocks)
    for i, blk in enumerate(blocks if every_block else [last]):
        where = f"visual.transformer.resblocks[{i if every_block else -1}]."
        for path in eclip._BLOCK + ("attn.num_heads",):
            obj = blk
            for name in path.split("."):
                if not hasattr(obj, name):
                    raise TypeError(f"clip_attn needs a CLIP of OpenAI's layout: {type(clipmodel).__name__} has no `{where}{path}`")
                obj = getattr(obj, name)
    H, D = int(last.attn.num_heads), int(visual.transformer.width)
    if H < 1 or D % H:
        raise TypeError(f"clip_attn: attn.num_heads = {H} does not divide the width {D}")
    return visual, blocks, H


def _native_tokens(visual, x):
    """x (1, 3, R, R) at the model's own resolution -> the (L, 1, D) input of the first block, as visual.forward (model.py:229-237)"""
    x = visual.conv1(x.to(visual.conv1.weight.dtype))
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    x = torch.cat([visual.class_embedding.to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype, device=x.device), x], dim=1)
    return visual.ln_pre(x + visual.positional_embedding.to(x.dtype)).permute(1, 0, 2)


def _block(blk, x, H):
    """One residual block on (L, 1, D) tokens in the reference's sequence of operations (auxilary.py:153-255, model.py:195-198) ->
    (the block's output, its attention probabilities (H, L, L), a node of the autograd graph)"""
    L, N, D = x.shape
    hd = D // H
    q, k, v = F.linear(blk.ln_1(x), blk.attn.in_proj_weight, blk.attn.in_proj_bias).chunk(3, dim=-1)
    q = q * (float(hd) ** -0.5)
    q, k, v = (t.contiguous().view(L, N * H, hd).transpose(0, 1) for t in (q, k, v))
    probs = F.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    out = torch.bmm(probs, v).transpose(0, 1).contiguous().view(L, N, D)
    x = x + F.linear(out, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
    return x + blk.mlp(blk.ln_2(x)), probs


def _logits(clipmodel, features, txt):
    """model.forward's logits of one image against its texts (model.py:369-374): features (1, E), txt (T, E) normalised -> (T,)"""
    features = features / features.norm(dim=-1, keepdim=True)
    return (clipmodel.logit_scale.exp() * features @ txt.t())[0]


def _checked_input(visual, x):
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"x must be (B, 3, H, W), got {tuple(x.shape)}")
    res = int(visual.input_resolution)
    if tuple(x.shape[2:]) != (res, res):
        raise NotImplementedError(f"clip_attn: x is {x.shape[2]} x {x.shape[3]}, the model's input_resolution is {res}: the reference's "
                                  "visual.forward adds the positional embedding without interpolating it, and its preprocess resizes "
                                  "with PIL's bicubic filter, which is not restated here")
    ksize = visual.conv1.kernel_size
    return res // ksize[0], res // ksize[1]


class ClsRows:
    """What cls_rows leaves: v (L, B, D); a0 (B, H, L), the class-token row of every head's attention in the last block; att_output
    (B, D), row 0 of the attention output; x_in0 (B, D), row 0 of the last block's input"""


def cls_rows(clipmodel, x):
    """The class-token row of the last visual block in its H heads for x (B, 3, R, R) on the model's HIP device -> ClsRows"""
    visual, blocks, H = check_layout(clipmodel)
    _checked_input(visual, x)
    last = blocks[-1]
    dev = hip_device(visual.conv1.weight.device)
    x = x.to(dev)
    B, D = x.shape[0], visual.transformer.width
    d = D // H
    w_in, b_in = last.attn.in_proj_weight, last.attn.in_proj_bias
    p = ClsRows()
    with torch.no_grad():
        for b in range(B):
            x_in = torch.nn.Sequential(*blocks[:-1])(_native_tokens(visual, x[b:b + 1]))
            if b == 0:
                L = x_in.shape[0]
                kv = torch.empty((L, B, 2 * D), dtype=x_in.dtype, device=dev)
                p.x_in0 = torch.empty((B, D), dtype=x_in.dtype, device=dev)
                p.a0 = torch.empty((B, H, L), dtype=x_in.dtype, device=dev)
                p.att_output = torch.empty((B, D), dtype=x_in.dtype, device=dev)
            normed = last.ln_1(x_in)
            p.x_in0[b] = x_in[0, 0]
            kv[:, b] = F.linear(normed[:, 0], w_in[D:], b_in[D:])
            q0 = F.linear(normed[:1, 0], w_in[:D], b_in[:D])
            # K75 with the heads as its batch axis: head h of K and V is the column block h * d .. of this image's rows
            k_heads, v_heads = (kv[:, b, o:o + D].unflatten(-1, (H, d)) for o in (0, D))
            attn, att_out = K.clip_cls_attention(q0.view(H, d), k_heads, v_heads)
            p.a0[b] = attn
            p.att_output[b] = att_out.reshape(D)
        p.v = kv[:, :, D:]
    return p


def _lrp_operands(clipmodel, visual, blocks, H, x, txt):
    """attn, grad (n, B, H, L, L) of lrp: per image the forward written out block by block, model.forward's logit of its one text, and
    one autograd.grad with respect to the n attention probabilities"""
    B, n = x.shape[0], len(blocks)
    attn = grad = None
    for b in range(B):
        with torch.enable_grad():
            # a leaf in front of the first block: the parameters of a frozen model ask for no graph, this does
            tok = _native_tokens(visual, x[b:b + 1]).detach().requires_grad_(True)
            probs = []
            for blk in blocks:
                tok, a = _block(blk, tok, H)
                probs.append(a)
            features = visual.ln_post(tok.permute(1, 0, 2)[:, 0, :]) @ visual.proj
            logit = _logits(clipmodel, features, txt[b])[0]
            grads = torch.autograd.grad(logit, probs)
        if attn is None:
            L = probs[0].shape[-1]
            attn = torch.empty((n, B, H, L, L), dtype=probs[0].dtype, device=x.device)
            grad = torch.empty_like(attn)
        for i in range(n):
            attn[i, b] = probs[i].detach()
            grad[i, b] = grads[i]
    return attn, grad


def attention_rows_batch(clipmodel, x, txt_embedding, method, img_hw=None):
    """The row `method` (game, rollout, lrp) of get_CLIP_attr for x (B, 3, R, R), R the model's input_resolution, and already
    normalised text embeddings (T, E), shared, or (B, T, E): (B, h, w) fp32 maps on the device (game: summed over the T texts;
    rollout: the texts count only through T; lrp: T = 1); with img_hw the harness's map, resized to (img_hw, img_hw) and absolute
    (evaluatePerturbation.py:443-445)."""
    if method not in METHODS:
        raise ValueError(f"attention_rows_batch: unknown row {method!r}; the served rows are {METHODS}")
    visual, blocks, H = check_layout(clipmodel, every_block=method == "lrp")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x: expected a torch.Tensor, got {type(x).__name__}")
    grid = _checked_input(visual, x)
    if not isinstance(txt_embedding, torch.Tensor) or txt_embedding.dim() not in (2, 3):
        raise ValueError("txt_embedding must be a (T, E) or (B, T, E) tensor")
    if method == "lrp" and txt_embedding.shape[-2] != 1:
        raise ValueError(f"attention_rows_batch: lrp takes one text (clip_lrp is called with txts[0]), got T = {txt_embedding.shape[-2]}")
    dev = hip_device(visual.conv1.weight.device)
    x = x.to(dev)
    B = x.shape[0]
    txt = eclip._texts(txt_embedding, B, visual.proj.dtype, dev)
    E = visual.proj.shape[1]
    if txt.shape[2] != E:
        raise ValueError(f"txt_embedding has {txt.shape[2]} features, the model embeds into {E}")
    T = txt.shape[1]
    if method == "lrp":
        attn, grad = _lrp_operands(clipmodel, visual, blocks, H, x, txt)
        maps = K.clip_lrp_row(K.clip_lrp_matrices(attn, grad))
    else:
        p = cls_rows(clipmodel, x)
        if method == "rollout":
            maps = K.clip_rollout_row(p.a0, texts=T)
        else:
            last = blocks[-1]
            g = torch.empty((B, T, p.att_output.shape[1]), dtype=p.att_output.dtype, device=dev)
            for b in range(B):
                with torch.enable_grad():
                    leaf = p.att_output[b:b + 1].clone().requires_grad_(True)
                    logits = _logits(clipmodel, eclip._tail(visual, last, leaf, p.x_in0[b]), txt[b])
                    for t in range(T):
                        g[b, t] = torch.autograd.grad(logits[t], leaf, retain_graph=t + 1 < T)[0][0]
            maps = K.clip_game_map(g, p.v, p.a0)
    maps = maps.reshape(B, *grid)
    if img_hw is None:
        return maps
    return K.resize_bilinear(maps.contiguous(), img_hw, img_hw, take_abs=True)
