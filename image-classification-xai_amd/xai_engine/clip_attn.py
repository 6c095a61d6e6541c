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
the input is input_resolution-square, anything else is refused.  The checks, the tokens, the written-out block and the per-image loop
are xai_engine/clip_tower.py's; lrp's autograd pass runs image by image too.  The model's HIP device is required; there is no CPU path.
"""
import torch
import torch.nn.functional as F

from . import clip_tower as T
from . import kernels as K
from .ig import hip_device

METHODS = ("game", "rollout", "lrp")


def check_layout(clipmodel, every_block=False):
    """The layout the rows read, `attn.num_heads` (of every block for lrp) included -> (visual, blocks, H)"""
    return T.check_layout(clipmodel, "clip_attn", every_block=every_block, heads=True)


def _logits(clipmodel, features, txt):
    """model.forward's logits of one image against its texts (model.py:369-374): features (1, E), txt (T, E) normalised -> (T,)"""
    features = features / features.norm(dim=-1, keepdim=True)
    return (clipmodel.logit_scale.exp() * features @ txt.t())[0]


class ClsRows:
    """What cls_rows leaves: v (L, B, D); a0 (B, H, L), the class-token row of every head's attention in the last block; att_output
    (B, D), row 0 of the attention output; x_in0 (B, D), row 0 of the last block's input"""


def cls_rows(clipmodel, x):
    """The class-token row of the last visual block in its H heads for x (B, 3, R, R) on the model's HIP device -> ClsRows"""
    visual, blocks, H = check_layout(clipmodel)
    T.native_input(visual, x, "clip_attn")
    last = blocks[-1]
    B, D = x.shape[0], visual.transformer.width
    d = D // H
    w_in, b_in = last.attn.in_proj_weight, last.attn.in_proj_bias
    p = ClsRows()
    with torch.no_grad():
        for b, x_in in T.per_image(visual, x, blocks[:-1], T.native_tokens):
            if b == 0:
                L, dev = x_in.shape[0], x_in.device
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


def lrp_operands(clipmodel, visual, blocks, H, x, txt):
    """attn, grad (n, B, H, L, L) of lrp: per image the forward written out block by block, model.forward's logit of its one text, and
    one autograd.grad with respect to the n attention probabilities"""
    B, n = x.shape[0], len(blocks)
    attn = grad = None
    for b in range(B):
        with torch.enable_grad():
            # a leaf in front of the first block: the parameters of a frozen model ask for no graph, this does
            tok = T.native_tokens(visual, x[b:b + 1]).detach().requires_grad_(True)
            probs = []
            for blk in blocks:
                tok, a = T.written_out_block(blk, tok, H)
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
    _, grid = T.native_input(visual, x, "clip_attn")
    T.texts(txt_embedding, x.shape[0], visual.proj.shape[1], "txt_embedding")
    if method == "lrp" and txt_embedding.shape[-2] != 1:
        raise ValueError(f"attention_rows_batch: lrp takes one text (clip_lrp is called with txts[0]), got T = {txt_embedding.shape[-2]}")
    dev = hip_device(visual.conv1.weight.device)
    x = x.to(dev)
    B = x.shape[0]
    txt = txt_embedding.to(device=dev, dtype=visual.proj.dtype).expand(B, -1, -1)
    n_texts = txt.shape[1]
    if method == "lrp":
        attn, grad = lrp_operands(clipmodel, visual, blocks, H, x, txt)
        maps = K.clip_lrp_row(K.clip_lrp_matrices(attn, grad))
    else:
        p = cls_rows(clipmodel, x)
        if method == "rollout":
            maps = K.clip_rollout_row(p.a0, texts=n_texts)
        else:
            last = blocks[-1]
            g = torch.empty((B, n_texts, p.att_output.shape[1]), dtype=p.att_output.dtype, device=dev)
            for b in range(B):
                with torch.enable_grad():
                    leaf = p.att_output[b:b + 1].clone().requires_grad_(True)
                    logits = _logits(clipmodel, T.tail(visual, last, leaf, p.x_in0[b]), txt[b])
                    for t in range(n_texts):
                        g[b, t] = torch.autograd.grad(logits[t], leaf, retain_graph=t + 1 < n_texts)[0][0]
            maps = K.clip_game_map(g, p.v, p.a0)
    return T.finish(maps, B, grid, img_hw)
