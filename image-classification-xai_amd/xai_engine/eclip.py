"""The Grad-ECLIP rows of the reference's get_CLIP_attr (XAI_Survey/evaluations/evaluatePerturbation.py:373-445) that hang on
`clip_encode_dense` (util/attribution_methods/CLIP/generate_emap.py:309-376) and the plain OpenAI CLIP model: eclip, eclip_wo,
eclip_nograd, maskclip and selfattn.

What the reference computes.  clip_encode_dense runs the last block of the visual transformer by hand: ONE attention head of width D
over all L tokens (attention_layer :288-307), out_proj, the residual, the MLP, ln_post and the projection, for every token.
grad_eclip (:453-485) then takes autograd.grad of the image-text cosine with respect to the attention output, and reads

    grad[:1, 0, :]      the class-token row of that gradient                      (:462)
    q_out[:1, 0, :]     the class-token row of out_proj(q)                        (:465)
    outputs[:, 0]       the class-token row of the embedding (the cosine)         (evaluatePerturbation.py:398)
    attn[0, :1, 1:]     the class-token row of the attention (the selfattn row)   (evaluatePerturbation.py:424)

Behind the attention every operation is token-wise, so, exactly and not approximately: the gradient of the cosine with respect to
att_output is zero outside row 0; row 0 of the attention needs one query; and for eclip* and selfattn the whole tail runs on one row
per image, next to the K, V and out_proj(K) GEMMs over all rows.  Only maskclip needs v_final for all rows.  `cls_pass` is that
one-row flow; what lies between its GEMMs are the kernels K75-K77 (include/xai_clip.h, which states their rounding rule).

`clip_encode_dense`, `attention_layer`, `grad_eclip` and `mask_clip` are the full-row functions under the reference's names,
signatures and return values, for callers that use them directly: plain torch operations, any device.

The layout check, the tokens, the per-image loop and the epilogue are xai_engine/clip_tower.py's, which states the rule that every
image of a batch gets the bytes of its own one-image call.

Refused here: surgery and m2ib need other models, and game, rollout and lrp are computed by the reference on a second model object
(`REFUSED` names them all).  That second model has plain CLIP's weights and forward, so xai_engine/clip_attn.py serves game, rollout
and lrp in closed form on the plain model; the harness does so only when asked (sweep.get_CLIP_attr, clip_attention_rows="plain"),
because this engine holds one model where the reference holds two.  `eclip_batch` itself refuses all five, as it always has.
"""
import torch
import torch.nn.functional as F

from . import clip_tower as T
from . import kernels as K

METHODS = ("eclip", "eclip_wo", "eclip_nograd", "maskclip", "selfattn")
# method -> (withksim, withgrad) of grad_eclip, evaluatePerturbation.py:401-409
_ECLIP_FLAGS = {"eclip": (True, True), "eclip_wo": (False, True), "eclip_nograd": (True, False)}
REFUSED = {"game": "the modified CLIP of Game_MM_CLIP (mm_interpret, testing_dict['models'][1])",
           "rollout": "the modified CLIP of Game_MM_CLIP (mm_interpret(rollout=True), testing_dict['models'][1])",
           "lrp": "the relprop CLIP of CLIP_lrp (clip_lrp, testing_dict['models'][1])",
           "surgery": "the CLIP Surgery model (clip_surgery_map, testing_dict['models'][2])",
           "m2ib": "the M2IB wrapper and its tokenizer (m2ib_clip_map, testing_dict['models'][3] and [4])"}


def check_layout(clipmodel):
    """The attributes the pass reads (OpenAI's names), or a TypeError naming the one that is missing.  -> (visual, last block)"""
    visual, blocks, _ = T.check_layout(clipmodel, "eclip")
    return visual, blocks[-1]


# ---------------------------------------------------------------------------------- the reference's full-row functions
def attention_layer(q, k, v, num_heads=1, attn_mask=None):
    """Scaled dot-product attention of (L, N, D) q, k, v -> (output (L, N, D), weights (N, L, S) averaged over the heads)"""
    L, N, D = q.shape
    hd = D // num_heads
    q, k, v = (t.contiguous().view(-1, N * num_heads, hd).transpose(0, 1) for t in (q * float(hd) ** -0.5, k, v))
    w = torch.bmm(q, k.transpose(1, 2))
    if attn_mask is not None:
        w = w + attn_mask
    w = F.softmax(w, dim=-1)
    out = torch.bmm(w, v).transpose(0, 1).contiguous().view(L, N, D)
    return out, w.view(N, num_heads, L, -1).sum(dim=1) / num_heads


def clip_encode_dense(x, clipmodel):
    """The reference's 9-tuple (outputs (N, L, E), v_final[:, 1:], x_in, v, q_out, k_out, attn, attn_output, (h, w)); attn_output is
    in the autograd graph of outputs.  x is cast to the model's dtype (the reference's x.half() on its GPU model)."""
    visual, last = check_layout(clipmodel)
    x, grid = T.interpolated_tokens(visual, x)
    x_in = torch.nn.Sequential(*visual.transformer.resblocks[:-1])(x)
    w, b = last.attn.out_proj.weight, last.attn.out_proj.bias
    q, k, v = F.linear(last.ln_1(x_in), last.attn.in_proj_weight, last.attn.in_proj_bias).chunk(3, dim=-1)
    attn_output, attn = attention_layer(q, k, v, 1)
    if torch.is_grad_enabled() and not attn_output.requires_grad:
        attn_output.requires_grad_(True)              # a frozen model: grad_eclip differentiates with respect to this tensor

    def tail(after_attn):
        y = after_attn + x_in
        y = y + last.mlp(last.ln_2(y))
        return visual.ln_post(y.transpose(0, 1)) @ visual.proj
    outputs = tail(F.linear(attn_output, w, b))
    with torch.no_grad():
        q_out, k_out, v_out = F.linear(torch.stack((q, k, v), dim=0), w, b)
        v_final = tail(v_out)
    return outputs, v_final[:, 1:], x_in, v, q_out, k_out, attn, attn_output, grid


def _ksim(first, k_out):
    """cosine of `first` (1, D) with the patch rows of k_out, image 0"""
    return (F.normalize(first, dim=-1) * F.normalize(k_out[1:, 0, :], dim=-1)).sum(-1)


def grad_eclip(c, q_out, k_out, v, att_output, map_size, withksim=True, withgrad=True):
    """The Grad-ECLIP map of image 0 for the cosine c, (h, w)"""
    rows = v[1:, 0, :]
    if withgrad:
        rows = torch.autograd.grad(c, att_output, retain_graph=True)[0].detach()[:1, 0, :] * rows
    if withksim:
        cos = _ksim(q_out[:1, 0, :], k_out)
        cos = (cos - cos.min()) / (cos.max() - cos.min())
        rows = rows * cos[:, None]
    return F.relu_(rows.detach().sum(-1)).reshape(*map_size)


def mask_clip(txt_feats, v_final, k_out, map_size):
    """The MaskCLIP maps of image 0 for the (E, T) text features, (T, h, w)"""
    cosine_v = (F.normalize(v_final, dim=-1) @ txt_feats)[0].transpose(1, 0)
    return (cosine_v * _ksim(k_out[:1, 0, :], k_out)[None, :]).detach().reshape(-1, *map_size)


# ---------------------------------------------------------------------------------- the one-row flow
class ClsPass:
    """What cls_pass leaves: k, v, k_out, x_in (L, B, D); attn (B, L); att_output, q_out0 (B, D); outputs0 (B, E), the class row of
    the embedding; grid (h, w).  `leaves[b]` is the (1, D) autograd leaf that is row b of att_output, and outputs0[b] hangs on it."""


def cls_pass(clipmodel, x, want_grad=True):
    """The class-token row of clip_encode_dense for x (B, 3, H, W), on the model's HIP device -> ClsPass.  want_grad: keep the one-row tail in
    the autograd graph, for eclip and eclip_wo."""
    visual, last = check_layout(clipmodel)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"x must be (B, 3, H, W), got {tuple(x.shape)}")
    ksize = visual.conv1.kernel_size
    if x.shape[2] % ksize[0] or x.shape[3] % ksize[1]:
        raise ValueError(f"x is {x.shape[2]} x {x.shape[3]}: H and W must be multiples of the patch size {tuple(ksize)}")
    B, D = x.shape[0], visual.transformer.width
    w_in, b_in = last.attn.in_proj_weight, last.attn.in_proj_bias
    w_out, b_out = last.attn.out_proj.weight, last.attn.out_proj.bias
    p = ClsPass()

    def tokens(visual, image):
        tok, p.grid = T.interpolated_tokens(visual, image)
        return tok
    with torch.no_grad():
        for b, x_in in T.per_image(visual, x, list(visual.transformer.resblocks)[:-1], tokens):
            if b == 0:
                L, dev = x_in.shape[0], x_in.device
                p.x_in = torch.empty((L, B, D), dtype=x_in.dtype, device=dev)
                kv = torch.empty((L, B, 2 * D), dtype=x_in.dtype, device=dev)
                p.k_out = torch.empty((L, B, D), dtype=x_in.dtype, device=dev)
                q0 = torch.empty((B, D), dtype=x_in.dtype, device=dev)
                p.q_out0 = torch.empty((B, D), dtype=x_in.dtype, device=dev)
            normed = last.ln_1(x_in)
            p.x_in[:, b] = x_in[:, 0]
            kv[:, b] = F.linear(normed[:, 0], w_in[D:], b_in[D:])
            q0[b] = F.linear(normed[:1, 0], w_in[:D], b_in[:D])[0]
            p.k_out[:, b] = F.linear(kv[:, b, :D], w_out, b_out)
            p.q_out0[b] = F.linear(q0[b:b + 1], w_out, b_out)[0]
        p.k, p.v = kv[:, :, :D], kv[:, :, D:]
        p.attn, p.att_output = K.clip_cls_attention(q0, p.k, p.v)
    p.leaves = [p.att_output[b:b + 1].clone().requires_grad_(want_grad) for b in range(B)]
    with torch.set_grad_enabled(want_grad):
        p.outputs0 = [T.tail(visual, last, leaf, p.x_in[0, b]) for b, leaf in enumerate(p.leaves)]
    return p


def eclip_batch(clipmodel, x, txt_embedding, method, img_hw=None):
    """The row `method` of get_CLIP_attr for x (B, 3, H, W) and already normalised text embeddings (T, E), shared, or (B, T, E):
    (B, h, w) fp32 maps on the device, summed over the T texts; with img_hw the harness's map, resized to (img_hw, img_hw) and
    absolute (evaluatePerturbation.py:443-445)."""
    if method in REFUSED:
        raise NotImplementedError(f"eclip_batch: the row {method!r} needs {REFUSED[method]}, which this engine does not build")
    if method not in METHODS:
        raise ValueError(f"eclip_batch: unknown row {method!r}; the served rows are {METHODS}")
    visual, last = check_layout(clipmodel)
    withksim, withgrad = _ECLIP_FLAGS.get(method, (False, False))
    p = cls_pass(clipmodel, x, want_grad=withgrad)
    B, dev = len(p.leaves), p.attn.device
    E = visual.proj.shape[1]
    # the feature count is checked where a kernel reads the features; the other rows multiply by them in torch, or only count T
    txt = T.texts(txt_embedding, B, E if method == "maskclip" else None, "txt_embedding")
    txt = txt.to(device=dev, dtype=p.attn.dtype).expand(B, -1, -1)
    if method == "selfattn":
        maps = p.attn[:, 1:].float()
    elif method == "maskclip":
        with torch.no_grad():
            v_final = torch.empty((B, p.k.shape[0] - 1, E), dtype=p.attn.dtype, device=dev)
            for b in range(B):
                v_final[b] = T.tail(visual, last, p.v[:, b], p.x_in[:, b])[1:]
        maps = K.clip_maskclip_map(v_final, txt.contiguous(), p.k_out)
    else:
        grad_cls = None
        if withgrad:
            grad_cls = torch.empty((B, txt.shape[1], p.k.shape[2]), dtype=p.attn.dtype, device=dev)
            for b, (leaf, out) in enumerate(zip(p.leaves, p.outputs0)):
                cosines = (F.normalize(out, dim=-1) @ txt[b].t())[0]
                for t, c in enumerate(cosines):
                    grad_cls[b, t] = torch.autograd.grad(c, leaf, retain_graph=True)[0][0]
        maps = K.clip_eclip_map(p.q_out0, p.k_out, p.v, grad_cls, texts=txt.shape[1], withksim=withksim, withgrad=withgrad)
    return T.finish(maps, B, p.grid, img_hw)

