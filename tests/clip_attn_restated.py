"""Restatements for the attention rows of CLIP (xai_engine/clip_attn.py, include/xai_cattn.h), independent of the engine:

  * the reference's flow for game, rollout and lrp (generate_emap.py: mm_interpret :133-174, compute_rollout_attention :269-285,
    clip_lrp :207-239, on the forward of Game_MM_CLIP/clip/model.py and auxilary.py:153-255) as functions of a state dict,
    parametrised by dtype like tests/clip_restated.py: `None` keeps the stored mixed precision, a torch dtype casts every weight;
  * the row form of lrp, r <- r + r C_i from the last block down, next to the matrix form;
  * K82-K85 in NumPy, in the accumulation orders and at the rounding points the header states.
"""
import numpy as np
import torch
import torch.nn.functional as F

import clip_restated as R
from clip_restated import f32, rT, wave_sum_rows

ROWS = ("game", "rollout", "lrp")
# (resolution, patch, width, layers, heads, embed)
MODELS = {"tiny": (16, 8, 32, 3, 2, 16),      # L = 5: fewer tokens than a wave, d = 16
          "mini": (32, 8, 64, 3, 4, 16),      # L = 17, d = 16
          "wave": (64, 8, 64, 3, 2, 16),      # L = 65: one past a wave, d = 32
          "long": (224, 16, 64, 2, 4, 16),    # L = 197
          "one": (32, 8, 32, 3, 1, 16)}       # H = 1, d = 32
TEXT = R.TEXT


def fixture_tokens(t_seed, n):
    """the fixtures' texts: n rows of seeded random token ids, (n, context_length) int64"""
    g = torch.Generator().manual_seed(t_seed)
    return torch.randint(0, TEXT["vocab_size"], (n, TEXT["context_length"]), generator=g)


def tokens(sd, x):
    """x (N, 3, R, R) -> the (L, N, D) input of the first block, as visual.forward (model.py:229-237); a leaf of the autograd graph in
    front, because the tensors of a state dict ask for none"""
    w = sd["visual.conv1.weight"]
    x = F.conv2d(x.to(w.dtype).clone().requires_grad_(True), w, stride=w.shape[-1])
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    x = torch.cat([sd["visual.class_embedding"].to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype), x], dim=1)
    return R._ln(x + sd["visual.positional_embedding"].to(x.dtype), sd, "visual.ln_pre").permute(1, 0, 2)


def block(sd, i, x, heads):
    """block i on (L, N, D) tokens in the reference's sequence (auxilary.py:153-255, model.py:195-198) -> (output, attention
    probabilities (N * heads, L, L))"""
    L, N, D = x.shape
    hd = D // heads
    pre = f"visual.transformer.resblocks.{i}."
    q, k, v = F.linear(R._ln(x, sd, pre + "ln_1"), sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]).chunk(3, dim=-1)
    q = q * (float(hd) ** -0.5)
    q, k, v = (t.contiguous().view(L, N * heads, hd).transpose(0, 1) for t in (q, k, v))
    a = F.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    out = torch.bmm(a, v).transpose(0, 1).contiguous().view(L, N, D)
    x = x + F.linear(out, sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"])
    return x + R._mlp(R._ln(x, sd, pre + "ln_2"), sd, pre), a


def forward(sd, x, heads, dtype=None):
    """visual.forward of the state dict for x (N, 3, R, R), every block written out -> (image features (N, E), [attention
    probabilities of block i, (N * heads, L, L), nodes of the autograd graph])"""
    sd = R.cast(sd, dtype)
    x = tokens(sd, x)
    probs = []
    for i in range(R._layers(sd)):
        x, a = block(sd, i, x, heads)
        probs.append(a)
    x = x.permute(1, 0, 2)
    return R._ln(x[:, 0, :], sd, "visual.ln_post") @ sd["visual.proj"], probs


def logits_of(sd, feats, txt):
    """model.forward's logits (model.py:369-374) of image features (N, E) against normalised texts (T, E) -> (N, T)"""
    feats = feats / feats.norm(dim=-1, keepdim=True)
    return sd["logit_scale"].exp() * feats @ txt.t()


def one_row(sd, x, txt, heads, dtype=torch.float64):
    """The class-token row of the last block alone, as xai_engine.clip_attn.cls_rows and the game row compute it, for one image x and
    already normalised texts (T, E) -> (g (T, D), v (L, D), a0 (heads, L)): one query per head, the tail on one row, a one-row
    backward of each text's logit"""
    sd = R.cast(sd, dtype)
    n = R._layers(sd)
    x_in = tokens(sd, x)
    for i in range(n - 1):
        x_in, _ = block(sd, i, x_in, heads)
    x_in = x_in.detach()
    D = x_in.shape[-1]
    d = D // heads
    pre = f"visual.transformer.resblocks.{n - 1}."
    iw, ib = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    y = R._ln(x_in, sd, pre + "ln_1")[:, 0]
    kv = F.linear(y, iw[D:], ib[D:])
    k, v = kv[:, :D], kv[:, D:]
    q0 = (F.linear(y[:1], iw[:D], ib[:D]) * (float(d) ** -0.5)).view(heads, 1, d)
    a0 = F.softmax(torch.bmm(q0, k.reshape(-1, heads, d).permute(1, 2, 0)), dim=-1)                 # (heads, 1, L)
    att0 = torch.bmm(a0, v.reshape(-1, heads, d).transpose(0, 1)).reshape(1, D).detach().requires_grad_(True)
    t = F.linear(att0, sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"]) + x_in[0, 0]
    t = t + R._mlp(R._ln(t, sd, pre + "ln_2"), sd, pre)
    logits = logits_of(sd, R._ln(t, sd, "visual.ln_post") @ sd["visual.proj"], txt.to(t.dtype))[0]
    g = torch.stack([torch.autograd.grad(c, att0, retain_graph=True)[0][0] for c in logits])
    return g, v.detach(), a0[:, 0].detach()


def probs_and_grads(sd, x, txt_raw, heads, dtype=None):
    """The image repeated once per text, model.forward's logits (model.py:364-378) against the raw text features txt_raw (T, E), and the
    gradients of the sum of the diagonal (generate_emap.py:134-142) -> ([A_i], [G_i]), each (T * heads, L, L)"""
    T = txt_raw.shape[0]
    feats, probs = forward(sd, x.repeat(T, 1, 1, 1), heads, dtype)
    txt = txt_raw.to(feats.dtype)
    feats = feats / feats.norm(dim=-1, keepdim=True)
    txt = txt / txt.norm(dim=-1, keepdim=True)
    scale = R.cast(sd, dtype)["logit_scale"].exp()
    logits = scale * feats @ txt.t()
    one_hot = torch.sum(torch.eye(T, dtype=torch.float32) * logits)
    grads = torch.autograd.grad(one_hot, probs)
    return [a.detach() for a in probs], [g.detach() for g in grads]


def _cam(a, g, T):
    L = a.shape[-1]
    return (g * a).reshape(T, -1, L, L).clamp(min=0).mean(dim=1)


def rows_from(probs, grads, T):
    """{row: (p, p) map} of the three rows as the harness takes them (evaluatePerturbation.py:410-437): game summed over the texts,
    rollout's first batch entry, lrp (T = 1 only) the first image"""
    L = probs[0].shape[-1]
    p = int((L - 1) ** 0.5)
    eye = torch.eye(L, dtype=probs[0].dtype).unsqueeze(0).expand(T, L, L)
    out = {}
    cam = _cam(probs[-1], grads[-1], T)
    out["game"] = (eye + torch.bmm(cam, eye))[:, 0, 1:].reshape(T, p, p).sum(0)
    avg = (probs[-1].sum(dim=0) / probs[-1].shape[0]).unsqueeze(0)
    aug = avg + torch.eye(L).expand(1, L, L)
    out["rollout"] = (aug / aug.sum(dim=-1, keepdim=True))[:, 0, 1:].reshape(1, p, p)[0]
    if T == 1:
        rel = eye
        for a, g in zip(probs, grads):
            rel = rel + torch.bmm(_cam(a, g, T), rel)
        out["lrp"] = rel[:, 0, 1:].reshape(-1, p, p)[0]
    return out


def lrp_matrix_form(cams):
    """cams: [C_i (L, L)] -> row 0 of R after R <- R + C_i @ R, i ascending, from R = I"""
    rel = torch.eye(cams[0].shape[-1], dtype=cams[0].dtype)
    for c in cams:
        rel = rel + c @ rel
    return rel[0]


def lrp_row_form(cams):
    """the same row as n vector-matrix products from the last block down: r <- r + r C_i"""
    r = torch.zeros(cams[0].shape[-1], dtype=cams[0].dtype)
    r[0] = 1
    for c in reversed(cams):
        r = r + r @ c
    return r


# ------------------------------------------------------------------------------------------------ K82-K85 in NumPy
def relu(x):
    """the header's relu: a NaN stays, -0 becomes +0"""
    return np.where(x > 0, x, np.where(np.isnan(x), x, f32(0))).astype(f32)


def k82(g, v, a0, dt):
    """g (B, T, D), v (L, B, D), a0 (B, H, L) as fp32 values of dtype dt -> out (B, L - 1) fp32"""
    L, B, D = v.shape
    H = a0.shape[1]
    d = D // H
    out = np.zeros((B, L - 1), dtype=f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            acc = np.zeros(L - 1, dtype=f32)
            for t in range(g.shape[1]):
                heads = np.zeros(L - 1, dtype=f32)
                for h in range(H):
                    sl = slice(h * d, (h + 1) * d)
                    grad = rT(wave_sum_rows(g[b, t, sl][None, :] * v[1:, b, sl]), dt)
                    heads = heads + relu(rT(grad * a0[b, h, 1:], dt))
                acc = acc + rT(heads / f32(H), dt)
            out[b] = rT(acc, dt)
    return out


def k83(a0, T, dt):
    """a0 (B, H, L) -> out (B, L - 1) fp32"""
    B, H, L = a0.shape
    with np.errstate(all="ignore"):
        s = np.zeros((B, L), dtype=f32)
        for _ in range(T):
            for h in range(H):
                s = s + a0[:, h]
        a = rT(rT(s, dt) / f32(T * H), dt)
        a[:, 0] = a[:, 0] + f32(1)
        pad = (-L) % 256
        ap = np.concatenate([a, np.zeros((B, pad), dtype=f32)], axis=1).reshape(B, -1, 256)
        lanes = np.zeros((B, 256), dtype=f32)
        for i in range(ap.shape[1]):
            lanes = lanes + ap[:, i]
        waves = wave_sum_rows(lanes.reshape(B, 4, 64))
        total = np.zeros(B, dtype=f32)
        for w in range(4):
            total = total + waves[:, w]
        return (a[:, 1:] / total[:, None]).astype(f32)


def k84(attn, grad, dt):
    """attn, grad (n, B, H, L, L) -> c (B, n, L, L) as fp32 values of dt"""
    n, B, H, L, _ = attn.shape
    with np.errstate(all="ignore"):
        acc = np.zeros((n, B, L, L), dtype=f32)
        for h in range(H):
            acc = acc + relu(rT(grad[:, :, h] * attn[:, :, h], dt))
        return np.ascontiguousarray(np.transpose(rT(acc / f32(H), dt), (1, 0, 2, 3)))


def k85(c, dt):
    """c (B, n, L, L) -> out (B, L - 1) fp32"""
    B, n, L, _ = c.shape
    r = np.zeros((B, L), dtype=f32)
    r[:, 0] = 1
    with np.errstate(all="ignore"):
        for i in range(n - 1, -1, -1):
            s = np.zeros((B, L), dtype=f32)
            for k in range(L):
                s = s + r[:, k, None] * c[:, i, k, :]
            r = rT(r + rT(s, dt), dt)
    return r[:, 1:].copy()
