"""Restatements for the CLIP Surgery row (xai_engine/surgery.py, include/xai_csurg.h), independent of the engine:

  * the reference's dual-path flow (CLIP_Surgery/clip/clip_surgery_model.py:71-103, :253-280, :314-355) and the tail of
    clip_surgery_map (generate_emap.py:117-129; clip.py:271-308) as functions of a state dict, parametrised by dtype like
    tests/clip_restated.py: `None` keeps the stored dtype, a torch dtype casts every weight;
  * the closed form the GPU path follows: one GEMM with K = 6 D behind the v-v attention of the six blocks, and
    sim[i][t] = sum_c f_ic (w_t t_tc - r_c) without the (L, T, E) tensor;
  * K86 and K87 in NumPy, in the accumulation orders the header states, and the header's bounds behind the first exp.
"""
import numpy as np
import torch
import torch.nn.functional as F

import clip_restated as R
from clip_restated import U, f32, wave_sum_rows

DUAL = 6
# (resolution, patch, width, layers, heads, embed)
MODELS = {"six": (32, 8, 32, 6, 2, 16),       # L = 17; the dual path starts at block 0
          "wave": (64, 8, 64, 7, 2, 16),      # L = 65: one past a wave
          "one": (32, 8, 64, 7, 1, 16),       # H = 1, d = 64
          "long": (224, 16, 32, 6, 2, 16)}    # L = 197
TEXT = R.TEXT
TEXTS = 60                                     # the caption and the reference's 59 context classes


def fixture_texts(t_seed, n, embed):
    """n normalised text rows, (n, embed) fp32: what encode_text_with_prompt_ensemble is stood in by"""
    return R.fixture_texts(t_seed, n, embed)


# ------------------------------------------------------------------------------------------------ the flows in torch
def tokens(sd, x):
    """x (N, 3, R, R) -> the (L, N, D) input of the first block (clip_surgery_model.py:329-347, at the native size)"""
    w = sd["visual.conv1.weight"]
    x = F.conv2d(x.to(w.dtype), w, stride=w.shape[-1])
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    x = torch.cat([sd["visual.class_embedding"].to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype), x], dim=1)
    return R._ln(x + sd["visual.positional_embedding"].to(x.dtype), sd, "visual.ln_pre").permute(1, 0, 2)


def plain_block(sd, i, x, heads):
    """a block in front of the dual path: torch's own nn.MultiheadAttention on the stored weights, called as the reference calls it"""
    pre = f"visual.transformer.resblocks.{i}."
    D = x.shape[-1]
    mha = torch.nn.MultiheadAttention(D, heads).to(x.dtype).eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(sd[pre + "attn.in_proj_weight"])
        mha.in_proj_bias.copy_(sd[pre + "attn.in_proj_bias"])
        mha.out_proj.weight.copy_(sd[pre + "attn.out_proj.weight"])
        mha.out_proj.bias.copy_(sd[pre + "attn.out_proj.bias"])
    y = R._ln(x, sd, pre + "ln_1")
    x = x + mha(y, y, y, need_weights=False, attn_mask=None)[0]
    return x + R._mlp(R._ln(x, sd, pre + "ln_2"), sd, pre)


def dual_attention(sd, pre, y, heads):
    """Attention.forward (:71-103) on y (N, L, D) -> (new path, original path, v (N, heads, L, d))"""
    B, N, C = y.shape
    qkv = F.linear(y, sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]).reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    scale = (C // heads) ** -0.5
    attn_ori = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    attn = ((v @ v.transpose(-2, -1)) * scale).softmax(dim=-1)
    x_ori = (attn_ori @ v).transpose(1, 2).reshape(B, N, C)
    x = (attn @ v).transpose(1, 2).reshape(B, N, C)
    w, b = sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"]
    return F.linear(x, w, b), F.linear(x_ori, w, b), v


def dual_path(sd, x, heads, dtype=None):
    """encode_image of the Surgery model in the reference's sequence of operations -> (N, L, E) features"""
    sd = R.cast(sd, dtype)
    n = R._layers(sd)
    with torch.no_grad():
        t = tokens(sd, x)
        for i in range(n - DUAL):
            t = plain_block(sd, i, t, heads)
        new, ori = t, t
        for i in range(n - DUAL, n):
            pre = f"visual.transformer.resblocks.{i}."
            res, ori_res, _ = dual_attention(sd, pre, R._ln(ori, sd, pre + "ln_1").transpose(0, 1), heads)
            ori = ori + ori_res.transpose(0, 1)
            ori = ori + R._mlp(R._ln(ori, sd, pre + "ln_2"), sd, pre)
            new = new + res.transpose(0, 1)
        new = torch.cat([ori[:1], new[1:]], dim=0).permute(1, 0, 2)
        return R._ln(new, sd, "visual.ln_post") @ sd["visual.proj"]


def closed_features(sd, x, heads, dtype=None):
    """The same features as the GPU path forms them: the original path alone through the six blocks, each block's v kept; the v-v
    attention of the six blocks; ONE GEMM with K = 6 D and the summed biases; row 0 from the original path -> (N, L, E)"""
    sd = R.cast(sd, dtype)
    n = R._layers(sd)
    with torch.no_grad():
        t = tokens(sd, x)
        for i in range(n - DUAL):
            t = plain_block(sd, i, t, heads)
        x_in, ori = t.transpose(0, 1), t
        outs, ws, bias = [], [], 0
        for i in range(n - DUAL, n):
            pre = f"visual.transformer.resblocks.{i}."
            _, ori_res, v = dual_attention(sd, pre, R._ln(ori, sd, pre + "ln_1").transpose(0, 1), heads)
            ori = ori + ori_res.transpose(0, 1)
            ori = ori + R._mlp(R._ln(ori, sd, pre + "ln_2"), sd, pre)
            B, _, N, d = v.shape
            attn = ((v @ v.transpose(-2, -1)) * d ** -0.5).softmax(dim=-1)
            outs.append((attn @ v).transpose(1, 2).reshape(B, N, heads * d))
            ws.append(sd[pre + "attn.out_proj.weight"])
            bias = bias + sd[pre + "attn.out_proj.bias"]
        new = x_in + (torch.cat(outs, dim=-1) @ torch.cat(ws, dim=1).t() + bias)
        new = torch.cat([ori.transpose(0, 1)[:, :1], new[:, 1:]], dim=1)
        return R._ln(new, sd, "visual.ln_post") @ sd["visual.proj"]


def v_thirds(sd, x, heads, dtype=None):
    """the V third of the six dual blocks' in-projections for one image x -> (6, L, 1, D): what K86 is handed"""
    sd = R.cast(sd, dtype)
    n = R._layers(sd)
    out = []
    with torch.no_grad():
        t = tokens(sd, x)
        for i in range(n - DUAL):
            t = plain_block(sd, i, t, heads)
        ori = t
        for i in range(n - DUAL, n):
            pre = f"visual.transformer.resblocks.{i}."
            y = R._ln(ori, sd, pre + "ln_1")
            out.append(F.linear(y, sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"])[..., 2 * y.shape[-1]:])
            _, ori_res, _ = dual_attention(sd, pre, y.transpose(0, 1), heads)
            ori = ori + ori_res.transpose(0, 1)
            ori = ori + R._mlp(R._ln(ori, sd, pre + "ln_2"), sd, pre)
    return torch.stack(out)


def reference_map(feats, txt, shape):
    """the tail of clip_surgery_map (generate_emap.py:121-128) in the reference's operations: feats (1, L, E), txt (T, E) ->
    ((1, H, W, T), the same map before the resize (1, p, p, T))"""
    f = feats / feats.norm(dim=1, keepdim=True)
    prob = f[:, :1, :] @ txt.t()
    prob = (prob * 2).softmax(-1)
    w = prob / prob.mean(-1, keepdim=True)
    b, n_t, n_i, c = f.shape[0], txt.shape[0], f.shape[1], f.shape[2]
    prod = f.reshape(b, n_i, 1, c) * txt.reshape(1, 1, n_t, c)
    prod = prod * w.reshape(1, 1, n_t, 1)
    prod = prod - prod.mean(2, keepdim=True)
    sm = prod.sum(-1)[:, 1:, :]
    sm = (sm - sm.min(1, keepdim=True)[0]) / (sm.max(1, keepdim=True)[0] - sm.min(1, keepdim=True)[0])
    side = int(sm.shape[1] ** 0.5)
    sm = sm.reshape(sm.shape[0], side, side, -1).permute(0, 3, 1, 2)
    return F.interpolate(sm, shape, mode="bilinear").permute(0, 2, 3, 1), sm.permute(0, 2, 3, 1)


def full_map(grid, shape):
    """get_similarity_map's resize of (p, p) maps (any leading axes) to `shape`, in the maps' dtype on the CPU"""
    g = torch.as_tensor(grid)
    lead = g.shape[:-2]
    return F.interpolate(g.reshape(1, -1, *g.shape[-2:]), tuple(shape), mode="bilinear").reshape(*lead, *shape)


def closed_similarity(feats, txt, texts_out=1):
    """K87's closed form in torch: feats (N, L, E), txt (T, E) -> the min-max-normalised (N, texts_out, L - 1)"""
    f = feats / feats.norm(dim=1, keepdim=True)
    p = ((f[:, 0, :] @ txt.t()) * 2).softmax(-1)                         # (N, T)
    w = p / p.mean(-1, keepdim=True)
    wt = w[:, :, None] * txt[None]                                       # (N, T, E)
    r = wt.mean(1, keepdim=True)
    sim = torch.einsum("nic,ntc->nti", f[:, 1:], wt[:, :texts_out] - r)
    lo, hi = sim.min(-1, keepdim=True)[0], sim.max(-1, keepdim=True)[0]
    return (sim - lo) / (hi - lo)


def closed_map(feats, txt, shape, texts_out=1):
    """closed_similarity and the bilinear resize -> (N, texts_out, H, W)"""
    sm = closed_similarity(feats, txt, texts_out)
    side = int(sm.shape[-1] ** 0.5)
    return F.interpolate(sm.reshape(sm.shape[0], texts_out, side, side), shape, mode="bilinear")


# ------------------------------------------------------------------------------------------------ K86, K87 in NumPy
def exp32(x):
    """exp evaluated in fp64 and rounded to fp32: within half an ulp (and a hair) of exp, subnormal results kept"""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, dtype=np.float64)).astype(f32)


def k86(v, H):
    """v (n, L, B, D) fp32 -> (scores (n, B, H, L, L), p (n, B, H, L, L), out (n, B, L, D)) in the header's orders"""
    v = np.asarray(v, dtype=f32)
    n, L, B, D = v.shape
    d = D // H
    scale = f32(float(d) ** -0.5)
    scores = np.zeros((n, B, H, L, L), dtype=f32)
    probs = np.zeros((n, B, H, L, L), dtype=f32)
    out = np.zeros((n, B, L, D), dtype=f32)
    with np.errstate(all="ignore"):
        for blk in range(n):
            for b in range(B):
                for h in range(H):
                    V = v[blk, :, b, h * d:(h + 1) * d]
                    s = np.zeros((L, L), dtype=f32)
                    for c in range(d):
                        s = s + V[:, c, None] * V[None, :, c]
                    s = s * scale
                    m = np.fmax.reduce(s, axis=1, initial=-np.inf).astype(f32)
                    e = exp32(s - m[:, None])
                    p = e / wave_sum_rows(e)[:, None]
                    o = np.zeros((L, d), dtype=f32)
                    for j in range(L):
                        o = o + p[:, j, None] * V[None, j, :]
                    scores[blk, b, h], probs[blk, b, h] = s, p
                    out[blk, b, :, h * d:(h + 1) * d] = o
    return scores, probs, out


def k86_bound(p_ref, v, H):
    """The header's bound behind K86's first exp on out (n, B, L, D), from the restated p (n, B, H, L, L) and v (n, L, B, D):
       dp_j = (10 + 2 m) u p_j + 3 * 2^-149, m = ceil(L / 64) + 6;  do_ic = sum_j dp_j |v_jc| + 2 L u sum_j |p_j v_jc|"""
    n, L, B, D = v.shape
    d = D // H
    m = -(-L // 64) + 6
    p = p_ref.astype(np.float64)
    dp = (10 + 2 * m) * U * p + 3 * 2.0 ** -149
    av = np.abs(v.astype(np.float64)).reshape(n, L, B, H, d)
    return (np.einsum("nbhij,njbhc->nbihc", dp, av) + 2 * L * U * np.einsum("nbhij,njbhc->nbihc", p, av)).reshape(n, B, L, D)


def k87(feats, txt, texts_out=1, w=None):
    """feats (B, L, E), txt (T, E) or (B, T, E) fp32 -> (out (B, texts_out, L - 1), w (B, T)) in the header's orders; `w`: these
    weights in place of the computed ones (the kernel's own, fed back)"""
    feats, txt = np.asarray(feats, dtype=f32), np.asarray(txt, dtype=f32)
    B, L, E = feats.shape
    if txt.ndim == 2:
        txt = np.broadcast_to(txt, (B,) + txt.shape)
    T = txt.shape[1]
    out = np.zeros((B, texts_out, L - 1), dtype=f32)
    ws = np.zeros((B, T), dtype=f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            Fb, t = feats[b], txt[b]
            s = np.zeros(E, dtype=f32)
            for i in range(L):
                s = s + Fb[i] * Fb[i]
            f = Fb / np.sqrt(s)
            if w is None:
                x = f32(2) * wave_sum_rows(f[0][None, :] * t)
                e = exp32(x - np.fmax.reduce(x, initial=-np.inf).astype(f32))
                p = e / wave_sum_rows(e)
                wb = p / (wave_sum_rows(p) / f32(T))
            else:
                wb = np.asarray(w[b], dtype=f32)
            r = np.zeros(E, dtype=f32)
            for k in range(T):
                r = r + wb[k] * t[k]
            r = r / f32(T)
            sim = wave_sum_rows(f[None, 1:, :] * (wb[:texts_out, None, None] * t[:texts_out, None, :] - r))      # (texts_out, L - 1)
            lo, hi = sim.min(axis=1, keepdims=True), sim.max(axis=1, keepdims=True)      # NumPy's return a NaN that is there, as torch's
            out[b] = (sim - lo) / (hi - lo)
            ws[b] = wb
    return out, ws


def k87_w_bound(w_ref):
    """the header's bound of K87's w: (24 + 6 m) u |w| + (3 T + 2) 2^-149, m = ceil(T / 64) + 6"""
    T = w_ref.shape[-1]
    m = -(-T // 64) + 6
    return (24 + 6 * m) * U * np.abs(w_ref.astype(np.float64)) + (3 * T + 2) * 2.0 ** -149
