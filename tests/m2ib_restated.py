"""Restatements for CLIP's M2IB row (xai_engine/m2ib.py, include/xai_hip_cm2ib.h), independent of the engine:

  * the reference's flow (M2IB/scripts/iba.py:89-194, methods.py:46-51, clip_wrapper.py) as a function of a state dict, parametrised
    by dtype like tests/clip_restated.py (`None` keeps the stored fp16: OpenAI's mixed precision; a torch dtype casts every weight):
    `literal=True` runs every block and the text tower on the `copies` rows in every step, as the reference does; the default is the
    closed form the GPU path follows: x9 once on one row, the blocks behind the bottleneck only, no mean over the equal copies;
  * text_encoder_wrapper.forward (clip_wrapper.py:90-108): no causal mask, the last position, text_projection twice;
  * K88, K89 and K90 in NumPy in the header's sequence of operations, and the header's bounds behind expf and logf.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import clip_restated as R
from clip_restated import U, f32, wave_sum_rows
from surgery_restated import exp32, tokens

# (resolution, patch, width, layers, heads, embed, layer): all of 12 layers, so that the harness's default layer = 9 is what is run
MODELS = {"five": (32, 16, 64, 12, 1, 16, 9),          # L = 5, H = 1 (d = 64)
          "seventeen": (32, 8, 64, 12, 2, 16, 9),      # L = 17
          "fifty": (224, 32, 64, 12, 2, 16, 9),        # L = 50, ViT-B/32's grid: the 224 x 224 map is a 32 x upsample of 7 x 7
          "ten": (32, 16, 64, 12, 2, 16, 10)}          # layer = 10: a single block behind the bottleneck
TEXT = R.TEXT                                          # transformer_width == embed == 16: the wrapper projects twice
MAP = 224
STEPS, COPIES, BETA, LR = 10, 10, 0.1, 1.0
GRID = 2.0 ** -9                                       # the stored weights are multiples of it (fp16 values that compress)


def tokens_of(model):
    res, patch = MODELS[model][:2]
    return (res // patch) ** 2 + 1


def fixture_ids(t_seed):
    """the caption's token ids, (1, context_length) int64"""
    g = torch.Generator().manual_seed(t_seed)
    return torch.randint(0, TEXT["vocab_size"], (1, TEXT["context_length"]), generator=g)


def fixture_noise(noise_seed, model, steps=STEPS, copies=COPIES):
    """the draws of a CPU-seeded reference run, in its order: one torch.empty(copies, L, D).normal_() per forward, `steps` of them
    -> (steps, copies, L, D) fp32; the last one feeds the step that is never read"""
    torch.manual_seed(noise_seed)
    L, D = tokens_of(model), MODELS[model][2]
    return torch.stack([torch.empty(copies, L, D).normal_() for _ in range(steps)])


def noise_probe(noise):
    """16 values of the first draw: a changed CPU generator fails loudly instead of comparing against other noise"""
    return noise[0].reshape(-1)[:16].clone()


# ------------------------------------------------------------------------------------------------ the flows in torch
def block_nld(sd, pre, x, heads):
    """permute_then_forward (clip_wrapper.py:11-16) on (N, L, D) tokens with torch's own nn.MultiheadAttention on the stored weights,
    called as the reference's ResidualAttentionBlock.attention calls it with need_weights False and no mask"""
    D = x.shape[-1]
    mha = torch.nn.MultiheadAttention(D, heads).to(x.dtype).eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(sd[pre + "attn.in_proj_weight"])
        mha.in_proj_bias.copy_(sd[pre + "attn.in_proj_bias"])
        mha.out_proj.weight.copy_(sd[pre + "attn.out_proj.weight"])
        mha.out_proj.bias.copy_(sd[pre + "attn.out_proj.bias"])
    x = x.permute(1, 0, 2)
    y = R._ln(x, sd, pre + "ln_1")
    x = x + mha(y, y, y, need_weights=False, attn_mask=None)[0]
    x = x + R._mlp(R._ln(x, sd, pre + "ln_2"), sd, pre)
    return x.permute(1, 0, 2)


def _run(sd, x, lo, hi, heads, cd):
    for i in range(lo, hi):
        x = block_nld(sd, f"visual.transformer.resblocks.{i}.", x.to(cd), heads)
    return x


def wrapper_text(sd, ids, heads, dtype=None):
    """text_encoder_wrapper.forward for ids (N, n) -> (N, E)"""
    sd = R.cast(sd, dtype)
    cd = sd["text_projection"].dtype
    n_blocks = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))
    with torch.enable_grad():             # as the reference calls it in every step: nn.MultiheadAttention's autograd path
        x = F.embedding(ids, sd["token_embedding.weight"]).to(cd)
        x = x + sd["positional_embedding"].to(cd)[:x.shape[1], :]
        for i in range(n_blocks):
            x = block_nld(sd, f"transformer.resblocks.{i}.", x.to(cd), heads)
        x = R._ln(x, sd, "ln_final").to(cd)
        x = x @ sd["text_projection"]
        return (x[torch.arange(x.shape[0]), -1] @ sd["text_projection"]).detach()


def flow(sd, x, txt, noise, heads, layer, dtype=None, beta=BETA, steps=STEPS, lr=LR, literal=False, ids=None):
    """vision_heatmap_iba in front of its resize for one image x (1, 3, R, R), the wrapper's text feature txt (1, E) and noise
    (>= steps - 1, copies, L, D) -> dict(grid (p, p), cap (L, D), alpha (1, L, D) after steps - 1 updates, g1 the first step's
    gradient).  alpha, the moments and the capacity are fp32 (fp64 when dtype is torch.float64).  literal with `ids`: the text tower
    too runs on the `copies` rows, as the reference's does, in place of txt."""
    if literal and ids is not None:
        txt = wrapper_text(sd, ids.expand(noise.shape[1], -1), TEXT["transformer_heads"], dtype)
    sd = R.cast(sd, dtype)
    cd = sd["visual.conv1.weight"].dtype
    pd = torch.float64 if cd == torch.float64 else torch.float32
    n, copies = R._layers(sd), noise.shape[1]
    with torch.enable_grad():             # nn.MultiheadAttention's autograd path, the one the reference's ten forwards take
        x9 = None if literal else _run(sd, tokens(sd, x).permute(1, 0, 2), 0, layer + 1, heads, cd).detach()  # (1, L, D)
        shape = tokens(sd, x).permute(1, 0, 2).shape
    alpha = torch.nn.Parameter(torch.full((1, shape[1], shape[2]), 5.0, dtype=pd))
    opt = torch.optim.Adam(lr=lr, params=[alpha])
    txt = txt.to(cd)
    g1 = cap = None
    for k in range(steps):
        opt.zero_grad()
        last = k == steps - 1
        with torch.set_grad_enabled(literal or not last):
            if literal:
                xb = _run(sd, tokens(sd, x.expand(copies, -1, -1, -1)).permute(1, 0, 2), 0, layer + 1, heads, cd)
            else:
                xb = x9.expand(1 if last else copies, -1, -1)
            lamb = torch.sigmoid(alpha).expand(xb.shape[0], xb.shape[1], -1)
            mu = xb * lamb
            var = (1 - lamb) ** 2
            cap = -0.5 * (1 + torch.log(var) - mu ** 2 - var)
            if last:
                break
            t = mu + var.sqrt() * noise[k].to(pd)
            y = _run(sd, t, layer + 1, n, heads, cd)
            feats = R._ln(y[:, 0, :], sd, "visual.ln_post").to(cd) @ sd["visual.proj"]
            fit = F.cosine_similarity(txt.expand(copies, -1), feats, eps=1e-6).mean()
            (beta * cap.mean() - fit).backward()
        if k == 0:
            g1 = alpha.grad.detach().clone()
        opt.step()
    cap = cap.detach()
    cap = cap.mean(axis=0) if literal else cap[0]
    sal = torch.nansum(cap, -1)[1:]
    side = int(sal.numel() ** 0.5)
    return {"grid": sal.reshape(side, side), "cap": cap, "alpha": alpha.detach().clone(), "g1": g1}


def full_map(grid):
    """IBAInterpreter.vision_heatmap behind the nansum (iba.py:155-159): the bilinear resize to 224 x 224 and the min-max, in the
    grid's dtype on the CPU.  (The reference's second normalize subtracts 0 and divides by 1 - 0: exact.)"""
    g = torch.as_tensor(grid)
    m = F.interpolate(g.reshape(1, 1, *g.shape), size=MAP, mode="bilinear")[0, 0]
    return (m - m.min()) / (m.max() - m.min())


def argmax_patch(full, model):
    """the patch of the (p, p) grid that holds the 224 x 224 map's argmax pixel"""
    res, patch = MODELS[model][:2]
    p = res // patch
    i, j = divmod(int(np.nanargmax(np.asarray(full))), MAP)
    return (i * p // MAP, j * p // MAP)


# ------------------------------------------------------------------------------------------------ K88-K90 in NumPy
def adam_scalars(k, lr=LR):
    """the header's host-made scalars of step k, formed in double and rounded to fp32 once"""
    b1, b2 = 0.9, 0.999
    return tuple(f32(s) for s in (1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** k), lr / (1 - b1 ** k), 1e-8))


def lam32(alpha):
    """lam = 1 / (1 + expf(-a)) with a correctly rounded exp"""
    with np.errstate(all="ignore"):
        return (f32(1) / (f32(1) + exp32(-np.asarray(alpha, dtype=f32)))).astype(f32)


def gate(alpha, x, lam=None):
    """the header's per-element values; `lam`: the device's in place of the restated one"""
    x = np.asarray(x).astype(f32)
    lam = lam32(alpha) if lam is None else np.asarray(lam, dtype=f32)
    with np.errstate(all="ignore"):
        om = f32(1) - lam
        var = om * om
        return lam, om, var, np.sqrt(var), x * lam, x


def k88(alpha, x9, eps, dt, lam=None):
    """alpha (B, L, D), x9 (B, L, D) of dt, eps (B, R, L, D) -> t (B, R, L, D) of dt"""
    _, _, _, sd, mu, _ = gate(alpha, x9, lam)
    with np.errstate(all="ignore"):
        return (mu[:, None] + sd[:, None] * np.asarray(eps, dtype=f32)).astype(dt)


def k89_gradient(gt, eps, x9, alpha, beta, lam=None):
    lam, om, var, sd, mu, x = gate(alpha, x9, lam)
    gt, eps = np.asarray(gt).astype(f32), np.asarray(eps, dtype=f32)
    L, D = alpha.shape[-2:]
    with np.errstate(all="ignore"):
        lamp = lam * om
        xl = x * lamp
        q = (f32(0.5) / sd) * (om + om)
        ql = q * lamp
        fit = np.zeros_like(lam)
        for r in range(gt.shape[1]):
            fit = fit + gt[:, r] * (xl - ql * eps[:, r])
        gv = f32(-0.5) * (f32(1) / var - f32(1))
        dcap = mu * xl - (gv * (om + om)) * lamp
        return fit + (f32(beta) / f32(L * D)) * dcap


def k89(gt, eps, x9, alpha, m, v, beta, scalars, lam=None):
    """-> (alpha, m, v, g) after the step; the operands are not changed"""
    w1, b2, w2, bc2s, step_size, adam_eps = (f32(s) for s in scalars)
    g = k89_gradient(gt, eps, x9, alpha, beta, lam)
    with np.errstate(all="ignore"):
        m = m + w1 * (g - m)
        v = v * b2 + (w2 * g) * g
        den = np.sqrt(v) / bc2s + adam_eps
        return (np.asarray(alpha, dtype=f32) - step_size * (m / den)).astype(f32), m.astype(f32), v.astype(f32), g


def log32(x):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(x, dtype=np.float64)).astype(f32)


def k90_cap(alpha, x9, lam=None):
    _, _, var, _, mu, _ = gate(alpha, x9, lam)
    with np.errstate(all="ignore"):
        return f32(-0.5) * (((f32(1) + log32(var)) - mu * mu) - var)


def k90_sum(cap):
    """cap (B, L, D) -> (B, L - 1): the header's SUM with a NaN counted as +0"""
    cap = np.asarray(cap, dtype=f32)
    return wave_sum_rows(np.where(np.isnan(cap), f32(0), cap)[:, 1:])


def lam_bound(lam_ref):
    """the header's bound of lam behind expf: 8 u |lam|"""
    return 8 * U * np.abs(np.asarray(lam_ref, dtype=np.float64))


def cap_bound(alpha, x9, lam):
    """the header's bound of cap GIVEN lam: 0.5 * (4 u |lg| + 2 u (|s1| + |s2| + |s3|))"""
    _, _, var, _, mu, _ = gate(alpha, x9, lam)
    with np.errstate(all="ignore"):
        lg = log32(var).astype(np.float64)
        s1 = 1 + lg
        s2 = s1 - mu.astype(np.float64) ** 2
        s3 = s2 - var
        return 0.5 * (4 * U * np.abs(lg) + 2 * U * (np.abs(s1) + np.abs(s2) + np.abs(s3)))
