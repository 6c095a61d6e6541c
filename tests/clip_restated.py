"""Restatements for the Grad-ECLIP rows of CLIP (xai_engine/eclip.py, include/xai_clip.h), independent of the engine:

  * the reference's full-row flow (generate_emap.py: clip_encode_dense :309-376, grad_eclip :453-485, mask_clip :500-529 and the five
    rows of get_CLIP_attr, evaluatePerturbation.py:398-424) as functions of a state dict, parametrised by dtype: `None` keeps the
    stored mixed precision (half GEMM weights, fp32 LayerNorms computing in fp32), a torch dtype casts every weight to it;
  * the one-row flow the engine runs instead (the class-token row only), for the identity test;
  * K75-K77 in NumPy, in the accumulation orders and at the rounding points the header states.
"""
import numpy as np
import torch
import torch.nn.functional as F

ROWS = ("eclip", "eclip_wo", "eclip_nograd", "maskclip", "selfattn")
MODELS = {"mini": (32, 8, 64, 2, 16), "short": (32, 16, 128, 1, 16), "long": (224, 16, 64, 1, 16), "b32": (224, 32, 64, 1, 16)}
TEXT = dict(context_length=4, vocab_size=8, transformer_width=16, transformer_heads=1, transformer_layers=1)


def fixture_image(x_seed, h, w):
    """the fixtures' images: 8-bit noise in [0, 1], (3, h, w) fp32"""
    g = torch.Generator().manual_seed(x_seed)
    return (torch.randint(0, 256, (1, 3, h, w), generator=g).float() / 255)[0]


def fixture_input(x_seed, h, w):
    """the fixtures' inputs: the image CLIP-normalised, (1, 3, h, w) fp32"""
    x = fixture_image(x_seed, h, w)[None]
    mean = torch.tensor((0.48145466, 0.4578275, 0.40821073)).view(1, 3, 1, 1)
    std = torch.tensor((0.26862954, 0.26130258, 0.27577711)).view(1, 3, 1, 1)
    return (x - mean) / std


def fixture_texts(t_seed, n, embed):
    """n normalised text embeddings, (n, embed) fp32 (the harness normalises a row of its embedding table)"""
    g = torch.Generator().manual_seed(t_seed)
    return F.normalize(torch.randn(n, embed, generator=g), dim=-1)


def cast(sd, dtype):
    return dict(sd) if dtype is None else {k: v.to(dtype) for k, v in sd.items()}


def _ln(x, sd, name):
    c = torch.float32 if x.dtype == torch.float16 else x.dtype
    return F.layer_norm(x.to(c), (x.shape[-1],), sd[name + ".weight"].to(c), sd[name + ".bias"].to(c), 1e-5).to(x.dtype)


def _mlp(x, sd, pre):
    h = F.linear(x, sd[pre + "mlp.c_fc.weight"], sd[pre + "mlp.c_fc.bias"])
    return F.linear(h * torch.sigmoid(1.702 * h), sd[pre + "mlp.c_proj.weight"], sd[pre + "mlp.c_proj.bias"])


def _attention(q, k, v, heads):
    L, N, D = q.shape
    hd = D // heads
    q = q * (float(hd) ** -0.5)
    q, k, v = (t.contiguous().view(-1, N * heads, hd).transpose(0, 1) for t in (q, k, v))
    w = F.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    out = torch.bmm(w, v).transpose(0, 1).contiguous().view(L, N, D)
    return out, w.view(N, heads, L, -1).sum(dim=1) / heads


def _block(x, sd, pre, heads):
    q, k, v = F.linear(_ln(x, sd, pre + "ln_1"), sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]).chunk(3, dim=-1)
    x = x + F.linear(_attention(q, k, v, heads)[0], sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"])
    return x + _mlp(_ln(x, sd, pre + "ln_2"), sd, pre)


def _layers(sd):
    return 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("visual.transformer.resblocks."))


def tokens_before_last_block(sd, x, resolution):
    """-> (x_in (L, N, D), (h, w))"""
    w = sd["visual.conv1.weight"]
    x = F.conv2d(x.to(w.dtype), w, stride=w.shape[-1])
    grid = tuple(x.shape[-2:])
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    x = torch.cat([sd["visual.class_embedding"].to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1]).to(x), x], dim=1)
    pos = sd["visual.positional_embedding"].to(x.dtype)
    side = resolution // w.shape[-1]
    img_pos = pos[1:].reshape(1, side, side, -1).permute(0, 3, 1, 2)
    img_pos = F.interpolate(img_pos, size=grid, mode="bicubic", align_corners=False)
    img_pos = img_pos.reshape(1, img_pos.shape[1], -1).permute(0, 2, 1)
    x = _ln(x + torch.cat((pos[None, :1], img_pos), dim=1), sd, "visual.ln_pre").permute(1, 0, 2)
    heads = max(1, x.shape[-1] // 64)
    for i in range(_layers(sd) - 1):
        x = _block(x, sd, f"visual.transformer.resblocks.{i}.", heads)
    return x, grid


def encode_dense(sd, x, resolution, dtype=None):
    """The reference's 9-tuple from the state dict `sd` (as stored for dtype None, else cast to `dtype`)"""
    sd = cast(sd, dtype)
    x_in, grid = tokens_before_last_block(sd, x, resolution)
    pre = f"visual.transformer.resblocks.{_layers(sd) - 1}."
    ow, ob = sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"]
    q, k, v = F.linear(_ln(x_in, sd, pre + "ln_1"), sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]).chunk(3, dim=-1)
    att_output, attn = _attention(q, k, v, 1)
    att_output.requires_grad_(True)

    def tail(t):
        t = t + x_in
        t = t + _mlp(_ln(t, sd, pre + "ln_2"), sd, pre)
        return _ln(t.permute(1, 0, 2), sd, "visual.ln_post") @ sd["visual.proj"]
    outputs = tail(F.linear(att_output, ow, ob))
    with torch.no_grad():
        qkv = F.linear(torch.stack((q, k, v), dim=0), ow, ob)
        v_final = tail(qkv[2])
    return outputs, v_final[:, 1:], x_in, v, qkv[0], qkv[1], attn, att_output, grid


def _cos_norm(first, k_out):
    c = (F.normalize(first, dim=-1) * F.normalize(k_out[1:, 0, :], dim=-1)).sum(-1)
    return c


def grad_eclip(c, q_out, k_out, v, att_output, map_size, withksim=True, withgrad=True):
    t = v[1:, 0, :]
    if withgrad:
        t = torch.autograd.grad(c, att_output, retain_graph=True)[0].detach()[:1, 0, :] * t
    if withksim:
        cos = _cos_norm(q_out[:1, 0, :], k_out)
        t = t * ((cos - cos.min()) / (cos.max() - cos.min()))[:, None]
    return F.relu_(t.detach().sum(-1)).reshape(*map_size)


def mask_clip(txt_feats, v_final, k_out, map_size):
    cosine_v = (F.normalize(v_final, dim=-1) @ txt_feats)[0].transpose(1, 0)
    return (cosine_v * _cos_norm(k_out[:1, 0, :], k_out)[None, :]).detach().reshape(-1, *map_size)


def rows_from_tuple(tup, txt, grad_eclip=grad_eclip, mask_clip=mask_clip):
    """The five rows of get_CLIP_attr (evaluatePerturbation.py:398-424) from a 9-tuple and normalised texts (T, E) in its dtype ->
    {row: (h, w) map}, and the cosine minima and maxima (for the fixtures' degeneracy rule)"""
    outputs, v_final, _x_in, v, q_out, k_out, attn, att_output, size = tup
    cosines = (F.normalize(outputs[:, 0], dim=-1) @ txt.T)[0]
    out = {}
    for row, kw in (("eclip", {}), ("eclip_wo", dict(withksim=False)), ("eclip_nograd", dict(withgrad=False))):
        out[row] = torch.stack([grad_eclip(c, q_out, k_out, v, att_output, size, **kw) for c in cosines], dim=0).sum(0)
    out["maskclip"] = mask_clip(txt.T, v_final, k_out, size).sum(0)
    out["selfattn"] = attn[0, :1, 1:].detach().reshape(*size)
    return out


def one_row(sd, x, resolution, txt, dtype=torch.float64):
    """The class-token row alone, as xai_engine.eclip.cls_pass computes it -> (outputs0 (E,), grad_cls (T, D), attn0 (L,),
    att_output0 (D,)): one query, the tail on one row, a one-row backward"""
    sd = cast(sd, dtype)
    x_in, _ = tokens_before_last_block(sd, x, resolution)
    D = x_in.shape[-1]
    pre = f"visual.transformer.resblocks.{_layers(sd) - 1}."
    iw, ib = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    y = _ln(x_in, sd, pre + "ln_1")[:, 0]
    kv = F.linear(y, iw[D:], ib[D:])
    k, v = kv[:, :D], kv[:, D:]
    q0 = F.linear(y[:1], iw[:D], ib[:D]) * (float(D) ** -0.5)
    p = F.softmax(q0 @ k.T, dim=-1)
    att0 = (p @ v).detach().requires_grad_(True)
    t = F.linear(att0, sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"]) + x_in[0, 0]
    t = t + _mlp(_ln(t, sd, pre + "ln_2"), sd, pre)
    out0 = _ln(t, sd, "visual.ln_post") @ sd["visual.proj"]
    cosines = (F.normalize(out0, dim=-1) @ txt.to(out0.dtype).T)[0]
    grads = torch.stack([torch.autograd.grad(c, att0, retain_graph=True)[0][0] for c in cosines])
    return out0[0].detach(), grads, p[0].detach(), att0[0].detach()


# ------------------------------------------------------------------------------------------------ K75-K77 in NumPy
f32 = np.float32


def rT(x, dt):
    """the header's rounding to the operand dtype, back in fp32"""
    return np.asarray(x, dtype=f32).astype(dt).astype(f32)


def wave_sum_rows(terms):
    """the header's SUM over the last axis of `terms` (..., n) fp32: lane partials in ascending i, then the xor butterfly"""
    terms = np.asarray(terms, dtype=f32)
    n = terms.shape[-1]
    pad = (-n) % 64
    if pad:
        terms = np.concatenate([terms, np.zeros(terms.shape[:-1] + (pad,), dtype=f32)], axis=-1)
    terms = terms.reshape(terms.shape[:-1] + (-1, 64))
    lanes = np.zeros(terms.shape[:-2] + (64,), dtype=f32)
    for i in range(terms.shape[-2]):
        lanes = lanes + terms[..., i, :]
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ off]
    return lanes[..., 0]


def denominator(rows, dt):
    with np.errstate(all="ignore"):
        n = rT(np.sqrt(wave_sum_rows(rows * rows)), dt)
        e = rT(f32(1e-12), dt)
        return np.where(n < e, e, n)


def normalize_rows(rows, dt):
    with np.errstate(all="ignore"):
        return rT(rows / denominator(rows, dt)[..., None], dt)


def k75_scores(q0, k, dt):
    """q0 (B, D), k (L, B, D) as fp32 values of dtype dt -> (round(q * scaling) (B, D), scores (B, L)): all that precedes the exp"""
    D = q0.shape[1]
    with np.errstate(all="ignore"):
        qs = rT(q0 * f32(float(D) ** -0.5), dt)
        return qs, rT(wave_sum_rows(qs[None] * k), dt).T


def k75(q0, k, v, dt):
    """-> (qs, scores, attn (B, L), att_out (B, D)) in the header's orders, NumPy's exp standing in for the device's"""
    L, B, D = k.shape
    qs, s = k75_scores(q0, k, dt)
    with np.errstate(all="ignore"):                                          # a NaN or an infinite score is a case, not a warning
        e = np.exp(s - s.max(axis=1, keepdims=True)).astype(f32)             # NumPy's max returns a NaN that is there, as torch's
    pad = (-L) % 1024
    ep = np.concatenate([e, np.zeros((B, pad), dtype=f32)], axis=1).reshape(B, -1, 1024)
    lanes = np.zeros((B, 1024), dtype=f32)
    for i in range(ep.shape[1]):
        lanes = lanes + ep[:, i]
    waves = wave_sum_rows(lanes.reshape(B, 16, 64))
    total = np.zeros(B, dtype=f32)
    for w in range(16):
        total = total + waves[:, w]
    with np.errstate(all="ignore"):
        p = rT(e / total[:, None], dt)
        acc = np.zeros((B, D), dtype=f32)
        for j in range(L):
            acc = acc + p[:, j, None] * v[j]
        return qs, s, p, rT(acc, dt)


def k76(q_out0, k_out, v, grad_cls, T, withksim, withgrad, dt):
    """-> (out (B, L - 1) fp32, the cosines before the min-max (B, L - 1) or None)"""
    L, B, D = v.shape
    cos = w = None
    with np.errstate(all="ignore"):
        if withksim:
            qn = normalize_rows(q_out0, dt)                                  # (B, D)
            kn = normalize_rows(k_out[1:], dt)                               # (L - 1, B, D)
            cos = rT(wave_sum_rows(rT(qn[None] * kn, dt)), dt).T            # (B, L - 1)
            lo, hi = cos.min(axis=1, keepdims=True), cos.max(axis=1, keepdims=True)   # NumPy's min and max return a NaN that is there
            w = rT(rT(cos - lo, dt) / rT(hi - lo, dt), dt)
        acc = np.zeros((B, L - 1), dtype=f32)
        vp = np.transpose(v[1:], (1, 0, 2))                                  # (B, L - 1, D)
        for t in range(T):
            if withgrad:
                terms = rT(grad_cls[:, t, None, :] * vp, dt)
                if withksim:
                    terms = rT(terms * w[..., None], dt)
            else:
                terms = rT(vp * w[..., None], dt) if withksim else vp
            s = rT(wave_sum_rows(terms), dt)
            acc = acc + np.where(s > 0, s, np.where(np.isnan(s), s, f32(0)))
        return rT(acc, dt), cos


def k77(v_final, txt, k_out, dt):
    """v_final (B, L - 1, E), txt (B, T, E), k_out (L, B, D) -> out (B, L - 1) fp32"""
    B, n, E = v_final.shape
    with np.errstate(all="ignore"):
        k0 = normalize_rows(k_out[0], dt)
        kn = normalize_rows(k_out[1:], dt)
        c = rT(wave_sum_rows(rT(k0[None] * kn, dt)), dt).T                  # (B, L - 1)
        fn = normalize_rows(v_final, dt)
        acc = np.zeros((B, n), dtype=f32)
        for t in range(txt.shape[1]):
            a = rT(wave_sum_rows(fn * txt[:, t, None, :]), dt)
            acc = acc + rT(a * c, dt)
        return rT(acc, dt)


# ------------------------------------------------------------------------------------------------ comparisons the GPU tests share
U = 2.0 ** -24


def spacing(x, dt):
    """distance between neighbouring values of dtype dt at |x| (its least subnormal spacing below the normal range)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    bits, emin = (10, -14) if dt == np.float16 else (23, -126)
    e = np.floor(np.log2(np.maximum(x, 2.0 ** emin)))
    return 2.0 ** (e - bits)


def same(got, want):
    """bit for bit, a NaN by position"""
    got, want = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(gn, wn) and got[~gn].tobytes() == want[~wn].tobytes()


def k75_bound(p, p_ref, o, o_ref, v, dt, subnormal=0.0):
    """The header's bound behind K75's first exp for attn p (B, L) and att_out o (B, D), all fp64, v (L, B, D) -> (dp, do):
         dp_j = (10 + 2n) u |p_ref_j| + spacing_T(max(|p_j|, |p_ref_j|)),  n = ceil(L / 1024) + 22  (no spacing term for fp32, where
                `subnormal` is added instead: the absolute error of two expf results below 2^-126 and of the quotient's rounding)
         do_d = sum_j dp_j |v_jd| + 2 L u sum_j |p_ref_j v_jd| + spacing_T(max(|o_d|, |o_ref_d|))"""
    L = v.shape[0]
    n = -(-L // 1024) + 22
    half = dt == np.float16
    with np.errstate(all="ignore"):
        dp = (10 + 2 * n) * U * np.abs(p_ref) + (spacing(np.maximum(np.abs(p), np.abs(p_ref)), dt) if half else subnormal)
        absv = np.abs(v.astype(np.float64))
        do = np.einsum("bj,jbd->bd", dp, absv) + 2 * L * U * np.einsum("bj,jbd->bd", np.abs(p_ref.astype(np.float64)), absv) \
            + (spacing(np.maximum(np.abs(o), np.abs(o_ref)), dt) if half else 0.0)
    return dp, do


def merge_ledger(path, entries, **meta):
    """Write {name, measured, bound} records into the JSON ledger at `path`, replacing those of the same name and keeping the rest
    (two test files share one ledger, and a run of a few tests leaves the others' records alone)"""
    import json
    import os
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    rows = {r["name"]: r for r in old.get("comparisons", [])}
    rows.update({r["name"]: r for r in entries})
    old.update(meta)
    old["comparisons"] = [rows[k] for k in sorted(rows)]
    with open(path, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")


# ------------------------------------------------------------------------------------------------ the edges of K75-K77
# (L, D, B), each the smallest shape that reaches its edge of csrc/clip/clip_kernels.hip
EDGES = {
    "the lane loop of row_sum": [(2, 1, 1), (2, 63, 2), (3, 64, 1), (3, 65, 2), (18, 70, 1)],
    "wave rounds over rows (16 waves)": [(16, 64, 1), (17, 64, 2), (18, 64, 1), (33, 5, 1)],
    "workgroup strides over L (BLOCKSUM depth n = 23, 24, 25)": [(1023, 8, 1), (1024, 8, 1), (1025, 8, 2), (1026, 8, 1), (2049, 4, 1)],
    "workgroup strides over D": [(5, 1023, 1), (5, 1024, 1), (3, 1025, 2), (3, 2049, 1)],
    "the shipped models (ViT-B/16, ViT-B/32, ViT-L/14)": [(197, 768, 2), (50, 768, 1), (257, 1024, 1)],
    "many workgroups": [(3, 7, 70)],
}
EDGE_SHAPES = [s for shapes in EDGES.values() for s in shapes]


def edge_operands(L, D, B, dt, E=None, T=3, names=("q0", "k", "v", "q_out0", "k_out", "grad", "v_final", "txt")):
    """The operands `names` of K75-K77 at (L, D, B), E = D // 2 + 1 unless given: seeded randn cast to dt, as fp32 values of dt"""
    E = D // 2 + 1 if E is None else E
    shapes = dict(q0=(B, D), k=(L, B, D), v=(L, B, D), q_out0=(B, D), k_out=(L, B, D), grad=(B, T, D), v_final=(B, L - 1, E), txt=(B, T, E))
    tdt = torch.float16 if dt == np.float16 else torch.float32
    return {n: torch.randn(shapes[n], generator=torch.Generator().manual_seed(100 + i)).to(tdt).float().numpy()
            for i, n in enumerate(shapes) if n in names}


def tiny_rows(rows, dt):
    """`rows` scaled so that their norm is below the clamp 1e-12 (float; the sum of squares stays a normal number) or inside the
    subnormal range of half (where the clamp rT(1e-12) is 0 and the norm itself is the denominator)"""
    if dt == np.float16:
        out = rT(rows * f32(2.0 ** -20), dt)
        norm = np.sqrt((out.astype(np.float64) ** 2).sum(-1))
        assert (norm > 0).all() and (norm < 2.0 ** -14).all()
        return out
    out = rows * f32(1e-15)
    sumsq = (out.astype(np.float64) ** 2).sum(-1)
    assert (np.sqrt(sumsq) < 1e-12).all() and (sumsq > 2.0 ** -100).all()
    return out
