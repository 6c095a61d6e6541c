"""The relevance pass of Transformer Attribution restated in plain torch, op for op: the specification xai_engine/lrp.py and K46-K52
(include/xai_hip_ext4.h) are held to.

Every function is the closed form of one relprop of the reference (util/attribution_methods/VIT_LRP/util/layers_ours.py,
ViT_LRP_timm.py) with alpha = 1, written with the torch expressions the reference uses, in any floating dtype and on any device.  The
two places where the engine pins an order of summation are restated with order-pinned operations:
  - the three sums of Add.relprop (K50): fp64, in the tree xai_hip_ext4.h states -- sequential adds are np.cumsum(...)[-1], the
    butterfly and the folds are element-wise adds;
  - the head mean and the row sums of the attention matrices (K52) and the vector-matrix chain of K19: sequential element-wise adds.
The GEMMs are torch.matmul with the operands laid out as the engine lays them out, so that on one device the two make the same calls.
"""
import numpy as np
import torch

from xai_engine.lrp import blocks_needed, needs_gradients, record, split_heads

ADD_CHUNK, ADD_LANES, WAVE, ROLL_WAVES = 4096, 256, 64, 16


def safe_divide(a, b):
    """layers_ours.py:10-13"""
    den = b.clamp(min=1e-9) + b.clamp(max=1e-9)
    den = den + den.eq(0).to(den.dtype) * 1e-9
    return a / den * b.ne(0).to(b.dtype)


# ------------------------------------------------------------------------------------------------ K46 - K49, K51
def split(x):
    return torch.clamp(x, min=0), torch.clamp(x, max=0)


def ratio(r, z1, z2=None):
    return safe_divide(r, z1 if z2 is None else z1 + z2)


def gather(x, g1, g2):
    return torch.clamp(x, min=0) * g1 + torch.clamp(x, max=0) * g2


def half_product(x, c):
    out = x * c
    out /= 2
    return out


def half_product_slot(x, c, out, slot):
    """x, c (B, h, N, d) into the slot's third of out (B, N, 3 * h * d): 'qkv b h n d -> b n (qkv h d)'"""
    B, h, N, d = x.shape
    out.view(B, N, 3, h, d)[:, :, slot] = half_product(x, c).permute(0, 2, 1, 3)
    return out


def clone(x, r1, r2):
    return x * (safe_divide(r1, x) + safe_divide(r2, x))


# ------------------------------------------------------------------------------------------------ K50
def _butterfly(v):
    """xor butterfly over the last axis (64 lanes): a + b at both partners"""
    idx = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    return v


def pinned_sum(values):
    """The fp64 sum of a flat array of one image in K50's tree -> numpy float64."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    P = -(-v.size // ADD_CHUNK)
    v = np.concatenate([v, np.zeros(P * ADD_CHUNK - v.size)])           # a lane adds only elements that exist; + (+0.0) changes nothing
    quads = ADD_CHUNK // (ADD_LANES * 4)
    lanes = v.reshape(P, quads, ADD_LANES, 4).transpose(0, 2, 1, 3).reshape(P, ADD_LANES, quads * 4)
    lanes = np.concatenate([np.zeros((P, ADD_LANES, 1)), lanes], axis=2)  # starting from +0.0
    lane = np.cumsum(lanes, axis=2)[:, :, -1]                            # ascending i, sequential
    waves = _butterfly(lane.reshape(P, ADD_LANES // WAVE, WAVE))[:, :, 0]
    part = np.zeros(P)
    for w in range(ADD_LANES // WAVE):
        part = part + waves[:, w]
    return np.cumsum(np.concatenate([[0.0], part]))[-1]                  # the chunks in ascending order, from +0.0


def add(x0, x1, R):
    """Add.relprop (layers_ours.py:106-125) per image of (B, ...), with a.sum(), b.sum(), R.sum() as pinned fp64 sums rounded once."""
    s = safe_divide(R, x0 + x1)
    a, b = x0 * s, x1 * s
    outs_a, outs_b = [], []
    for i in range(R.shape[0]):
        a_sum, b_sum, r_sum = (torch.tensor(pinned_sum(t[i].detach().cpu().numpy()), dtype=R.dtype, device=R.device) for t in (a, b, R))
        a_fact = safe_divide(a_sum.abs(), a_sum.abs() + b_sum.abs()) * r_sum
        b_fact = safe_divide(b_sum.abs(), a_sum.abs() + b_sum.abs()) * r_sum
        outs_a.append(a[i] * safe_divide(a_fact, a_sum))
        outs_b.append(b[i] * safe_divide(b_fact, b_sum))
    return torch.stack(outs_a), torch.stack(outs_b)


# ------------------------------------------------------------------------------------------------ K52, K19
def head_mean(cam, grad=None):
    """cam, grad (..., h, S, S) -> (..., S, S): clamp(grad * cam, min=0), the heads added in ascending order from +0, divided by h"""
    t = cam if grad is None else grad * cam
    t = t.clamp(min=0)
    s = torch.zeros_like(t[..., 0, :, :])
    for hh in range(t.shape[-3]):
        s = s + t[..., hh, :, :]
    # a true division: by a Python number torch multiplies with the rounded reciprocal on the device
    return s / torch.tensor(float(t.shape[-3]), dtype=s.dtype, device=s.device)


def row_sum(m):
    """the sum over the last axis in K52's tree: lane t adds its columns t, t + 64, ... ascending from +0, then the xor butterfly"""
    S = m.shape[-1]
    lanes = torch.zeros(m.shape[:-1] + (WAVE,), dtype=m.dtype, device=m.device)
    for j0 in range(0, S, WAVE):
        n = min(WAVE, S - j0)
        lanes[..., :n] = lanes[..., :n] + m[..., j0:j0 + n]
    idx = torch.arange(WAVE, device=m.device)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ off]
    return lanes[..., :1]


def attn_matrices(cams, grads, mode):
    """cams, grads (L, B, h, S, S) -> mode 0: (B, L, S, S) head means; 1: plus the identity, rows divided by their sums; 2: (B, L, S)"""
    m = head_mean(cams, grads).transpose(0, 1)
    if mode == 2:
        return m[:, :, 0, :]
    if mode == 1:
        m = m + torch.eye(m.shape[-1], dtype=m.dtype, device=m.device)
        m = m / row_sum(m)
    return m


def rollout_row(aug, t):
    """K19: aug (n, L, S, S) -> row t of aug[L-1] ... aug[0] as vector-matrix products: 16 waves share the k axis in chunks of
    ceil(S / 16), each adds its products in ascending k from +0, the 16 partial rows are added in ascending order from +0"""
    n, L, S, _ = aug.shape
    v = aug[:, L - 1, t, :]
    kc = -(-S // ROLL_WAVES)
    for l in range(L - 2, -1, -1):
        M = aug[:, l]
        total = torch.zeros_like(v)
        for w in range(ROLL_WAVES):
            part = torch.zeros_like(v)
            for k in range(w * kc, min(S, w * kc + kc)):
                part = part + v[:, k:k + 1] * M[:, k, :]
            total = total + part
        v = total
    return v


# ------------------------------------------------------------------------------------------------ the pass
def linear(R, X, W):
    """Linear.relprop with alpha = 1 (layers_ours.py:213-236): the activator term; autograd.grad(Z1, x1, S1) is S1 @ w1"""
    wp, wn = split(W)
    px, nx = split(X)
    s = ratio(R, torch.matmul(px, wp.t()), torch.matmul(nx, wn.t()))
    return gather(X, torch.matmul(s, wp), torch.matmul(s, wn))


def relevance_pass(model, tape, tgt, attns, need):
    """-> {block: attn_cam (B, h, S, S)} of the blocks in `need`; walks from the head down to the attention of block need[0]"""
    blocks = list(model.blocks)
    heads = attns[0].shape[1]
    B = attns[0].shape[0]
    cams = {}
    one_hot = torch.zeros_like(tape.logits).scatter_(1, tgt.view(-1, 1), 1.0)
    cam = linear(one_hot, tape.top["head_in"].contiguous(), model.head.weight.detach())
    x0 = tape.top["norm_out"][:, 0]
    R = torch.zeros_like(tape.top["norm_out"])
    R[:, 0] = x0 * safe_divide(cam, x0)
    for i in range(len(blocks) - 1, need[0] - 1, -1):
        blk, rec = blocks[i], tape.blocks[i]
        cam1, cam2 = add(rec["x_mid"], rec["mlp_out"], R)
        cam2 = linear(cam2, rec["g"].contiguous(), blk.mlp.fc2.weight.detach())
        cam2 = linear(cam2, rec["n2"].contiguous(), blk.mlp.fc1.weight.detach())
        R = clone(rec["x_mid"], cam1, cam2)
        cam1, cam2 = add(rec["x_in"], rec["attn_out"], R)
        c = linear(cam2, rec["pv"].contiguous(), blk.attn.proj.weight.detach())
        N, D = c.shape[1], c.shape[2]
        c = c.reshape(B, N, heads, D // heads).permute(0, 2, 1, 3).contiguous()
        q, k, v = split_heads(rec["qkv"], heads)
        A = attns[i].contiguous()
        s = ratio(c, torch.matmul(A, v))
        camA = half_product(A, torch.matmul(s, v.transpose(-1, -2)))
        if i in need:
            cams[i] = camA
        if i == need[0]:
            break
        cam_qkv = torch.empty((B, N, 3 * D), dtype=c.dtype, device=c.device)
        half_product_slot(v, torch.matmul(A.transpose(-1, -2), s), cam_qkv, 2)
        s = ratio(camA, torch.matmul(q, k.transpose(-1, -2)))
        half_product_slot(q, torch.matmul(s, k), cam_qkv, 0)
        half_product_slot(k, torch.matmul(s.transpose(-1, -2), q), cam_qkv, 1)
        cam2 = linear(cam_qkv, rec["n1"].contiguous(), blk.attn.qkv.weight.detach())
        R = clone(rec["x_in"], cam1, cam2)
    return cams


def generate(model, x, targets=None, method="transformer_attribution", is_ablation=False, start_layer=0, withgrad=True):
    """x (B, C, H, W) in the model's dtype and on its device, targets (B,) int64 or None (argmax) -> ((B, p, p), {block: attn_cam})"""
    depth = len(model.blocks)
    need = blocks_needed(method, depth, start_layer)
    gradients = needs_gradients(method, withgrad, is_ablation)
    tape, tgt, attns, grads = record(model, x, targets, gradients)
    B, h, S, _ = attns[0].shape
    cams = {}
    if method == "last_layer_attn":
        cam = 0
        for i in range(start_layer, depth):
            cam = cam + attns[i][:, :, 0, :]
        row = cam.clamp(min=0).mean(dim=1)
    else:
        cams = relevance_pass(model, tape, tgt, attns, need)
        stack = torch.stack([cams[i] for i in need])
        g = torch.stack([grads[i] for i in need]) if gradients else None
        if method in ("last_layer", "second_layer"):
            row = attn_matrices(stack, g, 2)[:, 0]
        else:
            row = rollout_row(attn_matrices(stack, g, 1), 0)
    side = int(np.sqrt(S - 1))
    return row[:, 1:].reshape(B, side, side), cams


# ------------------------------------------------------------------------------------------------ the fixtures of tests/golden/lrp.npz
FIXTURES = {"mini": "lrp.npz", "v16": "lrp_w224_16.npz", "v32": "lrp_w224_32.npz"}
IMAGES = 3
# key -> keyword arguments of generate_LRP (tests/golden/make_golden_lrp.py: CALLS)
CALLS = {"transformer_attribution": dict(method="transformer_attribution"),
         "grad": dict(method="grad"),
         "rollout": dict(method="rollout"),
         "last_layer": dict(method="last_layer"),
         "second_layer": dict(method="second_layer"),
         "last_layer_attn": dict(method="last_layer_attn"),
         "t_attr_nograd": dict(method="transformer_attribution", withgrad=False),
         "t_attr_start1": dict(method="transformer_attribution", start_layer=1),
         "rollout_start1": dict(method="rollout", start_layer=1),
         "last_layer_ablation": dict(method="last_layer", is_ablation=True),
         "second_layer_ablation": dict(method="second_layer", is_ablation=True)}


def fixture_input(x_seed, img):
    """make_golden_lrp.py's input recipe (the generator stores the input's sum, which `load_fixture` checks)"""
    g = torch.Generator().manual_seed(x_seed)
    return (torch.randint(0, 256, (1, 3, img, img), generator=g).float() / 255 - 0.5) / 0.25


def load_fixture(name, golden_dir):
    """-> (the engine's ViT with the fixture's weights, on the CPU; x (3, 3, img, img); targets (3,) int64; lrp.npz)"""
    import os
    from xai_engine import zoo
    g = np.load(os.path.join(golden_dir, "lrp.npz"), allow_pickle=False)
    if name == "mini":
        w = {k[len("mini/w_"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("mini/w_")}
    else:
        f = np.load(os.path.join(golden_dir, FIXTURES[name]), allow_pickle=False)
        w = {k[len("w_"):]: torch.from_numpy(f[k]) for k in f.files}
    img, patch, dim, depth, heads, classes = (int(v) for v in g[f"{name}/cfg"])
    model = zoo.VisionTransformer(img, patch, dim, depth, heads, classes).eval()
    model.load_state_dict(w)
    for p in model.parameters():
        p.requires_grad_(False)
    xs = [fixture_input(int(g[f"{name}/{j}/x_seed"]), img) for j in range(IMAGES)]
    for j, x in enumerate(xs):
        assert float(x.double().sum()) == float(g[f"{name}/{j}/x_sum"]), "torch's randint no longer makes the fixture's input"
    targets = torch.tensor([int(g[f"{name}/{j}/target"]) for j in range(IMAGES)])
    return model, torch.cat(xs), targets, g


def bound(gap):
    """Two valid fp32 evaluations each lie within the gap of the fp64 result, so at most twice that apart; the second factor of 2
    covers a GEMM summation order other than the reference's CPU one.  1e-5 is the project's bar."""
    return max(1e-5, 4.0 * float(gap))


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())
