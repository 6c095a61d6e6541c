"""The host plumbing the CLIP row modules share (eclip.py, clip_attn.py, surgery.py, m2ib.py): what they check of a model, an input
and its texts, the visual tower's tokens, its attention block written out, the per-image loop in front of a row's own part, and the
epilogue of a map.  Plain torch on whatever device the model is on; the only kernel reached from here is the harness's bilinear
resize in `finish`.

Every image of a batch gets the bytes of its own one-image call: a GEMM's summation order depends on its extents, so `per_image`
runs the tokens and the blocks image by image, and the kernels, which give every image its own workgroup, take the batch -- the
rule of xai_engine/lrp.py.  Eager only: nothing here is captured into a hipGraph.

Two token functions, because the reference has two: `interpolated_tokens` follows clip_encode_dense (generate_emap.py:316-338),
which interpolates the positional embedding to the conv grid and expands the class token; `native_tokens` follows visual.forward
(model.py:229-237), which adds the embedding as it is and adds the class token to zeros.  They are not the same arithmetic.
`written_out_block` is nn.MultiheadAttention's sequence, q * scale first; the original path of CLIP Surgery's dual blocks scales
(q @ k^T) and stays in surgery.py.
"""
import torch
import torch.nn.functional as F

from . import kernels as K
from .ig import hip_device

VISUAL = ("conv1", "class_embedding", "positional_embedding", "ln_pre", "transformer", "ln_post", "proj", "input_resolution",
          "transformer.width", "transformer.resblocks")
BLOCK = ("ln_1", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj", "ln_2", "mlp")
# the rows that refuse a ResNet visual tower by name, and why; the others report its missing `visual.transformer`
_NO_RESNET = {"surgery": "the reference's harness builds CS-ViT-B/16 and CS-ViT-B/32 only",
              "m2ib": "the reference's wrapper reads visual.transformer.resblocks"}


# ---------------------------------------------------------------------------------- checks
def check_layout(clipmodel, row, every_block=False, heads=False):
    """The attributes a row reads (OpenAI's names), or a TypeError naming the one that is missing: the visual tower and its last
    block, or every block; heads: `attn.num_heads` too, which has to divide the width.  -> (visual, blocks, H), H None without heads"""
    def missing(path):
        return TypeError(f"{row} needs a CLIP of OpenAI's layout: {type(clipmodel).__name__} has no `{path}`")

    def need(obj, path, where=""):
        for name in path.split("."):
            if not hasattr(obj, name):
                raise missing(where + path)
            obj = getattr(obj, name)
        return obj
    visual = need(clipmodel, "visual")
    if row in _NO_RESNET and not hasattr(visual, "transformer") and hasattr(visual, "attnpool"):
        raise NotImplementedError(f"{row}: a ResNet visual tower (AttentionPool2d) is not served; {_NO_RESNET[row]}")
    for path in VISUAL:
        need(visual, path, "visual.")
    blocks = list(visual.transformer.resblocks)
    if not blocks:
        raise missing("visual.transformer.resblocks[-1]")
    paths = BLOCK + ("attn.num_heads",) if heads else BLOCK
    for i, blk in [(-1, blocks[-1])] + (list(enumerate(blocks[:-1])) if every_block else []):
        for path in paths:
            need(blk, path, f"visual.transformer.resblocks[{i}].")
    if not heads:
        return visual, blocks, None
    H, D = int(blocks[-1].attn.num_heads), int(visual.transformer.width)
    if H < 1 or D % H:
        raise TypeError(f"{row}: attn.num_heads = {H} does not divide the width {D}")
    return visual, blocks, H


def tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    return t


def native_input(visual, x, row):
    """x must be (B, 3, R, R), R the model's input_resolution, for the rows that take the reference's preprocess(img) -> (R, grid)"""
    tensor(x, "x")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"x must be (B, 3, H, W), got {tuple(x.shape)}")
    res = int(visual.input_resolution)
    if tuple(x.shape[2:]) != (res, res):
        raise NotImplementedError(f"{row}: x is {x.shape[2]} x {x.shape[3]}, the model's input_resolution is {res}: the row takes the "
                                  "reference's preprocess(img), whose tower adds the positional embedding without interpolating it; "
                                  "PIL's bicubic resize is not built")
    ksize = visual.conv1.kernel_size
    return res, (res // ksize[0], res // ksize[1])


def embeds_into(t, E, name):
    if t.shape[-1] != E:
        raise ValueError(f"{name} has {t.shape[-1]} features, the model embeds into {E}")
    return t


def texts(t, B, E, name):
    """Text features (T, E), shared by the images, or (B, T, E), T >= 1, as they came; E None: a row that reads no feature"""
    tensor(t, name)
    if t.dim() not in (2, 3) or t.numel() == 0 or (t.dim() == 3 and t.shape[0] != B):
        raise ValueError(f"{name} must be (T, E) or ({B}, T, E) with T >= 1, got {tuple(t.shape)}")
    return t if E is None else embeds_into(t, E, name)


# ---------------------------------------------------------------------------------- the tower
def interpolated_tokens(visual, x):
    """x (N, 3, H, W) -> the (L, N, D) input of the first block and the conv grid (generate_emap.py:316-338): patch embedding, class
    token, the positional embedding through the reference's bicubic interpolation to the grid (an identity at the native size), ln_pre"""
    x = visual.conv1(x.to(visual.conv1.weight.dtype))
    grid = tuple(x.shape[-2:])
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((visual.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1), x), dim=1)
    pos = visual.positional_embedding.to(x.dtype)
    ksize = visual.conv1.kernel_size
    ph, pw = visual.input_resolution // ksize[0], visual.input_resolution // ksize[1]
    if pos.shape[0] != ph * pw + 1:
        raise ValueError(f"visual.positional_embedding has {pos.shape[0]} rows, input_resolution and the patch size give {ph * pw + 1}")
    img_pos = F.interpolate(pos[1:].reshape(1, ph, pw, -1).permute(0, 3, 1, 2), size=grid, mode="bicubic", align_corners=False)
    pos = torch.cat((pos[:1], img_pos.flatten(2)[0].t()), dim=0)
    return visual.ln_pre(x + pos).transpose(0, 1), grid


def native_tokens(visual, x):
    """x (N, 3, R, R) at the model's own resolution -> the (L, N, D) input of the first block, as visual.forward (model.py:229-237)"""
    x = visual.conv1(x.to(visual.conv1.weight.dtype))
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    x = torch.cat([visual.class_embedding.to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype, device=x.device), x], dim=1)
    return visual.ln_pre(x + visual.positional_embedding.to(x.dtype)).permute(1, 0, 2)


def written_out_block(blk, x, H):
    """One residual block on (L, N, D) tokens without a mask, in the sequence of nn.MultiheadAttention (auxilary.py:153-255,
    model.py:195-198) -> (the block's output, its attention probabilities (N * H, L, L), a node of the autograd graph)"""
    L, N, D = x.shape
    hd = D // H
    q, k, v = F.linear(blk.ln_1(x), blk.attn.in_proj_weight, blk.attn.in_proj_bias).chunk(3, dim=-1)
    q = q * (float(hd) ** -0.5)
    q, k, v = (t.contiguous().view(L, N * H, hd).transpose(0, 1) for t in (q, k, v))
    probs = F.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    out = torch.bmm(probs, v).transpose(0, 1).contiguous().view(L, N, D)
    x = x + F.linear(out, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
    return x + blk.mlp(blk.ln_2(x)), probs


def tail(visual, last, rows, residual):
    """out_proj, residual, MLP, ln_post and the projection of (n, D) rows behind the last block's attention"""
    y = F.linear(rows, last.attn.out_proj.weight, last.attn.out_proj.bias) + residual
    y = y + last.mlp(last.ln_2(y))
    return visual.ln_post(y) @ visual.proj


def per_image(tower, x, blocks, tokens):
    """For x (B, 3, H, W), moved to the tower's HIP device, yields (b, the (L, 1, D) activations behind `blocks`) image by image:
    `tokens(tower, x[b:b + 1])`, then the blocks, on that one image and without a graph.  The caller allocates its batch buffers
    when b == 0 and fills row b."""
    x = x.to(hip_device(tower.conv1.weight.device))          # the model's device: the harness hands host tensors in
    for b in range(x.shape[0]):
        with torch.no_grad():
            act = tokens(tower, x[b:b + 1])
            for blk in blocks:
                act = blk(act)
        yield b, act


# ---------------------------------------------------------------------------------- the epilogue
def resize_maps(maps, H, W):
    """get_similarity_map's F.interpolate(sm, shape, mode='bilinear') of (N, h, w) fp32 maps on the device -> (N, H, W).  torch's own
    operator: K3 (kernels.bilinear_up) computes the same two taps but does not round as torch's kernel does
    (tests/test_gpu_surgery.py measures the difference), and this step is the reference's last."""
    return F.interpolate(maps[:, None], (H, W), mode="bilinear")[:, 0]


def finish(maps, B, grid, img_hw):
    """(B, h * w) or (B, h, w) fp32 maps -> (B, h, w); with img_hw the harness's map, resized to (img_hw, img_hw) and absolute
    (evaluatePerturbation.py:443-445)"""
    maps = maps.reshape(B, *grid)
    if img_hw is None:
        return maps
    return K.resize_bilinear(maps.contiguous(), img_hw, img_hw, take_abs=True)
