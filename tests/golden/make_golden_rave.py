"""Regenerate tests/golden/vit_rave.npz and tests/golden/baselines_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rave.py

vit_rave.npz: the reference's own Baselines.generate_RAVE ("InFlow", ViT_explanation_generator.py:241-305) and
Baselines.generate_cam_attn (:161-178), unmodified, on the CPU, for
  - the mini hooked ViT of vit_mini.npz (32x32 image, patch 8, dim 32, depth 2, 4 heads; its weights are checked equal):
    keys rave_*, cam_*;
  - a seeded 224/16 hooked ViT (dim 48, depth 3, 12 heads, 10 classes; weights stored as w_*): keys x224, target224,
    rave224_*, cam224.
generate_RAVE reads accessors that only the reference's timm-based twin defines (ViT_new_timm.py): the blocks' residual
stream, the attention output and its projection input, and the per-block classification logits
head(norm(block_out).mean(dim=1)) of get_block_classification_probs (ViT_new_timm.py:475-495).  They are attached to the
reference's ViT_ig model below with torch forward hooks, so every number is still computed by the reference's functions.

baselines_api.json: parameter names and defaults (inspect.signature) of every public method of the reference's Baselines.
"""
import inspect
import json
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XAI_REFERENCE_ROOT")
if not REF or not os.path.isdir(REF):
    sys.exit("make_golden_rave.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from util.attribution_methods.VIT_LRP.ViT_ig import VisionTransformer                 # noqa: E402
from util.attribution_methods.VIT_LRP.ViT_explanation_generator import Baselines      # noqa: E402

torch.set_num_threads(4)


def hooked_vit(img, patch, dim, depth, heads, num_classes, seed):
    """The reference's ViT_ig model (qkv bias, LayerNorm eps 1e-6, parameters x3 to spread the logits, as vit_mini.npz) with the
    timm twin's accessors supplied by forward hooks."""
    torch.manual_seed(seed)
    model = VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=num_classes,
                              mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    probs = []

    def keep(store, key, from_input):
        def hook(module, inputs, output):
            store[key] = inputs[0] if from_input else output
        return hook

    for blk in model.blocks:
        st = {}
        blk.norm1.register_forward_hook(keep(st, "input", True))
        blk.attn.register_forward_hook(keep(st, "attn_out", False))
        blk.attn.proj.register_forward_hook(keep(st, "qkv_res", True))
        blk.norm2.register_forward_hook(keep(st, "input_plus_attn", True))
        blk.mlp.register_forward_hook(keep(st, "mlp_val", False))
        blk.register_forward_hook(lambda module, inputs, output: probs.append(model.head(model.norm(output).mean(dim=1))))
        blk.get_input = partial(st.__getitem__, "input")
        blk.get_input_plus_attn = partial(st.__getitem__, "input_plus_attn")
        blk.get_mlp_val = partial(st.__getitem__, "mlp_val")
        blk.attn.get_output = partial(st.__getitem__, "attn_out")
        blk.attn.get_qkv_res = partial(st.__getitem__, "qkv_res")
    model.register_forward_pre_hook(lambda module, inputs: probs.clear())
    model.get_block_classification_probs = lambda: list(probs)
    return model


def rave(b, x, target, **kw):
    sal, (b1, b2) = b.generate_RAVE(x.clone(), target, device="cpu", **kw)
    return sal.detach().numpy(), b1.detach().numpy(), b2.detach().numpy()


def vit_rave():
    out = {}
    g = np.load(os.path.join(HERE, "vit_mini.npz"))
    model = hooked_vit(32, 8, 32, 2, 4, 10, 77)
    assert all(np.array_equal(v.numpy(), g["w_" + k]) for k, v in model.state_dict().items())        # the model of vit_mini.npz
    x, target = torch.from_numpy(g["x"]), torch.tensor(int(g["target"]))
    b = Baselines(model)
    with torch.no_grad():
        model(x)                       # generate_RAVE reads blocks[-1]'s attention map before its own forward
    out["rave_default"], out["rave_default_b1"], out["rave_default_b2"] = rave(b, x, target)
    out["rave_nograd"] = rave(b, x, target, withgrad=False)[0]
    out["rave_ablate1"] = rave(b, x, target, ablate=1)[0]
    out["rave_token1"] = rave(b, x, target, target_token=1)[0]
    out["rave_stop0"], out["rave_stop0_b1"], out["rave_stop0_b2"] = rave(b, x, target, stop_layer=0)
    out["cam_last"] = b.generate_cam_attn(x.clone(), target, "cpu").detach().numpy()
    out["cam_first"] = b.generate_cam_attn(x.clone(), target, "cpu", layer=0).detach().numpy()

    model = hooked_vit(224, 16, 48, 3, 12, 10, 224)
    gen = torch.Generator().manual_seed(225)
    u8 = torch.randint(0, 256, (1, 3, 224, 224), generator=gen, dtype=torch.uint8)
    x = (u8.float() / 255.0 - 0.5) / 0.25                     # 256 distinct values: the stored input compresses
    with torch.no_grad():
        target = model(x).argmax(1)[0]
    out["x224"], out["target224"] = x.numpy(), np.int64(target.item())
    for k, v in model.state_dict().items():
        out["w224_" + k] = v.numpy().copy()
    b = Baselines(model)
    out["rave224_default"], out["rave224_default_b1"], out["rave224_default_b2"] = rave(b, x, target)
    out["rave224_nograd_ablate1"] = rave(b, x, target, withgrad=False, ablate=1)[0]
    out["cam224"] = b.generate_cam_attn(x.clone(), target, "cpu").detach().numpy()
    for k, v in out.items():
        if not k.startswith("w224_"):
            assert np.isfinite(v).all(), k
    np.savez_compressed(os.path.join(HERE, "vit_rave.npz"), **out)
    print("vit_rave.npz", {k: v.shape for k, v in out.items() if not k.startswith("w224_")})


def baselines_api():
    api = {}
    for name, fn in inspect.getmembers(Baselines, inspect.isfunction):
        if name.startswith("_"):
            continue
        params = list(inspect.signature(fn).parameters.values())[1:]            # without self
        api[name] = [{"name": p.name, "has_default": p.default is not inspect.Parameter.empty,
                      "default": None if p.default is inspect.Parameter.empty else p.default} for p in params]
    with open(os.path.join(HERE, "baselines_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    print("baselines_api.json", sorted(api))


if __name__ == "__main__":
    vit_rave()
    baselines_api()
