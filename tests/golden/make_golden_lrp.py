"""Regenerate tests/golden/lrp.npz, lrp_w224_16.npz, lrp_w224_32.npz and lrp_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lrp.py

The reference's own `LRP(model).generate_LRP` (ViT_explanation_generator.py:107-133) on its own timm-derived relprop model
(ViT_LRP_timm.VisionTransformer), both unmodified, on the CPU.  ViT_LRP_timm.py imports four timm modules (:43-46) of which it uses
three names when a model is built directly; timm is not needed for that, so stand-ins for exactly those imports are put into
sys.modules below.  Nothing of the reference is copied: every number is computed by its functions.

Three models, each from `torch.manual_seed(seed)`, the reference's constructor, every parameter times `scale`:
    mini      (img 32, patch 8, dim 32, depth 2, heads 4, classes 10), seed 2, scale 1   weights in lrp.npz as mini/w_*
    v16       (img 224, patch 16, dim 48, depth 3, heads 12, classes 10), seed 0, scale 3   weights in lrp_w224_16.npz as w_*
    v32       (img 224, patch 32, dim 48, depth 3, heads 12, classes 10), seed 7, scale 1   weights in lrp_w224_32.npz as w_*
and three inputs per model, from `torch.Generator().manual_seed(x_seed)` with the first three x_seed >= seed + 1 that pass the gap
rule below (stored as `<model>/<j>/x_seed`):
    x = (randint(0, 256, (1, 3, img, img)).float() / 255 - 0.5) / 0.25      (not stored: `fixture_input` below remakes it; its sum is)
The target is the argmax.  Every output is stored twice, `<model>/<j>/<key>/f32` from the reference as it is and `.../f64` from the same
call on model.double(), with `.../gap` = max|f32 - f64| / max|f64|.  The method divides by sums that can cancel, so its fp32 result is
ill-conditioned for some weights and inputs; the fixtures are chosen (the seeds above) so that every gap is at most 1e-5: an input with
a larger one is skipped, and the stored ones are asserted.
Keys: every served method at its defaults, `withgrad=False`, `start_layer=1`, `is_ablation=True` (last_layer and second_layer), and for
the mini model each block's attn_cam (`cam<i>`).

lrp_api.json: parameter names and defaults (inspect.signature) of the reference's LRP.generate_LRP.
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = {"mini": dict(cfg=(32, 8, 32, 2, 4, 10), seed=2, scale=1.0, weights="lrp.npz"),
          "v16": dict(cfg=(224, 16, 48, 3, 12, 10), seed=0, scale=3.0, weights="lrp_w224_16.npz"),
          "v32": dict(cfg=(224, 32, 48, 3, 12, 10), seed=7, scale=1.0, weights="lrp_w224_32.npz")}
IMAGES = 3
GAP_MAX = 1e-5
# key -> keyword arguments of generate_LRP
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
    g = torch.Generator().manual_seed(x_seed)
    return (torch.randint(0, 256, (1, 3, img, img), generator=g).float() / 255 - 0.5) / 0.25


def one_image(LRP, name, model, model64, x_seed, img):
    """every stored entry of one input, or None if one of its gaps is above GAP_MAX"""
    x = fixture_input(x_seed, img)
    target = int(model(x).argmax())
    if target != int(model64(x.double()).argmax()):
        return None
    got = {"x_seed": np.int64(x_seed), "x_sum": np.float64(x.double().sum()), "target": np.int64(target)}

    def store(key, a32, a64):
        gap = float(np.abs(a32 - a64).max() / np.abs(a64).max())
        print(f"{name}/seed {x_seed}/{key}: gap {gap:.2e}")
        got[f"{key}/f32"], got[f"{key}/f64"], got[f"{key}/gap"] = a32, a64, np.float64(gap)
        return gap <= GAP_MAX

    for key, kw in CALLS.items():
        a32 = LRP(model).generate_LRP(x, target, device="cpu", **kw).detach().numpy()
        a64 = LRP(model64).generate_LRP(x.double(), target, device="cpu", **kw).detach().numpy()
        assert a32.dtype == np.float32 and a64.dtype == np.float64
        if not store(key, a32, a64):
            return None
        if name == "mini" and key == "transformer_attribution":
            for i, (b32, b64) in enumerate(zip(model.blocks, model64.blocks)):
                if not store(f"cam{i}", b32.attn.get_attn_cam().detach().numpy(), b64.attn.get_attn_cam().detach().numpy()):
                    return None
    return got


def _stub_timm():
    """stand-ins for the four imports of ViT_LRP_timm.py:43-46"""
    def module(name, **names):
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
        return m

    def lecun_normal_(tensor):
        fan_in = tensor.shape[1] * (tensor[0][0].numel() if tensor.dim() > 2 else 1)
        return nn.init.trunc_normal_(tensor, std=(1.0 / fan_in) ** 0.5 / .87962566103423978)

    def unused(*a, **k):
        raise NotImplementedError("timm is not installed: only direct construction of the model is supported")

    timm = module("timm")
    timm.data = module("timm.data", IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225),
                       IMAGENET_INCEPTION_MEAN=(0.5, 0.5, 0.5), IMAGENET_INCEPTION_STD=(0.5, 0.5, 0.5))
    timm.models = module("timm.models")
    timm.models.helpers = module("timm.models.helpers", build_model_with_cfg=unused, named_apply=unused, adapt_input_conv=unused)
    timm.models.layers = module("timm.models.layers", DropPath=nn.Identity, trunc_normal_=nn.init.trunc_normal_, lecun_normal_=lecun_normal_)
    timm.models.registry = module("timm.models.registry", register_model=lambda fn: fn)


def main():
    ref = os.environ.get("XAI_REFERENCE_ROOT")
    if not ref or not os.path.isdir(ref):
        sys.exit("make_golden_lrp.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    _stub_timm()
    from util.attribution_methods.VIT_LRP.ViT_LRP_timm import VisionTransformer
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import LRP
    torch.set_num_threads(4)

    sig = inspect.signature(LRP.generate_LRP)
    api = {"generate_LRP": [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in sig.parameters.items()]}
    with open(os.path.join(HERE, "lrp_api.json"), "w") as f:
        json.dump(api, f, indent=1)

    out, worst = {}, 0.0
    for name, spec in MODELS.items():
        img, patch, dim, depth, heads, classes = spec["cfg"]
        torch.manual_seed(spec["seed"])
        model = VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=classes).eval()
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(spec["scale"])
        weights = {f"w_{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()}
        if spec["weights"] == "lrp.npz":
            out.update({f"{name}/{k}": v for k, v in weights.items()})
        else:
            np.savez_compressed(os.path.join(HERE, spec["weights"]), **weights)
        model64 = VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=classes).eval()
        model64.load_state_dict(model.state_dict())
        model64 = model64.double()
        out[f"{name}/cfg"] = np.asarray(spec["cfg"], np.int64)
        j, x_seed = 0, spec["seed"] + 1
        while j < IMAGES:
            got = one_image(LRP, name, model, model64, x_seed, img)
            if got is None:
                print(f"{name}: input seed {x_seed} skipped (a gap above {GAP_MAX})")
            else:
                out.update({f"{name}/{j}/{k}": v for k, v in got.items()})
                worst = max([worst] + [float(v) for k, v in got.items() if k.endswith("/gap")])
                j += 1
            x_seed += 1
    np.savez_compressed(os.path.join(HERE, "lrp.npz"), **out)
    print(f"largest gap {worst:.2e}")
    assert worst <= GAP_MAX


if __name__ == "__main__":
    main()
