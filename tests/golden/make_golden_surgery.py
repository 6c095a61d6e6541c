"""Regenerate tests/golden/surgery.npz, surgery_w_<model>.npz and surgery_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_surgery.py

The reference's own `CLIPSurgery` (util/attribution_methods/CLIP/CLIP_Surgery/clip/clip_surgery_model.py), `clip_surgery_map`
(generate_emap.py:117-129), `clip_feature_surgery` and `get_similarity_map` (CLIP_Surgery/clip/clip.py:271-308), imported unmodified
behind the stand-in modules of make_golden_clip.py, on the CPU, in fp32 (the reference leaves convert_weights commented out, so its
Surgery model computes in fp32).  `clip_surgery_map` itself is called; only `encode_text_with_prompt_ensemble`, which needs a
tokenizer and 85 prompt templates, is stood in by a function that returns the stored seeded normalised rows.  Nothing of the
reference is copied: every number is computed by its functions.

Models (surgery_restated.MODELS), each from `torch.manual_seed(seed)` and the reference's constructor with `visual` replaced by that
file's own `VisionTransformer(resolution, patch, width, layers, heads, embed)` (the CLIPSurgery constructor fixes the heads at
width // 64), then the LayerNorm / in_proj_bias perturbation of make_golden_clip.py, then every weight rounded to an fp16 value
(OpenAI's weights are fp16 values) and stored as fp16 in surgery_w_<model>.npz.

Inputs: two per model (`<model>/<j>`), remade from stored seeds (`x_seed`, `t_seed`).  Per input and T in (60, 2): `T<n>/ref32`, the
reference's map of text 0; `/hi`, the dual-path flow restated in fp64 (tests/surgery_restated.py); `/gap` = max|ref32 - hi| /
max|hi| over the maps at the image size; and once per input `feats/ref32` (L, E), what encode_image returned, and `feats/hi`.
`six/0/T1/ref32` is the one T = 1 case: the reference's all-NaN map.

A 224 x 224 map is 200 KB in fp32 and 400 KB in fp64, and the committed files stay under 1 MiB, so `ref32` and `hi` are stored in
front of get_similarity_map's last step, the bilinear resize: (p, p), p the patch grid.  `ref32` is what the reference's own
get_similarity_map returns for shape = (p, p) (a recorder around it calls it a second time with that shape; a bilinear resize to the
same size copies).  The script asserts that surgery_restated.full_map(ref32, image size), torch's F.interpolate(mode="bilinear"),
is within 2^-23 of the map clip_surgery_map returned (the maps lie in [0, 1]; torch's CPU kernel rounds a T-channel resize and a
one-channel resize differently in the last bit), so the stored grid and that one call are the reference's map to one rounding; `gap`
is computed from the map clip_surgery_map itself returned.

Before the restated flow is used as the high-precision side it is run in fp32 on this CPU and must equal the reference's features and
maps exactly (asserted).

Seeds are taken in ascending order from seed + 1; a seed is skipped (and logged) only if, by the reference alone, a map has a NaN,
max == min, or the argmax pixels of ref32 and hi differ.

surgery_api.json: parameter names and defaults (inspect.signature) of clip_surgery_map, clip_feature_surgery and get_similarity_map.
"""
import inspect
import json
import os
import sys

import numpy as np
import packaging.version  # noqa: F401  (before the stand-ins: torch's lazy imports look for it)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import clip_restated as R  # noqa: E402
import surgery_restated as S  # noqa: E402
from make_golden_clip import import_reference  # noqa: E402

SEEDS = {"six": 21, "wave": 22, "one": 23, "long": 24}
IMAGES = 2
CASES = (S.TEXTS, 2)


def build(ref_model, name):
    res, patch, width, layers, heads, embed = S.MODELS[name]
    torch.manual_seed(SEEDS[name])
    # the constructor's own visual tower (width 64, one layer) is replaced on the next line
    m = ref_model.CLIPSurgery(embed, res, 1, 64, patch, S.TEXT["context_length"], S.TEXT["vocab_size"], S.TEXT["transformer_width"],
                              S.TEXT["transformer_heads"], S.TEXT["transformer_layers"])
    m.visual = ref_model.VisionTransformer(res, patch, width, layers, heads, embed)
    m.eval()
    with torch.no_grad():
        for key, p in m.named_parameters():
            if ".ln_" in key or key.startswith("ln_"):
                p.copy_(1 + 0.1 * torch.randn(p.shape) if key.endswith("weight") else 0.1 * torch.randn(p.shape))
            elif key.endswith("in_proj_bias"):
                p.copy_(0.02 * torch.randn(p.shape))
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def reference_map(G, m, x, txt):
    """clip_surgery_map as get_CLIP_attr calls it (evaluatePerturbation.py:429), its text encoder stood in -> ((1, H, W, T) map, the
    (1, L, E) features its encode_image returned, the (1, p, p, T) map its get_similarity_map returns for the grid's own size)"""
    seen = {}
    encode = m.encode_image

    def keep(image):
        seen["feats"] = encode(image)
        return seen["feats"].clone()
    stood_in, resize = G.surgery_clip.encode_text_with_prompt_ensemble, G.surgery_clip.get_similarity_map

    def record(sm, shape):
        side = int(sm.shape[1] ** 0.5)
        seen["grid"] = resize(sm.clone(), (side, side))
        return resize(sm, shape)
    G.surgery_clip.encode_text_with_prompt_ensemble = lambda model, texts, device, prompt_templates=None: txt
    G.surgery_clip.get_similarity_map = record
    m.encode_image = keep
    try:
        out = G.clip_surgery_map(model=m, image=x, texts=["stood in"] * txt.shape[0], device="cpu")
    finally:
        G.surgery_clip.encode_text_with_prompt_ensemble, G.surgery_clip.get_similarity_map = stood_in, resize
        del m.encode_image
    return out, seen["feats"], seen["grid"]


def one_input(G, m, sd, name, x_seed, with_one_text):
    res, _patch, _width, _layers, heads, embed = S.MODELS[name]
    x = R.fixture_input(x_seed, res, res)
    out = {"x_seed": np.int64(x_seed), "t_seed": np.int64(1000 + x_seed)}
    txt_all = S.fixture_texts(1000 + x_seed, S.TEXTS, embed)
    low = S.dual_path(sd, x, heads, torch.float32)
    hi_feats = S.dual_path(sd, x, heads, torch.float64)
    for T in CASES + ((1,) if with_one_text else ()):
        txt = txt_all[:T]
        ref, feats, ref_grid = reference_map(G, m, x, txt)
        assert feats.dtype == torch.float32 and torch.equal(feats, low), "the restated flow is not the reference's: the features"
        again, again_grid = S.reference_map(low, txt, (res, res))
        assert ref.dtype == torch.float32 and tuple(ref.shape) == (1, res, res, T)
        assert R.same(ref.numpy(), again.numpy()), f"the restated flow is not the reference's: the map, T{T}"
        assert R.same(ref_grid.numpy(), again_grid.numpy()), f"the restated flow is not the reference's: the map before the resize, T{T}"
        a, a_grid = ref[0, :, :, 0], ref_grid[0, :, :, 0].contiguous()
        if T > 1:
            assert (S.full_map(a_grid, (res, res)) - a).abs().max() <= 2.0 ** -23, "the stored grid and F.interpolate are not the reference's map"
        if T == 1:
            assert torch.isnan(a).all() and torch.isnan(a_grid).all()
            out["T1/ref32"] = a_grid.numpy()
            continue
        h_grid = S.reference_map(hi_feats, txt.double(), (res, res))[1][0, :, :, 0].contiguous()
        h = S.full_map(h_grid, (res, res))
        if torch.isnan(a).any() or torch.isnan(h).any():
            return f"T{T}: a NaN"
        if a.max() == a.min():
            return f"T{T}: max == min"
        if int(a.argmax()) != int(h.argmax()):
            return f"T{T}: the argmax pixels of ref32 and hi differ"
        out[f"T{T}/ref32"] = a_grid.numpy()
        out[f"T{T}/hi"] = h_grid.numpy()
        out[f"T{T}/gap"] = np.float64((a.double() - h).abs().max() / h.abs().max())
    out["feats/ref32"] = low[0].numpy()
    out["feats/hi"] = hi_feats[0].numpy()
    return out


def main():
    G, _ = import_reference()
    from util.attribution_methods.CLIP.CLIP_Surgery.clip import clip_surgery_model as ref_model
    api = {}
    for owner, fn in ((G, "clip_surgery_map"), (G.surgery_clip, "clip_feature_surgery"), (G.surgery_clip, "get_similarity_map")):
        sig = inspect.signature(getattr(owner, fn))
        api[fn] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in sig.parameters.values()]
    with open(os.path.join(HERE, "surgery_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    store = {}
    for name in S.MODELS:
        m = build(ref_model, name)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("visual.")}
        assert all(torch.equal(v, v.half().float()) for v in sd.values())
        np.savez_compressed(os.path.join(HERE, f"surgery_w_{name}.npz"), **{k: v.half().numpy() for k, v in sd.items()})
        x_seed, skipped = SEEDS[name], 0
        for j in range(IMAGES):
            while True:
                x_seed += 1
                got = one_input(G, m, sd, name, x_seed, with_one_text=(name == "six" and j == 0))
                if isinstance(got, dict):
                    break
                skipped += 1
                print(f"{name}/{j}: x_seed {x_seed} skipped: {got}")
            for key, val in got.items():
                store[f"{name}/{j}/{key}"] = val
            gaps = {k: float(v) for k, v in got.items() if k.endswith("/gap")}
            print(f"{name}/{j}: x_seed {x_seed}, gaps " + ", ".join(f"{k[:-4]} {v:.2e}" for k, v in sorted(gaps.items())))
        assert skipped <= 1, f"{name}: {skipped} seeds skipped; something is wrong with this script, not the seeds"
    np.savez_compressed(os.path.join(HERE, "surgery.npz"), **store)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("surgery"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1 << 20, (f, size)
            print(f, size)


if __name__ == "__main__":
    main()
