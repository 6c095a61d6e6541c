"""Regenerate tests/golden/m2ib.npz, m2ib_w_<model>.npz and m2ib_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_m2ib.py

The reference's own `ClipWrapper` (util/attribution_methods/CLIP/M2IB/scripts/clip_wrapper.py), `vision_heatmap_iba` (methods.py:46-51),
`IBAInterpreter` and `InformationBottleneck` (iba.py:89-194), imported unmodified behind the stand-in modules of make_golden_clip.py
(plus matplotlib and tqdm as installed), on the CPU, on the plain CLIP class the reference vendors at
CLIP_Surgery/clip/clip_model.py (`need_weights = False` set on every block: an attribute, and the behaviour of the pip `clip` package
the reference's harness loads), in fp32 and in OpenAI's mixed fp16 (the vendored build_model.convert_weights).  Nothing of the
reference is copied: every number is computed by its functions.

Models (m2ib_restated.MODELS), each from `torch.manual_seed(seed)` and the reference's constructor with `visual` replaced by that
file's own `VisionTransformer(resolution, patch, width, layers, heads, embed)` (the CLIP constructor fixes the heads at width // 64),
then the LayerNorm / in_proj_bias perturbation of make_golden_clip.py, then every weight rounded to a multiple of 2^-9, an fp16 value
(OpenAI's weights are fp16 values; the coarser grid is what lets a 12-layer tower compress under the file limit), and stored as fp16
in m2ib_w_<model>.npz, both towers.

Inputs: two per model (`<model>/<j>`), remade from stored seeds (`x_seed`, `t_seed`, `noise_seed`); `probe`, 16 values of the first
CPU draw; `txt32`, `txt16` (1, E), what the wrapper's get_text_features returned; `ref32`, `ref16`, the reference's map in front of its
resize (a recorder around torch.nn.functional.interpolate keeps its (p, p) input; the script asserts that
m2ib_restated.full_map(ref) is within 2^-23 of what vision_heatmap_iba returned); `hi`, the closed-form flow restated in fp64 with the
same noise (tests/m2ib_restated.py); `gap32`, `gap16` = max|full_map(ref) - full_map(hi)| / max|full_map(hi)| at 224 x 224; `alpha9`,
hi's alpha after nine updates, fp64.

Before the restated flow is used as the high-precision side it is run in fp32 and in mixed fp16 on this CPU, literally (every block
and ten rows in every step), and must equal the reference's buffer_capacity and map exactly (asserted).  The closed form differs from
that in one place: x9 comes from one row, not from ten, and torch's CPU GEMMs round a one-row and a ten-row call differently in the
last bit; its fp32 map must lie within 1e-5 of the reference's at 224 x 224 (asserted; the floor of the rule the GPU test applies).

Seeds are taken in ascending order from seed + 1; a seed is skipped (and logged) only if, by the reference alone, a map has a NaN,
max == min, the argmax patches of ref and hi differ, or some element of the first step's gradient has |g1_hi| < 64 |g1_ref32 - g1_hi|
(Adam's first step is sign(g): the margin that keeps a GPU's last-bit GEMM differences from flipping it; 64 is a condition, not a
measurement).  At most one skip per model.

`fifty/<j>/agree`: on how many of four other noise seeds (noise_seed + 1 .. + 4) the closed fp32 flow's argmax patch is the stored
one: what the GPU test's device-noise check rests on.

m2ib_api.json: parameter names and defaults (inspect.signature) of m2ib_clip_map and vision_heatmap_iba.
"""
import copy
import inspect
import json
import os
import sys

import numpy as np
import packaging.version  # noqa: F401  (before the stand-ins: torch's lazy imports look for it)
import matplotlib.pyplot  # noqa: F401  (as installed, before the stand-ins)
import tqdm  # noqa: F401
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import clip_restated as R  # noqa: E402
import m2ib_restated as M  # noqa: E402
from make_golden_clip import import_reference  # noqa: E402

SEEDS = {"five": 31, "seventeen": 32, "fifty": 33, "ten": 34}
IMAGES = 2


def build(plain, name):
    res, patch, width, layers, heads, embed, _ = M.MODELS[name]
    torch.manual_seed(SEEDS[name])
    m = plain.CLIP(embed, res, 1, 64, patch, M.TEXT["context_length"], M.TEXT["vocab_size"], M.TEXT["transformer_width"],
                   M.TEXT["transformer_heads"], M.TEXT["transformer_layers"])
    m.visual = plain.VisionTransformer(res, patch, width, layers, heads, embed)
    m.eval()
    for tower in (m.visual.transformer, m.transformer):
        for blk in tower.resblocks:
            blk.need_weights = False
    with torch.no_grad():
        for key, p in m.named_parameters():
            if ".ln_" in key or key.startswith("ln_"):
                p.copy_(1 + 0.1 * torch.randn(p.shape) if key.endswith("weight") else 0.1 * torch.randn(p.shape))
            elif key.endswith("in_proj_bias"):
                p.copy_(0.02 * torch.randn(p.shape))
        for p in m.parameters():
            p.copy_((p / M.GRID).round() * M.GRID)
            assert torch.equal(p, p.half().float())
    return m


class Recorder:
    """the reference's functions are called as they are; this keeps what they pass along"""

    def __init__(self, methods):
        self.methods, self.seen = methods, {}

    def __enter__(self):
        seen, base, resize = self.seen, self.methods.IBAInterpreter, torch.nn.functional.interpolate

        class Kept(base):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                seen["reader"] = self

        def record(sal, *a, **k):
            seen["grid"] = sal.detach().clone()
            return resize(sal, *a, **k)
        self.undo = (base, resize)
        self.methods.IBAInterpreter = Kept
        torch.nn.functional.interpolate = record
        return seen

    def __exit__(self, *exc):
        self.methods.IBAInterpreter, torch.nn.functional.interpolate = self.undo


def reference_run(methods, wrapper, ids, x, layer, noise_seed, steps=M.STEPS):
    with Recorder(methods) as seen:
        torch.manual_seed(noise_seed)
        out = methods.vision_heatmap_iba(ids, x, wrapper, layer, M.BETA, 1, train_steps=steps, progbar=False, device="cpu")
    reader = seen["reader"]
    return out, seen["grid"][0, 0], reader.bottleneck.buffer_capacity.detach(), reader.bottleneck.alpha.grad.detach().clone()


def one_input(methods, wrappers, sds, name, x_seed):
    """-> the entries of one input, or the reason it is skipped"""
    res, _, _, _, heads, _, layer = M.MODELS[name]
    x = R.fixture_input(x_seed, res, res)
    t_seed, noise_seed = 1000 + x_seed, 2000 + x_seed
    ids = M.fixture_ids(t_seed)
    noise = M.fixture_noise(noise_seed, name)
    out = {"x_seed": np.int64(x_seed), "t_seed": np.int64(t_seed), "noise_seed": np.int64(noise_seed), "probe": M.noise_probe(noise).numpy()}
    txt64 = M.wrapper_text(sds[32], ids, M.TEXT["transformer_heads"], torch.float64)
    hi = M.flow(sds[32], x, txt64, noise.double(), heads, layer, torch.float64)
    full_hi = M.full_map(hi["grid"])
    if torch.isnan(full_hi).any():
        return "hi: a NaN"
    for bits, dtype in ((32, torch.float32), (16, None)):
        wrapper, sd = wrappers[bits], sds[bits]
        txt = wrapper.get_text_features(ids).detach()
        mine = M.wrapper_text(sd, ids, M.TEXT["transformer_heads"], dtype)
        assert txt.dtype == mine.dtype and torch.equal(txt, mine), f"the restated text tower is not the wrapper's, fp{bits}"
        ref_map, ref_grid, ref_cap, _ = reference_run(methods, wrapper, ids, x, layer, noise_seed)
        assert ref_grid.dtype == torch.float32 and ref_map.dtype == np.float32 and ref_map.shape == (M.MAP, M.MAP)
        again = M.full_map(ref_grid).numpy()
        both = np.isnan(again) & np.isnan(ref_map)
        assert (both | (np.abs(again - ref_map) <= 2.0 ** -23)).all(), "the stored grid, F.interpolate and the min-max are not the reference's map"
        lit = M.flow(sd, x, txt, noise, heads, layer, dtype, literal=True, ids=ids)
        assert R.same(lit["cap"].numpy(), ref_cap.mean(axis=0).numpy()), f"the restated flow is not the reference's: buffer_capacity, fp{bits}"
        assert R.same(lit["grid"].numpy(), ref_grid.numpy()), f"the restated flow is not the reference's: the map before the resize, fp{bits}"
        full_ref = torch.from_numpy(ref_map)
        if torch.isnan(full_ref).any():
            return f"fp{bits}: a NaN"
        if ref_grid.max() == ref_grid.min():
            return f"fp{bits}: max == min"
        if M.argmax_patch(full_ref, name) != M.argmax_patch(full_hi, name):
            return f"fp{bits}: the argmax patches of ref and hi differ"
        if bits == 32:
            closed = M.flow(sd, x, txt, noise, heads, layer, dtype)
            d = float((M.full_map(closed["grid"]) - full_ref).abs().max())
            assert d <= 1e-5, f"the closed form is {d:.2e} from the reference's fp32 map"
            out["closed32"] = np.float64(d)
            _, _, _, g1 = reference_run(methods, wrapper, ids, x, layer, noise_seed, steps=1)
            assert R.same(g1.numpy(), lit["g1"].numpy()), "the restated flow is not the reference's: the first gradient"
            thin = (hi["g1"].abs() < 64 * (g1.double() - hi["g1"]).abs())
            if thin.any():
                return f"{int(thin.sum())} elements of the first gradient are within 64 x the fp32 error of zero"
            if name == "fifty":
                want, agree = M.argmax_patch(M.full_map(closed["grid"]), name), 0
                for other in range(1, 5):
                    got = M.flow(sd, x, txt, M.fixture_noise(noise_seed + other, name), heads, layer, dtype)
                    agree += M.argmax_patch(M.full_map(got["grid"]), name) == want
                out["agree"] = np.int64(agree)
        out[f"txt{bits}"] = txt.numpy()
        out[f"ref{bits}"] = ref_grid.numpy()
        out[f"gap{bits}"] = np.float64((full_ref.double() - full_hi).abs().max() / full_hi.abs().max())
    out["hi"] = hi["grid"].numpy()
    out["alpha9"] = hi["alpha"][0].numpy()
    return out


def main():
    G, _ = import_reference()
    from util.attribution_methods.CLIP.CLIP_Surgery.clip import build_model as ref_build
    from util.attribution_methods.CLIP.CLIP_Surgery.clip import clip_model as plain
    from util.attribution_methods.CLIP.M2IB.scripts import methods
    api = {}
    for owner, fn in ((G, "m2ib_clip_map"), (methods, "vision_heatmap_iba")):
        sig = inspect.signature(getattr(owner, fn))
        api[fn] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in sig.parameters.values()]
    with open(os.path.join(HERE, "m2ib_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    store = {}
    for name in M.MODELS:
        m32 = build(plain, name)
        m16 = copy.deepcopy(m32)
        ref_build.convert_weights(m16)
        assert m16.dtype == torch.float16 and m32.dtype == torch.float32
        sd32 = {k: v.detach().clone() for k, v in m32.state_dict().items()}
        sds = {32: sd32, 16: {k: v.half() for k, v in sd32.items()}}
        np.savez_compressed(os.path.join(HERE, f"m2ib_w_{name}.npz"), **{k: v.numpy() for k, v in sds[16].items()})
        wrappers = {32: G.ClipWrapper(m32), 16: G.ClipWrapper(m16)}
        x_seed, skipped = SEEDS[name], 0
        for j in range(IMAGES):
            while True:
                x_seed += 1
                got = one_input(methods, wrappers, sds, name, x_seed)
                if isinstance(got, dict):
                    break
                skipped += 1
                print(f"{name}/{j}: x_seed {x_seed} skipped: {got}")
            for key, val in got.items():
                store[f"{name}/{j}/{key}"] = val
            print(f"{name}/{j}: x_seed {x_seed}, gap32 {got['gap32']:.2e}, gap16 {got['gap16']:.2e}, closed32 {got['closed32']:.2e}"
                  + (f", agree {got['agree']} of 4" if "agree" in got else ""))
        assert skipped <= 1, f"{name}: {skipped} seeds skipped; something is wrong with this script, not the seeds"
    np.savez_compressed(os.path.join(HERE, "m2ib.npz"), **store)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("m2ib"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1 << 20, (f, size)
            print(f, size)


if __name__ == "__main__":
    main()
