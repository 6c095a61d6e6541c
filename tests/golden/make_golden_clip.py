"""Regenerate tests/golden/clip.npz, clip_w_<model>.npz and clip_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clip.py

The reference's own `clip_encode_dense`, `grad_eclip` and `mask_clip` (util/attribution_methods/CLIP/generate_emap.py:309-376,
:453-485, :500-529), imported unmodified, on the CPU, on the `CLIP` of its Game_MM_CLIP/clip/model.py after that file's own
`convert_weights` (OpenAI's mixed fp16).  generate_emap.py imports cv2, clip, ftfy, torchvision, skimage.transform and transformers,
none of which these three functions use; stand-ins for exactly those imports are put into sys.modules below.  Nothing of the
reference is copied: every number is computed by its functions.

Models (resolution, patch, width, layers, embed), each from `torch.manual_seed(seed)` and the reference's constructor, then (from the
same generator) every LayerNorm weight 1 + 0.1 N(0,1), every LayerNorm bias 0.1 N(0,1) and every in_proj_bias 0.02 N(0,1), so that no
parameter the flow reads is at a trivial value; the text tower is the smallest the constructor takes (clip_restated.TEXT):
    mini   (32, 8, 64, 2, 16)     L = 17
    short  (32, 16, 128, 1, 16)   L = 5: fewer rows than a wave, D = 128
    long   (224, 16, 64, 1, 16)   L = 197: more than three waves of rows
    b32    (224, 32, 64, 1, 16)   L = 50
The weights are stored as converted (half and fp32) in clip_w_<model>.npz, one file per model to stay inside the committed-file limit.

Inputs: three per model (`<model>/<j>`), and `mini/wide`, a 32 x 48 input for the bicubic positional path.  Input and texts are
remade from seeds (clip_restated.fixture_input / fixture_texts; `x_seed`, `t_seed` stored).  Per input: `encode_image/ref16`, and for
T = 1 and T = 2 texts the five rows' maps as `<row>/T<n>/ref16`, `/hi` and `/gap`.  `hi` is the restated flow (tests/clip_restated.py)
in fp64 on the same fp16-valued weights, gap = max|ref16 - hi| / max|hi|; `/gap32` is the same figure for the restated flow in fp32
(every weight cast to fp32), the yardstick of an fp32 model: stored, because a CPU's fp32 GEMMs round as its BLAS pleases and a
bound must not depend on the machine a test runs on.  For j = 0 the reference's whole 9-tuple is stored
(`tuple/<name>`), for the other inputs its class-token rows.

Before the restated flow is used as the high-precision side it is run in the reference's dtype on this CPU and must equal the
reference's 9-tuple and maps exactly (asserted).

Seeds are taken in ascending order from seed + 1; a seed is skipped (and logged) unless, by the reference alone, no cosine min-max is
degenerate (no NaN in a map), no map is all zero (the relu can leave nothing of a 2 x 2 map), at least a quarter of the patches of every eclip map are positive, and the argmax patch of ref16 and hi
agree for every row.

clip_api.json: parameter names and defaults (inspect.signature) of the reference's clip_encode_dense, grad_eclip, mask_clip and
attention_layer.
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import packaging.version  # noqa: F401  (before the stand-ins: torch's lazy imports look for it)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_restated as R  # noqa: E402

SEEDS = {"mini": 1, "short": 2, "long": 3, "b32": 4}
IMAGES = 3
TUPLE = ("outputs", "v_final", "x_in", "v", "q_out", "k_out", "attn", "att_output")


class _Meta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


class _Anything(metaclass=_Meta):
    """what a stand-in module hands out: callable, subclassable, with any attribute"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def import_reference():
    root = os.environ["XAI_REFERENCE_ROOT"]
    for name in ("cv2", "clip", "ftfy", "torchvision", "torchvision.transforms", "skimage", "skimage.transform", "transformers"):
        sys.modules[name] = _Stub(name)
    sys.path.insert(0, root)
    from util.attribution_methods.CLIP import generate_emap
    from util.attribution_methods.CLIP.Game_MM_CLIP.clip import model as ref_model
    return generate_emap, ref_model


def build(ref_model, name):
    res, patch, width, layers, embed = R.MODELS[name]
    torch.manual_seed(SEEDS[name])
    m = ref_model.CLIP(embed, res, layers, width, patch, R.TEXT["context_length"], R.TEXT["vocab_size"], R.TEXT["transformer_width"],
                       R.TEXT["transformer_heads"], R.TEXT["transformer_layers"]).eval()
    with torch.no_grad():
        for key, p in m.named_parameters():
            if ".ln_" in key or key.startswith("ln_"):
                p.copy_(1 + 0.1 * torch.randn(p.shape) if key.endswith("weight") else 0.1 * torch.randn(p.shape))
            elif key.endswith("in_proj_bias"):
                p.copy_(0.02 * torch.randn(p.shape))
    ref_model.convert_weights(m)
    return m


def maps_of(rows):
    return {k: v.detach() for k, v in rows.items()}


def one_input(G, m, sd, res, x_seed, hw):
    """-> the entries of one input, or the reason it is skipped"""
    embed = sd["visual.proj"].shape[1]
    x = R.fixture_input(x_seed, *hw)
    out = {"x_seed": np.int64(x_seed), "t_seed": np.int64(1000 + x_seed)}
    txt2 = R.fixture_texts(1000 + x_seed, 2, embed)
    ref_tuple = G.clip_encode_dense(x, m)
    mine = R.encode_dense(sd, x, res, None)
    for a, b, name in zip(ref_tuple[:8], mine[:8], TUPLE):
        assert a.dtype == b.dtype == torch.float16 and torch.equal(a, b), f"the restated flow is not the reference's: {name}"
    assert tuple(ref_tuple[8]) == tuple(mine[8])
    hi_tuple = R.encode_dense(sd, x, res, torch.float64)
    low_tuple = R.encode_dense(sd, x, res, torch.float32)
    if hw == (res, res):              # not under no_grad: the reference's blocks hang a hook on their attention weights
        out["encode_image/ref16"] = m.encode_image(x)[0].detach().numpy()
    for T in (1, 2):
        txt = txt2[:T]
        ref = maps_of(R.rows_from_tuple(ref_tuple, txt.half(), G.grad_eclip, G.mask_clip))
        again = maps_of(R.rows_from_tuple(mine, txt.half()))
        hi = maps_of(R.rows_from_tuple(hi_tuple, txt.half().double()))
        low = maps_of(R.rows_from_tuple(low_tuple, txt.half().float()))
        for row in R.ROWS:
            a, b, h = ref[row], again[row], hi[row]
            assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(7), b.nan_to_num(7)), row
            if torch.isnan(a).any() or torch.isnan(h).any():
                return f"{row} T{T}: a degenerate cosine min-max"
            if not (a != 0).any() or not (h != 0).any():
                return f"{row} T{T}: an all-zero map"
            if row == "eclip" and (a > 0).float().mean() < 0.25:
                return f"eclip T{T}: only {(a > 0).float().mean():.2f} of the patches are positive"
            if int(a.float().argmax()) != int(h.argmax()):
                return f"{row} T{T}: the argmax patches of ref16 and hi differ"
            pre = f"{row}/T{T}/"
            out[pre + "ref16"] = a.numpy()
            out[pre + "hi"] = h.numpy()
            out[pre + "gap"] = np.float64((a.double() - h).abs().max() / h.abs().max())
            out[pre + "gap32"] = np.float64((low[row].double() - h).abs().max() / h.abs().max())
    out["_tuple"] = ref_tuple
    return out


def main():
    G, ref_model = import_reference()
    api = {}
    for fn in ("clip_encode_dense", "grad_eclip", "mask_clip", "attention_layer"):
        sig = inspect.signature(getattr(G, fn))
        api[fn] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in sig.parameters.values()]
    with open(os.path.join(HERE, "clip_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    store = {}
    for name, (res, patch, width, layers, embed) in R.MODELS.items():
        m = build(ref_model, name)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        np.savez_compressed(os.path.join(HERE, f"clip_w_{name}.npz"), **{k: v.numpy() for k, v in sd.items()})
        wanted = [(str(j), (res, res)) for j in range(IMAGES)] + ([("wide", (32, 48))] if name == "mini" else [])
        x_seed = SEEDS[name]
        for tag, hw in wanted:
            while True:
                x_seed += 1
                got = one_input(G, m, sd, res, x_seed, hw)
                if isinstance(got, dict):
                    break
                print(f"{name}/{tag}: x_seed {x_seed} skipped: {got}")
            tup = got.pop("_tuple")
            for key, val in got.items():
                store[f"{name}/{tag}/{key}"] = val
            for t, tname in zip(tup[:8], TUPLE):
                t = t.detach()
                if tag == "0":
                    store[f"{name}/{tag}/tuple/{tname}"] = t.numpy()
                elif tname in ("outputs", "attn"):
                    store[f"{name}/{tag}/cls/{tname}"] = t[0, 0].numpy()
                elif tname in ("q_out", "att_output"):
                    store[f"{name}/{tag}/cls/{tname}"] = t[0, 0].numpy()
            gaps = {k: float(v) for k, v in got.items() if k.endswith("/gap")}
            print(f"{name}/{tag}: x_seed {x_seed}, gaps {min(gaps.values()):.2e} .. {max(gaps.values()):.2e}")
    path = os.path.join(HERE, "clip.npz")
    np.savez_compressed(path, **store)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("clip"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
