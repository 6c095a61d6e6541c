"""Regenerate tests/golden/clip_attn.npz, clip_attn_w_<model>.npz and clip_attn_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clip_attn.py

The reference's own `mm_interpret`, `compute_rollout_attention` and `clip_lrp` (util/attribution_methods/CLIP/generate_emap.py:133-285),
imported unmodified behind the stand-in modules of make_golden_clip.py, on the CPU, on the `CLIP` of its Game_MM_CLIP/clip/model.py
whose `visual` is that file's own `VisualTransformer(resolution, patch, width, layers, heads, embed)` (the CLIP constructor fixes the
heads at width // 64), after that file's own `convert_weights` (OpenAI's mixed fp16).  Nothing of the reference is copied: every
number is computed by its functions.

Models (clip_attn_restated.MODELS), each from `torch.manual_seed(seed)`, then the LayerNorm / in_proj_bias perturbation of
make_golden_clip.py; the text tower is the smallest the constructor takes.  The reference's functions call `model(images, texts)` on
token ids: the fixtures' are seeded random ids (clip_attn_restated.fixture_tokens), and what the model's own encode_text makes of them
is stored per input as `txt_raw/T<n>` (T, E), the text features before model.forward normalises them.  The weights are stored as
converted in clip_attn_w_<model>.npz.

Inputs: two per model (`<model>/<j>`), remade from stored seeds (`x_seed`, `t_seed`).  Per input `<row>/T<n>/ref16`, `/hi`, `/gap` and
`/gap32` for game, rollout and lrp at T = 1 and for game at T = 2: `hi` is the restated flow (tests/clip_attn_restated.py) in fp64 on
the same fp16-valued weights, gap = max|ref16 - hi| / max|hi|, gap32 the same figure for the restated flow in fp32.

Before the restated flow is used as the high-precision side it is run in the reference's dtype on this CPU and must equal the
reference's maps, attn_probs and gradients exactly (asserted).

Seeds are taken in ascending order from seed + 1; a seed is skipped (and logged) unless, by the reference alone, no map has a NaN or is
all zero, at least a quarter of the patches of every game map are positive, and the argmax patch of ref16 and hi agree for every row.

clip_attn_api.json: parameter names and defaults (inspect.signature) of the reference's three functions.
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
import clip_attn_restated as A  # noqa: E402
import clip_restated as R  # noqa: E402
from make_golden_clip import import_reference  # noqa: E402

SEEDS = {"tiny": 11, "mini": 12, "wave": 13, "long": 14, "one": 15}
IMAGES = 2
CASES = (("game", 1), ("game", 2), ("rollout", 1), ("lrp", 1))


def build(ref_model, name):
    res, patch, width, layers, heads, embed = A.MODELS[name]
    torch.manual_seed(SEEDS[name])
    # the constructor's own visual tower (width 64, one layer: its heads are width // 64) is replaced on the next line
    m = ref_model.CLIP(embed, res, 1, 64, patch, A.TEXT["context_length"], A.TEXT["vocab_size"], A.TEXT["transformer_width"],
                       A.TEXT["transformer_heads"], A.TEXT["transformer_layers"])
    m.visual = ref_model.VisualTransformer(res, patch, width, layers, heads, embed)
    m.eval()
    with torch.no_grad():
        for key, p in m.named_parameters():
            if ".ln_" in key or key.startswith("ln_"):
                p.copy_(1 + 0.1 * torch.randn(p.shape) if key.endswith("weight") else 0.1 * torch.randn(p.shape))
            elif key.endswith("in_proj_bias"):
                p.copy_(0.02 * torch.randn(p.shape))
    ref_model.convert_weights(m)
    return m


def reference_rows(G, m, x, tokens):
    """the three rows by the reference's functions as get_CLIP_attr calls them (evaluatePerturbation.py:410-437) -> ({row: map},
    the attn_probs and attn_grad its visual blocks hold afterwards: after clip_lrp (T = 1) every block's gradient is of this call,
    after mm_interpret only the last block's)"""
    T = tokens.shape[0]
    out = {"game": G.mm_interpret(model=m, image=x, texts=tokens, device="cpu").sum(0).detach()}
    attentions = G.mm_interpret(model=m, image=x, texts=tokens, device="cpu", rollout=True)
    out["rollout"] = G.compute_rollout_attention(attentions)[0].detach()
    if T == 1:
        _, hm = G.clip_lrp(x, tokens, m, "cpu")
        side = int(hm.shape[-1] ** 0.5)
        out["lrp"] = hm.reshape((-1, side, side))[0].detach()
    blocks = list(m.visual.transformer.resblocks)
    return out, [b.attn_probs.detach() for b in blocks], [b.attn_grad for b in blocks]


def one_input(G, m, sd, name, x_seed):
    res, _patch, _width, _layers, heads, embed = A.MODELS[name]
    x = R.fixture_input(x_seed, res, res)
    out = {"x_seed": np.int64(x_seed), "t_seed": np.int64(1000 + x_seed)}
    for T in (1, 2):
        tokens = A.fixture_tokens(1000 + x_seed, 2)[:T]
        raw = m.encode_text(tokens).detach()
        assert raw.dtype == torch.float16 and tuple(raw.shape) == (T, embed)
        assert torch.equal(torch.nn.functional.normalize(raw, dim=-1), raw / raw.norm(dim=-1, keepdim=True))
        out[f"txt_raw/T{T}"] = raw.numpy()
        ref, ref_probs, ref_grads = reference_rows(G, m, x, tokens)
        probs, grads = A.probs_and_grads(sd, x, raw, heads, None)
        for i, (a, b) in enumerate(zip(ref_probs, probs)):
            assert a.dtype == b.dtype == torch.float16 and torch.equal(a, b), f"the restated flow is not the reference's: attn_probs {i}"
        for i, (a, b) in enumerate(zip(ref_grads, grads)):
            if T == 1 or i == len(grads) - 1:
                assert a is not None and torch.equal(a, b), f"the restated flow is not the reference's: the gradient of attn_probs {i}"
        again = A.rows_from(probs, grads, T)
        hi = A.rows_from(*A.probs_and_grads(sd, x, raw, heads, torch.float64), T)
        low = A.rows_from(*A.probs_and_grads(sd, x, raw, heads, torch.float32), T)
        for row, t in CASES:
            if t != T:
                continue
            a, h = ref[row], hi[row]
            assert torch.equal(a, again[row]), f"the restated flow is not the reference's: {row} T{T}"
            if torch.isnan(a).any() or torch.isnan(h).any():
                return f"{row} T{T}: a NaN"
            if not (a != 0).any() or not (h != 0).any():
                return f"{row} T{T}: an all-zero map"
            if row == "game" and (a > 0).float().mean() < 0.25:
                return f"game T{T}: only {(a > 0).float().mean():.2f} of the patches are positive"
            if int(a.float().argmax()) != int(h.argmax()):
                return f"{row} T{T}: the argmax patches of ref16 and hi differ"
            pre = f"{row}/T{T}/"
            out[pre + "ref16"] = a.numpy()
            out[pre + "hi"] = h.numpy()
            out[pre + "gap"] = np.float64((a.double() - h).abs().max() / h.abs().max())
            out[pre + "gap32"] = np.float64((low[row].double() - h).abs().max() / h.abs().max())
    return out


def main():
    G, ref_model = import_reference()
    api = {}
    for fn in ("mm_interpret", "clip_lrp", "compute_rollout_attention"):
        sig = inspect.signature(getattr(G, fn))
        api[fn] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in sig.parameters.values()]
    with open(os.path.join(HERE, "clip_attn_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    store = {}
    for name in A.MODELS:
        m = build(ref_model, name)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        np.savez_compressed(os.path.join(HERE, f"clip_attn_w_{name}.npz"), **{k: v.numpy() for k, v in sd.items()})
        x_seed = SEEDS[name]
        for j in range(IMAGES):
            while True:
                x_seed += 1
                got = one_input(G, m, sd, name, x_seed)
                if isinstance(got, dict):
                    break
                print(f"{name}/{j}: x_seed {x_seed} skipped: {got}")
            for key, val in got.items():
                store[f"{name}/{j}/{key}"] = val
            gaps = {k: float(v) for k, v in got.items() if k.endswith("/gap")}
            assert all(v.nbytes < 4096 for v in got.values())
            print(f"{name}/{j}: x_seed {x_seed}, gaps " + ", ".join(f"{k[:-4]} {v:.2e}" for k, v in sorted(gaps.items())))
    np.savez_compressed(os.path.join(HERE, "clip_attn.npz"), **store)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("clip_attn"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
