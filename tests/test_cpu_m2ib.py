"""CLIP's M2IB row without a GPU: the reference-made fixtures (tests/golden/m2ib.npz), the restated flows (tests/m2ib_restated.py)
against them, wrapper_text_features against the reference wrapper's text features, the kernel restatements against autograd and
torch.optim.Adam, the library libxai_cm2ib.so and its header, the argument checks that need no device, the opt-in of the harness and
the CLI flags."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import clip_restated as R
import m2ib_restated as M
import abi_libs
from abi_libs import built, declared, exported, exported_elsewhere
from conftest import GOLDEN, ROOT

# The literal version pin of the key cm2ib, which tests/test_cpu_abi_libs.py reads for every key of the table (a key without one
# fails there).  It is registered here, at import, and not written into tests/abi_libs.py: a feature adds test files and leaves the
# existing ones as they are.  pytest imports every test module before it runs a test, so the whole-table tests find it; a header
# that moves has to move this line too.
assert abi_libs.PINNED.setdefault("cm2ib", (1, 0)) == (1, 0)

HEADER = os.path.join(ROOT, "include", "xai_hip_cm2ib.h")
ENTRIES = ["xai_cm2ib_adam_step_f16", "xai_cm2ib_adam_step_f32", "xai_cm2ib_max_copies", "xai_cm2ib_max_tokens", "xai_cm2ib_max_width",
           "xai_cm2ib_saliency_f32", "xai_cm2ib_sample_f16", "xai_cm2ib_sample_f32"]
FIXTURES = [(m, str(j)) for m in M.MODELS for j in range(2)]
_p, _i, _f = C.c_void_p, C.c_int, C.c_float


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "m2ib.npz"), allow_pickle=False)


_WEIGHTS, _FLOWS = {}, {}


def weights(model):
    """the stored fp16 weights of both towers"""
    if model not in _WEIGHTS:
        z = np.load(os.path.join(GOLDEN, f"m2ib_w_{model}.npz"), allow_pickle=False)
        assert all(z[k].dtype == np.float16 for k in z.files)
        _WEIGHTS[model] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _WEIGHTS[model]


def fixture_noise(G, model, tag):
    noise = M.fixture_noise(int(G[f"{model}/{tag}/noise_seed"]), model)
    assert np.array_equal(M.noise_probe(noise).numpy(), G[f"{model}/{tag}/probe"]), "torch's CPU generator draws other numbers than the fixtures'"
    return noise


def restated(G, model, tag, dtype):
    """the closed-form flow of one fixture, computed once and shared"""
    key = (model, tag, dtype)
    if key not in _FLOWS:
        res, _, _, _, heads, _, layer = M.MODELS[model]
        bits = 16 if dtype is None else 32
        x = R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), res, res)
        txt = torch.from_numpy(G[f"{model}/{tag}/txt{bits}"])
        noise = fixture_noise(G, model, tag)
        if dtype == torch.float64:
            txt, noise = M.wrapper_text(weights(model), M.fixture_ids(int(G[f"{model}/{tag}/t_seed"])), 1, dtype), noise.double()
        _FLOWS[key] = M.flow(weights(model), x, txt, noise, heads, layer, dtype)
    return _FLOWS[key]


def zoo_model(model, fp16=True, layers=None, **sizes):
    from xai_engine import zoo
    res, patch, width, n, heads, embed, _ = M.MODELS[model]
    m = zoo.clip_vit(0, **dict(dict(embed_dim=embed, image_resolution=res, vision_layers=layers or n, vision_width=width,
                                    vision_patch_size=patch, vision_heads=heads, **M.TEXT), **sizes))
    if layers is None and not sizes:
        m.load_state_dict({k: v.float() for k, v in weights(model).items()}, strict=True)
    return zoo.convert_weights_fp16(m) if fp16 else m


# ------------------------------------------------------------------------------------------------ the fixtures
def test_fixture_files_hold_every_model_and_input(G):
    assert {m: M.tokens_of(m) for m in M.MODELS} == {"five": 5, "seventeen": 17, "fifty": 50, "ten": 5}
    assert all(v[3] == 12 and v[5] == M.TEXT["transformer_width"] for v in M.MODELS.values())
    assert M.MODELS["five"][4] == 1 and M.MODELS["ten"][6] == 10 and all(v[6] == 9 for k, v in M.MODELS.items() if k != "ten")
    for model, tag in FIXTURES:
        pre = f"{model}/{tag}/"
        side = int((M.tokens_of(model) - 1) ** 0.5)
        hi = G[pre + "hi"]
        full_hi = M.full_map(hi).numpy()
        assert hi.dtype == np.float64 and hi.shape == (side, side) and G[pre + "alpha9"].shape == (M.tokens_of(model), M.MODELS[model][2])
        for bits, lo_gap, hi_gap in ((32, 1e-8, 4e-6), (16, 1e-4, 1e-2)):
            ref, gap = G[pre + f"ref{bits}"], float(G[pre + f"gap{bits}"])
            assert ref.dtype == np.float32 and ref.shape == (side, side) and not np.isnan(ref).any() and ref.max() > ref.min()
            full_ref = M.full_map(ref).double().numpy()
            again = np.abs(full_ref - full_hi).max() / np.abs(full_hi).max()
            assert abs(again - gap) <= 2.0 ** -22 and lo_gap < gap < hi_gap, (pre, bits, gap, again)
            assert M.argmax_patch(full_ref, model) == M.argmax_patch(full_hi, model)
            assert G[pre + f"txt{bits}"].shape == (1, M.MODELS[model][5]) and G[pre + f"txt{bits}"].dtype == (np.float32 if bits == 32 else np.float16)
    assert max(int(G[f"fifty/{j}/agree"]) for j in "01") >= 3
    for f in os.listdir(GOLDEN):
        if f.startswith("m2ib"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f
    for model in M.MODELS:                                                     # fp16 values on the stated grid
        assert all(torch.equal((w.float() / M.GRID).round() * M.GRID, w.float()) for w in weights(model).values())


def test_api_names_match_the_reference():
    from xai_engine import m2ib, sweep
    api = json.load(open(os.path.join(GOLDEN, "m2ib_api.json")))
    assert sorted(api) == ["m2ib_clip_map", "vision_heatmap_iba"]
    ref = dict(api["m2ib_clip_map"])
    assert (ref["vbeta"], ref["vvar"], ref["vlayer"]) == ("0.1", "1", "9")
    iba = dict(api["vision_heatmap_iba"])
    assert (iba["lr"], iba["train_steps"]) == ("1", "10")
    p = inspect.signature(m2ib.m2ib_batch).parameters
    assert list(p) == ["clipmodel", "x", "text_features", "img_hw", "layer", "beta", "steps", "lr", "copies", "noise", "seed"]
    assert (p["layer"].default, p["beta"].default, p["steps"].default, p["lr"].default, p["copies"].default) == (9, 0.1, 10, 1.0, 10)
    assert (p["img_hw"].default, p["noise"].default, p["seed"].default) == (None, "device", None)
    # vvar scales an estimator whose mean and std the bottleneck's forward never reads (iba.py:121-128): it has no counterpart
    assert "var" not in p and m2ib.MAP_SIZE == M.MAP == 224 and m2ib.INITIAL_ALPHA == 5.0
    assert (M.BETA, M.STEPS, M.LR, M.COPIES) == (0.1, 10, 1.0, 10) and "m2ib" in sweep.CLIP_ATTR_FUNCS
    assert "graphs" not in p and "no `graphs=True` is offered" in m2ib.__doc__


# ------------------------------------------------------------------------------------------------ the text tower of the wrapper
@pytest.mark.parametrize("fp16", [False, True])
def test_wrapper_text_features_are_the_reference_wrappers(G, fp16):
    """fp32: the engine's attention is written out, the reference's is nn.MultiheadAttention, so sums of at most 64 products are
    ordered differently: 64 u per GEMM through two GEMMs of a block and two projections, 1e-5 of the largest feature is generous.
    fp16: every operator rounds to 11 bits; 2^-8 of the largest feature allows eight such roundings in a row."""
    from xai_engine import m2ib
    bits = 16 if fp16 else 32
    for model in ("five", "seventeen"):
        m = zoo_model(model, fp16=fp16)
        for tag in "01":
            ids = M.fixture_ids(int(G[f"{model}/{tag}/t_seed"]))
            want = G[f"{model}/{tag}/txt{bits}"]
            got = m2ib.wrapper_text_features(m, ids)
            assert got.dtype == (torch.float16 if fp16 else torch.float32) and tuple(got.shape) == want.shape
            err = np.abs(got.float().numpy().astype(np.float64) - want.astype(np.float64)).max()
            assert err <= (2.0 ** -8 if fp16 else 1e-5) * np.abs(want.astype(np.float64)).max(), (model, tag, err)
            # not encode_text's: the causal mask, the position and the second projection all differ
            assert not torch.allclose(m.encode_text(ids).float(), got.float(), rtol=1e-2, atol=0)
    assert m.transformer.resblocks[0].attn_mask is not None                    # the model's own block keeps its mask


def test_wrapper_text_features_restated_equals_the_fixture_and_refuses_what_the_reference_cannot_do(G):
    from xai_engine import m2ib
    for model, tag in FIXTURES[:2]:
        ids = M.fixture_ids(int(G[f"{model}/{tag}/t_seed"]))
        assert torch.equal(M.wrapper_text(weights(model), ids, 1, torch.float32), torch.from_numpy(G[f"{model}/{tag}/txt32"]))
        assert torch.equal(M.wrapper_text(weights(model), ids, 1, None), torch.from_numpy(G[f"{model}/{tag}/txt16"]))
    m = zoo_model("five", embed_dim=8)
    with pytest.raises(ValueError, match="second time"):
        m2ib.wrapper_text_features(m, torch.zeros(1, 4, dtype=torch.int64))
    m = zoo_model("five")
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(1, 4), torch.zeros(1, 0, dtype=torch.int64), [[1, 2]]):
        with pytest.raises(ValueError, match="token_ids must be"):
            m2ib.wrapper_text_features(m, bad)
    with pytest.raises(ValueError, match="context length is 4"):
        m2ib.wrapper_text_features(m, torch.zeros(1, 5, dtype=torch.int64))
    with pytest.raises(TypeError, match="has no `token_embedding`"):
        m2ib.wrapper_text_features(torch.nn.Linear(2, 2), torch.zeros(1, 4, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ the restated flow
@pytest.mark.parametrize("model,tag", FIXTURES)
def test_restated_flow_agrees_with_ref_and_hi_within_the_stored_gaps(G, model, tag):
    pre = f"{model}/{tag}/"
    hi = restated(G, model, tag, torch.float64)
    assert np.abs(hi["grid"].numpy() - G[pre + "hi"]).max() <= 1e-12 * np.abs(G[pre + "hi"]).max()
    assert np.abs(hi["alpha"][0].numpy() - G[pre + "alpha9"]).max() <= 1e-9
    full_hi = M.full_map(G[pre + "hi"]).numpy()
    for bits, dtype in ((32, torch.float32), (16, None)):
        got = M.full_map(restated(G, model, tag, dtype)["grid"]).double().numpy()
        ref = M.full_map(G[pre + f"ref{bits}"]).double().numpy()
        gap = float(G[pre + f"gap{bits}"])
        bound = max(1e-5, 4 * gap) * np.abs(full_hi).max()
        assert np.abs(got - full_hi).max() <= bound and np.abs(got - ref).max() <= bound, (bits, np.abs(got - full_hi).max(), bound)
        assert M.argmax_patch(got, model) == M.argmax_patch(full_hi, model)


# ------------------------------------------------------------------------------------------------ the kernels' restatements
def _operands(B, R, L, D, seed=0, half=False):
    g = np.random.default_rng(seed)
    dt = np.float16 if half else np.float32
    alpha = (5 + g.standard_normal((B, L, D))).astype(np.float32)
    x9 = g.standard_normal((B, L, D)).astype(dt)
    eps = g.standard_normal((B, R, L, D)).astype(np.float32)
    gt = (1e-3 * g.standard_normal((B, R, L, D))).astype(dt)
    return alpha, x9, eps, gt, dt


@pytest.mark.parametrize("half", [False, True])
def test_restated_gradient_is_autograds_and_the_step_is_torchs_adam(half):
    """K89's closed-form gradient against autograd through the reference's expressions in fp64, and nine restated steps against
    torch.optim.Adam fed the restated gradients (fp32 arithmetic: 1e-6 of the largest value per step)"""
    B, Rr, L, D = 2, 10, 3, 5
    alpha, x9, eps, gt, dt = _operands(B, Rr, L, D, 1, half)
    a = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
    lamb = torch.sigmoid(a)[:, None].expand(B, Rr, L, D)
    mu, var = torch.tensor(x9.astype(np.float64))[:, None] * lamb, (1 - lamb) ** 2
    t = mu + var.sqrt() * torch.tensor(eps, dtype=torch.float64)
    cap = -0.5 * (1 + torch.log(var) - mu ** 2 - var)
    # per image: the loss whose d / dt is gt, plus beta * mean of the image's (R, L, D) capacities
    loss = (t * torch.tensor(gt.astype(np.float64))).sum() + M.BETA * cap.mean(dim=(1, 2, 3)).sum()
    want = torch.autograd.grad(loss, a)[0].numpy()
    got = M.k89_gradient(gt, eps, x9, alpha, M.BETA)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    p = torch.nn.Parameter(torch.tensor(alpha))
    opt = torch.optim.Adam([p], lr=M.LR)
    mine, m, v = alpha, np.zeros_like(alpha), np.zeros_like(alpha)
    for k in range(1, 10):
        g = M.k89_gradient(gt, eps, x9, mine, M.BETA)
        p.grad = torch.tensor(M.k89_gradient(gt, eps, x9, p.detach().numpy(), M.BETA))
        opt.step()
        mine, m, v, g2 = M.k89(gt, eps, x9, mine, m, v, M.BETA, M.adam_scalars(k))
        assert R.same(g, g2)
        assert np.abs(mine - p.detach().numpy()).max() <= 1e-5, k
    assert np.abs(mine - alpha).max() > 1                                        # lr = 1: the steps are of the order of 1


def test_restated_kernels_are_the_references_expressions_and_keep_its_nan():
    B, Rr, L, D = 1, 2, 3, 4
    alpha, x9, eps, gt, _ = _operands(B, Rr, L, D, 2)
    lam = torch.sigmoid(torch.tensor(alpha))
    want_t = (torch.tensor(x9) * lam)[:, None] + ((1 - lam) ** 2).sqrt()[:, None] * torch.tensor(eps)
    assert np.abs(M.k88(alpha, x9, eps, np.float32) - want_t.numpy()).max() <= 1e-6
    var = (1 - lam) ** 2
    want_cap = -0.5 * (1 + torch.log(var) - (torch.tensor(x9) * lam) ** 2 - var)
    cap = M.k90_cap(alpha, x9)
    assert np.abs(cap - want_cap.numpy()).max() <= 1e-5
    assert np.abs(M.k90_sum(cap) - torch.nansum(want_cap, -1)[:, 1:].numpy()).max() <= 1e-5
    # lam rounds to 1 at alpha = 20: autograd's 0 * Inf, the moments and alpha a NaN for good; the capacity +Inf - ... a NaN too
    alpha[0, 1, 2] = 20
    a = torch.tensor(alpha, requires_grad=True)
    lam = torch.sigmoid(a)
    (((torch.tensor(x9) * lam) + ((1 - lam) ** 2).sqrt() * torch.tensor(eps[:, 0])) * torch.tensor(gt[:, 0])).sum().backward()
    assert torch.isnan(a.grad[0, 1, 2]) and int(torch.isnan(a.grad).sum()) == 1
    new, m, v, g = M.k89(gt, eps, x9, alpha, np.zeros_like(alpha), np.zeros_like(alpha), M.BETA, M.adam_scalars(1))
    for arr in (new, m, v, g):
        assert np.isnan(arr[0, 1, 2]) and int(np.isnan(arr).sum()) == 1
    cap = M.k90_cap(alpha, x9)
    assert np.isinf(cap[0, 1, 2]) and np.isinf(M.k90_sum(cap)[0, 0])            # var = 0 alone: +Inf, kept by nansum
    cap = M.k90_cap(new, x9)
    assert np.isnan(cap[0, 1, 2]) and np.isfinite(M.k90_sum(cap)).all()          # a NaN alpha: the term is left out
    first, _, _, g = M.k89(gt, eps, x9, np.full_like(alpha, 5), np.zeros_like(alpha), np.zeros_like(alpha), M.BETA, M.adam_scalars(1))
    size = np.abs(g.astype(np.float64))                                          # Adam's first step is sign(g) * lr, up to adam_eps
    assert np.abs(np.abs(first - 5) - size / (size + 1e-8)).max() <= 1e-5 and ((first < 5) == (g > 0)).all()


# ------------------------------------------------------------------------------------------------ the harness and the CLI
def harness_dict(model="five", **more):
    return dict({"attr_func": "m2ib", "models": [zoo_model(model)], "img_hw": M.MODELS[model][0], "embeddings": torch.ones(2, 16),
                 "device": "cpu"}, **more)


def test_harness_serves_the_row_only_on_request():
    from xai_engine import _lib, eclip, sweep
    img = torch.zeros(3, 32, 32)
    table = torch.ones(2, 16)
    today = f"get_CLIP_attr: the row 'm2ib' needs {eclip.REFUSED['m2ib']}, which this engine does not build"
    assert today == ("get_CLIP_attr: the row 'm2ib' needs the M2IB wrapper and its tokenizer (m2ib_clip_map, testing_dict['models'][3] "
                     "and [4]), which this engine does not build")
    for td in (harness_dict(), harness_dict(clip_m2ib="modified"), harness_dict(clip_m2ib=None), {"attr_func": "m2ib"},
               harness_dict(clip_attention_rows="plain", m2ib_text_features=table),
               harness_dict(clip_surgery="plain", surgery_text_features=torch.ones(59, 16), m2ib_text_features=table)):
        with pytest.raises(NotImplementedError) as e:
            sweep.get_CLIP_attr(img, 0, td)
        assert str(e.value) == today
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):               # "plain" reaches the model, which is on the CPU here
        sweep.get_CLIP_attr(img, 1, harness_dict(clip_m2ib="plain", m2ib_text_features=table))
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):
        sweep.get_CLIP_attr(img, 1, harness_dict(clip_m2ib="plain", m2ib_text_features=table, m2ib_noise="host", m2ib_seed=3))
    with pytest.raises(ValueError, match="needs testing_dict\\['m2ib_text_features'\\]"):
        sweep.get_CLIP_attr(img, 0, harness_dict(clip_m2ib="plain"))
    for bad in (table[0], table[:, :8], [1.0]):
        with pytest.raises(ValueError, match="m2ib_text_features must be"):
            sweep.get_CLIP_attr(img, 0, harness_dict(clip_m2ib="plain", m2ib_text_features=bad))
    for bad in ("Plain", "", True, 1):
        for row in ("m2ib", "eclip", "surgery"):
            with pytest.raises(ValueError, match="clip_m2ib must be 'plain' or 'modified'"):
                sweep.get_CLIP_attr(img, 0, dict(harness_dict(clip_m2ib=bad), attr_func=row))
    with pytest.raises(ValueError, match="noise must be 'device', 'host' or a tensor"):
        sweep.get_CLIP_attr(img, 0, harness_dict(clip_m2ib="plain", m2ib_text_features=table, m2ib_noise="cpu"))
    for hw in ((32, 48), (48, 48), (16, 16)):
        with pytest.raises(NotImplementedError, match="preprocess"):
            sweep.get_CLIP_attr(torch.zeros(3, *hw), 0, harness_dict(clip_m2ib="plain", m2ib_text_features=table))
    for row in ("surgery", "game"):                                            # the opt-in does not reach the other refused rows
        with pytest.raises(NotImplementedError, match=row):
            sweep.get_CLIP_attr(img, 0, dict(harness_dict(clip_m2ib="plain", m2ib_text_features=table), attr_func=row))
    assert "m2ib" in eclip.REFUSED
    with pytest.raises(NotImplementedError, match="M2IB wrapper"):
        eclip.eclip_batch(zoo_model("five"), torch.zeros(1, 3, 32, 32), torch.zeros(1, 16), "m2ib")
    doc = sweep.get_CLIP_attr.__doc__
    assert "m2ib_text_features" in doc and "m2ib_noise" in doc and "m2ib_seed" in doc


def test_pass_refuses_before_it_needs_a_device():
    from xai_engine import _lib, m2ib
    m = zoo_model("five")
    x, txt = torch.zeros(1, 3, 32, 32), torch.zeros(16)
    for layer in (-1, 11, 12):
        with pytest.raises(ValueError, match=r"is outside 0 \.\. 10"):
            m2ib.m2ib_batch(m, x, txt, layer=layer)
    with pytest.raises(TypeError, match="layer: expected an int"):
        m2ib.m2ib_batch(m, x, txt, layer=9.0)
    for hw in ((32, 48), (64, 64)):
        with pytest.raises(NotImplementedError, match="input_resolution is 32"):
            m2ib.m2ib_batch(m, torch.zeros(1, 3, *hw), txt)
    with pytest.raises(ValueError, match=r"x must be \(B, 3, H, W\)"):
        m2ib.m2ib_batch(m, x[0], txt)
    with pytest.raises(TypeError, match="x: expected a torch.Tensor"):
        m2ib.m2ib_batch(m, None, txt)
    for bad in (torch.zeros(2, 16), torch.zeros(1, 1, 16), torch.zeros(())):
        with pytest.raises(ValueError, match=r"text_features must be \(E,\), \(1, E\) or \(1, E\)"):
            m2ib.m2ib_batch(m, x, bad)
    with pytest.raises(TypeError, match="text_features: expected a torch.Tensor"):
        m2ib.m2ib_batch(m, x, None)
    with pytest.raises(ValueError, match="text_features has 8 features, the model embeds into 16"):
        m2ib.m2ib_batch(m, x, torch.zeros(8))
    with pytest.raises(ValueError, match="steps must be >= 1"):
        m2ib.m2ib_batch(m, x, txt, steps=0)
    with pytest.raises(ValueError, match="copies must be >= 1"):
        m2ib.m2ib_batch(m, x, txt, copies=0)
    with pytest.raises(TypeError, match="seed: expected an int"):
        m2ib.m2ib_batch(m, x, txt, seed=0.5)
    with pytest.raises(ValueError, match="noise must be 'device', 'host' or a tensor"):
        m2ib.m2ib_batch(m, x, txt, noise="gpu")
    with pytest.raises(TypeError, match="noise: expected"):
        m2ib.m2ib_batch(m, x, txt, noise=3)
    for bad in (torch.zeros(10, 10, 5, 64), torch.zeros(9, 10, 5, 32), torch.zeros(2, 9, 10, 5, 64)):
        with pytest.raises(ValueError, match=r"noise must be \(9, 10, 5, 64\) or that with a leading 1"):
            m2ib.m2ib_batch(m, x, txt, noise=bad)
    with pytest.raises(TypeError, match=r"Linear has no `visual`"):
        m2ib.m2ib_batch(torch.nn.Linear(2, 2), x, txt)

    class ResNetTower(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.attnpool = torch.nn.Identity()
    resnet = torch.nn.Module()
    resnet.visual = ResNetTower()
    with pytest.raises(NotImplementedError, match="ResNet visual tower"):
        m2ib.m2ib_batch(resnet, x, txt)
    for ok in (dict(), dict(layer=0), dict(layer=10), dict(noise="host", seed=1), dict(noise=torch.zeros(9, 10, 5, 64)),
               dict(noise=torch.zeros(1, 9, 10, 5, 64)), dict(steps=1, noise=torch.zeros(0, 10, 5, 64))):
        with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):
            m2ib.m2ib_batch(m, x, txt[None] if ok else txt, **ok)
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):
        m2ib.m2ib_batch(zoo_model("five", fp16=False), x, txt)
    del m.visual.transformer.resblocks[0].attn.num_heads
    with pytest.raises(TypeError, match=r"`visual\.transformer\.resblocks\[0\]\.attn\.num_heads`"):
        m2ib.m2ib_batch(m, x, txt)


def test_cli_flags_and_their_defaults():
    from xai_engine import evaluate_clip as cli
    d = cli.build_parser().parse_args([])
    assert d.clip_m2ib == "modified" and d.m2ib_text_features is None and d.m2ib_noise == "device"
    args = cli.build_parser().parse_args(["--attr_func", "m2ib", "--clip_m2ib", "plain", "--m2ib_text_features", "t.pt", "--m2ib_noise", "host"])
    assert (args.attr_func, args.clip_m2ib, args.m2ib_text_features, args.m2ib_noise) == ("m2ib", "plain", "t.pt", "host")
    for bad in (["--clip_m2ib", "third"], ["--m2ib_noise", "gpu"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(bad)
    src = inspect.getsource(cli.main)
    assert '"clip_m2ib": args.clip_m2ib' in src and '"m2ib_text_features": m2ib_table' in src and '"m2ib_noise": args.m2ib_noise' in src


# ------------------------------------------------------------------------------------------------ the library and its header
def test_header_entries_limits_and_argument_types():
    """what is particular to libxai_cm2ib.so; what holds for every library alike is tests/test_cpu_abi_libs.py's, for the key cm2ib"""
    from xai_engine import _lib
    rec = _lib.LIBRARIES["cm2ib"]
    assert os.path.samefile(rec.header_path, HEADER)
    names = sorted(ENTRIES + ["xai_cm2ib_version", "xai_cm2ib_version_minor"])
    assert declared(HEADER) == names == sorted(rec.signatures) and all(rec.restypes[n] is _i for n in ENTRIES)
    assert exported(built("cm2ib")) == names
    lib = _lib.load("cm2ib")
    assert (lib.xai_cm2ib_max_tokens(), lib.xai_cm2ib_max_width(), lib.xai_cm2ib_max_copies()) == (4096, 8192, 1024)
    for sfx in ("f32", "f16"):
        assert rec.signatures[f"xai_cm2ib_sample_{sfx}"] == [_p, _p, _p, _i, _i, _i, _i, _p, _p]
        assert rec.signatures[f"xai_cm2ib_adam_step_{sfx}"] == [_p, _p, _p, _i, _i, _i, _i] + [_f] * 7 + [_p, _p, _p, _p]
    assert rec.signatures["xai_cm2ib_saliency_f32"] == [_p, _p, _i, _i, _i, _p, _p, _p]
    text = open(HEADER).read()
    for word in ("THE ARITHMETIC RULE", "THE NaN RULE", "THE LIMITS", "THE BOUNDS BEHIND expf AND logf", "in ascending r from +0",
                 "_single_tensor_adam", "0 * Inf = NaN", "8u relatively"):
        assert word in text, word
    make = open(os.path.join(ROOT, "image-classification-xai_amd", "csrc", "Makefile")).read()
    assert "SRCS_cm2ib := clip/clip_m2ib_kernels.hip\n" in make and "HEADER_cm2ib" not in make and "-ffp-contract=off" in make
    import __graft_entry__ as g
    assert re.search(r"import .*\bm2ib\b", inspect.getsource(g.build))
    kernel = open(os.path.join(ROOT, "image-classification-xai_amd", "csrc", "clip", "clip_m2ib_kernels.hip")).read()
    assert not re.search(r"atomic|hipMalloc|hipMemset|__builtin_amdgcn_mfma", kernel)


def test_no_other_library_exports_a_cm2ib_name():
    assert not [(o, n) for o, n in exported_elsewhere("cm2ib") if n.startswith("xai_cm2ib_")]


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """the checks come first, so a refused call needs no device: null pointers, extents, limits"""
    from xai_engine import _lib
    built("cm2ib")
    lib = _lib.load("cm2ib")
    NUL, SHAPE, UNSUP = -1, -2, -3
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    ok = dict(B=1, R=1, L=2, D=2)
    bad_extents = (dict(B=0), dict(R=0), dict(L=0), dict(D=0), dict(B=-1))
    over = (dict(B=65536), dict(R=1025), dict(L=4097), dict(D=8193))
    for sfx in ("f32", "f16"):
        def sample(alpha=p, x9=p, eps=p, t=p, **kw):
            a = dict(ok, **kw)
            return getattr(lib, f"xai_cm2ib_sample_{sfx}")(alpha, x9, eps, a["B"], a["R"], a["L"], a["D"], t, None)

        def step(gt=p, eps=p, x9=p, alpha=p, m=p, v=p, **kw):
            a = dict(ok, **kw)
            return getattr(lib, f"xai_cm2ib_adam_step_{sfx}")(gt, eps, x9, a["B"], a["R"], a["L"], a["D"], 0.1, 0.1, 0.999, 0.001, 0.03, 10.0,
                                                             1e-8, alpha, m, v, None)
        for name in ("alpha", "x9", "eps", "t"):
            assert sample(**{name: None}) == NUL, name
        for name in ("gt", "eps", "x9", "alpha", "m", "v"):
            assert step(**{name: None}) == NUL, name
        for fn in (sample, step):
            for kw in bad_extents:
                assert fn(**kw) == SHAPE, kw
            for kw in over:
                assert fn(**kw) == UNSUP, kw

    def sal(alpha=p, x9=p, out=p, B=1, L=2, D=2):
        return lib.xai_cm2ib_saliency_f32(alpha, x9, B, L, D, None, out, None)
    assert sal(alpha=None) == NUL and sal(x9=None) == NUL and sal(out=None) == NUL
    for kw in (dict(B=0), dict(L=1), dict(L=0), dict(D=0)):
        assert sal(**kw) == SHAPE, kw
    for kw in (dict(B=65536), dict(L=4097), dict(D=8193)):
        assert sal(**kw) == UNSUP, kw
    assert all(v == 0 for v in buf)                                             # nothing was launched, nothing was written


def test_wrappers_refuse_what_is_no_device_tensor():
    from xai_engine import kernels as K, _lib
    built("cm2ib")
    a, x, e = torch.zeros(1, 3, 4), torch.zeros(1, 3, 4), torch.zeros(1, 2, 3, 4)
    g, m, v = torch.zeros(1, 2, 3, 4), torch.zeros(1, 3, 4), torch.zeros(1, 3, 4)
    s = (0.1, 0.999, 0.001, 0.03, 10.0, 1e-8)
    with pytest.raises(TypeError, match="alpha: expected a torch.Tensor"):
        K.m2ib_sample(None, x, e)
    with pytest.raises(TypeError, match="alpha: expected torch.float32"):
        K.m2ib_sample(a.half(), x, e)
    with pytest.raises(TypeError, match="x9: expected torch.float32 or torch.float16"):
        K.m2ib_sample(a, x.double(), e)
    with pytest.raises(TypeError, match="eps: expected"):
        K.m2ib_sample(a, x, None)
    with pytest.raises(ValueError, match=r"alpha must be \(B, L, D\)"):
        K.m2ib_sample(a[0], x[0], e)
    with pytest.raises(ValueError, match=r"x9 must be \(1, 3, 4\) like alpha"):
        K.m2ib_sample(a, x[:, :2], e)
    with pytest.raises(ValueError, match=r"eps must be \(1, R, 3, 4\)"):
        K.m2ib_sample(a, x, e[:, :, :2])
    with pytest.raises(ValueError, match="over the limits of K88-K90"):
        K.m2ib_sample(torch.zeros(1, 1, 8193), torch.zeros(1, 1, 8193), torch.zeros(1, 1, 1, 8193))
    with pytest.raises(TypeError, match="gt: expected torch.float32"):
        K.m2ib_adam_step(g.half(), e, x, a, m, v, 0.1, *s)
    with pytest.raises(ValueError, match="gt must have the shape of eps"):
        K.m2ib_adam_step(g[:, :1], e, x, a, m, v, 0.1, *s)
    with pytest.raises(ValueError, match="m must have the shape of alpha"):
        K.m2ib_adam_step(g, e, x, a, m[:, :2], v, 0.1, *s)
    with pytest.raises(TypeError, match="v: expected torch.float32"):
        K.m2ib_adam_step(g, e, x, a, m, v.double(), 0.1, *s)
    with pytest.raises(TypeError, match="x9: expected torch.float32"):
        K.m2ib_saliency(a, x.half())
    with pytest.raises(ValueError, match="L >= 2"):
        K.m2ib_saliency(a[:, :1], x[:, :1])
    for call in (lambda: K.m2ib_sample(a, x, e), lambda: K.m2ib_sample(a, x.half(), e), lambda: K.m2ib_adam_step(g, e, x, a, m, v, 0.1, *s),
                 lambda: K.m2ib_saliency(a, x), lambda: K.m2ib_saliency(a, x, want_capacity=True)):
        with pytest.raises(_lib.XaiHipError, match="HIP device only"):
            call()
