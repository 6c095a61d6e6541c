"""CLIP's game, rollout and lrp rows without a GPU: the restated flow (tests/clip_attn_restated.py) against the reference-made fixtures
(tests/golden/clip_attn.npz), the closed forms the engine's pass rests on, the kernel restatements against plain torch expressions, the
library libxai_cattn.so and its header, the argument checks that need no device, the opt-in of the harness and the CLI flag."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import clip_attn_restated as A
import clip_restated as R
from abi_libs import built, declared, exported, exported_elsewhere
from clip_restated import spacing
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "xai_cattn.h")
ENTRIES = [f"xai_cattn_{k}_{s}" for k in ("game_map", "rollout_row", "lrp_matrices", "lrp_row") for s in ("f16", "f32")] + \
    ["xai_cattn_max_texts", "xai_cattn_max_tokens", "xai_cattn_max_width"]
CASES = (("game", 1), ("game", 2), ("rollout", 1), ("lrp", 1))
FIXTURES = [(m, str(j)) for m in A.MODELS for j in range(2)]
_p, _i, _l = C.c_void_p, C.c_int, C.c_int64
f16, f32 = np.float16, np.float32


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "clip_attn.npz"), allow_pickle=False)


_WEIGHTS = {}


def weights(model):
    if model not in _WEIGHTS:
        z = np.load(os.path.join(GOLDEN, f"clip_attn_w_{model}.npz"), allow_pickle=False)
        _WEIGHTS[model] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _WEIGHTS[model]


def fixture_x(G, model, tag):
    return R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), A.MODELS[model][0], A.MODELS[model][0])


def raw_texts(G, model, tag, T):
    return torch.from_numpy(G[f"{model}/{tag}/txt_raw/T{T}"])


def bound_vs_hi(hi, gap, out_dt):
    """the project's rule (tests/test_gpu_eclip.py:12-14)"""
    return max(float(spacing(np.abs(hi).max(), out_dt)), 4.0 * gap * float(np.abs(hi).max()))


def same_values(got, want):
    """equal values, a NaN by position; +0 and -0 are one value (a sum from +0 cannot tell them apart, torch's clamp can)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got, nan=7.0),
                                                                                                       np.nan_to_num(want, nan=7.0))


# ------------------------------------------------------------------------------------------------ the fixtures
def test_fixture_files_hold_every_model_input_and_row(G):
    sizes = {m: (v[0] // v[1]) ** 2 + 1 for m, v in A.MODELS.items()}
    assert sorted(sizes.values()) == [5, 17, 17, 65, 197] and A.MODELS["one"][4] == 1 and A.MODELS["long"][3:5] == (2, 4)
    assert all(v[4] >= 2 and v[3] == 3 for m, v in A.MODELS.items() if m in ("tiny", "mini", "wave"))
    for model, tag in FIXTURES:
        side = A.MODELS[model][0] // A.MODELS[model][1]
        for row, T in CASES:
            pre = f"{model}/{tag}/{row}/T{T}/"
            ref, hi, gap = G[pre + "ref16"], G[pre + "hi"], float(G[pre + "gap"])
            assert ref.dtype == (np.float32 if row == "rollout" else np.float16) and hi.dtype == np.float64
            assert ref.shape == hi.shape == (side, side)
            assert not np.isnan(ref).any() and (ref != 0).any() and ref.astype(np.float64).argmax() == hi.argmax()
            assert gap == np.abs(ref.astype(np.float64) - hi).max() / np.abs(hi).max() and 0 < gap < 1e-2
            assert 0 <= float(G[pre + "gap32"]) < 1e-4
            if row == "game":
                assert (ref > 0).mean() >= 0.25
        assert G[f"{model}/{tag}/txt_raw/T2"].shape == (2, A.MODELS[model][5]) and G[f"{model}/{tag}/txt_raw/T1"].dtype == np.float16
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("clip_attn"))
    for f in os.listdir(GOLDEN):
        if f.startswith("clip_attn"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= largest, f


_FLOWS = {}


def flow(G, model, tag, T, dtype):
    """([A_i], [G_i]) of the restated flow, shared among the tests"""
    key = (model, tag, T, dtype)
    if key not in _FLOWS:
        _FLOWS[key] = A.probs_and_grads(weights(model), fixture_x(G, model, tag), raw_texts(G, model, tag, T), A.MODELS[model][4], dtype)
    return _FLOWS[key]


@pytest.mark.parametrize("model", list(A.MODELS))
def test_restated_flow_in_the_references_dtype_gives_the_references_maps(G, model):
    """Bound: none.  In mixed fp16 on the CPU the restated flow makes the reference's calls in the reference's order, so every stored
    map is equal bit for bit, as the fixture script asserted (together with attn_probs and their gradients) when it ran."""
    for tag in "01":
        for T in (1, 2):
            rows = A.rows_from(*flow(G, model, tag, T, None), T)
            for row, t in CASES:
                if t == T:
                    assert rows[row].numpy().tobytes() == G[f"{model}/{tag}/{row}/T{T}/ref16"].tobytes(), (tag, row, T)


@pytest.mark.parametrize("model", list(A.MODELS))
def test_restated_flow_in_fp64_is_the_stored_high_precision_side(G, model):
    """Bound: 1e-12 relative.  `hi` was made by this very flow in fp64; only the BLAS of the machine may differ."""
    for T in (1, 2):
        rows = A.rows_from(*flow(G, model, "0", T, torch.float64), T)
        for row, t in CASES:
            if t == T:
                want = G[f"{model}/0/{row}/T{T}/hi"]
                assert np.abs(rows[row].numpy() - want).max() <= 1e-12 * np.abs(want).max(), (row, T)


# ------------------------------------------------------------------------------------------------ the closed forms
@pytest.mark.parametrize("model", list(A.MODELS))
def test_last_block_gradient_is_one_row_and_that_row_is_g_dot_v_in_fp64(G, model):
    """What the game row rests on: behind the last attention everything is token-wise and the tower reads token 0, so the gradient
    of the logits with respect to the last block's attention probabilities is exactly zero outside row 0, and row 0 is <g_h, V_h[j]>
    with g the one-row gradient.  Bound: 1e-12 relative in fp64 (the GEMM extents differ), exactly zero for the other rows."""
    heads = A.MODELS[model][4]
    probs, grads = flow(G, model, "0", 2, torch.float64)
    raw = raw_texts(G, model, "0", 2).double()
    g, v, a0 = A.one_row(weights(model), fixture_x(G, model, "0"), raw / raw.norm(dim=-1, keepdim=True), heads, torch.float64)
    L, D = v.shape
    last = grads[-1].reshape(2, heads, L, L)
    assert (last[:, :, 1:] == 0).all() and last[:, :, 0].abs().max() > 0
    closed = torch.einsum("thd,jhd->thj", g.reshape(2, heads, D // heads), v.reshape(L, heads, D // heads))
    assert (closed - last[:, :, 0]).abs().max() <= 1e-12 * last.abs().max()
    assert (a0 - probs[-1].reshape(2, heads, L, L)[0, :, 0]).abs().max() <= 1e-12


def test_row_form_of_lrp_is_the_matrix_form_in_fp64(G):
    """e_0^T (I + C_n-1) ... (I + C_0) as n vector-matrix products from the last block down against R <- R + C_i @ R from the first
    block up.  Bound: 1e-13 relative (n L-term sums of non-negative numbers in fp64, associated differently)."""
    for model in A.MODELS:
        probs, grads = flow(G, model, "0", 1, torch.float64)
        cams = [A._cam(a, g, 1)[0] for a, g in zip(probs, grads)]
        want, got = A.lrp_matrix_form(cams), A.lrp_row_form(cams)
        assert (got - want).abs().max() <= 1e-13 * want.abs().max() and got[0] >= 1 and (got >= 0).all()
        hi = G[f"{model}/0/lrp/T1/hi"]
        assert np.abs(want[1:].numpy() - hi.reshape(-1)).max() <= 1e-12 * np.abs(hi).max()
    torch.manual_seed(3)
    cams = [torch.rand(6, 6, dtype=torch.float64) for _ in range(12)]
    assert (A.lrp_row_form(cams) - A.lrp_matrix_form(cams)).abs().max() <= 1e-13 * A.lrp_matrix_form(cams).abs().max()


@pytest.mark.parametrize("model", list(A.MODELS))
def test_closed_forms_in_the_headers_arithmetic_stay_inside_the_rule_against_hi(G, model):
    """The pass the engine runs, on the CPU: the reference's half attention probabilities and gradients through the NumPy K84 and K85
    (the row form of lrp), the one-row flow in mixed fp16 through K82, the class rows through K83, each against `hi` by the rule the
    GPU test holds the device to: max|got - hi| <= max(one ulp of half at max|hi|, 4 x gap x max|hi|).  K84's matrices are the
    reference's own `cam`, value for value."""
    heads = A.MODELS[model][4]
    sd = weights(model)
    for tag in "01":
        x = fixture_x(G, model, tag)
        probs, grads = flow(G, model, tag, 1, None)
        L = probs[0].shape[-1]
        attn = np.stack([a.float().numpy() for a in probs])[:, None]
        grad = np.stack([g.float().numpy() for g in grads])[:, None]
        c = A.k84(attn, grad, f16)
        for i, (a, g) in enumerate(zip(probs, grads)):
            assert same_values(c[0, i], A._cam(a, g, 1)[0].float().numpy()), i
        got = {("lrp", 1): A.k85(c, f16)[0]}
        a0 = probs[-1][:, 0].float().numpy()[None]
        got["rollout", 1] = A.k83(a0, 1, f16)[0]
        for T in (1, 2):
            raw = raw_texts(G, model, tag, T)
            g, v, a0_one = A.one_row(sd, x, raw / raw.norm(dim=-1, keepdim=True), heads, None)
            assert g.dtype == torch.float16
            got["game", T] = A.k82(g.float().numpy()[None], v.float().numpy()[:, None], a0_one.float().numpy()[None], f16)[0]
        for (row, T), val in got.items():
            pre = f"{model}/{tag}/{row}/T{T}/"
            hi = G[pre + "hi"].reshape(-1)
            bound = bound_vs_hi(hi, float(G[pre + "gap"]), f32 if row == "rollout" else f16)
            err = float(np.abs(val.astype(np.float64) - hi).max())
            print(f"{pre}: measured {err:.3e}, bound {bound:.3e}")
            assert err <= bound and val.argmax() == hi.argmax(), pre
        assert L == (A.MODELS[model][0] // A.MODELS[model][1]) ** 2 + 1


# ------------------------------------------------------------------------------------------------ the kernel restatements
def exact_operands(seed, shape, denom, signed=True):
    """fp32 arrays of multiples of 1 / denom in [-1, 1] (or [0, 1]): sums of a few hundred of them, and of their pairwise products,
    are exact in fp32, so a sum's value does not depend on its order and a torch expression can be compared bit for bit"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-denom if signed else 0, denom + 1, shape, generator=g).float() / denom).numpy()


@pytest.mark.parametrize("dt", (f32, f16), ids=("float32", "float16"))
@pytest.mark.parametrize("H", (1, 2, 3, 12))
def test_k84_and_k85_restatements_are_the_torch_expressions(dt, H):
    """K84 against `(grad * cam).clamp(min=0).mean(dim=1)`: torch's half mean is an fp32 sum divided once and rounded once.  K85
    against `R + bmm(C, R)` on exactly summable operands, where the row form and the matrix form agree bit for bit."""
    tdt = torch.float16 if dt == f16 else torch.float32
    n, L = 3, 7
    attn = exact_operands(1, (n, 1, H, L, L), 64, signed=False)
    grad = exact_operands(2, (n, 1, H, L, L), 64)
    grad[0, 0, 0, 0, 0], grad[0, 0, 0, 0, 1], attn[0, 0, 0, 0, 1] = np.nan, -0.0, 0.5
    grad[1, 0, :, 2, 3] = -1.0                                            # every head negative: +0, not -0, and not skipped
    c = A.k84(attn, grad, dt)
    want = (torch.from_numpy(grad).to(tdt) * torch.from_numpy(attn).to(tdt)).reshape(n, H, L, L).clamp(min=0).mean(dim=1)
    assert same_values(c[0], want.float().numpy()) and np.isnan(c[0, 0, 0, 0]) and c[0, 1, 2, 3] == 0 and (c[0, 1:] > 0).any()
    # torch's mean, not a sum rounded to T and then divided: on random half operands the two differ, and K84 is the first
    torch.manual_seed(5)
    a16, g16 = torch.rand(1, 1, H, 40, 40).half(), torch.randn(1, 1, H, 40, 40).half()
    got = A.k84(a16.float().numpy(), g16.float().numpy(), f16)[0, 0]
    assert same_values(got, (g16 * a16)[0, 0].clamp(min=0).mean(dim=0).float().numpy())
    # K85: entries 0, 1/4 and 1/2 keep every product and sum of two steps a multiple of 1/16 below 8: exact in half and in fp32
    small = exact_operands(3, (1, 2, 5, 5), 2, signed=False) / f32(2)
    rel = torch.eye(5, dtype=tdt)[None]
    for i in range(2):
        rel = rel + torch.bmm(torch.from_numpy(small[:, i]).to(tdt), rel)
    assert same_values(A.k85(small, dt)[0], rel[0, 0, 1:].float().numpy())


@pytest.mark.parametrize("dt", (f32, f16), ids=("float32", "float16"))
def test_k82_and_k83_restatements_are_the_torch_expressions(dt):
    """mm_interpret's last-block arithmetic and compute_rollout_attention's on exactly summable operands (see exact_operands)"""
    tdt = torch.float16 if dt == f16 else torch.float32
    B, T, H, d, L = 2, 3, 3, 5, 9
    g = exact_operands(11, (B, T, H * d), 8)
    v = exact_operands(12, (L, B, H * d), 8)
    a0 = exact_operands(13, (B, H, L), 16, signed=False)
    v[3, 0, :] = np.abs(v[3, 0, :]) * -np.sign(g[0, 0] + 0.01)            # patch 3 of image 0, text 0: every product negative
    got = A.k82(g, v, a0, dt)
    for b in range(B):
        tg, tv, ta = (torch.from_numpy(t).to(tdt) for t in (g[b], v[:, b], a0[b]))
        grad = torch.einsum("thd,jhd->thj", tg.view(T, H, d).float(), tv.view(L, H, d).float()).to(tdt)      # exact sums: any order
        cam = (grad * ta[None]).clamp(min=0).mean(dim=1)                                                       # (T, L)
        assert same_values(got[b], cam[:, 1:].sum(0).float().numpy()), b
    a0 = exact_operands(14, (B, 2, L), 256, signed=False)                 # T * H = 4: the mean is exact, the row sum too
    got = A.k83(a0, 2, dt)
    for b in range(B):
        cam = torch.from_numpy(a0[b]).to(tdt).repeat(2, 1).reshape(4, 1, L).expand(4, L, L)
        avg = (cam.sum(dim=0) / cam.shape[0]).unsqueeze(0)
        aug = avg + torch.eye(L).expand(1, L, L)
        want = (aug / aug.sum(dim=-1, keepdim=True))[:, 0, 1:]
        assert want.dtype == torch.float32 and same_values(got[b], want[0].numpy()), b


# ------------------------------------------------------------------------------------------------ the zoo, names, the opt-in
def zoo_model(model, fp16=True):
    from xai_engine import zoo
    res, patch, width, layers, heads, embed = A.MODELS[model]
    m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=layers, vision_width=width, vision_patch_size=patch,
                     vision_heads=heads, **A.TEXT)
    return zoo.convert_weights_fp16(m) if fp16 else m


@pytest.mark.parametrize("model", list(A.MODELS))
def test_zoo_clip_with_vision_heads_loads_the_reference_state_dict_strictly(model):
    from xai_engine import zoo
    sd = weights(model)
    m = zoo_model(model)
    own = m.state_dict()
    assert set(own) == set(sd) and all(own[k].dtype == sd[k].dtype and own[k].shape == sd[k].shape for k in sd)
    m.load_state_dict(sd, strict=True)
    assert [b.attn.num_heads for b in m.visual.transformer.resblocks] == [A.MODELS[model][4]] * A.MODELS[model][3]
    p = inspect.signature(zoo.CLIP).parameters["vision_heads"]
    assert p.default is None and "vision_heads or max(1, vision_width // 64)" in inspect.getsource(zoo.CLIP.__init__)


def test_api_names_and_the_shim_leaves_the_references_names_alone():
    from xai_engine import clip_attn, sweep
    api = json.load(open(os.path.join(GOLDEN, "clip_attn_api.json")))
    assert sorted(api) == ["clip_lrp", "compute_rollout_attention", "mm_interpret"]
    assert ["start_layer", "-1"] in api["mm_interpret"] and ["start_layer", "0"] in api["clip_lrp"]
    p = inspect.signature(clip_attn.attention_rows_batch).parameters
    assert list(p) == ["clipmodel", "x", "txt_embedding", "method", "img_hw"] and p["img_hw"].default is None
    assert clip_attn.METHODS == A.ROWS == sweep.CLIP_ATTENTION_ROWS
    shim = open(os.path.join(ROOT, "image-classification-xai_amd", "util", "attribution_methods", "CLIP", "generate_emap.py")).read()
    for name in api:
        assert not re.search(rf"^def {name}\b", shim, flags=re.M), name


def harness_dict(model, row, **more):
    return dict({"attr_func": row, "models": [zoo_model(model)], "img_hw": A.MODELS[model][0], "embeddings": torch.zeros(2, 16),
                 "device": "cpu"}, **more)


def test_harness_serves_the_rows_only_on_request():
    from xai_engine import _lib, eclip, sweep
    img = torch.zeros(3, 32, 32)
    for row in A.ROWS:
        today = f"get_CLIP_attr: the row {row!r} needs {eclip.REFUSED[row]}, which this engine does not build"
        for td in (harness_dict("mini", row), harness_dict("mini", row, clip_attention_rows="modified"), {"attr_func": row}):
            with pytest.raises(NotImplementedError) as e:
                sweep.get_CLIP_attr(img, 0, td)
            assert str(e.value) == today
        with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):           # "plain" reaches the model, which is on the CPU here
            sweep.get_CLIP_attr(img, 0, harness_dict("mini", row, clip_attention_rows="plain"))
        for bad in ("Plain", "", True, 1):
            with pytest.raises(ValueError, match="clip_attention_rows must be 'plain' or 'modified'"):
                sweep.get_CLIP_attr(img, 0, harness_dict("mini", row, clip_attention_rows=bad))
        for hw in ((32, 48), (48, 48), (16, 16)):
            with pytest.raises(NotImplementedError, match="preprocess"):
                sweep.get_CLIP_attr(torch.zeros(3, *hw), 0, harness_dict("mini", row, clip_attention_rows="plain"))
    for row in ("surgery", "m2ib"):                                            # the opt-in does not reach the rows of other models
        with pytest.raises(NotImplementedError, match=row):
            sweep.get_CLIP_attr(img, 0, harness_dict("mini", row, clip_attention_rows="plain"))
    with pytest.raises(ValueError, match="clip_attention_rows"):
        sweep.get_CLIP_attr(img, 0, harness_dict("mini", "eclip", clip_attention_rows="yes"))


def test_pass_refuses_before_it_needs_a_device():
    from xai_engine import _lib, clip_attn
    m = zoo_model("mini")
    x, txt = torch.zeros(1, 3, 32, 32), torch.zeros(1, 16)
    with pytest.raises(ValueError, match="unknown row 'eclip'"):
        clip_attn.attention_rows_batch(m, x, txt, "eclip")
    with pytest.raises(ValueError, match="lrp takes one text"):
        clip_attn.attention_rows_batch(m, x, torch.zeros(2, 16), "lrp")
    with pytest.raises(ValueError, match="lrp takes one text"):
        clip_attn.attention_rows_batch(m, x, torch.zeros(1, 2, 16), "lrp")
    for hw in ((32, 48), (64, 64)):
        with pytest.raises(NotImplementedError, match="input_resolution is 32"):
            clip_attn.attention_rows_batch(m, torch.zeros(1, 3, *hw), txt, "game")
    with pytest.raises(ValueError, match=r"x must be \(B, 3, H, W\)"):
        clip_attn.attention_rows_batch(m, x[0], txt, "rollout")
    for row in A.ROWS:
        with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):
            clip_attn.attention_rows_batch(m, x, txt, row)
    with pytest.raises(TypeError, match=r"Linear has no `visual`"):
        clip_attn.attention_rows_batch(torch.nn.Linear(2, 2), x, txt, "game")
    del m.visual.transformer.resblocks[0].attn.num_heads
    with pytest.raises(TypeError, match=r"`visual\.transformer\.resblocks\[0\]\.attn\.num_heads`"):
        clip_attn.attention_rows_batch(m, x, txt, "lrp")
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):                # game reads the last block only
        clip_attn.attention_rows_batch(m, x, txt, "game")


def test_cli_flag_and_its_default():
    from xai_engine import evaluate_clip as cli
    d = cli.build_parser().parse_args([])
    assert d.clip_attention_rows == "modified"
    args = cli.build_parser().parse_args(["--attr_func", "lrp", "--clip_attention_rows", "plain"])
    assert (args.attr_func, args.clip_attention_rows) == ("lrp", "plain")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--clip_attention_rows", "hooked"])
    src = inspect.getsource(cli.main)
    assert '"clip_attention_rows": args.clip_attention_rows' in src


# ------------------------------------------------------------------------------------------------ the library and its header
def test_header_entries_limits_and_argument_types():
    """what is particular to libxai_cattn.so; what holds for every library alike is tests/test_cpu_abi_libs.py's, for the key cattn"""
    from xai_engine import _lib
    rec = _lib.LIBRARIES["cattn"]
    assert os.path.samefile(rec.header_path, HEADER)
    names = sorted(ENTRIES + ["xai_cattn_version", "xai_cattn_version_minor"])
    assert declared(HEADER) == names == sorted(rec.signatures) and all(rec.restypes[n] is _i for n in ENTRIES)
    assert not [n for n in exported(built("cattn")) if n.startswith("xai_clip_")]
    lib = _lib.load("cattn")
    assert (lib.xai_cattn_max_tokens(), lib.xai_cattn_max_width(), lib.xai_cattn_max_texts()) == (4096, 8192, 1024)
    game = [_p, _p, _l, _l, _p, _i, _i, _i, _i, _i, _p, _p]
    for sfx in ("f32", "f16"):
        assert rec.signatures[f"xai_cattn_game_map_{sfx}"] == game
        assert rec.signatures[f"xai_cattn_rollout_row_{sfx}"] == [_p, _i, _i, _i, _i, _p, _p]
        assert rec.signatures[f"xai_cattn_lrp_matrices_{sfx}"] == [_p, _p, _i, _i, _i, _i, _p, _p]
        assert rec.signatures[f"xai_cattn_lrp_row_{sfx}"] == [_p, _i, _i, _i, _p, _p]
    make = open(os.path.join(ROOT, "image-classification-xai_amd", "csrc", "Makefile")).read()
    assert "SRCS_cattn := clip/clip_attn_kernels.hip\n" in make


def test_no_other_library_exports_a_cattn_name():
    assert not [(o, n) for o, n in exported_elsewhere("cattn") if n.startswith("xai_cattn_")]


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """the checks come first, so a refused call needs no device: null pointers, extents, strides, limits"""
    from xai_engine import _lib
    built("cattn")
    lib = _lib.load("cattn")
    NUL, SHAPE, UNSUP = -1, -2, -3
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    for sfx in ("f32", "f16"):
        game, roll = getattr(lib, f"xai_cattn_game_map_{sfx}"), getattr(lib, f"xai_cattn_rollout_row_{sfx}")
        mats, row = getattr(lib, f"xai_cattn_lrp_matrices_{sfx}"), getattr(lib, f"xai_cattn_lrp_row_{sfx}")
        ok = dict(B=1, L=2, D=4, H=2, T=1)

        def g(ptrs=(p, p, p, p), ld=(4, 4), **kw):
            a = dict(ok, **kw)
            return game(ptrs[0], ptrs[1], ld[0], ld[1], ptrs[2], a["B"], a["L"], a["D"], a["H"], a["T"], ptrs[3], None)
        for k in range(4):
            assert g(ptrs=tuple(None if i == k else p for i in range(4))) == NUL, k
        for kw in (dict(B=0), dict(L=1), dict(D=0), dict(H=0), dict(T=0), dict(H=3), dict(ld=(3, 4)), dict(B=2, ld=(8, 3))):
            assert g(**kw) == SHAPE, kw
        for kw in (dict(B=65536), dict(L=4097), dict(D=8194, ld=(8194, 8194)), dict(T=1025)):
            assert g(**kw) == UNSUP, kw
        assert roll(None, 1, 1, 2, 1, p, None) == NUL and roll(p, 1, 1, 2, 1, None, None) == NUL
        for args in ((0, 1, 2, 1), (1, 0, 2, 1), (1, 1, 1, 1), (1, 1, 2, 0)):
            assert roll(p, *args, p, None) == SHAPE, args
        for args in ((65536, 1, 2, 1), (1, 8193, 2, 1), (1, 1, 4097, 1), (1, 1, 2, 1025)):
            assert roll(p, *args, p, None) == UNSUP, args
        for k in range(3):
            assert mats(*(None if i == k else p for i in range(2)), 1, 1, 1, 2, None if k == 2 else p, None) == NUL, k
        for args in ((0, 1, 1, 2), (1, 0, 1, 2), (1, 1, 0, 2), (1, 1, 1, 1)):
            assert mats(p, p, *args, p, None) == SHAPE, args
        for args in ((256, 256, 1, 2), (1, 65536, 1, 2), (1, 1, 8193, 2), (1, 1, 1, 4097)):
            assert mats(p, p, *args, p, None) == UNSUP, args
        assert row(None, 1, 1, 2, p, None) == NUL and row(p, 1, 1, 2, None, None) == NUL
        for args in ((0, 1, 2), (1, 0, 2), (1, 1, 1)):
            assert row(p, *args, p, None) == SHAPE, args
        for args in ((256, 256, 2), (1, 65536, 2), (1, 1, 4097)):
            assert row(p, *args, p, None) == UNSUP, args


def test_wrappers_refuse_what_is_no_device_tensor():
    from xai_engine import kernels as K, _lib
    built("cattn")
    v, a0, g = torch.zeros(5, 1, 8, dtype=torch.float16), torch.zeros(1, 2, 5, dtype=torch.float16), torch.zeros(1, 1, 8, dtype=torch.float16)
    c = torch.zeros(1, 2, 5, 5)
    with pytest.raises(TypeError, match="a0: expected a torch.Tensor"):
        K.clip_rollout_row(None)
    with pytest.raises(ValueError, match=r"a0 must be \(B, H, L\)"):
        K.clip_rollout_row(a0[0])
    with pytest.raises(ValueError, match=r"attn must be \(n, B, H, L, L\)"):
        K.clip_lrp_matrices(c, c)
    with pytest.raises(ValueError, match=r"c must be \(B, n, L, L\)"):
        K.clip_lrp_row(c[0])
    with pytest.raises(TypeError, match="texts: expected an int"):
        K.clip_rollout_row(a0, texts=1.0)
    for call in (lambda: K.clip_game_map(g, v, a0), lambda: K.clip_rollout_row(a0), lambda: K.clip_lrp_matrices(c[None], c[None]),
                 lambda: K.clip_lrp_row(c)):
        with pytest.raises(_lib.XaiHipError, match="HIP device only"):
            call()
