"""The CLIP Surgery row without a GPU: the restated flows (tests/surgery_restated.py) against the reference-made fixtures
(tests/golden/surgery.npz), the closed form the engine's pass follows, the kernel restatements against the torch flows, the library
libxai_csurg.so and its header, the argument checks that need no device, the opt-in of the harness and the CLI flags."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import clip_restated as R
import surgery_restated as S
from abi_libs import built, declared, exported, exported_elsewhere
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "xai_csurg.h")
ENTRIES = ["xai_csurg_lds_floats", "xai_csurg_max_texts", "xai_csurg_max_tokens", "xai_csurg_max_width", "xai_csurg_similarity_map_f32",
           "xai_csurg_vv_attention_f32", "xai_csurg_vv_waves"]
FIXTURES = [(m, str(j)) for m in S.MODELS for j in range(2)]
CASES = (S.TEXTS, 2)
_p, _i, _l, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "surgery.npz"), allow_pickle=False)


_WEIGHTS, _FEATS = {}, {}


def weights(model):
    """the stored fp16 weights of the visual tower, as the fp32 values the reference computes on"""
    if model not in _WEIGHTS:
        z = np.load(os.path.join(GOLDEN, f"surgery_w_{model}.npz"), allow_pickle=False)
        assert all(z[k].dtype == np.float16 for k in z.files)
        _WEIGHTS[model] = {k: torch.from_numpy(z[k]).float() for k in z.files}
    return _WEIGHTS[model]


def fixture_x(G, model, tag):
    return R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), S.MODELS[model][0], S.MODELS[model][0])


def fixture_txt(G, model, tag, T):
    return S.fixture_texts(int(G[f"{model}/{tag}/t_seed"]), S.TEXTS, S.MODELS[model][5])[:T]


def feats(G, model, tag, flow, dtype):
    """(1, L, E) features of a restated flow, shared among the tests"""
    key = (model, tag, flow.__name__, dtype)
    if key not in _FEATS:
        _FEATS[key] = flow(weights(model), fixture_x(G, model, tag), S.MODELS[model][4], dtype)
    return _FEATS[key]


def bound_vs_hi(hi, gap):
    """the rule lrp.npz is held to: max(1e-5, 4 x gap) of max|hi|"""
    return max(1e-5, 4.0 * gap) * float(np.abs(hi).max())


# ------------------------------------------------------------------------------------------------ the fixtures
def test_fixture_files_hold_every_model_input_and_case(G):
    sizes = {m: (v[0] // v[1]) ** 2 + 1 for m, v in S.MODELS.items()}
    assert sizes == {"six": 17, "wave": 65, "one": 17, "long": 197} and S.MODELS["one"][2:5] == (64, 7, 1)
    assert S.MODELS["six"][3] == S.MODELS["long"][3] == S.DUAL and S.MODELS["wave"][3] == 7
    for model, tag in FIXTURES:
        res, patch, _, _, _, embed = S.MODELS[model]
        side = res // patch
        for T in CASES:
            pre = f"{model}/{tag}/T{T}/"
            ref, hi, gap = G[pre + "ref32"], G[pre + "hi"], float(G[pre + "gap"])
            assert ref.dtype == np.float32 and hi.dtype == np.float64 and ref.shape == hi.shape == (side, side)
            assert not np.isnan(ref).any() and ref.min() == 0 and ref.max() == 1 and ref.argmax() == hi.argmax()
            # gap recomputed: it was taken at the image size, from the map clip_surgery_map returned, whose last step is torch's
            # bilinear resize of `ref32`; that step on this CPU may round the last bit differently (2^-23 on maps in [0, 1])
            full_ref, full_hi = S.full_map(ref, (res, res)).double().numpy(), S.full_map(hi, (res, res)).numpy()
            again = np.abs(full_ref - full_hi).max() / np.abs(full_hi).max()
            assert abs(again - gap) <= 2.0 ** -23 and 1e-8 < gap < 1e-6
            assert full_ref.argmax() == full_hi.argmax()
        assert G[f"{model}/{tag}/feats/ref32"].shape == G[f"{model}/{tag}/feats/hi"].shape == (sizes[model], embed)
        assert G[f"{model}/{tag}/feats/ref32"].dtype == np.float32 and G[f"{model}/{tag}/feats/hi"].dtype == np.float64
    one = G["six/0/T1/ref32"]
    assert one.shape == (4, 4) and np.isnan(one).all()
    for f in os.listdir(GOLDEN):
        if f.startswith("surgery"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f
    api = json.load(open(os.path.join(GOLDEN, "surgery_api.json")))
    assert sorted(api) == ["clip_feature_surgery", "clip_surgery_map", "get_similarity_map"]
    assert [n for n, _ in api["clip_surgery_map"]] == ["model", "image", "texts", "device"] and ["t", "2"] in api["clip_feature_surgery"]


@pytest.mark.parametrize("model", list(S.MODELS))
def test_restated_dual_path_in_fp64_is_the_stored_high_precision_side(G, model):
    """Bound: 1e-12 relative.  `hi` was made by this very flow in fp64; only the BLAS of the machine may differ."""
    res = S.MODELS[model][0]
    for tag in "01":
        f = feats(G, model, tag, S.dual_path, torch.float64)
        want = G[f"{model}/{tag}/feats/hi"]
        assert np.abs(f[0].numpy() - want).max() <= 1e-12 * np.abs(want).max()
        for T in CASES:
            grid = S.reference_map(f, fixture_txt(G, model, tag, T).double(), (res, res))[1][0, :, :, 0].numpy()
            want = G[f"{model}/{tag}/T{T}/hi"]
            assert np.abs(grid - want).max() <= 1e-12 * np.abs(want).max(), (tag, T)


@pytest.mark.parametrize("flow", [S.dual_path, S.closed_features], ids=["dual_path", "closed_form"])
@pytest.mark.parametrize("model", list(S.MODELS))
def test_restated_flows_in_fp32_are_within_the_references_own_gap(G, model, flow):
    """Bound: max(1e-5, 4 x gap) of max|hi|, gap the reference's own fp32-to-fp64 distance stored in the fixture.  The dual path is
    the reference's sequence of operations; the closed form is what the GPU path follows: one GEMM with K = 6 D, sim without the
    (L, T, E) tensor."""
    res = S.MODELS[model][0]
    for tag in "01":
        f = feats(G, model, tag, flow, torch.float32)
        assert f.dtype == torch.float32
        for T in CASES:
            txt = fixture_txt(G, model, tag, T)
            hi, gap = S.full_map(G[f"{model}/{tag}/T{T}/hi"], (res, res)).numpy(), float(G[f"{model}/{tag}/T{T}/gap"])
            if flow is S.dual_path:
                got = S.reference_map(f, txt, (res, res))[0][0, :, :, 0]
            else:
                got = S.closed_map(f, txt, (res, res))[0, 0]
            assert np.abs(got.double().numpy() - hi).max() <= bound_vs_hi(hi, gap), (tag, T)
            assert int(got.argmax()) == int(hi.argmax()), (tag, T)


def test_one_text_gives_the_references_all_nan_map(G):
    f = feats(G, "six", "0", S.closed_features, torch.float32)
    txt = fixture_txt(G, "six", "0", 1)
    assert torch.isnan(S.closed_map(f, txt, (32, 32))).all() and torch.isnan(S.reference_map(f, txt, (32, 32))[0]).all()
    out, w = S.k87(f.numpy(), txt.numpy())
    assert np.isnan(out).all() and w.tolist() == [[1.0]]


# ------------------------------------------------------------------------------------------------ the kernel restatements
@pytest.mark.parametrize("model", ["six", "one"])
def test_numpy_k86_is_the_torch_vv_attention(G, model):
    """Bound: 1e-5 of max|.|: fp32 sums of d and L terms in another order, and another exp."""
    heads = S.MODELS[model][4]
    v = S.v_thirds(weights(model), fixture_x(G, model, "0"), heads, torch.float32)              # (6, L, 1, D)
    n, L, _, D = v.shape
    d = D // heads
    scores, p, out = S.k86(v.numpy(), heads)
    vh = v.double().reshape(n, L, heads, d).permute(0, 2, 1, 3)
    s = (vh @ vh.transpose(-2, -1)) * d ** -0.5
    want = (s.softmax(-1) @ vh).transpose(1, 2).reshape(n, L, D)
    assert np.abs(scores[:, 0] - s.numpy()).max() <= 1e-5 * s.abs().max()
    assert np.array_equal(scores, np.swapaxes(scores, -1, -2))
    assert np.abs(p.sum(-1) - 1).max() <= 1e-5
    assert np.abs(out[:, 0] - want.numpy()).max() <= 1e-5 * want.abs().max()
    assert S.k86_bound(p, v.numpy(), heads).shape == out.shape


@pytest.mark.parametrize("model", ["six", "long"])
def test_numpy_k87_is_the_closed_similarity_and_the_references_map(G, model):
    """Bound: max(1e-5, 4 x gap) against the fp64 side, as for the flows."""
    res, patch = S.MODELS[model][:2]
    side = res // patch
    f = feats(G, model, "1", S.closed_features, torch.float32)
    for T in CASES:
        txt = fixture_txt(G, model, "1", T)
        out, w = S.k87(f.numpy(), txt.numpy(), texts_out=2)
        want = S.closed_similarity(f.double(), txt.double(), 2).numpy()
        assert out.shape == (1, 2, side * side) and np.abs(out - want).max() <= 1e-5
        hi, gap = G[f"{model}/1/T{T}/hi"], float(G[f"{model}/1/T{T}/gap"])
        assert np.abs(out[0, 0].reshape(side, side) - hi).max() <= bound_vs_hi(hi, gap)
        p = ((f[0, :1].double() / f[0].double().norm(dim=0)) @ txt.double().t() * 2).softmax(-1)
        w64 = (p / p.mean()).numpy()
        assert np.abs(w - w64).max() <= 1e-5 * np.abs(w64).max() and S.k87_w_bound(w64).shape == w.shape
        again, _ = S.k87(f.numpy(), txt.numpy(), texts_out=2, w=w)
        assert R.same(again, out)


# ------------------------------------------------------------------------------------------------ the zoo, names, the opt-in
def zoo_model(model, fp16=True, layers=None):
    from xai_engine import zoo
    res, patch, width, n, heads, embed = S.MODELS[model]
    m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=layers or n, vision_width=width, vision_patch_size=patch,
                     vision_heads=heads, **S.TEXT)
    if layers is None:
        missing = m.load_state_dict(weights(model), strict=False)
        assert not missing.unexpected_keys and not [k for k in missing.missing_keys if k.startswith("visual.")]
    return zoo.convert_weights_fp16(m) if fp16 else m


def test_api_names(G):
    from xai_engine import surgery, sweep
    p = inspect.signature(surgery.surgery_batch).parameters
    assert list(p) == ["clipmodel", "x", "text_features", "img_hw", "texts_out"] and p["img_hw"].default is None and p["texts_out"].default == 1
    assert surgery.DUAL_BLOCKS == S.DUAL == 6 and "surgery" in sweep.CLIP_ATTR_FUNCS
    assert "350 MB" in surgery.surgery_batch.__doc__ and callable(surgery.clear_cache)


def harness_dict(model, **more):
    return dict({"attr_func": "surgery", "models": [zoo_model(model)], "img_hw": S.MODELS[model][0], "embeddings": torch.ones(2, 16),
                 "device": "cpu"}, **more)


def test_harness_serves_the_row_only_on_request():
    from xai_engine import _lib, eclip, sweep
    img = torch.zeros(3, 32, 32)
    ctx = torch.ones(59, 16)
    today = f"get_CLIP_attr: the row 'surgery' needs {eclip.REFUSED['surgery']}, which this engine does not build"
    for td in (harness_dict("six"), harness_dict("six", clip_surgery="modified"), harness_dict("six", clip_surgery=None),
               harness_dict("six", clip_attention_rows="plain", surgery_text_features=ctx), {"attr_func": "surgery"}):
        with pytest.raises(NotImplementedError) as e:
            sweep.get_CLIP_attr(img, 0, td)
        assert str(e.value) == today
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):               # "plain" reaches the model, which is on the CPU here
        sweep.get_CLIP_attr(img, 0, harness_dict("six", clip_surgery="plain", surgery_text_features=ctx))
    with pytest.raises(ValueError, match="surgery_text_features"):
        sweep.get_CLIP_attr(img, 0, harness_dict("six", clip_surgery="plain"))
    for bad in (ctx[0], ctx[:, :8], [1.0]):
        with pytest.raises(ValueError, match="surgery_text_features must be"):
            sweep.get_CLIP_attr(img, 0, harness_dict("six", clip_surgery="plain", surgery_text_features=bad))
    for bad in ("Plain", "", True, 1):
        for row in ("surgery", "eclip", "game"):
            with pytest.raises(ValueError, match="clip_surgery must be 'plain' or 'modified'"):
                sweep.get_CLIP_attr(img, 0, dict(harness_dict("six", clip_surgery=bad), attr_func=row))
    for hw in ((32, 48), (48, 48), (16, 16)):
        with pytest.raises(NotImplementedError, match="preprocess"):
            sweep.get_CLIP_attr(torch.zeros(3, *hw), 0, harness_dict("six", clip_surgery="plain", surgery_text_features=ctx))
    for row in ("m2ib", "game"):                                               # the opt-in does not reach the other refused rows
        with pytest.raises(NotImplementedError, match=row):
            sweep.get_CLIP_attr(img, 0, dict(harness_dict("six", clip_surgery="plain", surgery_text_features=ctx), attr_func=row))
    assert "surgery" in eclip.REFUSED
    with pytest.raises(NotImplementedError, match="CLIP Surgery model"):
        eclip.eclip_batch(zoo_model("six"), torch.zeros(1, 3, 32, 32), torch.zeros(1, 16), "surgery")
    doc = sweep.get_CLIP_attr.__doc__
    assert "prompt-ensembles the caption" in doc and "surgery_text_features" in doc


def test_pass_refuses_before_it_needs_a_device():
    from xai_engine import _lib, surgery
    m = zoo_model("six")
    x, txt = torch.zeros(1, 3, 32, 32), torch.zeros(3, 16)
    with pytest.raises(ValueError, match="has 5 blocks; the dual path takes the last 6"):
        surgery.surgery_batch(zoo_model("six", layers=5), x, txt)
    for hw in ((32, 48), (64, 64)):
        with pytest.raises(NotImplementedError, match="input_resolution is 32"):
            surgery.surgery_batch(m, torch.zeros(1, 3, *hw), txt)
    with pytest.raises(ValueError, match=r"x must be \(B, 3, H, W\)"):
        surgery.surgery_batch(m, x[0], txt)
    with pytest.raises(TypeError, match="x: expected a torch.Tensor"):
        surgery.surgery_batch(m, None, txt)
    for bad in (txt[0], torch.zeros(2, 3, 16), torch.zeros(1, 1, 3, 16), torch.zeros(0, 16)):
        with pytest.raises(ValueError, match=r"text_features must be \(T, E\) or \(1, T, E\)"):
            surgery.surgery_batch(m, x, bad)
    with pytest.raises(TypeError, match="text_features: expected a torch.Tensor"):
        surgery.surgery_batch(m, x, None)
    with pytest.raises(ValueError, match="text_features has 8 features, the model embeds into 16"):
        surgery.surgery_batch(m, x, torch.zeros(3, 8))
    with pytest.raises(ValueError, match="texts_out = 4 of T = 3"):
        surgery.surgery_batch(m, x, txt, texts_out=4)
    with pytest.raises(ValueError, match="texts_out must be >= 1"):
        surgery.surgery_batch(m, x, txt, texts_out=0)
    with pytest.raises(TypeError, match=r"Linear has no `visual`"):
        surgery.surgery_batch(torch.nn.Linear(2, 2), x, txt)

    class ResNetTower(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.attnpool = torch.nn.Identity()
    resnet = torch.nn.Module()
    resnet.visual = ResNetTower()
    with pytest.raises(NotImplementedError, match="ResNet visual tower"):
        surgery.surgery_batch(resnet, x, txt)
    for t in (txt, txt[:1], txt[None]):                                        # T = 1 is not refused
        with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):
            surgery.surgery_batch(m, x, t)
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):
        surgery.surgery_batch(zoo_model("six", fp16=False), x, txt)
    assert surgery.cached_towers() == 0                                        # nothing was copied for a call that was refused
    del m.visual.transformer.resblocks[0].attn.num_heads
    with pytest.raises(TypeError, match=r"`visual\.transformer\.resblocks\[0\]\.attn\.num_heads`"):
        surgery.surgery_batch(m, x, txt)


def test_cli_flags_and_their_defaults():
    from xai_engine import evaluate_clip as cli
    d = cli.build_parser().parse_args([])
    assert d.clip_surgery == "modified" and d.surgery_text_features is None and d.clip_attention_rows == "modified"
    args = cli.build_parser().parse_args(["--attr_func", "surgery", "--clip_surgery", "plain", "--surgery_text_features", "ctx.pt"])
    assert (args.attr_func, args.clip_surgery, args.surgery_text_features) == ("surgery", "plain", "ctx.pt")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--clip_surgery", "third"])
    src = inspect.getsource(cli.main)
    assert '"clip_surgery": args.clip_surgery' in src and '"surgery_text_features": context' in src
    assert "torch.randn(59, embed" in src


# ------------------------------------------------------------------------------------------------ the library and its header
def test_header_entries_limits_and_argument_types():
    """what is particular to libxai_csurg.so; what holds for every library alike is tests/test_cpu_abi_libs.py's, for the key csurg"""
    from xai_engine import _lib
    rec = _lib.LIBRARIES["csurg"]
    assert os.path.samefile(rec.header_path, HEADER)
    names = sorted(ENTRIES + ["xai_csurg_version", "xai_csurg_version_minor"])
    assert declared(HEADER) == names == sorted(rec.signatures) and all(rec.restypes[n] is _i for n in ENTRIES)
    assert not [n for n in names if n.endswith(("_f16", "_f64"))]              # fp32 is the reference's dtype for this row
    assert not [n for n in exported(built("csurg")) if n.startswith(("xai_clip_", "xai_cattn_"))]
    lib = _lib.load("csurg")
    assert (lib.xai_csurg_max_tokens(), lib.xai_csurg_max_width(), lib.xai_csurg_max_texts()) == (4096, 8192, 1024)
    assert (lib.xai_csurg_lds_floats(), lib.xai_csurg_vv_waves()) == (16384, 4)
    assert rec.signatures["xai_csurg_vv_attention_f32"] == [_p, _l, _l, _l, _i, _i, _i, _i, _i, _f, _p, _p, _p]
    assert rec.signatures["xai_csurg_similarity_map_f32"] == [_p, _p, _l, _i, _i, _i, _i, _i, _p, _p, _p]
    text = open(HEADER).read()
    for word in ("THE ARITHMETIC RULE", "THE LIMITS", "THE BOUND AFTER THE FIRST EXP", "THE BOUND OF K87's w", "in ascending c from +0",
                 "in ascending j from +0", "XAI_CSURG_LDS_FLOATS", "L <= 237 at d = 64"):
        assert word in text, word
    make = open(os.path.join(ROOT, "image-classification-xai_amd", "csrc", "Makefile")).read()
    assert "SRCS_csurg := clip/clip_surgery_kernels.hip\n" in make and "-ffp-contract=off" in make
    import __graft_entry__ as g
    assert re.search(r"import .*\bsurgery\b", inspect.getsource(g.build))
    kernel = open(os.path.join(ROOT, "image-classification-xai_amd", "csrc", "clip", "clip_surgery_kernels.hip")).read()
    assert not re.search(r"atomic|hipMalloc|hipMemset|__builtin_amdgcn_mfma", kernel)


def test_no_other_library_exports_a_csurg_name():
    assert not [(o, n) for o, n in exported_elsewhere("csurg") if n.startswith("xai_csurg_")]


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """the checks come first, so a refused call needs no device: null pointers, extents, strides, limits"""
    from xai_engine import _lib
    built("csurg")
    lib = _lib.load("csurg")
    NUL, SHAPE, UNSUP = -1, -2, -3
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    ok = dict(n=1, B=1, L=2, D=4, H=2)

    def vv(v=p, out=p, ld=(8, 4, 4), **kw):
        a = dict(ok, **kw)
        return lib.xai_csurg_vv_attention_f32(v, ld[0], ld[1], ld[2], a["n"], a["B"], a["L"], a["D"], a["H"], 0.5, None, out, None)
    assert vv(v=None) == NUL and vv(out=None) == NUL
    for kw in (dict(n=0), dict(B=0), dict(L=1), dict(D=0), dict(H=0), dict(H=3), dict(ld=(8, 3, 4)), dict(B=2, ld=(8, 8, 3)),
               dict(n=2, ld=(3, 4, 4))):
        assert vv(**kw) == SHAPE, kw
    for kw in (dict(B=65536), dict(n=256, B=256, ld=(1 << 20, 1024, 4)), dict(L=4097), dict(D=8194, H=8194, ld=(1 << 20, 8194, 8194)),
               dict(H=65536, D=65536, ld=(1 << 20, 65536, 65536))):
        assert vv(**kw) == UNSUP, kw
    # the LDS limit: L * (d + 1 + 4) <= 16384 floats
    assert 237 * 69 <= 16384 < 238 * 69
    assert vv(L=238, D=64, H=1, ld=(1 << 20, 64, 64)) == UNSUP and vv(L=238, D=128, H=2, ld=(1 << 20, 128, 128)) == UNSUP
    assert vv(L=2731, D=1, H=1, ld=(1 << 20, 1, 1)) == UNSUP

    def sm(F=p, txt=p, out=p, ld=0, B=1, L=2, E=4, T=2, T_out=1):
        return lib.xai_csurg_similarity_map_f32(F, txt, ld, B, L, E, T, T_out, None, out, None)
    assert sm(F=None) == NUL and sm(txt=None) == NUL and sm(out=None) == NUL
    for kw in (dict(B=0), dict(L=1), dict(E=0), dict(T=0), dict(T_out=0), dict(T_out=3), dict(ld=-1), dict(ld=7), dict(B=2, ld=4)):
        assert sm(**kw) == SHAPE, kw
    for kw in (dict(B=65536), dict(L=4097), dict(E=8193), dict(T=1025), dict(E=8192, T=2), dict(E=7681, T=1023)):
        assert sm(**kw) == UNSUP, kw


def test_wrappers_refuse_what_is_no_device_tensor():
    from xai_engine import kernels as K, _lib
    built("csurg")
    v, f, t = torch.zeros(6, 5, 1, 8), torch.zeros(1, 5, 16), torch.zeros(3, 16)
    with pytest.raises(TypeError, match="v: expected a torch.Tensor"):
        K.clip_vv_attention(None, 2)
    with pytest.raises(TypeError, match="v: expected torch.float32"):
        K.clip_vv_attention(v.half(), 2)
    with pytest.raises(TypeError, match="heads: expected an int"):
        K.clip_vv_attention(v, 2.0)
    with pytest.raises(ValueError, match=r"v must be \(n, L, B, D\)"):
        K.clip_vv_attention(v[0], 2)
    with pytest.raises(ValueError, match="heads dividing D"):
        K.clip_vv_attention(v, 3)
    with pytest.raises(ValueError, match="over the limits of K86"):
        K.clip_vv_attention(torch.zeros(1, 238, 1, 64), 1)
    with pytest.raises(TypeError, match="features: expected a torch.Tensor"):
        K.clip_surgery_similarity(None, t)
    with pytest.raises(TypeError, match="txt: expected torch.float32"):
        K.clip_surgery_similarity(f, t.double())
    with pytest.raises(ValueError, match=r"features must be \(B, L, E\)"):
        K.clip_surgery_similarity(f[0], t)
    with pytest.raises(ValueError, match=r"txt must be \(T, 16\) or \(1, T, 16\)"):
        K.clip_surgery_similarity(f, t[:, :8])
    with pytest.raises(ValueError, match="texts_out = 4 of T = 3"):
        K.clip_surgery_similarity(f, t, texts_out=4)
    with pytest.raises(ValueError, match="over the limits of K87"):
        K.clip_surgery_similarity(torch.zeros(1, 2, 8192), torch.zeros(1, 8192))
    for call in (lambda: K.clip_vv_attention(v, 2), lambda: K.clip_vv_attention(v, 1, want_scores=True),
                 lambda: K.clip_surgery_similarity(f, t), lambda: K.clip_surgery_similarity(f, t[None], texts_out=3, want_weights=True)):
        with pytest.raises(_lib.XaiHipError, match="HIP device only"):
            call()
