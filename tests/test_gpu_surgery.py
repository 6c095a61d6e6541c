"""The CLIP Surgery row on the device: the driver xai_engine/surgery.py and sweep.get_CLIP_attr (with the opt-in) against the
reference-made fixtures (tests/golden/surgery.npz), the batch rule, the fp32 copy of a mixed-fp16 model, and the bilinear step.

Bound, the rule lrp.npz is held to.  The driver against `hi` (the dual-path flow restated in fp64 on the fp16-valued weights, resized
to the image size in fp64): max|got - hi| <= max(1e-5, 4 x gap) x max|hi|, gap the reference's own fp32-to-fp64 distance stored
beside `hi`; the 4 x and the 1e-5 floor are the project's margin for fp32 flows whose order of summation differs from the
reference's (the one GEMM with K = 6 D, the sums of K86 and K87, the device's GEMMs).  Every measured error is written to
profiles/surgery_parity.json."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_restated as R
import surgery_restated as S
from clip_restated import same
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = (S.TEXTS, 2)
_LEDGER = []


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "surgery.npz"), allow_pickle=False)


@pytest.fixture(scope="module", autouse=True)
def _write_the_ledger():
    yield
    path = os.path.join(ROOT, "profiles", "surgery_parity.json")
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "comparisons": _LEDGER}, f, indent=1)
        f.write("\n")


_MODELS, _HI = {}, {}


def dev_model(model, fp16=True):
    """the zoo's CLIP with the fixture's visual tower on the device, frozen: in OpenAI's mixed fp16, or (fp16=False) the same
    fp16-valued weights as fp32, what evaluate_clip's --clip_fp32 builds"""
    if (model, fp16) not in _MODELS:
        from xai_engine import zoo
        res, patch, width, layers, heads, embed = S.MODELS[model]
        m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=layers, vision_width=width, vision_patch_size=patch,
                         vision_heads=heads, **S.TEXT)
        if fp16:
            zoo.convert_weights_fp16(m)
        z = np.load(os.path.join(GOLDEN, f"surgery_w_{model}.npz"), allow_pickle=False)
        missing = m.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files}, strict=False)
        assert not missing.unexpected_keys and not [k for k in missing.missing_keys if k.startswith("visual.")]
        _MODELS[model, fp16] = m.to(DEV).eval()
    return _MODELS[model, fp16]


def fixture_x(G, model, tag):
    return R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), S.MODELS[model][0], S.MODELS[model][0])


def fixture_txt(G, model, tag, T):
    return S.fixture_texts(int(G[f"{model}/{tag}/t_seed"]), S.TEXTS, S.MODELS[model][5])[:T]


def hi_map(G, model, tag, T):
    """`hi` at the image size: the stored grid through get_similarity_map's resize in fp64, computed once"""
    key = (model, tag, T)
    if key not in _HI:
        res = S.MODELS[model][0]
        _HI[key] = S.full_map(G[f"{model}/{tag}/T{T}/hi"], (res, res)).numpy()
    return _HI[key]


def bound_vs_hi(hi, gap):
    return max(1e-5, 4.0 * gap) * float(np.abs(hi).max())


def record(name, got, hi, bound):
    err = float(np.abs(np.asarray(got, np.float64) - hi).max())
    _LEDGER.append({"name": name, "measured": err, "bound": bound, "max_abs_hi": float(np.abs(hi).max())})
    print(f"{name}: measured {err:.3e}, bound {bound:.3e}")
    return err


@pytest.mark.parametrize("fp16", [True, False], ids=["mixed_fp16", "fp32"])
@pytest.mark.parametrize("model", list(S.MODELS))
def test_surgery_batch_agrees_with_hi_and_its_argmax_for_every_fixture(G, model, fp16):
    """L = 17, 65 (one past a wave) and 197, H = 1 and 2, d = 16, 32 and 64, the dual path from block 0 and from block 1; T = 60
    and T = 2"""
    from xai_engine import surgery
    m = dev_model(model, fp16)
    res = S.MODELS[model][0]
    for tag in "01":
        x = fixture_x(G, model, tag)
        for T in CASES:
            pre = f"{model}/{tag}/T{T}/"
            hi, gap = hi_map(G, model, tag, T), float(G[pre + "gap"])
            got = surgery.surgery_batch(m, x, fixture_txt(G, model, tag, T))
            assert got.dtype == torch.float32 and tuple(got.shape) == (1, res, res) and got.is_cuda
            got = got[0].cpu().numpy()
            bound = bound_vs_hi(hi, gap)
            assert record(f"surgery_batch/{pre}{'fp16' if fp16 else 'fp32'}", got, hi, bound) <= bound, pre
            assert got.argmax() == hi.argmax(), pre


def test_image_features_agree_with_the_stored_features(G):
    """Bound: max(1e-5, 4 x the reference's own feature gap) of max|hi|, the same rule one step earlier"""
    from xai_engine import surgery
    for model in S.MODELS:
        ref, hi = G[f"{model}/0/feats/ref32"], G[f"{model}/0/feats/hi"]
        gap = float(np.abs(ref - hi).max() / np.abs(hi).max())
        got = surgery.image_features(dev_model(model), fixture_x(G, model, "0"))
        assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + hi.shape
        bound = bound_vs_hi(hi, gap)
        assert record(f"image_features/{model}/0", got[0].cpu().numpy(), hi, bound) <= bound, model


def test_texts_out_returns_the_maps_of_the_first_texts(G):
    from xai_engine import surgery
    m, x, txt = dev_model("wave"), fixture_x(G, "wave", "0"), fixture_txt(G, "wave", "0", S.TEXTS)
    three = surgery.surgery_batch(m, x, txt, texts_out=3)
    assert tuple(three.shape) == (1, 3, 64, 64)
    assert same(three[:, 0].cpu().numpy(), surgery.surgery_batch(m, x, txt).cpu().numpy())
    want = S.closed_map(torch.from_numpy(G["wave/0/feats/hi"])[None], txt.double(), (64, 64), texts_out=3)[0].numpy()
    assert np.abs(three[0].cpu().numpy() - want).max() <= bound_vs_hi(want, float(G["wave/0/T60/gap"]))


def test_one_text_gives_the_references_all_nan_map(G):
    from xai_engine import surgery
    assert np.isnan(G["six/0/T1/ref32"]).all()
    got = surgery.surgery_batch(dev_model("six"), fixture_x(G, "six", "0"), fixture_txt(G, "six", "0", 1))
    assert tuple(got.shape) == (1, 32, 32) and torch.isnan(got).all()
    got = surgery.surgery_batch(dev_model("six"), fixture_x(G, "six", "0"), fixture_txt(G, "six", "0", 1), img_hw=32)
    assert tuple(got.shape) == (1, 32, 32) and torch.isnan(got).all()


def test_every_image_of_a_batch_has_the_bytes_of_its_own_call(G):
    from xai_engine import surgery
    for model in ("six", "one"):
        m = dev_model(model)
        x = torch.cat([fixture_x(G, model, "0"), fixture_x(G, model, "1")])
        shared = fixture_txt(G, model, "0", S.TEXTS)
        both = surgery.surgery_batch(m, x, shared, texts_out=2)
        for b in range(2):
            assert same(both[b:b + 1].cpu().numpy(), surgery.surgery_batch(m, x[b:b + 1], shared, texts_out=2).cpu().numpy()), (model, b)
        own = torch.stack([fixture_txt(G, model, "0", 2), fixture_txt(G, model, "1", 2)])
        both = surgery.surgery_batch(m, x, own)
        for b in range(2):
            assert same(both[b:b + 1].cpu().numpy(), surgery.surgery_batch(m, x[b:b + 1], own[b]).cpu().numpy()), (model, b)
        assert same(both.cpu().numpy(), surgery.surgery_batch(m, x, own).cpu().numpy())          # and the same bytes on a second run


def test_a_mixed_fp16_model_and_its_fp32_twin_give_the_same_bytes_and_clear_cache_frees_the_copy(G):
    from xai_engine import surgery
    surgery.clear_cache()
    half, full = dev_model("wave"), dev_model("wave", fp16=False)
    assert half.visual.conv1.weight.dtype == torch.float16 and full.visual.conv1.weight.dtype == torch.float32
    x, txt = fixture_x(G, "wave", "1"), fixture_txt(G, "wave", "1", S.TEXTS)
    a = surgery.surgery_batch(full, x, txt)
    assert surgery.cached_towers() == 0                                        # an fp32 model needs no copy
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    b = surgery.surgery_batch(half, x, txt)
    assert surgery.cached_towers() == 1 and half.visual.conv1.weight.dtype == torch.float16
    assert same(a.cpu().numpy(), b.cpu().numpy())
    tower = surgery._FP32_TOWERS[half]
    assert surgery.surgery_batch(half, x, txt) is not None and surgery._FP32_TOWERS[half] is tower      # made once
    nbytes = sum(p.numel() * 4 for p in half.visual.parameters())
    del b, tower
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() >= before + nbytes
    surgery.clear_cache()
    assert surgery.cached_towers() == 0 and torch.cuda.memory_allocated() < before + nbytes


def test_the_harness_row_with_the_opt_in(G):
    """get_CLIP_attr: text 0 from the embedding table, the context rows from surgery_text_features, both normalised there; the
    harness's resize to img_hw and abs behind the map"""
    from xai_engine import sweep
    model, tag = "six", "0"
    m = dev_model(model)
    txt = fixture_txt(G, model, tag, S.TEXTS)
    emb = torch.stack([torch.zeros(16), 3.0 * txt[0]]).to(DEV)                 # the target class is row 1; the rows are not normalised
    img = R.fixture_image(int(G[f"{model}/{tag}/x_seed"]), 32, 32)
    td = {"attr_func": "surgery", "models": [m], "img_hw": 32, "embeddings": emb, "device": DEV, "clip_surgery": "plain",
          "surgery_text_features": 0.5 * txt[1:]}
    got = sweep.get_CLIP_attr(img, 1, td)
    hi, gap = hi_map(G, model, tag, S.TEXTS), float(G[f"{model}/{tag}/T{S.TEXTS}/gap"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (32, 32)
    bound = bound_vs_hi(hi, gap)
    assert record(f"get_CLIP_attr/{model}/{tag}/T{S.TEXTS}", got, hi, bound) <= bound and got.argmax() == hi.argmax()
    dev_map = sweep.get_CLIP_attr(img, 1, dict(td, device_maps=True))
    assert dev_map.is_cuda and same(dev_map.cpu().numpy(), got)
    with pytest.raises(NotImplementedError, match="CLIP Surgery model"):
        sweep.get_CLIP_attr(img, 1, dict(td, clip_surgery="modified"))


@pytest.mark.parametrize("small,large", [(2, 32), (7, 224), (14, 224)])
def test_the_bilinear_step_is_torchs_interpolate_on_the_device(small, large):
    """get_similarity_map's F.interpolate(sm, shape, mode='bilinear') bit for bit, a NaN map included.  This test decided which
    operator the row resizes with: K3 (kernels.bilinear_up) computes the same two taps but is not bit-identical to torch's kernel on
    an MI355X (2 -> 32 differs already), so surgery.resize_maps is torch's operator; K3's distance is written to the ledger."""
    from xai_engine import kernels as K
    from xai_engine import surgery
    g = torch.Generator().manual_seed(small)
    maps = torch.rand(3, small, small, generator=g)
    maps[2] = float("nan")
    maps = maps.to(DEV)
    got = surgery.resize_maps(maps, large, large)
    want = F.interpolate(maps[:, None], (large, large), mode="bilinear")[:, 0]
    assert tuple(got.shape) == (3, large, large) and same(got.cpu().numpy(), want.cpu().numpy())
    k3 = K.bilinear_up(maps[:2].contiguous(), large, large)
    # a figure, not a check: K3 is not what the row uses; maps in [0, 1], 2^-22 is four roundings
    record(f"figure_only/bilinear_up_vs_interpolate/{small}_to_{large}", k3.cpu().numpy(), want[:2].double().cpu().numpy(), 2.0 ** -22)
