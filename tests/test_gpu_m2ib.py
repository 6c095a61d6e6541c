"""CLIP's M2IB row on the device: the driver xai_engine/m2ib.py and sweep.get_CLIP_attr (with the opt-in) against the
reference-made fixtures (tests/golden/m2ib.npz), the batch rule, and the two sources of noise.

Bound, the rule lrp.npz and surgery.npz are held to.  The driver with the fixture's own CPU noise against `hi` (the closed-form flow
restated in fp64 on the fp16-valued weights, resized to 224 x 224 and min-max-normalised in fp64): max|got - hi| <= max(1e-5, 4 x gap)
x max|hi|, gap the REFERENCE's own distance from `hi` in the same dtype (gap32 for a model in fp32, gap16 for one in mixed fp16),
stored beside `hi`; the 4 x and the 1e-5 floor are the project's margin for flows whose order of summation differs from the
reference's (the device's GEMMs, the sums of K89 and K90).  Every measured error is written to profiles/m2ib_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import clip_restated as R
import m2ib_restated as M
from clip_restated import same
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_LEDGER = []


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "m2ib.npz"), allow_pickle=False)


@pytest.fixture(scope="module", autouse=True)
def _write_the_ledger():
    yield
    path = os.path.join(ROOT, "profiles", "m2ib_parity.json")
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "comparisons": _LEDGER}, f, indent=1)
        f.write("\n")


_MODELS, _HI = {}, {}


def dev_model(model, fp16=True):
    """the zoo's CLIP with the fixture's two towers on the device, frozen: in OpenAI's mixed fp16, or (fp16=False) the same
    fp16-valued weights as fp32, what evaluate_clip's --clip_fp32 builds"""
    if (model, fp16) not in _MODELS:
        from xai_engine import zoo
        res, patch, width, layers, heads, embed, _ = M.MODELS[model]
        m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=layers, vision_width=width, vision_patch_size=patch,
                         vision_heads=heads, **M.TEXT)
        z = np.load(os.path.join(GOLDEN, f"m2ib_w_{model}.npz"), allow_pickle=False)
        m.load_state_dict({k: torch.from_numpy(z[k]).float() for k in z.files}, strict=True)
        if fp16:
            zoo.convert_weights_fp16(m)
        _MODELS[model, fp16] = m.to(DEV).eval()
    return _MODELS[model, fp16]


def fixture_x(G, model, tag):
    return R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), M.MODELS[model][0], M.MODELS[model][0])


def fixture_txt(G, model, tag, fp16=True):
    return torch.from_numpy(G[f"{model}/{tag}/txt{16 if fp16 else 32}"])


def hi_map(G, model, tag):
    """`hi` at 224 x 224: the stored grid through the resize and the min-max in fp64, computed once"""
    if (model, tag) not in _HI:
        _HI[model, tag] = M.full_map(G[f"{model}/{tag}/hi"]).numpy()
    return _HI[model, tag]


def bound_vs_hi(hi, gap):
    return max(1e-5, 4.0 * gap) * float(np.abs(hi).max())


def record(name, got, hi, bound):
    err = float(np.abs(np.asarray(got, np.float64) - hi).max())
    _LEDGER.append({"name": name, "measured": err, "bound": bound, "max_abs_hi": float(np.abs(hi).max())})
    print(f"{name}: measured {err:.3e}, bound {bound:.3e}")
    return err


def host_map(G, model, tag, fp16=True, **kw):
    from xai_engine import m2ib
    seed = int(G[f"{model}/{tag}/noise_seed"])
    assert np.array_equal(M.noise_probe(M.fixture_noise(seed, model, steps=1)).numpy(), G[f"{model}/{tag}/probe"]), \
        "torch's CPU generator draws other numbers than the fixtures'"
    return m2ib.m2ib_batch(dev_model(model, fp16), fixture_x(G, model, tag), fixture_txt(G, model, tag, fp16), layer=M.MODELS[model][6],
                           noise="host", seed=seed, **kw)


@pytest.mark.parametrize("fp16", [True, False], ids=["mixed_fp16", "fp32"])
@pytest.mark.parametrize("model", list(M.MODELS))
def test_m2ib_batch_agrees_with_hi_and_its_argmax_patch_for_every_fixture(G, model, fp16):
    """L = 5, 17 and 50, H = 1 and 2, two blocks and one block behind the bottleneck; the reference's CPU noise draw for draw"""
    for tag in "01":
        pre = f"{model}/{tag}/"
        hi, gap = hi_map(G, model, tag), float(G[pre + ("gap16" if fp16 else "gap32")])
        got = host_map(G, model, tag, fp16)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, M.MAP, M.MAP) and got.is_cuda
        got = got[0].cpu().numpy()
        bound = bound_vs_hi(hi, gap)
        err = record(f"m2ib_batch/{pre}{'fp16' if fp16 else 'fp32'}", got, hi, bound)
        assert err <= bound, (pre, err, bound)
        assert M.argmax_patch(got, model) == M.argmax_patch(hi, model), pre
        assert got.min() == 0 and got.max() == 1


def test_a_noise_tensor_is_taken_as_given_and_equals_the_host_draws(G):
    from xai_engine import m2ib
    model, tag = "seventeen", "0"
    noise = M.fixture_noise(int(G[f"{model}/{tag}/noise_seed"]), model)[:M.STEPS - 1]
    want = host_map(G, model, tag).cpu().numpy()
    m, x, txt = dev_model(model), fixture_x(G, model, tag), fixture_txt(G, model, tag)
    assert same(m2ib.m2ib_batch(m, x, txt, noise=noise).cpu().numpy(), want)
    assert same(m2ib.m2ib_batch(m, x, txt[0], noise=noise[None].to(DEV)).cpu().numpy(), want)
    assert not same(m2ib.m2ib_batch(m, x, txt, noise=noise.flip(0)).cpu().numpy(), want)


def test_every_image_of_a_batch_has_the_bytes_of_its_own_call(G):
    """B = 3 against three one-image calls, byte for byte, each image with its own noise and its own text"""
    from xai_engine import m2ib
    for model in ("five", "seventeen"):
        m = dev_model(model)
        x = torch.cat([fixture_x(G, model, "0"), fixture_x(G, model, "1"), fixture_x(G, model, "0").flip(-1)])
        txt = torch.cat([fixture_txt(G, model, "0"), fixture_txt(G, model, "1"), fixture_txt(G, model, "1")])
        g = torch.Generator().manual_seed(7)
        noise = torch.randn(3, M.STEPS - 1, M.COPIES, M.tokens_of(model), M.MODELS[model][2], generator=g)
        three = m2ib.m2ib_batch(m, x, txt, noise=noise)
        assert tuple(three.shape) == (3, M.MAP, M.MAP)
        for b in range(3):
            one = m2ib.m2ib_batch(m, x[b:b + 1], txt[b], noise=noise[b])
            assert same(three[b:b + 1].cpu().numpy(), one.cpu().numpy()), (model, b)
        assert same(three.cpu().numpy(), m2ib.m2ib_batch(m, x, txt, noise=noise).cpu().numpy())      # and the same bytes on a second run
        shared = m2ib.m2ib_batch(m, x, txt[:1], noise=noise[0])                                      # one text, one noise for all
        assert same(shared[:1].cpu().numpy(), three[:1].cpu().numpy())


def test_device_noise_is_seeded_and_lands_on_the_host_noise_maps_argmax_patch(G):
    """The reference draws on its device, so between runs it offers statistical agreement only.  On fifty/0 the restated CPU flow
    keeps its argmax patch on 4 of 4 other noise seeds (`agree`, made by the reference's own flow); the device draw must on 3 of 4."""
    from xai_engine import m2ib
    model, tag = "fifty", "0"
    assert int(G[f"{model}/{tag}/agree"]) >= 3
    m, x, txt = dev_model(model), fixture_x(G, model, tag), fixture_txt(G, model, tag)
    want = M.argmax_patch(host_map(G, model, tag)[0].cpu().numpy(), model)
    maps = [m2ib.m2ib_batch(m, x, txt, seed=s)[0].cpu().numpy() for s in (1, 2, 3, 4)]
    assert same(m2ib.m2ib_batch(m, x, txt, noise="device", seed=1)[0].cpu().numpy(), maps[0])
    assert not same(maps[0], maps[1])
    hits = sum(M.argmax_patch(mp, model) == want for mp in maps)
    _LEDGER.append({"name": "device_noise/fifty/0/argmax_patch_hits_of_4", "measured": hits, "bound": 3})
    assert hits >= 3
    assert not np.isnan(m2ib.m2ib_batch(m, x, txt)[0].cpu().numpy()).any()                           # unseeded: it runs


def test_steps_one_reads_the_initial_alpha_and_img_hw_resizes(G):
    """steps = 1: no update is read, the map is the capacity at alpha = 5, which K90 and the restatement give alike"""
    from xai_engine import m2ib
    model, tag = "five", "0"
    m, x, txt = dev_model(model, fp16=False), fixture_x(G, model, tag), fixture_txt(G, model, tag, fp16=False)
    got = m2ib.m2ib_batch(m, x, txt, steps=1)[0].cpu().numpy()
    assert got.min() == 0 and got.max() == 1
    small = m2ib.m2ib_batch(m, x, txt, steps=1, img_hw=32)
    assert tuple(small.shape) == (1, 32, 32) and small.dtype == torch.float32 and float(small.min()) >= 0


def test_the_harness_row_with_the_opt_in(G):
    """get_CLIP_attr: the text feature is the target class's row of m2ib_text_features as it is; the harness's resize to img_hw and
    abs behind the map"""
    from xai_engine import sweep
    model, tag = "seventeen", "1"
    m = dev_model(model)
    table = torch.cat([torch.zeros(1, 16, dtype=torch.float16), fixture_txt(G, model, tag)]).to(DEV)      # the target class is row 1
    img = R.fixture_image(int(G[f"{model}/{tag}/x_seed"]), 32, 32)
    td = {"attr_func": "m2ib", "models": [m], "img_hw": M.MAP, "embeddings": torch.ones(2, 16, device=DEV), "device": DEV,
          "clip_m2ib": "plain", "m2ib_text_features": table, "m2ib_noise": "host", "m2ib_seed": int(G[f"{model}/{tag}/noise_seed"])}
    got = sweep.get_CLIP_attr(img, 1, td)
    hi, gap = hi_map(G, model, tag), float(G[f"{model}/{tag}/gap16"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (M.MAP, M.MAP)
    bound = bound_vs_hi(hi, gap)
    assert record(f"get_CLIP_attr/{model}/{tag}", got, hi, bound) <= bound and M.argmax_patch(got, model) == M.argmax_patch(hi, model)
    small = sweep.get_CLIP_attr(img, 1, dict(td, img_hw=32, device_maps=True))
    assert small.is_cuda and tuple(small.shape) == (32, 32)
    assert sweep.get_CLIP_attr(img, 1, dict(td, m2ib_noise="device", m2ib_seed=5)).shape == (M.MAP, M.MAP)
    with pytest.raises(NotImplementedError, match="M2IB wrapper"):
        sweep.get_CLIP_attr(img, 1, dict(td, clip_m2ib="modified"))


def test_wrapper_text_features_on_the_device(G):
    """the same bound as on the CPU (tests/test_cpu_m2ib.py): 2^-8 of the largest feature in mixed fp16, 1e-5 in fp32"""
    from xai_engine import m2ib
    for fp16 in (True, False):
        for model, tag in (("five", "0"), ("fifty", "1")):
            want = fixture_txt(G, model, tag, fp16).double().numpy()
            got = m2ib.wrapper_text_features(dev_model(model, fp16), M.fixture_ids(int(G[f"{model}/{tag}/t_seed"])))
            assert got.is_cuda and got.dtype == (torch.float16 if fp16 else torch.float32)
            bound = (2.0 ** -8 if fp16 else 1e-5) * np.abs(want).max()
            assert record(f"wrapper_text_features/{model}/{tag}/{'fp16' if fp16 else 'fp32'}", got.double().cpu().numpy(), want, bound) <= bound
