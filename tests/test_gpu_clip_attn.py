"""CLIP's game, rollout and lrp rows on the device: the driver xai_engine/clip_attn.py and sweep.get_CLIP_attr (with the opt-in) against
the reference-made fixtures (tests/golden/clip_attn.npz), the batch rule, the harness, and one run at ViT-B/16 size.

Bound, the project's existing rule (tests/test_gpu_eclip.py:12-14).  The driver against `hi` (the restated flow in fp64 on the
fp16-valued weights): max|got - hi| <= max(one ulp of the output dtype at max|hi|, 4 x gap x max|hi|), gap the reference's own
low-to-high precision error stored beside `hi` (gap32, the fp32 restated flow's, for an fp32 model); the margin of 4 because the
device's GEMMs round differently from the CPU's.  lrp runs the row form r <- r + r C_i (K85), which associates the products
differently from the reference's matrix chain, and is held to the same rule.  Every measured error is written to
profiles/clip_attn_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import clip_attn_restated as A
import clip_restated as R
from clip_restated import rT, same, spacing
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = (("game", 1), ("game", 2), ("rollout", 1), ("lrp", 1))
_LEDGER = []


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "clip_attn.npz"), allow_pickle=False)


@pytest.fixture(scope="module", autouse=True)
def _write_the_ledger():
    yield
    path = os.path.join(ROOT, "profiles", "clip_attn_parity.json")
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "comparisons": _LEDGER}, f, indent=1)
        f.write("\n")


_WEIGHTS, _MODELS = {}, {}


def weights(model):
    if model not in _WEIGHTS:
        z = np.load(os.path.join(GOLDEN, f"clip_attn_w_{model}.npz"), allow_pickle=False)
        _WEIGHTS[model] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _WEIGHTS[model]


def dev_model(model, fp16=True):
    """the zoo's CLIP with the fixture weights and heads on the device, frozen; fp16=False: the same fp16-valued weights as fp32"""
    if (model, fp16) not in _MODELS:
        from xai_engine import zoo
        res, patch, width, layers, heads, embed = A.MODELS[model]
        m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=layers, vision_width=width, vision_patch_size=patch,
                         vision_heads=heads, **A.TEXT)
        if fp16:
            zoo.convert_weights_fp16(m)
            m.load_state_dict(weights(model), strict=True)
        else:
            m.load_state_dict({k: v.float() for k, v in weights(model).items()}, strict=True)
        _MODELS[model, fp16] = m.to(DEV).eval()
    return _MODELS[model, fp16]


def fixture_x(G, model, tag):
    return R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), A.MODELS[model][0], A.MODELS[model][0])


def fixture_txt(G, model, tag, T, fp16=True):
    """the reference's normalised text features: model.forward's division on what its encode_text returned (stored), in the model's dtype"""
    raw = torch.from_numpy(G[f"{model}/{tag}/txt_raw/T{T}"])
    raw = raw if fp16 else raw.float()
    return raw / raw.norm(dim=-1, keepdim=True)


def bound_vs_hi(hi, gap, out_dt):
    return max(float(spacing(np.abs(hi).max(), out_dt)), 4.0 * gap * float(np.abs(hi).max()))


def record(name, got, hi, bound):
    err = float(np.abs(np.asarray(got, np.float64) - hi).max())
    _LEDGER.append({"name": name, "measured": err, "bound": bound, "max_abs_hi": float(np.abs(hi).max())})
    print(f"{name}: measured {err:.3e}, bound {bound:.3e}")
    return err


@pytest.mark.parametrize("model", list(A.MODELS))
def test_attention_rows_agree_with_hi_and_its_argmax_for_every_fixture(G, model):
    """L = 5, 17, 65 (one past a wave) and 197, H = 1, 2 and 4, n = 2 and 3; the output dtype of game and lrp is the model's half, of
    rollout fp32 (its eye is fp32)"""
    from xai_engine import clip_attn
    m = dev_model(model)
    for tag in "01":
        x = fixture_x(G, model, tag)
        for row, T in CASES:
            pre = f"{model}/{tag}/{row}/T{T}/"
            hi, gap = G[pre + "hi"], float(G[pre + "gap"])
            got = clip_attn.attention_rows_batch(m, x, fixture_txt(G, model, tag, T), row)
            assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + hi.shape and got.is_cuda
            got = got[0].cpu().numpy()
            bound = bound_vs_hi(hi, gap, np.float32 if row == "rollout" else np.float16)
            assert record(f"attention_rows_batch/{pre}fp16", got, hi, bound) <= bound, pre
            assert got.argmax() == hi.argmax(), pre


@pytest.mark.parametrize("model", list(A.MODELS))
def test_an_fp32_model_agrees_with_hi_to_four_times_the_restatements_fp32_gap(G, model):
    """gap32 is the fixture's: the restated flow in fp32 against `hi`, computed when the fixture was made"""
    from xai_engine import clip_attn
    m = dev_model(model, fp16=False)
    x = fixture_x(G, model, "0")
    for row, T in CASES:
        pre = f"{model}/0/{row}/T{T}/"
        hi, gap32 = G[pre + "hi"], float(G[pre + "gap32"])
        got = clip_attn.attention_rows_batch(m, x, fixture_txt(G, model, "0", T, fp16=False), row)[0].cpu().numpy()
        bound = bound_vs_hi(hi, gap32, np.float32)
        assert record(f"attention_rows_batch/{pre}fp32", got, hi, bound) <= bound, (row, gap32)
        assert got.argmax() == hi.argmax(), pre


def test_every_image_of_a_batch_of_three_has_the_bytes_of_its_own_call(G):
    from xai_engine import clip_attn
    for model in ("mini", "one"):
        m = dev_model(model)
        side = A.MODELS[model][0] // A.MODELS[model][1]
        x = torch.cat([fixture_x(G, model, "0"), fixture_x(G, model, "1"), R.fixture_input(999, 32, 32)])
        txt2 = torch.stack([fixture_txt(G, model, "0", 2), fixture_txt(G, model, "1", 2), fixture_txt(G, model, "0", 2).flip(0)])
        for row in A.ROWS:
            txt = txt2[:, :1] if row == "lrp" else txt2
            batch = clip_attn.attention_rows_batch(m, x, txt, row)
            resized = clip_attn.attention_rows_batch(m, x, txt, row, img_hw=32)
            assert tuple(batch.shape) == (3, side, side) and tuple(resized.shape) == (3, 32, 32) and (resized >= 0).all()
            for b in range(3):
                assert same(clip_attn.attention_rows_batch(m, x[b:b + 1], txt[b], row).cpu().numpy(), batch[b:b + 1].cpu().numpy()), (row, b)
                assert same(clip_attn.attention_rows_batch(m, x[b:b + 1], txt[b:b + 1], row, img_hw=32).cpu().numpy(),
                            resized[b:b + 1].cpu().numpy())
            assert not same(batch[0].cpu().numpy(), batch[1].cpu().numpy())


@pytest.mark.parametrize("fp16", (True, False), ids=("fp16", "fp32"))
def test_game_with_two_texts_is_the_rounded_sum_of_its_two_single_text_maps(G, fp16):
    """Bound: none.  A text's gradient does not depend on the other texts of the call (the backward of the logits multiplies by a
    one-hot row), so K82's m_tj are those of the single-text calls, and its output is their fp32 sum rounded once to the model's dtype."""
    from xai_engine import clip_attn
    for model in A.MODELS:
        m = dev_model(model, fp16)
        x, txt = fixture_x(G, model, "0"), fixture_txt(G, model, "0", 2, fp16)
        both = clip_attn.attention_rows_batch(m, x, txt, "game").cpu().numpy()
        parts = [clip_attn.attention_rows_batch(m, x, txt[t:t + 1], "game").cpu().numpy() for t in range(2)]
        assert same(both, rT(parts[0] + parts[1], np.float16 if fp16 else np.float32)), model


def test_rollout_does_not_depend_on_the_text_and_lrp_and_game_do(G):
    from xai_engine import clip_attn
    m = dev_model("wave")
    x = fixture_x(G, "wave", "0")
    a, b = fixture_txt(G, "wave", "0", 1), fixture_txt(G, "wave", "1", 1)
    assert same(clip_attn.attention_rows_batch(m, x, a, "rollout").cpu().numpy(), clip_attn.attention_rows_batch(m, x, b, "rollout").cpu().numpy())
    for row in ("game", "lrp"):
        assert not same(clip_attn.attention_rows_batch(m, x, a, row).cpu().numpy(), clip_attn.attention_rows_batch(m, x, b, row).cpu().numpy())


def _testing_dict(model, row, emb, **more):
    return dict({"models": [dev_model(model)], "img_hw": A.MODELS[model][0], "batch_size": 8, "device": DEV, "attr_func": row,
                 "model_name": "CLIP16", "embeddings": emb, "num_patches": A.MODELS[model][0] // A.MODELS[model][1],
                 "clip_attention_rows": "plain"}, **more)


def test_get_clip_attr_with_the_opt_in_agrees_with_hi_resized_to_a_224_image(G):
    """get_CLIP_attr normalises row `target` of the embedding table itself; the table's row 1 is what the reference's encode_text
    returned for the fixture's text, so `hi` is the fixture's.  The bilinear resize is a convex combination and |.| is 1-Lipschitz, so
    the bound on the patch map holds for the image map; its own fp32 arithmetic adds 4 ulp of fp32."""
    from xai_engine import sweep
    res = A.MODELS["long"][0]
    assert res == 224
    img = R.fixture_image(int(G["long/0/x_seed"]), res, res)
    table = torch.cat([torch.from_numpy(G["long/1/txt_raw/T1"]), torch.from_numpy(G["long/0/txt_raw/T1"])]).to(DEV)
    for row in A.ROWS:
        got = sweep.get_CLIP_attr(img, 1, _testing_dict("long", row, table))
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (res, res)
        hi = torch.from_numpy(G[f"long/0/{row}/T1/hi"])
        want = torch.nn.functional.interpolate(hi[None, None], size=(res, res), mode="bilinear", align_corners=False)[0, 0].abs().numpy()
        gap = float(G[f"long/0/{row}/T1/gap"])
        bound = bound_vs_hi(hi.numpy(), gap, np.float32 if row == "rollout" else np.float16) + 4 * 2.0 ** -23 * float(np.abs(want).max())
        assert record(f"get_CLIP_attr/long/0/{row}", got, want, bound) <= bound, row
        with pytest.raises(NotImplementedError, match=row):                       # without the opt-in: today's refusal
            sweep.get_CLIP_attr(img, 1, _testing_dict("long", row, table, clip_attention_rows="modified"))


def test_harness_runs_each_row_on_the_mini_model(G, tmp_path):
    """model_name "CLIP16": two synthetic images as files through harness.evaluate_perturbation with the opt-in, whose selection is
    replayed here by hand, and get_CLIP_attr against the direct call"""
    from PIL import Image
    from xai_engine import clip_attn, harness, sweep
    m = dev_model("mini")
    imgs = [R.fixture_image(int(G[f"mini/{tag}/x_seed"]), 32, 32) for tag in "01"]
    with torch.no_grad():
        protos = torch.cat([m.encode_image(sweep.clip_keepsize_input(i).to(DEV)) for i in imgs])
    # an embedding table in which image j is of class j: its own normalised embedding (the cosine with itself is the largest)
    table = torch.cat([torch.nn.functional.normalize(protos.float().cpu(), dim=-1), R.fixture_texts(5, 6, 16)]).to(DEV).half()
    root = str(tmp_path / "val")
    os.makedirs(root)
    blur = harness.GaussianBlur(31, 31, DEV)
    want = []
    for j, img in enumerate(imgs):
        Image.fromarray((img * 255).byte().permute(1, 2, 0).numpy()).save(os.path.join(root, f"ILSVRC2012_val_0000000{j + 1}.JPEG"), format="PNG")
        x = sweep.clip_keepsize_input(img).to(DEV)
        (t, p0), (tb, pb), (tk, pk) = (harness.get_CLIP_pred(v, m, table) for v in (x, blur(x), torch.zeros_like(x)))
        assert t == j
        if not (pb >= p0 or pk >= p0 or t == tk or t == tb):
            want.append(f"ILSVRC2012_val_0000000{j + 1}.JPEG")
    for row in A.ROWS:
        td = _testing_dict("mini", row, table, image_count=2, num_classes=8, imagenet_dataset=root)
        attribution = sweep.get_CLIP_attr(imgs[0], 0, td)
        direct = clip_attn.attention_rows_batch(m, sweep.clip_keepsize_input(imgs[0]), torch.nn.functional.normalize(table[0][None], dim=-1),
                                                row, img_hw=32)[0]
        assert same(attribution, direct.cpu().numpy()) and (attribution >= 0).all() and attribution.max() > 0
        total, used, names = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"))
        assert names == want and used == len(want)
        if used:
            assert all(np.isfinite(total[k]) for k in sweep.KEYS)
            assert os.path.exists(tmp_path / "out" / "CLIP16" / f"{row}_2_images.csv")


def test_rows_at_vit_b16_size_are_finite_and_lrp_relevance_is_non_negative():
    """zoo.clip_vit_b16, seeded, in OpenAI's mixed fp16: n = 12, H = 12, L = 197, D = 768; L * L is odd, so K84 takes its scalar flavour"""
    from xai_engine import clip_attn, zoo
    m = zoo.convert_weights_fp16(zoo.clip_vit_b16(0)).to(DEV).eval()
    x = R.fixture_input(5, 224, 224)
    txt = R.fixture_texts(6, 1, 512)
    for row in A.ROWS:
        maps = clip_attn.attention_rows_batch(m, x, txt, row)
        assert tuple(maps.shape) == (1, 14, 14) and torch.isfinite(maps).all() and (maps >= 0).all(), row
        assert maps.max() > 0 or row == "game"
        out = clip_attn.attention_rows_batch(m, x, txt, row, img_hw=224)
        assert tuple(out.shape) == (1, 224, 224) and out.dtype == torch.float32 and torch.isfinite(out).all()
