"""The Grad-ECLIP rows of CLIP on the device: K75-K77 (csrc/clip/clip_kernels.hip) against tests/clip_restated.py at the fixtures' shapes
in both dtypes, the driver xai_engine/eclip.py and sweep.get_CLIP_attr against the reference-made fixtures (tests/golden/clip.npz),
and one harness run.

Bounds.
  K76, K77 and what K75 computes before its first exp (the rounded scaled query is inside the scores; the scores themselves) are
  compared bit for bit, a NaN by position: the header states every accumulation order and every rounding point.
  K75 after the exp: the bound derived in include/xai_clip.h from the documented 1 ulp of the device expf, u = 2^-24:
      |p_dev - p_ref| <= (10 + 2n) u |p_ref| + spacing_T(max(|p_dev|, |p_ref|)),  n = ceil(L / 1024) + 22   (no spacing term for fp32)
      |o_dev - o_ref|_d <= sum_j dp_j |v_jd| + 2 L u sum_j |p_j v_jd| + spacing_T(max(|o_dev|, |o_ref|)_d)
  where dp_j is the first bound and spacing_T(x) is the distance between neighbouring values of T at x.
  The driver against `hi` (the restated flow in fp64 on the fp16-valued weights): max|got - hi| <= max(one ulp of the output dtype
  at max|hi|, 4 x gap x max|hi|), gap the reference's own low-to-high precision error stored beside `hi`: the project's lrp rule,
  the margin of 4 because the device's GEMMs round differently from the CPU's.  Every measured error is written to
  profiles/r21_eclip_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import clip_restated as R
from clip_restated import same, spacing
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIXTURES = {m: [str(j) for j in range(3)] + (["wide"] if m == "mini" else []) for m in R.MODELS}
_LEDGER = []


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "clip.npz"), allow_pickle=False)


@pytest.fixture(scope="module", autouse=True)
def _write_the_ledger():
    yield
    path = os.path.join(ROOT, "profiles", "r21_eclip_parity.json")
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "comparisons": _LEDGER}, f, indent=1)
        f.write("\n")


_WEIGHTS, _MODELS = {}, {}


def weights(model):
    if model not in _WEIGHTS:
        z = np.load(os.path.join(GOLDEN, f"clip_w_{model}.npz"), allow_pickle=False)
        _WEIGHTS[model] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _WEIGHTS[model]


def dev_model(model, fp16=True):
    """the zoo's CLIP with the fixture weights on the device, frozen; fp16=False: the same fp16-valued weights as fp32"""
    if (model, fp16) not in _MODELS:
        from xai_engine import zoo
        res, patch, width, layers, embed = R.MODELS[model]
        m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=layers, vision_width=width, vision_patch_size=patch, **R.TEXT)
        if fp16:
            zoo.convert_weights_fp16(m)
            m.load_state_dict(weights(model), strict=True)
        else:
            m.load_state_dict({k: v.float() for k, v in weights(model).items()}, strict=True)
        _MODELS[model, fp16] = m.to(DEV).eval()
    return _MODELS[model, fp16]


def hw_of(model, tag):
    return (32, 48) if tag == "wide" else (R.MODELS[model][0],) * 2


def fixture_x(G, model, tag):
    return R.fixture_input(int(G[f"{model}/{tag}/x_seed"]), *hw_of(model, tag))


def fixture_txt(G, model, tag, T):
    return R.fixture_texts(int(G[f"{model}/{tag}/t_seed"]), 2, R.MODELS[model][4])[:T]


def bound_vs_hi(hi, gap, out_dt):
    return max(float(spacing(np.abs(hi).max(), out_dt)), 4.0 * gap * float(np.abs(hi).max()))


def record(name, got, hi, bound):
    err = float(np.abs(np.asarray(got, np.float64) - hi).max())
    _LEDGER.append({"name": name, "measured": err, "bound": bound, "max_abs_hi": float(np.abs(hi).max())})
    print(f"{name}: measured {err:.3e}, bound {bound:.3e}")
    return err


# ------------------------------------------------------------------------------------------------ the kernels' operands
_OPERANDS = {}


def operands(G, model, dt):
    """The operands of K75-K77 for the three square inputs of `model` as one batch of B = 3 differing images, made on the CPU by the
    restated flow in dtype dt (fp16: mixed, as stored; fp32: every weight cast): numpy fp32 arrays holding values of dt, and the
    same values as device tensors of dt, K and V as the two halves of one (L, B, 2 D) buffer (so their row strides are not D)."""
    if (model, dt) in _OPERANDS:
        return _OPERANDS[model, dt]
    res, embed = R.MODELS[model][0], R.MODELS[model][4]
    tdt = torch.float16 if dt == np.float16 else torch.float32
    tups = [R.encode_dense(weights(model), fixture_x(G, model, tag), res, None if dt == np.float16 else torch.float32) for tag in "012"]
    cat = lambda i: torch.cat([t[i].detach() for t in tups], dim=1)           # (L, B, D) operands  # noqa: E731
    q_out, k_out, v = cat(4), cat(5), cat(3)
    v_final = torch.cat([t[1].detach() for t in tups], dim=0)                  # (B, L - 1, E)
    L, B, D = v.shape
    gen = torch.Generator().manual_seed(11)
    grad = (torch.randn(B, 2, D, generator=gen) * 0.05).to(tdt)
    txt = torch.stack([fixture_txt(G, model, tag, 2) for tag in "012"]).to(tdt)
    host = dict(q0=q_out[0], k=k_out, v=v, q_out0=q_out[0], k_out=k_out, v_final=v_final, grad=grad, txt=txt)
    assert all(t.dtype == tdt for t in host.values())
    kv = torch.empty((L, B, 2 * D), dtype=tdt, device=DEV)
    kv[:, :, :D], kv[:, :, D:] = k_out.to(DEV), v.to(DEV)
    dev = {n: t.to(DEV).contiguous() for n, t in host.items()}
    dev["k"] = dev["k_out"] = kv[:, :, :D]
    dev["v"] = kv[:, :, D:]
    assert dev["k"].stride(0) == 2 * B * D and not dev["v"].is_contiguous()
    _OPERANDS[model, dt] = ({n: t.float().numpy() for n, t in host.items()}, dev)
    return _OPERANDS[model, dt]


CASES = [(m, dt) for m in R.MODELS for dt in (np.float32, np.float16)]
IDS = [f"{m}-{np.dtype(dt).name}" for m, dt in CASES]


@pytest.mark.parametrize("model,dt", CASES, ids=IDS)
def test_k75_scores_are_exact_and_the_softmax_row_is_within_the_derived_bound(G, K, model, dt):
    """L = 17, 5 (fewer rows than a wave, D = 128), 197 (more than three waves of rows) and 50; B = 3 differing images"""
    h, d = operands(G, model, dt)
    L, B, D = h["k"].shape
    attn, att_out, scores = K.clip_cls_attention(d["q0"], d["k"], d["v"], want_scores=True)
    torch.cuda.synchronize()
    assert attn.dtype == att_out.dtype == scores.dtype == d["k"].dtype and tuple(attn.shape) == (B, L) and tuple(att_out.shape) == (B, D)
    _qs, s_ref, p_ref, o_ref = R.k75(h["q0"], h["k"], h["v"], dt)
    assert same(scores.float().cpu().numpy(), s_ref)
    p, o = attn.double().cpu().numpy(), att_out.double().cpu().numpy()
    half = dt == np.float16
    dp, do = R.k75_bound(p, p_ref, o, o_ref, h["v"], dt)
    assert (np.abs(p - p_ref) <= dp).all(), float((np.abs(p - p_ref) / dp).max())
    assert (np.abs(o - o_ref) <= do).all(), float((np.abs(o - o_ref) / do).max())
    assert abs(p.sum(axis=1) - 1).max() < (1e-2 if half else 1e-5)
    one = K.clip_cls_attention(d["q0"][1:2], d["k"][:, 1:2], d["v"][:, 1:2])        # an image alone: its own bytes
    assert same(one[0].cpu().numpy(), attn[1:2].cpu().numpy()) and same(one[1].cpu().numpy(), att_out[1:2].cpu().numpy())


@pytest.mark.parametrize("model,dt", CASES, ids=IDS)
def test_k76_is_the_restatement_bit_for_bit_for_every_flag_pair(G, K, model, dt):
    h, d = operands(G, model, dt)
    for withksim in (True, False):
        for withgrad in (True, False):
            for T in (1, 2):
                got = K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], d["grad"][:, :T].contiguous() if withgrad else None, texts=T,
                                       withksim=withksim, withgrad=withgrad)
                want, _ = R.k76(h["q_out0"], h["k_out"], h["v"], h["grad"][:, :T], T, withksim, withgrad, dt)
                assert got.dtype == torch.float32 and same(got.cpu().numpy(), want), (withksim, withgrad, T)
    assert (want != 0).any()


@pytest.mark.parametrize("dt", (np.float32, np.float16), ids=("float32", "float16"))
def test_k76_keeps_the_references_nan_when_all_cosines_are_equal_and_propagates_a_nan_cosine(G, K, dt):
    """image 1: every patch row of k_out is the same row, so max - min = 0 and the min-max is 0 / 0; image 2: one NaN in a patch row"""
    h, d = operands(G, "mini", dt)
    k_host = h["k_out"].copy()
    k_host[1:, 1] = k_host[1, 1]
    k_host[3, 2, 5] = np.nan
    k_dev = torch.from_numpy(k_host).to(d["v"].dtype).to(DEV)
    got = K.clip_eclip_map(d["q_out0"], k_dev, d["v"], d["grad"], withksim=True, withgrad=True).cpu().numpy()
    want, cos = R.k76(h["q_out0"], k_host, h["v"], h["grad"], 2, True, True, dt)
    assert same(got, want)
    assert not np.isnan(got[0]).any() and np.isnan(got[1]).all() and np.isnan(got[2]).all() and (cos[1] == cos[1, 0]).all()


@pytest.mark.parametrize("model,dt", CASES, ids=IDS)
def test_k77_is_the_restatement_bit_for_bit_for_shared_and_per_image_texts(G, K, model, dt):
    h, d = operands(G, model, dt)
    for T in (1, 2):
        got = K.clip_maskclip_map(d["v_final"], d["txt"][:, :T].contiguous(), d["k_out"])
        assert got.dtype == torch.float32 and same(got.cpu().numpy(), R.k77(h["v_final"], h["txt"][:, :T], h["k_out"], dt)), T
    shared = K.clip_maskclip_map(d["v_final"], d["txt"][0], d["k_out"])
    want = R.k77(h["v_final"], np.broadcast_to(h["txt"][:1], h["txt"].shape), h["k_out"], dt)
    assert same(shared.cpu().numpy(), want) and (want != 0).any()


def test_wrappers_refuse_wrong_operands_on_the_device(G, K):
    h, d = operands(G, "short", np.float16)
    L, B, D = h["k"].shape
    with pytest.raises(TypeError, match="v: expected torch.float16"):
        K.clip_cls_attention(d["q0"], d["k"], d["v"].float())
    with pytest.raises(ValueError, match="contiguous in its last axis"):
        K.clip_cls_attention(d["q0"], d["k"].transpose(1, 2), d["v"])
    with pytest.raises(ValueError, match=r"L >= 2"):
        K.clip_cls_attention(d["q0"], d["k"][:1], d["v"][:1])
    with pytest.raises(ValueError, match="q0 must be"):
        K.clip_cls_attention(d["q0"][:, :4].contiguous(), d["k"], d["v"])
    with pytest.raises(ValueError, match="over the limits"):
        K.clip_cls_attention(torch.zeros(1, 8200, device=DEV), torch.zeros(2, 1, 8200, device=DEV), torch.zeros(2, 1, 8200, device=DEV))
    with pytest.raises(ValueError, match=r"grad_cls must be"):
        K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], d["grad"][:1])
    with pytest.raises(TypeError, match="texts=T"):
        K.clip_eclip_map(d["q_out0"], d["k_out"], d["v"], withgrad=False)
    with pytest.raises(ValueError, match="v_final must be"):
        K.clip_maskclip_map(d["v_final"][:, :1].contiguous(), d["txt"], d["k_out"])
    with pytest.raises(ValueError, match="txt must be"):
        K.clip_maskclip_map(d["v_final"], d["txt"][:2].contiguous(), d["k_out"])


# ------------------------------------------------------------------------------------------------ the driver against the fixtures
@pytest.mark.parametrize("model", list(R.MODELS))
def test_eclip_batch_agrees_with_hi_for_every_fixture_row_and_text_count(G, model):
    from xai_engine import eclip
    m = dev_model(model)
    for tag in FIXTURES[model]:
        x = fixture_x(G, model, tag)
        for T in (1, 2):
            txt = fixture_txt(G, model, tag, T)
            for row in R.ROWS:
                pre = f"{model}/{tag}/{row}/T{T}/"
                hi, gap = G[pre + "hi"], float(G[pre + "gap"])
                got = eclip.eclip_batch(m, x, txt, row)
                assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + hi.shape and got.is_cuda
                bound = bound_vs_hi(hi, gap, np.float16)
                assert record(f"eclip_batch/{pre}fp16", got[0].cpu().numpy(), hi, bound) <= bound, pre


def test_every_image_of_a_batch_of_three_has_the_bytes_of_its_own_call(G):
    from xai_engine import eclip
    m = dev_model("mini")
    x = torch.cat([fixture_x(G, "mini", tag) for tag in "012"])
    txt = torch.stack([fixture_txt(G, "mini", tag, 2) for tag in "012"])
    for row in R.ROWS:
        batch = eclip.eclip_batch(m, x, txt, row)
        resized = eclip.eclip_batch(m, x, txt, row, img_hw=32)
        assert tuple(batch.shape) == (3, 4, 4) and tuple(resized.shape) == (3, 32, 32) and (resized >= 0).all()
        for b in range(3):
            assert same(eclip.eclip_batch(m, x[b:b + 1], txt[b], row).cpu().numpy(), batch[b:b + 1].cpu().numpy()), (row, b)
            assert same(eclip.eclip_batch(m, x[b:b + 1], txt[b:b + 1], row, img_hw=32).cpu().numpy(), resized[b:b + 1].cpu().numpy())
        assert not same(batch[0].cpu().numpy(), batch[1].cpu().numpy())


@pytest.mark.parametrize("model", list(R.MODELS))
def test_two_texts_are_the_sum_of_the_two_single_text_calls(G, model):
    """the same bound as against hi, at max|hi| of the two-text map: each single-text map is within its own bound of its exact
    value and the sum over the texts is one more rounding to the output dtype"""
    from xai_engine import eclip
    m = dev_model(model)
    x, txt = fixture_x(G, model, "0"), fixture_txt(G, model, "0", 2)
    for row in ("eclip", "eclip_wo", "eclip_nograd", "maskclip"):
        pre = f"{model}/0/{row}/T2/"
        both = eclip.eclip_batch(m, x, txt, row)[0].double().cpu().numpy()
        parts = sum(eclip.eclip_batch(m, x, txt[t:t + 1], row)[0].double().cpu().numpy() for t in range(2))
        bound = bound_vs_hi(G[pre + "hi"], float(G[pre + "gap"]), np.float16)
        assert record(f"two_texts/{pre}", both, parts, bound) <= bound


@pytest.mark.parametrize("model", list(R.MODELS))
def test_an_fp32_model_agrees_with_hi_to_four_times_the_restatements_fp32_gap(G, model):
    """gap32 is the fixture's: the restated flow in fp32 against `hi`, computed when the fixture was made (a CPU's fp32 GEMMs round
    as its BLAS pleases, so the figure is stored, not remade on whatever machine runs this test)"""
    from xai_engine import eclip
    m = dev_model(model, fp16=False)
    x, txt = fixture_x(G, model, "0"), fixture_txt(G, model, "0", 2)
    for row in R.ROWS:
        hi, gap32 = G[f"{model}/0/{row}/T2/hi"], float(G[f"{model}/0/{row}/T2/gap32"])
        got = eclip.eclip_batch(m, x, txt.half().float(), row)[0].cpu().numpy()
        bound = bound_vs_hi(hi, gap32, np.float32)
        assert record(f"eclip_batch/{model}/0/{row}/T2/fp32", got, hi, bound) <= bound, (row, gap32)


def _testing_dict(G, model, tag, row, emb):
    return {"models": [dev_model(model)], "img_hw": hw_of(model, tag)[0], "batch_size": 8, "device": DEV, "attr_func": row,
            "model_name": "CLIP16", "embeddings": emb, "num_patches": 4}


@pytest.mark.parametrize("model", list(R.MODELS))
def test_get_clip_attr_agrees_with_hi_resized_to_the_image(G, model):
    """get_CLIP_attr normalises row `target` of the embedding table itself, so `hi` is remade here by the same restated flow in fp64
    with that text; the gap is the fixture's.  The bilinear resize is a convex combination and |.| is 1-Lipschitz, so the bound on
    the patch map holds for the image map; its own fp32 arithmetic adds 4 ulp of fp32."""
    from xai_engine import sweep
    res = R.MODELS[model][0]
    img = R.fixture_image(int(G[f"{model}/0/x_seed"]), res, res)
    table = 3.0 * R.fixture_texts(int(G[f"{model}/0/t_seed"]), 2, R.MODELS[model][4])
    txt = torch.nn.functional.normalize(table[1][None], dim=-1).half().double()
    tup = R.encode_dense(weights(model), R.fixture_input(int(G[f"{model}/0/x_seed"]), res, res), res, torch.float64)
    hi_rows = R.rows_from_tuple(tup, txt)
    for row in R.ROWS:
        got = sweep.get_CLIP_attr(img, 1, _testing_dict(G, model, "0", row, table.to(DEV)))
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (res, res)
        hi = hi_rows[row].detach()
        want = torch.nn.functional.interpolate(hi[None, None], size=(res, res), mode="bilinear", align_corners=False)[0, 0].abs().numpy()
        gap = float(G[f"{model}/0/{row}/T1/gap"])
        bound = bound_vs_hi(hi.numpy(), gap, np.float16) + 4 * 2.0 ** -23 * float(np.abs(want).max())
        assert record(f"get_CLIP_attr/{model}/0/{row}", got, want, bound) <= bound, row


def test_harness_rows_on_the_mini_model_give_ten_finite_numbers_and_the_direct_attribution(G, tmp_path):
    """model_name "CLIP16": two synthetic images through get_CLIP_attr and run_perturbation with CLIP_test_info, and the same two
    as files through harness.evaluate_perturbation, whose selection is replayed here by hand."""
    from PIL import Image
    from xai_engine import eclip, harness, sweep
    m = dev_model("mini")
    imgs = [R.fixture_image(int(G[f"mini/{tag}/x_seed"]), 32, 32) for tag in "01"]
    with torch.no_grad():
        protos = torch.cat([m.encode_image(sweep.clip_keepsize_input(i).to(DEV)) for i in imgs])
    # an embedding table in which image j is of class j: its own normalised embedding (the cosine with itself is the largest)
    table = torch.cat([torch.nn.functional.normalize(protos.float().cpu(), dim=-1), R.fixture_texts(5, 6, 16)]).to(DEV).half()
    td = dict(_testing_dict(G, "mini", "0", "eclip", table), image_count=2, num_classes=8, imagenet_dataset=str(tmp_path / "val"))
    os.makedirs(td["imagenet_dataset"])
    for j, img in enumerate(imgs):
        x = sweep.clip_keepsize_input(img)
        target, p = harness.get_CLIP_pred(x.to(DEV), m, table)
        assert target == j and 0 < p <= 1
        attribution = sweep.get_CLIP_attr(img, target, td)
        direct = eclip.eclip_batch(m, x, torch.nn.functional.normalize(table[target][None], dim=-1), "eclip", img_hw=32)[0]
        assert same(attribution, direct.cpu().numpy()) and (attribution >= 0).all() and attribution.max() > 0
        info = {"input": x.to(DEV), "embeddings": table, "prediction_function": harness.get_CLIP_pred}
        c = sweep.run_perturbation(x, attribution, td, info)
        assert sorted(c) == sorted(sweep.KEYS) and all(np.isfinite(c[k]) for k in sweep.KEYS)
        Image.fromarray((img * 255).byte().permute(1, 2, 0).numpy()).save(os.path.join(td["imagenet_dataset"], f"ILSVRC2012_val_0000000{j + 1}.JPEG"),
                                                                         format="PNG")
    blur = harness.GaussianBlur(31, 31, DEV)
    want = []
    for j, img in enumerate(imgs):
        x = sweep.clip_keepsize_input(img).to(DEV)
        (t, p0), (tb, pb), (tk, pk) = (harness.get_CLIP_pred(v, m, table) for v in (x, blur(x), torch.zeros_like(x)))
        if not (pb >= p0 or pk >= p0 or t == tk or t == tb):
            want.append(f"ILSVRC2012_val_0000000{j + 1}.JPEG")
    total, used, names = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"))
    assert names == want and used == len(want)
    if used:
        assert all(np.isfinite(total[k]) for k in sweep.KEYS)
        assert os.path.exists(tmp_path / "out" / "CLIP16" / "eclip_2_images.csv")
