"""Transformer Attribution on the device: K46-K52 (csrc/lrp_kernels.hip) at their edges against the torch expressions they replace and
against tests/lrp_restated.py, the driver xai_engine/lrp.py against the reference-made goldens (tests/golden/lrp.npz) and against
the restated flow, and the harness row `t_attr`.

Bounds.  The kernels are compared bit for bit (a NaN by position): K46-K49 and K51 with the torch expression evaluated by torch on the
same device, K50 and K52 with the order-pinned restatement.  Against the reference's fp64 goldens the bound is lrp_restated.bound:
max(1e-5, 4 x the reference's own fp32-to-fp64 gap).  Eagerly and for one image the driver makes the restated flow's GEMM calls and
its kernels are exact, so the two are equal bit for bit; replayed from a graph or for a batch the GEMM shapes differ, and the
yardstick is the restated flow in fp64 on the device: the driver may be at most twice as far from it as the restated fp32 flow is
(floor 1e-5), both errors recorded through conftest.check."""
import copy
import itertools

import numpy as np
import pytest
import torch

import lrp_restated as R
from conftest import GOLDEN, check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 3, 4, 5, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _free_the_cache():
    yield
    from xai_engine import lrp
    lrp.clear_cache()


def _offset(a, by):
    """the array on the device, its first element `by` elements past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[by:by + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * by) % 16
    return view


def _out_like(t, by):
    return _offset(np.full(tuple(t.shape), -7.0, np.float32), by)


def _same(got, want):
    """bit for bit, a NaN by position"""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and got[~gn].tobytes() == want[~wn].tobytes()


# safe_divide's special cases: every divisor with every dividend
DIVISORS = np.array([0.0, -0.0, 1e-9, -1e-9, 1e-40, -1e-40, np.nan, np.inf, -np.inf, 2e-9, -3.0], np.float32)
DIVIDENDS = np.array([0.0, 1.5, -2.5, np.nan], np.float32)
PAIRS = np.array(list(itertools.product(DIVIDENDS, DIVISORS)), np.float32)          # (44, 2): (a, b)


def _with_specials(n, rng):
    """(dividend, divisor) of n elements: random, with the special pairs laid over the front (all of them once n >= 44)"""
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    b[rng.random(n) < 0.1] = 0.0
    m = min(n, len(PAIRS))
    start = int(rng.integers(0, len(PAIRS)))
    idx = (start + np.arange(m)) % len(PAIRS)
    a[:m], b[:m] = PAIRS[idx, 0], PAIRS[idx, 1]
    return a, b


def test_safe_divide_special_cases_are_all_there():
    assert np.float32(1e-9) + np.float32(-1e-9) == 0 and 0 < abs(np.float32(1e-40)) < np.finfo(np.float32).tiny
    a, b = _with_specials(4099, np.random.default_rng(0))
    assert {(x.tobytes(), y.tobytes()) for x, y in zip(a[:44], b[:44])} == {(x.tobytes(), y.tobytes()) for x, y in PAIRS}


CASES = [(n, by, B) for n in SIZES for by in (0, 1) for B in (1, 3)]


@pytest.mark.parametrize("n,by,B", CASES)
def test_k46_k47_k48_k51_equal_their_torch_expressions_bit_for_bit(K, n, by, B):
    rng = np.random.default_rng(1000 * n + 10 * by + B)
    a, b = (_offset(t.reshape(B, n), by) for t in _with_specials(B * n, rng))
    g2 = _offset(rng.standard_normal((B, n)).astype(np.float32), by)
    # K46 on the divisors: +-0, denormals, NaN, +-Inf
    pos, neg = K.lrp_split(b, pos=_out_like(b, by), neg=_out_like(b, by))
    assert _same(pos, torch.clamp(b, min=0)) and _same(neg, torch.clamp(b, max=0)), "K46"
    # K47 with one and with two divisors; -0 as the second keeps every special divisor what it is
    assert _same(K.lrp_ratio(a, b, out=_out_like(a, by)), R.safe_divide(a, b)), "K47 / z1"
    z2 = _offset(np.where(np.arange(B * n) < 44, -0.0, rng.standard_normal(B * n)).astype(np.float32).reshape(B, n), by)
    assert _same(K.lrp_ratio(a, b, z2, out=_out_like(a, by)), R.safe_divide(a, b + z2)), "K47 / z1 + z2"
    # K48: x with the specials, two gradients
    assert _same(K.lrp_gather(b, a, g2, out=_out_like(a, by)), R.gather(b, a, g2)), "K48"
    # K51: the divisor is x itself
    assert _same(K.lrp_clone(b, a, g2, out=_out_like(a, by)), R.clone(b, a, g2)), "K51"
    # K49, plain
    assert _same(K.lrp_half_product(b, a, out=_out_like(a, by)), R.half_product(b, a)), "K49"


def test_k47_k48_k51_may_write_over_an_operand(K):
    rng = np.random.default_rng(5)
    for n in (5, 4099, 8192):
        a, b = (torch.from_numpy(t).to(DEV).reshape(1, n) for t in _with_specials(n, rng))
        g2 = torch.from_numpy(rng.standard_normal((1, n)).astype(np.float32)).to(DEV)
        want = R.safe_divide(a, b + g2)
        z = b.clone()
        assert K.lrp_ratio(a, z, g2, out=z) is z and _same(z, want)
        want = R.gather(b, a, g2)
        g = a.clone()
        assert K.lrp_gather(b, g, g2, out=g) is g and _same(g, want)
        want = R.clone(b, a, g2)
        r = g2.clone()
        assert K.lrp_clone(b, a, r, out=r) is r and _same(r, want)


@pytest.mark.parametrize("h,N,d", [(1, 5, 8), (4, 17, 8), (2, 5, 3)])
@pytest.mark.parametrize("by", [0, 1])
def test_k49_stores_into_its_third_of_cam_qkv_and_touches_nothing_else(K, h, N, d, by):
    rng = np.random.default_rng(h * 100 + N)
    for B in (1, 3):
        before = _offset(rng.standard_normal((B, N, 3 * h * d)).astype(np.float32), by)
        for slot in (0, 1, 2):
            x, c = (_offset(t.reshape(B, h, N, d), by) for t in _with_specials(B * h * N * d, rng))
            got, want = before.clone() if by == 0 else _offset(before.cpu().numpy(), by), before.clone()
            assert K.lrp_half_product(x, c, out=got, slot=slot) is got
            R.half_product_slot(x, c, want, slot)
            assert _same(got, want), (B, slot)
            others = [s for s in (0, 1, 2) if s != slot]
            assert torch.equal(got.view(B, N, 3, h, d)[:, :, others].view(torch.int32), before.view(B, N, 3, h, d)[:, :, others].view(torch.int32))
    with pytest.raises(ValueError, match="cam_qkv"):
        K.lrp_half_product(x, c, out=torch.empty((B, N, 3 * h * d + 1), device=DEV), slot=0)


# ------------------------------------------------------------------------------------------------ K50
def _k50_case(kind, B, n, rng):
    x0, x1, r = (rng.standard_normal((B, n)).astype(np.float32) for _ in range(3))
    if kind == "a_sum_zero":
        x0[:] = 0.0                                        # a = 0 * s everywhere
    elif kind == "r_sum_zero":
        r[:, 1::2] = -r[:, 0:n - 1:2]                      # neighbours of one lane cancel exactly (n even)
    elif kind == "specials":
        flat_r, flat_z = _with_specials(B * n, rng)
        r, x0, x1 = flat_r.reshape(B, n), flat_z.reshape(B, n), np.zeros((B, n), np.float32)
        x1[:] = -0.0
    return x0, x1, r


@pytest.mark.parametrize("n", [1, 5, 4095, 4096, 4097, 8192, 8193, 12291])
@pytest.mark.parametrize("by", [0, 1])
def test_k50_equals_the_order_pinned_restatement_bit_for_bit(K, n, by):
    chunk = K.lrp_add_chunk()
    assert chunk == R.ADD_CHUNK and {4095, 4096, 4097} == {chunk - 1, chunk, chunk + 1}
    rng = np.random.default_rng(n + by)
    for kind in ("random", "a_sum_zero", "specials") + (("r_sum_zero",) if n % 2 == 0 else ()):
        x0, x1, r = (_offset(t, by) for t in _k50_case(kind, 3, n, rng))
        a, b = K.lrp_add(x0, x1, r, a=_out_like(r, by), b=_out_like(r, by))
        want_a, want_b = R.add(x0, x1, r)
        assert _same(a, want_a) and _same(b, want_b), (kind, n, by)
        if kind == "a_sum_zero":
            assert not a.any()
        if kind == "r_sum_zero":
            assert all(R.pinned_sum(r[i].cpu().numpy()) == 0.0 for i in range(3)) and not a.any() and not b.any()
        # no image's sums leak into another's: every image alone gives the same bytes
        for i in range(3):
            ai, bi = K.lrp_add(x0[i:i + 1].clone(), x1[i:i + 1].clone(), r[i:i + 1].clone())
            assert _same(ai, a[i:i + 1]) and _same(bi, b[i:i + 1]), (kind, n, i)


# ------------------------------------------------------------------------------------------------ K52
@pytest.mark.parametrize("L,h,S", [(1, 1, 5), (2, 4, 17), (3, 12, 50)])
@pytest.mark.parametrize("B", [1, 2])
def test_k52_equals_the_restated_head_order_bit_for_bit(K, L, h, S, B):
    rng = np.random.default_rng(L * 1000 + S + B)
    cam = torch.from_numpy(rng.standard_normal((L, B, h, S, S)).astype(np.float32)).to(DEV)
    grad = torch.from_numpy(rng.standard_normal((L, B, h, S, S)).astype(np.float32)).to(DEV)
    cam[0, 0, 0, 1, 2] = float("nan")
    cam[-1, -1, :, 2, :] = -1.0                                # a row that clamps to zero: its normalised row is the identity's
    for g in (None, grad):
        if g is not None:
            g[-1, -1, :, 2, :] = 1.0
        for mode in (K.LRP_MATRICES, K.LRP_ROLLOUT, K.LRP_CLS_ROW):
            got = K.lrp_attn_matrices(cam, g, mode)
            want = R.attn_matrices(cam, g, mode)
            assert got.shape == ((B, L, S) if mode == K.LRP_CLS_ROW else (B, L, S, S))
            assert _same(got, want.contiguous()), (g is not None, mode)
        aug = K.lrp_attn_matrices(cam, g, K.LRP_ROLLOUT)
        assert torch.equal(aug[-1, -1, 2], torch.eye(S, device=DEV)[2])
        finite = ~torch.isnan(aug).any(dim=-1)
        assert ((aug.sum(-1) - 1).abs()[finite] < 1e-5).all()


def test_the_restated_k19_is_k19(K):
    rng = np.random.default_rng(19)
    for n, L, S in ((1, 1, 5), (2, 3, 17), (1, 2, 50)):
        aug = torch.from_numpy(rng.random((n, L, S, S)).astype(np.float32)).to(DEV)
        assert _same(K.rollout_row(aug, 0), R.rollout_row(aug, 0))


# ------------------------------------------------------------------------------------------------ against the reference's goldens
@pytest.fixture(scope="module", params=list(R.FIXTURES))
def fixture(request):
    model, xs, targets, g = R.load_fixture(request.param, GOLDEN)
    return request.param, model.to(DEV), xs.to(DEV), targets, g


def test_generate_lrp_and_the_batch_meet_the_reference_fp64_goldens(fixture):
    from xai_engine.lrp import LRP, transformer_attribution_batch
    name, model, xs, targets, g = fixture
    side = xs.shape[-1] // int(g[f"{name}/cfg"][1])
    misses = []
    for key, kw in R.CALLS.items():
        batch = transformer_attribution_batch(xs, model, targets, graphs=False, **kw)
        assert batch.shape == (R.IMAGES, side, side) and batch.is_cuda and batch.dtype == torch.float32
        for j in range(R.IMAGES):
            want, gap = g[f"{name}/{j}/{key}/f64"], g[f"{name}/{j}/{key}/gap"]
            one = LRP(model).generate_LRP(xs[j:j + 1], int(targets[j]), device=DEV, **kw)
            assert one.shape == (1, side, side) == want.shape and one.is_cuda
            assert _same(batch[j:j + 1], one), (name, j, key, "the image's own one-image call gives other bytes")
            for how, got in (("generate_LRP", one), ("batch", batch[j:j + 1])):
                try:                                                       # every figure is measured and recorded before the first miss raises
                    check(f"lrp/{name}/{j}/{key}/{how}", got.cpu().numpy(), want, R.bound(gap))
                except AssertionError as e:
                    misses.append(e.args[0])
    assert not misses, misses
    none = LRP(model).generate_LRP(xs[:1], None, device=DEV)            # the fixtures' targets are the argmax
    assert torch.equal(none, LRP(model).generate_LRP(xs[:1], int(targets[0]), device=DEV))


def test_the_attn_cams_of_the_mini_model_meet_the_goldens():
    from xai_engine.lrp import transformer_attribution_batch
    model, xs, targets, g = R.load_fixture("mini", GOLDEN)
    _, cams = transformer_attribution_batch(xs.to(DEV), model.to(DEV), targets, graphs=False, return_cams=True)
    assert cams.shape[:2] == (2, R.IMAGES)
    for j in range(R.IMAGES):
        for i in range(2):
            check(f"lrp/mini/{j}/cam{i}", cams[i, j:j + 1].cpu().numpy(), g[f"mini/{j}/cam{i}/f64"], R.bound(g[f"mini/{j}/cam{i}/gap"]))


# ------------------------------------------------------------------------------------------------ against the restated flow
def _zoo_vit(depth, seed=3, **kw):
    from xai_engine import zoo
    cfg = dict(img=32, patch=8, dim=32, depth=depth, heads=4, num_classes=10)
    cfg.update(kw)
    model = zoo.vit_base_patch16_224(seed, **cfg).to(DEV)
    model.cfg = cfg
    return model


def _fp64_twin(model):
    """the same weights in fp64 (a model that has run holds tensors of its last forward, which deepcopy does not take)"""
    from xai_engine import zoo
    twin = zoo.VisionTransformer(**model.cfg).to(DEV).eval()
    twin.load_state_dict(model.state_dict())
    for p in twin.parameters():
        p.requires_grad_(False)
    return twin.double()


def _inputs(B, img=32, seed=0):
    return torch.cat([R.fixture_input(seed + j, img) for j in range(B)]).to(DEV)


METHOD_KW = [dict(method="transformer_attribution"), dict(method="grad"), dict(method="rollout"),
             dict(method="last_layer"), dict(method="last_layer", is_ablation=True), dict(method="last_layer_attn"),
             dict(method="transformer_attribution", withgrad=False)]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_eager_generate_lrp_equals_the_restated_flow_bit_for_bit(depth):
    from xai_engine.lrp import LRP
    model, x = _zoo_vit(depth), _inputs(1)
    calls = METHOD_KW + ([dict(method="second_layer"), dict(method="second_layer", is_ablation=True),
                          dict(method="transformer_attribution", start_layer=1)] if depth > 1 else [])
    for kw in calls:
        for target in (None, 3):
            got = LRP(model).generate_LRP(x, target, device=DEV, **kw)
            want, _ = R.generate(model, x, None if target is None else torch.tensor([target], device=DEV), **kw)
            assert got.shape == (1, 4, 4) and _same(got, want), (depth, kw, target)
    if depth == 1:                                               # the early stop in the only block; the reference's self.blocks[1]
        with pytest.raises(IndexError):
            LRP(model).generate_LRP(x, 3, method="second_layer", device=DEV)
        with pytest.raises(IndexError):
            LRP(model).generate_LRP(x, 3, start_layer=1, device=DEV)


def test_eager_generate_lrp_equals_the_restated_flow_at_vit_b16():
    from xai_engine import lrp
    model, x = _zoo_vit(12, seed=0, img=224, patch=16, dim=768, heads=12, num_classes=1000), _inputs(1, img=224)
    got = lrp.LRP(model).generate_LRP(x, None, device=DEV)
    want, _ = R.generate(model, x, None)
    assert got.shape == (1, 14, 14) and _same(got, want)
    lrp.clear_cache()


def _fp64_yardstick(model, x, targets, kw):
    """(the restated flow in fp64 on the device, the restated fp32 flow on the device)"""
    want, _ = R.generate(_fp64_twin(model), x.double(), targets, **kw)
    own, _ = R.generate(model, x, targets, **kw)
    return want.cpu().numpy(), own.cpu().numpy()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_replayed_and_batched_calls_stay_within_twice_the_restated_flows_own_error(depth):
    """Image by image: the driver's error against the restated fp64 flow may be at most twice the restated fp32 flow's own error for
    that image (floor 1e-5).  Both errors of every comparison go to the ledger (conftest.check)."""
    from xai_engine import lrp
    model, x = _zoo_vit(depth), _inputs(3)
    targets = torch.tensor([3, 1, 7], device=DEV)
    for kw in (dict(method="transformer_attribution"), dict(method="last_layer", is_ablation=True)):
        name = f"lrp/restated/depth{depth}/{kw['method']}"

        def held(tag, got, want, restated):
            got = got.cpu().numpy()
            for j in range(len(want)):
                tol = max(1e-5, 2 * R.rel_err(restated[j], want[j]))
                check(f"{name}/{tag}/{j}/restated_fp32", restated[j], want[j], tol, against="fp64")     # the yardstick's own error
                check(f"{name}/{tag}/{j}", got[j], want[j], tol, against="fp64")

        want, restated = _fp64_yardstick(model, x, targets, kw)
        before = dict(lrp.LRP_COUNTS)
        eager = lrp.transformer_attribution_batch(x, model, targets, graphs=False, **kw)
        first = lrp.transformer_attribution_batch(x, model, targets, graphs=True, **kw)
        second = lrp.transformer_attribution_batch(x, model, targets, graphs=True, **kw)
        third = lrp.transformer_attribution_batch(x.flip(0), model, targets.flip(0), graphs=True, **kw)
        after = dict(lrp.LRP_COUNTS)
        held("eager_B3", eager, want, restated)
        held("replayed_B3", first, want, restated)
        held("replayed_B3_reordered", third.flip(0), want, restated)
        assert _same(second, first), "a second replay equals the first"
        captured = after["captures"] - before["captures"]
        assert captured + after["captures_refused"] - before["captures_refused"] == 1
        assert after["eager"] - before["eager"] == 1 + 3 * (1 - captured) and after["replayed"] - before["replayed"] == 3 * captured
        assert captured == 1, "the capture was refused"
        # one image, replayed
        want1, restated1 = _fp64_yardstick(model, x[:1], targets[:1], kw)
        one = lrp.LRP(model, graphs=True).generate_LRP(x[:1], 3, device=DEV, **kw)
        again = lrp.LRP(model, graphs=True).generate_LRP(x[:1], 3, device=DEV, **kw)
        assert _same(one, again)
        held("replayed_B1", one, want1, restated1)


def test_a_rewritten_weight_gets_new_clamped_copies():
    from xai_engine import lrp
    model, x = _zoo_vit(2), _inputs(1)
    a = lrp.LRP(model).generate_LRP(x, 3, device=DEV)
    with torch.no_grad():
        model.blocks[1].mlp.fc1.weight.mul_(-1.0)
    b = lrp.LRP(model).generate_LRP(x, 3, device=DEV)
    want, _ = R.generate(model, x, torch.tensor([3], device=DEV))
    assert _same(b, want) and not _same(a, b)


# ------------------------------------------------------------------------------------------------ the harness row
def test_the_harness_row_t_attr(K):
    from xai_engine import sanity, segeval, sweep
    hw = 64
    model = _zoo_vit(2, img=hw, patch=16)
    rand = sanity.randomize_VIT_model(copy.deepcopy(model))
    td = {"models": [model, model, rand, rand], "img_hw": hw, "device": DEV, "attr_func": "t_attr", "num_patches": 4, "batch_size": 25}
    x = R.fixture_input(5, hw)
    patch = sweep.vit_patch_map(x, torch.tensor(1), td)
    assert patch.shape == (1, 4, 4) and patch.is_cuda
    want, _ = R.generate(model, x.to(DEV), torch.tensor([1], device=DEV))
    own = R.generate(_fp64_twin(model), x.to(DEV).double(), torch.tensor([1], device=DEV))[0].cpu().numpy()
    assert R.rel_err(patch.cpu().numpy(), own) <= max(1e-5, 2 * R.rel_err(want.cpu().numpy(), own))
    got = sweep.get_VIT_attr(x, None, torch.tensor(1), td)
    assert got.shape == (hw, hw) and got.dtype == np.float32
    assert np.array_equal(got, K.bilinear_up(patch, hw, hw, scale=1.0, take_abs=True)[0].cpu().numpy())
    other = sweep.get_VIT_attr(x, None, torch.tensor(1), dict(td, models=[rand, rand]))
    vals = sanity.get_sanity(got, other, abs=True)
    assert list(vals) == ["SSIM", "SPR", "HOG"] and all(np.isfinite(v) for v in vals.values())
    with pytest.raises(NotImplementedError, match="t_attr"):                  # the segmentation evaluation keeps refusing the row
        segeval.evaluate_imagenet_seg(dict(td, model_name="VIT16", segmentation_dataloader=[]))


def test_evaluate_perturbation_runs_the_t_attr_row_end_to_end(tmp_path, monkeypatch):
    """a sweep of a few synthetic images with --attr_func t_attr through the harness, on three streams (each stream worker captures
    and replays its own pass): every image attributed, the CSV written"""
    import os
    from PIL import Image
    from xai_engine import harness, lrp
    model = _zoo_vit(2, img=64, patch=16)
    rng = np.random.default_rng(5)
    names = []
    for i in range(4):
        name = f"ILSVRC2012_val_{i + 1:08d}.png"
        Image.fromarray((rng.random((70, 76, 3)) * 255).astype(np.uint8)).save(tmp_path / name)
        names.append(name)
    norm = (harness.VIT_MEAN, harness.VIT_STD)
    monkeypatch.setattr(harness, "select_images", lambda td, cc, rank=0, world=1, lazy=False:
                        (names, harness.SelectedImages(str(tmp_path), names, 64, *norm), [0, 0, 0, 0]))
    td = {"models": [model, model], "img_hw": 64, "batch_size": 25, "device": DEV, "attr_func": "t_attr", "normalize": norm,
          "imagenet_dataset": str(tmp_path), "model_name": "VIT16", "image_count": 4, "num_patches": 4}
    before = dict(lrp.LRP_COUNTS)
    total, used, _ = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"), streams=3)
    assert used == 4 and all(np.isfinite(float(v)) for v in total.values())
    assert os.path.exists(tmp_path / "out" / "VIT16" / "t_attr_4_images.csv")
    assert lrp.LRP_COUNTS["replayed"] + lrp.LRP_COUNTS["eager"] - before["replayed"] - before["eager"] == 4
