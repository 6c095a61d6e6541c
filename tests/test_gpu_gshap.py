"""GradientShap on the device: K34 at tolerance 0 against the torch expression on the same device, K35 at tolerance 0 against a
Python loop in the stated order (torch ops on the host: every difference, product, sum and the division rounds once), and the whole
method (fused, fused + forked, unfused) against the restatement of captum's flow (tests/gshap_restated.py) on the unfused model with
the same draws and the same pass shapes -- same convolutions under deterministic solvers (conftest), fused sites bitwise PyTorch's,
so the expected difference is 0 and the bar is the project's 1e-5."""
import os

import numpy as np
import pytest
import torch

import gshap_restated as R
from conftest import BAR, check
from test_gpu_guided import _model, _sprinkle, _variant        # _sprinkle: test_gpu_guided.SPECIAL at random places

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                      # floats in front of and behind every output that must keep their sentinel


def _bits_equal_nan_aware(a, b):
    """the same NaN positions and, everywhere else, the same bit patterns (-0 is not +0)"""
    na, nb = a.isnan(), b.isnan()
    ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(ia.masked_fill(na, 0), ib.masked_fill(nb, 0))


def _floats(n, gen, misaligned):
    """n random floats whose base pointer is 16-byte aligned, or off it by one float"""
    store = torch.randn(n + 1, device=DEV, generator=gen)
    return store[1:] if misaligned else store[:n]


def _guarded(n, misaligned):
    """-> (the whole NaN-filled buffer, the n floats in its middle, their offset)"""
    off = GUARD + (1 if misaligned else 0)
    buf = torch.full((off + n + GUARD,), float("nan"), device=DEV)
    return buf, buf[off:off + n], off


def _untouched_around(buf, off, n):
    return bool(buf[:off].isnan().all()) and bool(buf[off + n:].isnan().all())


def _rows(B, n, n_base, gen):
    """alpha with an exact 0 and an exact 1, idx with repeats covering every baseline"""
    R_ = B * n
    alpha = torch.rand(R_, device=DEV, generator=gen)
    alpha[0], alpha[min(1, R_ - 1)] = 0.0, 1.0
    idx = (torch.arange(R_, device=DEV) * 2 // 3 + 2) % n_base               # 2, 2, 0, 0, 1, 2, 2, ... for three baselines
    return alpha, idx


# name, B, n, (C, H, W), N_b, x per row, base pointers off by one float
KERNEL_CASES = [("scalar147", 2, 5, (3, 7, 7), 1, False, False),            # E = 147: the scalar path
                ("scalar147_rows", 2, 5, (3, 7, 7), 3, True, False),
                ("vec192", 2, 5, (3, 8, 8), 3, False, False),               # E = 192: the 16-byte path
                ("vec192_rows", 2, 5, (3, 8, 8), 1, True, False),
                ("vec192_off", 2, 5, (3, 8, 8), 3, False, True),            # the same E on pointers that are 4-byte aligned only
                ("vec192_off_rows", 2, 5, (3, 8, 8), 3, True, True),
                ("n1", 3, 1, (3, 8, 8), 3, False, False),
                ("n1_scalar_rows", 3, 1, (3, 7, 7), 1, True, False),
                ("n7_c1", 2, 7, (1, 12, 12), 3, True, False),
                ("n7_c4_blocks", 3, 7, (4, 36, 36), 3, False, False),       # several workgroups, a partial last one
                ("c4_scalar", 2, 5, (4, 5, 7), 3, False, False),
                ("224", 2, 5, (3, 224, 224), 1, False, False)]


def _kernel_inputs(case, seed):
    name, B, n, shape, n_base, per_row, off = case
    gen = torch.Generator(device=DEV).manual_seed(seed)
    E = shape[0] * shape[1] * shape[2]
    x = _floats((B * n if per_row else B) * E, gen, off).view(-1, *shape)
    base = _floats(n_base * E, gen, off).view(n_base, *shape)
    alpha_store = _floats(B * n, gen, off)
    alpha, idx = _rows(B, n, n_base, gen)
    alpha_store.copy_(alpha)
    return x, base, alpha_store, idx


# ------------------------------------------------------------------------------------------------ K34
@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_k34_equals_the_torch_expression_bit_for_bit(case):
    from xai_engine import kernels as K
    name, B, n, shape, n_base, per_row, off = case
    x, base, alpha, idx = _kernel_inputs(case, 51)
    gen = torch.Generator(device=DEV).manual_seed(52)
    _sprinkle(x, gen, every=7)
    _sprinkle(base, gen, every=9)
    assert float(alpha[0]) == 0.0 and float(alpha[min(1, B * n - 1)]) == 1.0
    seen = set(idx.tolist())
    assert n_base == 1 or (len(seen) < idx.numel() and (idx.numel() < 5 or len(seen) == n_base))    # repeats, and every baseline
    E = x[0].numel()
    xr = (x if per_row else x.repeat_interleave(n, 0)).reshape(B * n, E)
    a = alpha.clone()
    want = a.view(-1, 1) * xr + (1 - a).view(-1, 1) * base.reshape(n_base, E)[idx]
    assert bool(want.isnan().any()) and bool(want.isinf().any())
    buf, out, at = _guarded(B * n * E, off)
    got = K.gshap_scale(x, base, alpha, idx, n, out=out.view(B * n, *shape))
    assert got.data_ptr() == out.data_ptr() and (got.data_ptr() % 16 != 0) == off
    assert _bits_equal_nan_aware(got.reshape(B * n, E), want)
    assert _untouched_around(buf, at, B * n * E)
    # alpha == 1 hands the input through and alpha == 0 the baseline, up to the 0 * value term: finite values exactly
    fin = xr[min(1, B * n - 1)].isfinite() & base.reshape(n_base, E)[idx[min(1, B * n - 1)]].isfinite()
    assert torch.equal(got.reshape(B * n, E)[min(1, B * n - 1)][fin], xr[min(1, B * n - 1)][fin])
    if name == "vec192":                                                            # the allocating form
        assert _bits_equal_nan_aware(K.gshap_scale(x, base, alpha, idx, n).reshape(B * n, E), want)


# ------------------------------------------------------------------------------------------------ K35
_WANT35 = {}


def _k35_case(case):
    """inputs on the device and the loop's result, computed once per case on the host"""
    name, B, n, shape, n_base, per_row, off = case
    if name not in _WANT35:
        x, base, _, idx = _kernel_inputs(case, 61)
        gen = torch.Generator(device=DEV).manual_seed(62)
        grads = _floats(B * n * x[0].numel(), gen, off).view(B * n, *shape)
        # one pixel of image 0 whose terms are all -0: the difference is +0 there, the gradient negative
        base[:, 0, 1, 2] = 0.25
        (x[:n] if per_row else x[:1])[:, 0, 1, 2] = 0.25
        grads[:n, 0, 1, 2] = -grads[:n, 0, 1, 2].abs() - 1.0
        xc, bc, gc, ic = x.cpu(), base.cpu(), grads.cpu(), idx.cpu()
        attr = torch.zeros(B, *shape)
        for b in range(B):
            acc = torch.zeros(shape)                                               # +0
            for s in range(n):                                                     # ascending
                r = b * n + s
                acc = acc + (xc[r if per_row else b] - bc[ic[r]]) * gc[r]
            attr[b] = acc / torch.tensor(float(n))                                 # a true fp32 division
        m = attr[:, 0]
        for c in range(1, shape[0]):                                               # channels ascending
            m = m + attr[:, c]
        _WANT35[name] = (x, base, idx, grads, attr.to(DEV), m.abs().to(DEV))
    return _WANT35[name]


@pytest.mark.parametrize("outputs", ["attr", "map", "both"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_k35_equals_the_loop_in_the_stated_order_bit_for_bit(case, outputs):
    from xai_engine import kernels as K
    name, B, n, shape, n_base, per_row, off = case
    x, base, idx, grads, want_attr, want_map = _k35_case(case)
    Cc, H, W = shape
    n_attr, n_map = B * Cc * H * W, B * H * W
    abuf, attr, a_at = _guarded(n_attr, off)
    mbuf, map_, m_at = _guarded(n_map, off)
    wa, wm = outputs in ("attr", "both"), outputs in ("map", "both")
    out = K.gshap_finish(grads, x, base, idx, n, want_attr=wa, want_map=wm, attr=attr.view(B, Cc, H, W) if wa else None,
                         map=map_.view(B, H, W) if wm else None)
    got_attr, got_map = out if outputs == "both" else ((out, None) if wa else (None, out))
    if wa:
        assert got_attr.data_ptr() == attr.data_ptr() and _bits_equal_nan_aware(got_attr, want_attr)
        assert int(got_attr[0, 0, 1, 2].view(torch.int32)) == 0                    # all terms -0: the sum from +0 is +0
        assert float(got_attr.abs().max()) > 0
    else:
        assert bool(abuf.isnan().all())                                            # the buffer not asked for is untouched
    if wm:
        assert got_map.data_ptr() == map_.data_ptr() and _bits_equal_nan_aware(got_map, want_map)
    else:
        assert bool(mbuf.isnan().all())
    assert _untouched_around(abuf, a_at, n_attr) and _untouched_around(mbuf, m_at, n_map)
    if name == "vec192" and outputs == "both":                                     # the allocating form
        a2, m2 = K.gshap_finish(grads, x, base, idx, n, want_attr=True, want_map=True)
        assert _bits_equal_nan_aware(a2, want_attr) and _bits_equal_nan_aware(m2, want_map)


def test_k35_reference_has_the_minus_zero_pixel_and_the_division_is_no_reciprocal():
    """the yardstick itself: the marked pixel's terms are all -0, and x / 7 differs from x * (1 / 7) somewhere in the n = 7 case"""
    case = next(c for c in KERNEL_CASES if c[0] == "n7_c4_blocks")
    x, base, idx, grads, want_attr, _ = _k35_case(case)
    n = case[2]
    terms = (x[:1, 0, 1, 2] - base[idx[:n], 0, 1, 2]) * grads[:n, 0, 1, 2]
    assert torch.equal(terms.view(torch.int32), torch.full((n,), -2 ** 31, dtype=torch.int32, device=DEV))
    acc = want_attr.cpu() * 0
    xc, bc, gc, ic = x.cpu(), base.cpu(), grads.cpu(), idx.cpu()
    for b in range(case[1]):
        for s in range(n):
            acc[b] = acc[b] + (xc[b] - bc[ic[b * n + s]]) * gc[b * n + s]
    assert not torch.equal(acc * torch.tensor(1.0 / 7.0), want_attr.cpu())


def test_wrappers_refuse_inconsistent_arguments_before_the_launch():
    from xai_engine import kernels as K
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)      # noqa: E731
    x, base, alpha, idx, g = z(2, 3, 8, 8), z(3, 3, 8, 8), z(10), z(10, dtype=torch.int64), z(10, 3, 8, 8)
    for bad in (dict(alpha=z(7)), dict(base=z(3, 3, 8, 9)), dict(base=z(3, 8, 8)), dict(base=z(0, 3, 8, 8)), dict(x=z(3, 3, 8, 8)),
                dict(idx=z(9, dtype=torch.int64)), dict(n=0)):
        kw = dict(x=x, base=base, alpha=alpha, idx=idx, n=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            K.gshap_scale(kw["x"], kw["base"], kw["alpha"], kw["idx"], kw["n"])
    with pytest.raises(TypeError):
        K.gshap_scale(x, base, alpha, z(10, dtype=torch.int32), 5)
    with pytest.raises(ValueError):
        K.gshap_scale(x, base, alpha, idx, 5, out=z(9, 3, 8, 8))
    for bad in (dict(g=z(10, 3, 64)), dict(g=z(7, 3, 8, 8)), dict(x=z(2, 3, 8, 4)), dict(base=z(3, 1, 8, 8)), dict(idx=z(5, dtype=torch.int64))):
        kw = dict(g=g, x=x, base=base, idx=idx)
        kw.update(bad)
        with pytest.raises(ValueError):
            K.gshap_finish(kw["g"], kw["x"], kw["base"], kw["idx"], 5)
    with pytest.raises(ValueError):
        K.gshap_finish(g, x, base, idx, 5, want_attr=False, want_map=False)
    with pytest.raises(ValueError):
        K.gshap_finish(g, x, base, idx, 5, want_map=True, map=z(2, 8, 7))
    assert tuple(K.gshap_scale(x, base, alpha, idx, 5).shape) == (10, 3, 8, 8)
    assert tuple(K.gshap_finish(g, z(10, 3, 8, 8), base, idx, 5, want_attr=False, want_map=True).shape) == (2, 8, 8)      # one input per row


# ------------------------------------------------------------------------------------------------ the whole classifier
_CACHE = {}


def _inputs(B, hw):
    x = torch.randn(B, 3, hw, hw, generator=torch.Generator().manual_seed(15 + hw)).to(DEV)
    t = torch.tensor([3, 7, 1][:B]).to(DEV)
    return x, t


def _baselines(n_base, hw):
    return (torch.randn(n_base, 3, hw, hw, generator=torch.Generator().manual_seed(25 + hw)) * 0.5 + 0.1).to(DEV)


def _draws(n_base, rows, seed=0):
    """not NumPy's global state: every run of a case gets the same arrays"""
    rs = np.random.RandomState(100 + seed)
    return rs.randint(0, n_base, rows).astype(np.int64), rs.uniform(0.0, 1.0, rows).astype(np.float32)


def _restated(B, hw, n_base, pass_images=None, full=False):
    """computed once per shape and cut, shared, never written to"""
    key = ("restated", B, hw, n_base, pass_images, full)
    if key not in _CACHE:
        x, t = _inputs(B, hw)
        _CACHE[key] = R.gradient_shap(_model(full), x, t, _baselines(n_base, hw), n_samples=5, pass_images=pass_images,
                                      draws=_draws(n_base, 5 * B))
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["fused", "forked", "unfused"])
@pytest.mark.parametrize("n_base", [1, 3])
@pytest.mark.parametrize("B,hw", [(2, 64), (1, 80)])
def test_gradient_shap_equals_the_restated_captum_flow(kind, B, hw, n_base):
    from xai_engine.gshap import gradient_shap_batch
    assert torch.backends.cudnn.deterministic
    model = _variant(kind)
    x, t = _inputs(B, hw)
    base = _baselines(n_base, hw)
    want = _restated(B, hw, n_base)
    assert float(want.abs().max()) > 0
    for graphs in (False, True):
        tag = f"{kind}/B{B}x{hw}/Nb{n_base}/{'replay' if graphs else 'eager'}"
        attr, m = gradient_shap_batch(x, model, t, base, n_samples=5, want_attr=True, want_map=True, graphs=graphs, draws=_draws(n_base, 5 * B))
        assert tuple(attr.shape) == (B, 3, hw, hw) and tuple(m.shape) == (B, hw, hw)
        check(f"gshap/attr/{tag}", attr.cpu().numpy(), want.cpu().numpy(), BAR, against="restated")
        for b in range(B):
            check(f"gshap/map{b}/{tag}", m[b].cpu().numpy(), R.harness_map(want[b]), BAR, against="restated")


@pytest.mark.parametrize("pass_images", [1, 2])
def test_a_batch_cut_into_passes_equals_the_restatement_run_at_that_cut(pass_images):
    from xai_engine.gshap import gradient_shap_batch
    model = _variant("forked")
    x, t = _inputs(3, 64)
    base = _baselines(3, 64)
    want = _restated(3, 64, 3, pass_images=pass_images)
    got = gradient_shap_batch(x, model, t, base, pass_images=pass_images, draws=_draws(3, 15))
    check(f"gshap/attr/forked/B3x64/cut{pass_images}", got.cpu().numpy(), want.cpu().numpy(), BAR, against="restated")
    only_map = gradient_shap_batch(x, model, t, base, want_attr=False, want_map=True, pass_images=pass_images, draws=_draws(3, 15))
    check(f"gshap/map/forked/B3x64/cut{pass_images}", only_map[2].cpu().numpy(), R.harness_map(want[2]), BAR, against="restated")


def test_noise_comes_from_the_device_generator_in_the_restated_order():
    from xai_engine.gshap import gradient_shap_batch
    model = _variant("fused")
    x, t = _inputs(2, 64)
    base = _baselines(1, 64)
    torch.cuda.manual_seed(11)
    want = R.gradient_shap(_model(), x, t, base, n_samples=5, stdevs=0.1, draws=_draws(1, 10))
    torch.cuda.manual_seed(11)
    got = gradient_shap_batch(x, model, t, base, stdevs=0.1, draws=_draws(1, 10))
    check("gshap/attr/fused/B2x64/stdevs0.1", got.cpu().numpy(), want.cpu().numpy(), BAR, against="restated")
    assert float((want - _restated(2, 64, 1)).abs().max()) > 1e-3 * float(want.abs().max())     # the noise is no detail
    torch.cuda.manual_seed(11)
    cut = gradient_shap_batch(x, model, t, base, stdevs=0.1, pass_images=1, draws=_draws(1, 10))  # drawn before the batch is cut
    torch.cuda.manual_seed(11)
    want_cut = R.gradient_shap(_model(), x, t, base, n_samples=5, stdevs=0.1, pass_images=1, draws=_draws(1, 10))
    check("gshap/attr/fused/B2x64/stdevs0.1/cut1", cut.cpu().numpy(), want_cut.cpu().numpy(), BAR, against="restated")


def test_graph_replay_is_bitwise_the_eager_pass_and_is_captured_once():
    from xai_engine import gshap
    assert torch.backends.cudnn.deterministic
    model = _variant("forked")
    x, t = _inputs(2, 64)
    base = _baselines(3, 64)
    runs = [(x, _draws(3, 10, seed=1)), (x.flip(0).contiguous(), _draws(3, 10, seed=2))]
    assert not np.array_equal(runs[0][1][1], runs[1][1][1])
    gshap._PASSES.entries().clear()
    before = dict(gshap.GSHAP_COUNTS)

    def run(v, d, graphs):
        return gshap.gradient_shap_batch(v, model, t, base, want_attr=True, want_map=True, graphs=graphs, draws=d)
    eager = [run(v, d, False) for v, d in runs]
    replay = [run(v, d, True) for v, d in runs + runs[:1]]
    for e, r in zip(eager + eager[:1], replay):
        assert torch.equal(e[0].view(torch.int32), r[0].view(torch.int32)) and torch.equal(e[1].view(torch.int32), r[1].view(torch.int32))
    assert not torch.equal(run(x, runs[1][1], False)[0], eager[0][0])              # the draws matter, not only the input
    d = {k: gshap.GSHAP_COUNTS[k] - before[k] for k in before}
    assert d == {"captures": 1, "captures_refused": 0, "replayed": 3, "eager": 3}, d
    assert len(gshap._PASSES.entries()) == 1


def test_two_streams_equal_one_stream_bit_for_bit():
    from xai_engine.gshap import gradient_shap_batch
    model = _variant("forked")
    x, t = _inputs(2, 64)
    base = _baselines(3, 64)
    one = gradient_shap_batch(x, model, t, base, want_attr=True, want_map=True, pass_images=1, streams=1, draws=_draws(3, 10))
    two = gradient_shap_batch(x, model, t, base, want_attr=True, want_map=True, pass_images=1, streams=2, draws=_draws(3, 10))
    torch.cuda.synchronize()
    assert torch.equal(one[0].view(torch.int32), two[0].view(torch.int32)) and torch.equal(one[1].view(torch.int32), two[1].view(torch.int32))


def test_harness_row_returns_the_restated_map():
    from xai_engine.sweep import get_CNN_attr
    model = _variant("forked")
    x, t = _inputs(1, 80)
    torch.manual_seed(7)
    np.random.seed(7)
    base = torch.randn(1, 3, 80, 80).to(DEV)                                       # the row's baseline: the CPU generator, then uploaded
    want = R.harness_map(R.gradient_shap(_model(), x, t, base, n_samples=5)[0])
    td = {"models": [model], "batch_size": 50, "img_hw": 80, "device": DEV, "attr_func": "gs"}
    torch.manual_seed(7)
    np.random.seed(7)
    host = get_CNN_attr(x.cpu(), None, t[0], td)
    assert isinstance(host, np.ndarray) and host.shape == (80, 80) and host.dtype == np.float32
    check("gshap/harness/numpy", host, want, BAR, against="restated")
    torch.manual_seed(7)
    np.random.seed(7)
    dev_map = get_CNN_attr(x, None, t[0], dict(td, device_maps=True))
    assert torch.is_tensor(dev_map) and dev_map.is_cuda and tuple(dev_map.shape) == (80, 80)
    check("gshap/harness/device", dev_map.cpu().numpy(), want, BAR, against="restated")
    # the row is no `grad` row: the map of the plain gradient is far from it
    xr = x.clone().requires_grad_(True)
    (plain,) = torch.autograd.grad(_model()(xr).gather(1, t.view(-1, 1)).sum(), xr)
    assert np.abs(R.harness_map(plain[0]) - want).max() > 0.1 * want.max()


def test_evaluate_perturbation_runs_the_gs_row_end_to_end(tmp_path, monkeypatch):
    """a sweep of a few synthetic images with --attr_func gs through the harness: every image attributed, the CSV written"""
    from PIL import Image
    from xai_engine import harness
    model = _variant("forked")
    rng = np.random.default_rng(5)
    names = []
    for i in range(3):
        name = f"ILSVRC2012_val_{i + 1:08d}.png"
        Image.fromarray((rng.random((70, 76, 3)) * 255).astype(np.uint8)).save(tmp_path / name)
        names.append(name)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    monkeypatch.setattr(harness, "select_images", lambda td, cc, rank=0, world=1, lazy=False:
                        (names, harness.SelectedImages(str(tmp_path), names, 64, *norm), [0, 0, 0]))
    td = {"models": [model, model], "img_hw": 64, "batch_size": 25, "device": DEV, "attr_func": "gs", "normalize": norm,
          "imagenet_dataset": str(tmp_path), "model_name": "R50", "image_count": 3}
    total, used, _ = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"), streams=3)
    assert used == 3 and all(np.isfinite(float(v)) for v in total.values())
    assert os.path.exists(tmp_path / "out" / "R50" / "gs_3_images.csv")


def test_captum_shaped_class_equals_the_driver():
    from xai_engine import gshap
    model = _variant("fused")
    x, t = _inputs(2, 64)
    base = _baselines(3, 64)
    np.random.seed(3)
    want = gshap.gradient_shap_batch(x, model, t, base)
    np.random.seed(3)
    got = gshap.GradientShap(model).attribute(x, base, target=t)
    assert got.is_cuda and torch.equal(got.view(torch.int32), want.view(torch.int32))
    np.random.seed(3)
    idx, alpha = R.draw(3, 10)                                                     # and both drew what the restatement draws
    check("gshap/class/fused/B2x64", got.cpu().numpy(),
          R.gradient_shap(_model(), x, t, base, draws=(idx, alpha)).cpu().numpy(), BAR, against="restated")
    seven = gshap.GradientShap(model).attribute(x, base, n_samples=7, target=t)
    assert tuple(seven.shape) == tuple(x.shape) and not torch.equal(seven, got)


def test_resnet50_at_224_equals_the_restated_flow():
    from xai_engine.gshap import gradient_shap_batch
    model = _variant("forked", full=True)
    x, t = _inputs(1, 224)
    base = _baselines(1, 224)
    want = _restated(1, 224, 1, full=True)
    attr, m = gradient_shap_batch(x, model, t, base, n_samples=5, want_attr=True, want_map=True, draws=_draws(1, 5))
    check("gshap/attr/resnet50_224/forked/replay", attr.cpu().numpy(), want.cpu().numpy(), BAR, against="restated")
    check("gshap/map/resnet50_224/forked/replay", m[0].cpu().numpy(), R.harness_map(want[0]), BAR, against="restated")
