"""AGI on the MI355X: K24 step by step against the reference's own recorded runs (tests/golden/agi.npz), K25 against live
np.percentile, K23's argmax against torch, agi_batch end to end, the device's own per-iteration values at full size replayed
through the NumPy restatement (tests/agi_restated.py), graphs / streams / repeats, and the harness row."""
import os

import numpy as np
import pytest
import torch

import agi_restated as R
import gig_edges
from conftest import check, load_golden
from helpers import tiny_from

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("a", "b", "c", "d", "e")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_map(name, got, want):
    """equal NaN positions, equal infinities, and the finite rest exactly (through conftest.check, tol 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]) and np.isinf(got).sum() == np.isinf(want).sum(), name
    fin = np.isfinite(want)
    check(name, got[fin] if fin.any() else np.zeros(1), want[fin] if fin.any() else np.zeros(1), 0.0, absolute=True, against="NumPy")


def _case(g, tag):
    eps, max_iter = g[f"{tag}_params"].tolist()
    return g[f"{tag}_data"], g[f"{tag}_classes"].tolist(), int(g[f"{tag}_init_pred"]), float(eps), int(max_iter)


@pytest.mark.parametrize("tag", CASES)
def test_k24_step_by_step_matches_the_reference(tag):
    """K23 on the reference's initial logits, then K24 fed the reference's logits and gradients of every iteration: every x_i,
    c_delta, break iteration and state word bit for bit; K25 gives the reference's step_grad and map."""
    from xai_engine import kernels as K
    g = load_golden("agi.npz")
    data_h, classes, ip, eps, max_iter = _case(g, tag)
    pair, fx, fl, fga, fgl = (g[f"{tag}_{k}"] for k in ("pair", "fx", "fl", "fga", "fgl"))
    Kc, n_out = len(classes), g[f"{tag}_init_logits"].shape[0]
    data = torch.from_numpy(data_h).to(DEV)
    cls = torch.tensor(classes, dtype=torch.int32).to(DEV)
    x = torch.empty((Kc,) + data_h.shape[1:], device=DEV)
    cd, state = torch.empty_like(x), torch.empty((Kc, 4), dtype=torch.int32, device=DEV)
    ipd = torch.empty(1, dtype=torch.int64, device=DEV)
    K.agi_init(torch.from_numpy(g[f"{tag}_init_logits"][None]).to(DEV), data, cls, ipd, x, cd, state)
    assert int(ipd[0]) == ip
    fwd = [np.flatnonzero(pair == c) for c in classes]
    for i in range(max_iter):
        lg = np.zeros((Kc, n_out), np.float32)
        ga, gl = np.zeros((Kc,) + data_h.shape[1:], np.float32), np.zeros((Kc,) + data_h.shape[1:], np.float32)
        for k in range(Kc):
            if i < len(fwd[k]):
                j = fwd[k][i]
                np.testing.assert_array_equal(_bits(x[k].cpu().numpy()), _bits(fx[j]), err_msg=f"{tag}: x of forward {i}, pair {k}")
                lg[k], ga[k], gl[k] = fl[j], fga[j], fgl[j]
        K.agi_step(torch.from_numpy(lg).to(DEV), torch.from_numpy(ga).to(DEV), torch.from_numpy(gl).to(DEV), data, cls, eps, max_iter,
                   x, cd, state)
    st = state.cpu().numpy()
    pairs, step_grad = R.run(data_h[0], classes, ip, eps, max_iter, lambda k: (lambda i, xx: (fl[fwd[k][i]], fga[fwd[k][i]], fgl[fwd[k][i]])))
    for k, c in enumerate(classes):
        if pairs[k] is None:
            assert st[k].tolist() == [0, 0, 2, 0], (tag, k, st[k])
            continue
        _, c_want, n, broke = pairs[k]
        assert st[k, 0] == 0 and st[k, 1] == n and st[k, 2] == (1 if broke else 3), (tag, k, st[k], n, broke)
        np.testing.assert_array_equal(_bits(cd[k].cpu().numpy()), _bits(c_want))
    hm = torch.empty((1,) + data_h.shape[2:], device=DEV)
    sg = torch.empty_like(data)
    K.agi_heatmap(cd, 1, 80, 99, out=hm, step_grad=sg)
    if g[f"{tag}_zero"]:
        assert (st[:, 1] == 0).all() and not sg.any()
        return
    np.testing.assert_array_equal(_bits(sg[0].cpu().numpy()), _bits(g[f"{tag}_adv"]))
    _same_map(f"agi/k25/{tag}/map", hm[0].cpu().numpy(), g[f"{tag}_hm"])
    np.testing.assert_array_equal(_bits(hm[0].cpu().numpy()), _bits(g[f"{tag}_hm"]))


def _maps():
    rng = np.random.default_rng(21)
    out = []
    for n in (50176, 1, 2, 7, 50177, 1023, 1025, 2049):
        out.append((f"random_{n}", rng.standard_normal(n).astype(np.float32)))
    out.append(("ties", np.round(rng.standard_normal(50176) * 2).astype(np.float32)))
    out.append(("constant", np.full(50176, 0.25, np.float32)))
    z = rng.standard_normal(50176).astype(np.float32)
    z[::3] = -0.0
    z[1::7] = 0.0
    out.append(("signed_zeros", z))
    w = rng.standard_normal(50176).astype(np.float32)
    w[5], w[77] = np.inf, -np.inf
    out.append(("infinities", w))
    w2 = rng.standard_normal(7).astype(np.float32)
    w2[3] = np.inf
    out.append(("inf_7", w2))
    # where the three-pass radix select has to work (select_digit, which K22 shares): keys that share their top 22 bits, their top 11
    # bits, and keys on both sides of digit boundaries (powers of two +- 1 ulp); the gradient kinds of tests/gig_edges.py
    gen = np.random.default_rng(22)
    for kind in ("band", "mid_band", "pow2"):
        for n in (50176, 2049):
            out.append((f"{kind}_{n}", gig_edges.gradient(kind, n, gen).numpy()))
    v = rng.standard_normal(50176).astype(np.float32)
    v[1234] = np.nan
    out.append(("nan", v))
    return out


@pytest.mark.parametrize("qs", [(80, 99), (0, 100), (50, 50.5)])
def test_k25_matches_numpy_percentile_and_the_clip(qs):
    from xai_engine import kernels as K
    for name, m in _maps():
        n = m.size
        cd = torch.from_numpy(m).view(1, 1, 1, n).to(DEV)
        qu = torch.empty((1, 2), device=DEV)
        sg = torch.empty((1, 1, 1, n), device=DEV)
        out = K.agi_heatmap(cd, 1, qs[0], qs[1], step_grad=sg, qu=qu)
        step_grad = (np.float32(0) + m).astype(np.float32)          # the reference's `step_grad = 0; step_grad += c_delta`
        np.testing.assert_array_equal(_bits(sg.cpu().numpy().ravel()), _bits(step_grad))
        with np.errstate(invalid="ignore"):
            want_q = [np.percentile(step_grad, q) for q in qs]
        np.testing.assert_array_equal(qu.cpu().numpy()[0], np.array(want_q, np.float32), err_msg=f"{name} {qs}")
        _same_map(f"agi/k25/numpy/{name}/{qs[0]}_{qs[1]}", out.cpu().numpy()[0, 0], R.harness_map(step_grad[None, None], *qs)[0])


def test_k25_sums_pairs_in_class_order_and_averages_channels():
    from xai_engine import kernels as K
    rng = np.random.default_rng(5)
    B, Kc, C, H, W = 3, 4, 3, 224, 224
    cd = rng.standard_normal((B * Kc, C, H, W)).astype(np.float32) * 1e-3
    out = torch.empty((B, H, W), device=DEV)
    sg = torch.empty((B, C, H, W), device=DEV)
    K.agi_heatmap(torch.from_numpy(cd).to(DEV), B, 80, 99, out=out, step_grad=sg)
    for b in range(B):
        s = np.zeros((C, H, W), np.float32)
        for k in range(Kc):
            s = (s + cd[b * Kc + k]).astype(np.float32)
        np.testing.assert_array_equal(_bits(sg[b].cpu().numpy()), _bits(s))
        _same_map(f"agi/k25/pairs/{b}", out[b].cpu().numpy(), R.harness_map(s))


def test_k23_argmax_matches_torch_with_ties_and_nan():
    from xai_engine import kernels as K
    lg = torch.randn(9, 1000, generator=torch.Generator().manual_seed(2))
    lg[1, 7] = lg[1, 900] = lg[1].max() + 1                              # tie: the first
    lg[2, 500] = float("nan")
    lg[3, 10] = lg[3, 999] = float("nan")                                # NaNs: the first
    lg[4, 999] = float("nan")
    lg[4, 0] = float("inf")
    lg[5] = 0.0                                                           # all equal
    lg[6, 3] = float("inf")
    lg[6, 4] = float("inf")
    lg[7] = float("-inf")
    lg[8, :3] = float("nan")
    want = lg.max(1)[1]
    data = torch.zeros((9, 4), device=DEV)
    cls = torch.tensor([0], dtype=torch.int32).to(DEV)
    x, cd = torch.empty_like(data), torch.empty_like(data)
    state = torch.empty((9, 4), dtype=torch.int32, device=DEV)
    ip = torch.empty(9, dtype=torch.int64, device=DEV)
    K.agi_init(lg.to(DEV), data, cls, ip, x, cd, state)
    assert torch.equal(ip.cpu(), want), (ip.cpu(), want)
    assert state.cpu()[:, 0].tolist() == [int(w != 0) for w in want.tolist()]
    # K24 decides with the same rule: a pair whose argmax is its class stops
    lg2 = torch.zeros((9, 1000))
    lg2[:, 0] = float("nan")
    K.agi_step(lg2.to(DEV), torch.ones_like(data), torch.ones_like(data), data, cls, 0.05, 20, x, cd, state)
    assert (state.cpu()[:, 0] == 0).all() and (state.cpu()[:, 3] == 0).all()


@pytest.mark.parametrize("tag", CASES)
def test_agi_batch_matches_the_reference(tag):
    from xai_engine.agi import agi_batch
    g = load_golden("agi.npz")
    data_h, classes, ip, eps, max_iter = _case(g, tag)
    model = tiny_from(g, DEV)
    sg, init_pred, iters, m = agi_batch(torch.from_numpy(data_h).to(DEV), model, classes, epsilon=eps, max_iter=max_iter,
                                        normalize=(g["mean"], g["std"]), want_map=True)
    assert int(init_pred[0]) == ip
    for k, c in enumerate(classes):
        n_fwd = int((g[f"{tag}_pair"] == c).sum())
        broke = n_fwd > 0 and int(np.argmax(g[f"{tag}_fl"][np.flatnonzero(g[f"{tag}_pair"] == c)[-1]])) == c
        assert int(iters[0, k]) == n_fwd - int(broke), (tag, c, int(iters[0, k]), n_fwd, broke)
    if g[f"{tag}_zero"]:
        assert int(iters.max()) == 0 and not sg.any()
        return
    check(f"agi/agi_batch/{tag}/step_grad", sg[0].cpu().numpy(), g[f"{tag}_adv"], 1e-5)
    check(f"agi/agi_batch/{tag}/map", m[0].cpu().numpy(), np.abs(g[f"{tag}_hm"]), 1e-5)


def _record(monkeypatch):
    from xai_engine import kernels as K
    log = []
    real = K.agi_step

    def recording(logits, g_adv, g_lab, data, classes, epsilon, max_iter, x_cur, c_delta, state):
        before = x_cur.cpu()
        real(logits, g_adv, g_lab, data, classes, epsilon, max_iter, x_cur, c_delta, state)
        log.append((logits.cpu(), g_adv.cpu(), g_lab.cpu(), before, state.cpu()))
    monkeypatch.setattr(K, "agi_step", recording)
    return log


def _replay_device(log, data, classes, init_pred, eps, max_iter, step_grad, iters, m):
    """the device's own per-iteration values through the restatement: x, state, step_grad and map bit for bit"""
    Kc = len(classes)
    assert len(log) == max_iter
    for b in range(data.shape[0]):
        def oracle_of(k, b=b):
            p = b * Kc + k

            def oracle(i, x):
                logits, ga, gl, before, _ = log[i]
                np.testing.assert_array_equal(_bits(x), _bits(before[p].numpy()), err_msg=f"x of iteration {i}, image {b}, pair {k}")
                return logits[p].numpy(), ga[p].numpy(), gl[p].numpy()
            return oracle
        pairs, sgr = R.run(data[b], classes, int(init_pred[b]), eps, max_iter, oracle_of)
        final = log[-1][4]
        for k in range(Kc):
            n = 0 if pairs[k] is None else pairs[k][2]
            assert int(iters[b, k]) == n and int(final[b * Kc + k, 1]) == n, (b, k)
            if pairs[k] is not None:
                assert int(final[b * Kc + k, 2]) == (1 if pairs[k][3] else 3), (b, k, final[b * Kc + k])
        if sgr is None:
            assert not step_grad[b].any()
            continue
        np.testing.assert_array_equal(_bits(step_grad[b].cpu().numpy()), _bits(sgr))
        np.testing.assert_array_equal(_bits(m[b].cpu().numpy()), _bits(np.abs(R.harness_map(sgr))))


def test_tinynet_224_records_replay_through_the_restatement(monkeypatch):
    from xai_engine.agi import agi_batch, pre_processing
    g = load_golden("agi.npz")
    model = tiny_from(g, DEV)
    rng = np.random.default_rng(8)
    img = rng.random((224, 224, 3)).astype(np.float32)
    data = pre_processing(img, DEV)
    log = _record(monkeypatch)
    sg, ip, iters, m = agi_batch(data, model, [0], normalize=(g["mean"], g["std"]), graphs=False, want_map=True)
    assert int(iters.max()) > 0
    _replay_device(log, data.cpu().numpy(), [0], ip.cpu(), 0.05, 20, sg, iters, m)


def test_resnet50_records_replay_through_the_restatement(monkeypatch):
    from xai_engine.agi import agi_batch
    from xai_engine.harness import CNN_MEAN, CNN_STD
    from xai_engine.zoo import resnet50
    model = resnet50(seed=0).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    data = (torch.rand(4, 3, 224, 224, generator=torch.Generator().manual_seed(6)) / 255).to(DEV)
    classes = list(range(0, 999, int(1000 / 3)))
    log = _record(monkeypatch)
    sg, ip, iters, m = agi_batch(data, model, classes, normalize=(CNN_MEAN, CNN_STD), graphs=False, want_map=True)
    _replay_device(log, data.cpu().numpy(), classes, ip.cpu(), 0.05, 20, sg, iters, m)
    assert torch.isfinite(sg).all()


def _tiny_batch(B=5, hw=32, seed=3):
    g = load_golden("agi.npz")
    model = tiny_from(g, DEV)
    x = (torch.rand(B, 3, hw, hw, generator=torch.Generator().manual_seed(seed)) / 255).to(DEV)
    return model, x, (g["mean"], g["std"])


def test_graphs_streams_and_repeats_are_bit_identical():
    from xai_engine import agi
    model, x, norm = _tiny_batch()
    kw = dict(normalize=norm, want_map=True, images_per_pass=2)
    eager = agi.agi_batch(x, model, [0, 3, 7], graphs=False, **kw)
    before = dict(agi.AGI_COUNTS)
    first = agi.agi_batch(x, model, [0, 3, 7], **kw)
    assert agi.AGI_COUNTS["captures"] > before["captures"], agi.AGI_COUNTS
    again = agi.agi_batch(x, model, [0, 3, 7], **kw)
    assert agi.AGI_COUNTS["replayed"] >= before["replayed"] + 3 + 3, agi.AGI_COUNTS
    s3 = agi.agi_batch(x, model, [0, 3, 7], streams=3, **kw)
    for got in (first, again, s3):
        for a, b in zip(got, eager):
            assert torch.equal(a.cpu().view(torch.int32) if a.is_floating_point() else a.cpu(),
                               b.cpu().view(torch.int32) if b.is_floating_point() else b.cpu())
    assert agi.AGI_COUNTS["pair_iterations"] > agi.AGI_COUNTS["pair_iterations_used"] > 0


def _harness_td(model, norm, hw):
    return {"models": [model, model], "img_hw": hw, "batch_size": 25, "device": DEV, "attr_func": "agi", "normalize": norm}


def test_harness_row_equals_agi_batch():
    from xai_engine.agi import agi_batch, pre_processing
    from xai_engine.harness import normalize
    from xai_engine.sweep import get_CNN_attr
    g = load_golden("agi.npz")
    model = tiny_from(g, DEV)
    norm = (tuple(g["mean"].tolist()), tuple(g["std"].tolist()))
    trans = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(12))
    x = normalize(trans, *norm).unsqueeze(0)
    td = _harness_td(model, norm, 32)
    host = get_CNN_attr(x, trans, 5, td)
    devm = get_CNN_attr(x, trans, 5, dict(td, device_maps=True))
    want = agi_batch(pre_processing(trans.permute(1, 2, 0).numpy(), DEV), model, [0], normalize=norm, want_map=True)[3][0]
    assert host.shape == (32, 32) and host.dtype == np.float32
    np.testing.assert_array_equal(_bits(devm.cpu().numpy()), _bits(want.cpu().numpy()))
    np.testing.assert_array_equal(_bits(host), _bits(want.cpu().numpy()))
    with pytest.raises(ValueError, match="trans_img"):
        get_CNN_attr(x, None, 5, td)


class _Biased(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        out = self.inner(x)
        return out + torch.nn.functional.one_hot(torch.zeros(1, dtype=torch.int64, device=out.device), out.shape[1]).float() * 100.0


def test_the_reference_crash_raises_a_value_error():
    """an image predicted as class 0, the harness's only selected class: AGI.test returns (0, 0, 0) and the reference dies"""
    from xai_engine import agi
    from xai_engine.harness import normalize
    from xai_engine.sweep import get_CNN_attr
    g = load_golden("agi.npz")
    model = _Biased(tiny_from(g, DEV))
    norm = (tuple(g["mean"].tolist()), tuple(g["std"].tolist()))
    trans = torch.rand(3, 16, 16, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="class 0 has no attribution"):
        get_CNN_attr(normalize(trans, *norm).unsqueeze(0), trans, 0, _harness_td(model, norm, 16))
    assert agi.test(torch.nn.Sequential(agi.Normalize(*norm), model).to(DEV), DEV, trans.permute(1, 2, 0).numpy(), 0.05, 1, [0], 20) == (0, 0, 0)


def test_evaluate_perturbation_hands_the_row_load_images_tensor(tmp_path, monkeypatch):
    from PIL import Image
    from xai_engine import harness, sweep
    g = load_golden("agi.npz")
    model = tiny_from(g, DEV)
    rng = np.random.default_rng(4)
    names = []
    for i in range(2):
        name = f"ILSVRC2012_val_{i + 1:08d}.png"
        Image.fromarray((rng.random((40, 52, 3)) * 255).astype(np.uint8)).save(tmp_path / name)
        names.append(name)
    norm = (tuple(g["mean"].tolist()), tuple(g["std"].tolist()))
    seen = {}

    def fake_select(testing_dict, cc, rank=0, world=1, lazy=False):
        return names, harness.SelectedImages(str(tmp_path), names, 32, *norm), [0, 0]

    def recording_row(input_tensor, trans_img, target_class, testing_dict):
        seen[len(seen)] = trans_img
        return input_tensor.to(DEV)[0].sum(0).abs()
    monkeypatch.setattr(harness, "select_images", fake_select)
    monkeypatch.setattr(sweep, "get_CNN_attr", recording_row)
    td = dict(_harness_td(model, norm, 32), imagenet_dataset=str(tmp_path), model_name="R50", image_count=2)
    _, used, _ = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"), streams=1)
    assert used == 2 and len(seen) == 2
    for i, name in enumerate(names):
        want = harness.load_image(os.path.join(str(tmp_path), name), 32)
        assert seen[i].dtype == want.dtype and torch.equal(seen[i].view(torch.int32), want.view(torch.int32))


def test_evaluate_perturbation_runs_the_agi_row_end_to_end(tmp_path, monkeypatch):
    """the real row through the harness on three stream workers: every image attributed, the CSV written, and each image's map
    the one agi_batch gives for load_image's tensor"""
    from PIL import Image
    from xai_engine import harness, sweep
    from xai_engine.agi import agi_batch, pre_processing
    g = load_golden("agi.npz")
    model = tiny_from(g, DEV)
    rng = np.random.default_rng(9)
    names = []
    for i in range(3):
        name = f"ILSVRC2012_val_{i + 1:08d}.png"
        Image.fromarray((rng.random((36, 40, 3)) * 255).astype(np.uint8)).save(tmp_path / name)
        names.append(name)
    norm = (tuple(g["mean"].tolist()), tuple(g["std"].tolist()))
    maps = {}
    real = sweep.get_CNN_attr

    def keeping_row(input_tensor, trans_img, target_class, testing_dict):
        m = real(input_tensor, trans_img, target_class, testing_dict)
        maps[len(maps)] = (trans_img, m.cpu())
        return m
    monkeypatch.setattr(harness, "select_images", lambda td, cc, rank=0, world=1, lazy=False:
                        (names, harness.SelectedImages(str(tmp_path), names, 32, *norm), [0, 0, 0]))
    monkeypatch.setattr(sweep, "get_CNN_attr", keeping_row)
    td = dict(_harness_td(model, norm, 32), imagenet_dataset=str(tmp_path), model_name="R50", image_count=3)
    total, used, _ = harness.evaluate_perturbation(td, out_dir=str(tmp_path / "out"), streams=3)
    assert used == 3 and len(maps) == 3 and all(np.isfinite(float(v)) for v in total.values())
    assert os.path.exists(tmp_path / "out" / "R50" / "agi_3_images.csv")
    for trans, m in maps.values():
        want = agi_batch(pre_processing(trans.permute(1, 2, 0).numpy(), DEV), model, [0], normalize=norm, want_map=True)[3][0]
        np.testing.assert_array_equal(_bits(m.numpy()), _bits(want.cpu().numpy()))
