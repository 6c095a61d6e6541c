"""Feature Ablation / Occlusion without a GPU: the harness rows and the CLI, the captum-shaped interface of xai_engine.ablation and
its own opt-in overlay, the argument checks of K26 / K27 (made before any HIP call), and the restatement
(tests/ablation_restated.py) against the DEFINITION of the two methods computed by independent loops -- not against captum, which
is on neither machine (parity with captum itself is unpinned: DESIGN.md)."""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ablation_restated as R
from conftest import PKG
from helpers import TinyNet


def _tiny(seed=0):
    torch.manual_seed(seed)
    m = TinyNet().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_fa_and_occ_are_cnn_attributions_of_the_harness_and_the_cli():
    from xai_engine.sweep import CNN_ATTR_FUNCS
    from xai_engine.evaluate_perturbation import build_parser
    assert "fa" in CNN_ATTR_FUNCS and "occ" in CNN_ATTR_FUNCS
    text = build_parser().format_help()
    assert " fa," in text and " occ}" in text


def test_classes_carry_captums_parameter_names():
    from xai_engine import ablation
    fa = list(inspect.signature(ablation.FeatureAblation.attribute).parameters)
    assert fa[:6] == ["self", "inputs", "baselines", "target", "feature_mask", "perturbations_per_eval"]
    occ = list(inspect.signature(ablation.Occlusion.attribute).parameters)
    assert occ[:7] == ["self", "inputs", "sliding_window_shapes", "strides", "baselines", "target", "perturbations_per_eval"]
    sig = inspect.signature(ablation.Occlusion.attribute).parameters
    assert sig["strides"].default is None and sig["perturbations_per_eval"].default == 1
    assert list(inspect.signature(ablation.FeatureAblation.__init__).parameters) == ["self", "forward_func"]
    for fn in (ablation.feature_ablation_batch, ablation.occlusion_batch):
        p = inspect.signature(fn).parameters
        assert list(p)[:3] == ["x", "model", "targets"] and p["baseline"].default == 0 and "pass_size" in p and "want_map" in p


def test_engine_refuses_the_cpu_and_unsupported_call_shapes():
    from xai_engine import XaiHipError, ablation
    from xai_engine import kernels as K
    x, ident = torch.zeros(1, 3, 8, 8), torch.nn.Identity()
    mask = torch.zeros(8, 8, dtype=torch.int64)
    with pytest.raises(XaiHipError):
        ablation.feature_ablation_batch(x, ident, 0, mask)
    with pytest.raises(XaiHipError):
        ablation.occlusion_batch(x, ident, 0, (3, 4, 4), 2)
    with pytest.raises(XaiHipError):
        ablation.FeatureAblation(ident).attribute(x, target=0, feature_mask=mask)
    with pytest.raises(XaiHipError):
        ablation.Occlusion(ident).attribute(x, (3, 4, 4), strides=2, target=0)
    with pytest.raises(XaiHipError):
        K.ablate_features(x, mask.int(), 0, 1, 0, 0, 1)
    with pytest.raises(XaiHipError):
        K.ablation_finish_windows(torch.zeros(1), torch.zeros(1, 9), (4, 4), (2, 2), (1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        ablation.FeatureAblation(ident).attribute((x, x), target=0, feature_mask=mask)
    with pytest.raises(NotImplementedError):
        ablation.FeatureAblation(ident).attribute(x, target=0, feature_mask=mask, additional_forward_args=(1,))
    with pytest.raises(NotImplementedError):
        ablation.Occlusion(ident).attribute(x, (3, 4, 4), target=0, additional_forward_args=(1,))
    with pytest.raises(NotImplementedError):                           # a window that does not span all channels
        ablation._window_args((1, 4, 4), 2, x, "occ")
    assert ablation._window_args((3, 4, 4), None, x, "occ") == ((4, 4), (4, 4))
    assert ablation._window_args((3, 4, 4), 32, x, "occ") == ((4, 4), (32, 32))
    assert K.window_counts(224, 224, (64, 64), (32, 32)) == (6, 6) and K.window_counts(40, 40, (16, 16), (10, 10)) == (4, 4)
    with pytest.raises(ValueError):
        K.window_counts(40, 40, (16, 16), (17, 10))
    assert K.window_counts(40, 40, (40, 16), (99, 10)) == (1, 4)          # captum: any stride where the window cannot move
    pm = ablation.prepare_mask(ablation.harness_patch_mask(224), (1, 3, 224, 224), "cpu")
    assert (pm.id_min, pm.n_total) == (0, 196) and pm.ids.dtype == torch.int32 and tuple(pm.ids.shape) == (224, 224)
    assert torch.equal(pm.ids.long(), R.patch_mask(224))
    with pytest.raises(ValueError):
        ablation.harness_patch_mask(225)


def test_k26_k27_entry_points_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    lib = _lib.load()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def feat(x=p, ids=p, out=p, ids_C=1, n_total=4, B=1, C=3, H=8, W=8, first=0, n=2):
        return lib.xai_ablate_features_f32(x, ids, ids_C, 0, n_total, None, 0.0, B, C, H, W, first, n, out, None)
    assert feat(x=None) == -1 and feat(ids=None) == -1 and feat(out=None) == -1
    assert feat(ids_C=2) == -2 and feat(n_total=0) == -2 and feat(B=0) == -2 and feat(C=0) == -2 and feat(H=0) == -2 and feat(W=0) == -2
    assert feat(n=0) == -2 and feat(first=-1) == -2 and feat(first=3, n=2) == -2
    assert feat(B=1 << 20, n_total=1 << 20) == -3

    def win(x=p, out=p, wh=4, ww=4, sh=2, sw=2, B=1, C=3, H=8, W=8, first=0, n=2):
        return lib.xai_ablate_windows_f32(x, wh, ww, sh, sw, None, 0.0, B, C, H, W, first, n, out, None)
    assert win(x=None) == -1 and win(out=None) == -1
    assert win(wh=9) == -2 and win(ww=0) == -2 and win(sh=5) == -2 and win(sw=0) == -2 and win(H=0) == -2
    assert win(first=8, n=2) == -2 and win(n=0) == -2 and win(B=0) == -2            # 3 x 3 = 9 windows

    def ffin(s0=p, sc=p, ids=p, attr=p, samples=p, ids_C=1, n_total=4, B=1, C=3, H=8, W=8, g=2):
        return lib.xai_ablation_finish_features_f32(s0, sc, ids, ids_C, 0, n_total, B, C, H, W, g, attr, samples, None)
    assert ffin(s0=None) == -1 and ffin(sc=None) == -1 and ffin(ids=None) == -1 and ffin(attr=None, samples=None) == -1
    assert ffin(ids_C=2) == -2 and ffin(n_total=0) == -2 and ffin(B=0) == -2 and ffin(H=0) == -2 and ffin(g=0) == -2

    def wfin(s0=p, sc=p, attr=p, samples=p, wh=4, ww=4, sh=2, sw=2, B=1, C=3, H=8, W=8, g=2):
        return lib.xai_ablation_finish_windows_f32(s0, sc, wh, ww, sh, sw, B, C, H, W, g, attr, samples, None)
    assert wfin(s0=None) == -1 and wfin(sc=None) == -1 and wfin(attr=None, samples=None) == -1
    assert wfin(wh=9) == -2 and wfin(sh=5) == -2 and wfin(B=0) == -2 and wfin(C=0) == -2 and wfin(g=-1) == -2


CAPTUM = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])          # build first, then the tree holding a (stub) captum
    import captum.attr
    before = dict(vars(captum.attr))
    from util import model_utils                                               # the harness's first util import (:17)
    import xai_engine.ablation as ab
    import xai_engine.gradcam as gc
    assert captum.attr.FeatureAblation.WHO == "captum" and captum.attr.Occlusion.WHO == "captum"      # not asked: untouched
    old = ab.patch_captum()
    assert old == (before["FeatureAblation"], before["Occlusion"])
    from captum.attr import FeatureAblation, Occlusion, LayerGradCam, GuidedBackprop                  # :43
    assert FeatureAblation is ab.FeatureAblation and Occlusion is ab.Occlusion
    changed = sorted(k for k, v in vars(captum.attr).items() if before.get(k) is not v)
    assert changed == ["FeatureAblation", "Occlusion"], changed
    assert LayerGradCam.WHO == "captum" and GuidedBackprop.WHO == "captum"
    assert ab.patch_captum() == (ab.FeatureAblation, ab.Occlusion)             # idempotent
    gc.patch_captum()                                                          # the other overlay still touches its one name only
    assert captum.attr.LayerGradCam is gc.LayerGradCam and captum.attr.FeatureAblation is ab.FeatureAblation
    print("captum ok")
""")


def test_patch_captum_rebinds_exactly_the_two_names(tmp_path):
    """Stub captum in tmp_path (the technique of tests/test_cpu_shim.py); XAI_PATCH_CAPTUM=1 stays LayerGradCam's switch alone."""
    pkg = tmp_path / "site" / "captum" / "attr"
    pkg.mkdir(parents=True)
    (tmp_path / "site" / "captum" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("".join(f"class {n}: WHO = 'captum'\n" for n in ("LayerGradCam", "GuidedBackprop", "FeatureAblation", "Occlusion")))
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "XAI_PATCH_CAPTUM")}
    r = subprocess.run([sys.executable, "-c", CAPTUM, PKG, str(tmp_path / "site")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "captum ok" in r.stdout, r.stdout + r.stderr
    env["XAI_PATCH_CAPTUM"] = "1"                                  # the Grad-CAM switch does not reach these two names
    code = ("import sys; sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1]); from util import model_utils; import captum.attr as a; "
            "assert a.FeatureAblation.WHO == 'captum' and a.Occlusion.WHO == 'captum'; print('flag ok')")
    r = subprocess.run([sys.executable, "-c", code, PKG, str(tmp_path / "site")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "flag ok" in r.stdout, r.stdout + r.stderr
    env.pop("XAI_PATCH_CAPTUM")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); import xai_engine.ablation as a; "
                        "assert a.patch_captum() is None; print('none ok')", PKG], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "none ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the restatement vs the definition
def test_window_enumeration_order_and_counts():
    counts, strides = R.window_counts((3, 224, 224), (3, 64, 64), 32)
    assert counts == (1, 6, 6) and strides == (32, 32, 32)
    starts = R.window_starts((3, 224, 224), (3, 64, 64), 32)
    assert len(starts) == 36 and starts[0] == (0, 0, 0) and starts[1] == (0, 32, 0) and starts[6] == (0, 0, 32) and starts[35] == (0, 160, 160)
    # the expression of the issue, written out independently
    for k, st in enumerate(starts):
        assert st == ((k % 1) * 32, (k // 1 % 6) * 32, (k // 6 % 6) * 32)
    counts, _ = R.window_counts((3, 40, 40), (3, 16, 16), 10)
    assert counts == (1, 4, 4)
    masks = list(R.window_masks((3, 40, 40), (3, 16, 16), 10))
    last = masks[3]                                                # k = 3: row shift 3 -> rows 30..39 (clipped from 30..45), columns 0..15
    assert last[:, 30:40, 0:16].all() and last.sum() == 3 * 10 * 16
    assert masks[15][:, 30:40, 30:40].all() and masks[15].sum() == 3 * 10 * 10
    assert R.window_counts((3, 40, 40), (3, 40, 40), 7)[0] == (1, 1, 1)


def test_nearest_exact_indices_are_interpolates():
    assert R.nearest_exact_index(224, 14)[:3] == [8, 24, 40]
    for n_in, n_out in ((224, 14), (40, 14), (30, 7), (31, 5), (17, 17), (9, 4)):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1).expand(1, 1, n_in, n_in).contiguous()
        got = F.interpolate(src, size=(n_out, n_out), mode="nearest-exact")[0, 0, :, 0].long().tolist()
        assert got == R.nearest_exact_index(n_in, n_out), (n_in, n_out)


@pytest.mark.parametrize("batching", [None, 5])
def test_feature_ablation_restated_is_the_definition(batching):
    """attr[:, :, patch j] == s0 - model(x with patch j zeroed), by an independent loop with index assignment (no masks, no float
    blend); an id that occurs nowhere contributes nothing"""
    model = _tiny(0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 16, 16, generator=g)
    ids = torch.arange(16).reshape(4, 4).repeat_interleave(4, 0).repeat_interleave(4, 1)
    ids = torch.where(ids == 7, torch.tensor(6), ids)             # id 7 is absent
    t = torch.tensor([3, 8])
    attr, s0, sc = R.feature_ablation(model, x, t, ids, batching=batching)
    assert sc.shape == (2, 16) and attr.shape == x.shape
    for b in range(2):
        base = model(x[b:b + 1])[0, t[b]]
        for j in range(16):
            xj = x[b].clone()
            xj[:, ids == j] = 0.0
            want = base - model(xj[None])[0, t[b]]
            region = attr[b][:, ids == j]
            if j == 7:
                assert region.numel() == 0 and abs(float(sc[b, 7] - s0[b])) <= 1e-6 * abs(float(s0[b]))
                continue
            assert region.numel() and bool((region == region.flatten()[0]).all())
            assert abs(float(region.flatten()[0] - want)) <= 2e-6 * abs(float(base)), (b, j)


@pytest.mark.parametrize("shape,window,strides", [((3, 40, 40), (3, 16, 16), 10), ((3, 32, 32), (3, 16, 16), 8), ((3, 16, 16), (3, 16, 16), None)])
def test_occlusion_restated_is_the_definition(shape, window, strides):
    """per pixel: the mean over the windows covering it of s0 - model(x with that window zeroed), windows found by an independent
    double loop over row and column shifts; with overhang, without, and window == image"""
    model = _tiny(2)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1,) + shape, generator=g)
    st = window[1:] if strides is None else (strides, strides)
    attr, s0, sc = R.occlusion(model, x, 4, window, window if strides is None else strides)
    H, W = shape[1:]
    rows = [r0 for r0 in range(0, H, st[0]) if r0 == 0 or r0 - st[0] + window[1] < H]
    cols = [c0 for c0 in range(0, W, st[1]) if c0 == 0 or c0 - st[1] + window[2] < W]
    assert sc.shape == (1, len(rows) * len(cols))
    base = model(x)[0, 4]
    total, cover = torch.zeros(H, W, dtype=torch.float64), torch.zeros(H, W)
    for c0 in cols:
        for r0 in rows:
            xk = x.clone()
            xk[:, :, r0:r0 + window[1], c0:c0 + window[2]] = 0.0
            total[r0:r0 + window[1], c0:c0 + window[2]] += float(base - model(xk)[0, 4])
            cover[r0:r0 + window[1], c0:c0 + window[2]] += 1
    assert cover.min() >= 1
    want = (total / cover).float()
    for c in range(3):
        assert float((attr[0, c] - want).abs().max()) <= 4e-6 * abs(float(base))


def test_signed_zeros_follow_the_float_blend_not_a_select():
    x = torch.tensor([-0.0, 0.0, -1.5, 2.0]).view(1, 2, 2).expand(3, 2, 2).contiguous()
    m = torch.tensor([[1.0, 0.0], [1.0, 0.0]]).expand(3, 2, 2)
    out = R.ablated(x, m, 0)
    assert np.signbit(out.numpy()).sum() == 0 and out[0, 1, 1] == 2.0 and out[0, 0, 1] == 0.0      # -0 kept nowhere: -0 + 0 = +0
    out = R.ablated(x, 1 - m, -2.0)
    assert bool(np.signbit(out[0, 0, 0].numpy())) and out[0, 0, 0] == 0 and out[0, 0, 1] == -2.0   # baseline * 0 = -0 keeps -0
    a = R.accumulate(-0.0, [0.0, 5.0], [torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])], False)
    assert not np.signbit(a[0].numpy()) and a[0] == 0 and a[1] == -5.0                             # +0 + (-0 - 0) * 1 = +0
