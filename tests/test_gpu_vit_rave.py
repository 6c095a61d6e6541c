"""Baselines.generate_RAVE ("InFlow") and Baselines.generate_cam_attn on the HIP kernels K17-K21 (csrc/vit_kernels.hip):
the reference's own outputs (tests/golden/vit_rave.npz, tests/golden/make_golden_rave.py), each kernel against an fp64 torch
restatement over ViT-B/16 and odd shapes, bit-identical repeats, agreement with the mirror's compute_RAVE and the harness row."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _zoo_from(npz, prefix, device, **arch):
    from xai_engine.zoo import VisionTransformer
    m = VisionTransformer(**arch).eval()
    m.load_state_dict({k: torch.from_numpy(npz[prefix + k]) for k in m.state_dict()})
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(device)


def mini(g=None, device=DEV):
    return _zoo_from(load_golden("vit_mini.npz"), "w_", device, img=32, patch=8, dim=32, depth=2, heads=4, num_classes=10)


def vit224(g, device=DEV):
    """the seeded 224/16 model of vit_rave.npz: dim 48, depth 3, 12 heads, 10 classes"""
    return _zoo_from(g, "w224_", device, img=224, patch=16, dim=48, depth=3, heads=12, num_classes=10)


def baselines(model):
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import Baselines      # the reference module path
    return Baselines(model)


# ------------------------------------------------------------------------------ fp64 restatements of K17-K21
def ref_head_importance(A, G):                      # (L,H,S,S) x2
    m = (A.double().transpose(-1, -2) @ G.double()).abs().mean((-1, -2))
    return m / m.sum(1, keepdim=True)


def ref_shares(xs, ats, rs, ms):                    # L tensors (S,D) each
    def pair(a, b):
        n = torch.stack((a.double().norm(dim=-1), b.double().norm(dim=-1)))
        return F.normalize(n, p=1, dim=0)
    return (torch.stack([pair(a, b) for a, b in zip(xs, ats)]), torch.stack([pair(a, b) for a, b in zip(rs, ms)]))


def ref_matrices(A, Ih, b1, b2, Gb, ablate):
    M = (A.double() * Ih.double()[:, :, None, None]).amax(1)
    if Gb is not None:
        M = (Gb.double().mean(1) * M).clamp(min=0)
    b1, b2 = b1.double(), b2.double()
    r = M * b1[:, 1, None, :] + torch.diag_embed(b1[:, 0])
    if ablate == 0:
        ratio = F.normalize(b2[:, 1] / b2[:, 0], p=1, dim=-1)
        r = r @ torch.diag_embed(ratio * b2[:, 1] + b2[:, 0])
    return r / r.sum(-1, keepdim=True)


def ref_row(aug, t):
    joint = aug[0].double()
    for i in range(1, aug.shape[0]):
        joint = aug[i].double() @ joint
    return joint[t]


def ref_cam(A, G):                                  # (H,S,S) x2
    c = (A.double()[:, 0, 1:] * G.double()[:, 0, 1:]).mean(0).clamp(min=0)
    return (c - c.min()) / (c.max() - c.min())


def torch_rave(model, x, target, withgrad=True, ablate=0, target_token=0, stop_layer=12):
    """generate_RAVE's math as plain torch ops on the model's device (the reference's sequence, fp32)"""
    x = x.detach().requires_grad_(True)
    out = model(x, register_hook=True)
    blocks = list(model.blocks)[:stop_layer + 1]
    out[0][target].sum().backward(retain_graph=True)
    A = torch.stack([b.attn.get_attention_map().detach()[0] for b in blocks])
    G = torch.stack([b.attn.get_attn_gradients()[0] for b in blocks])
    Gb = None
    if withgrad:
        Gb = torch.stack([torch.autograd.grad(model.head(model.norm(b.get_block_out()).mean(dim=1))[:, target].sum(),
                                              b.attn.get_attention_map(), retain_graph=True)[0][0] for b in blocks])
    Ih = torch.matmul(A.transpose(-1, -2), G).abs().mean((-1, -2))
    Ih = Ih / Ih.sum(1, keepdim=True)
    M = (A * Ih[:, :, None, None]).max(1)[0]
    if withgrad:
        M = (Gb.mean(1) * M).clamp(0)

    def share(a, b):
        return F.normalize(torch.stack((torch.linalg.norm(a[0], dim=1), torch.linalg.norm(b[0], dim=1))), p=1, dim=0)
    b1 = torch.stack([share(b.get_input().detach(), b.attn.get_output().detach()) for b in blocks])
    b2 = torch.stack([share(b.get_input_plus_attn().detach(), b.get_mlp_val().detach()) for b in blocks])
    from xai_engine.vit_attr import compute_RAVE
    roll, _ = compute_RAVE([m[None] for m in M], list(b1), list(b2), ablate)
    side = int(np.sqrt(roll.shape[-1] - 1))
    return roll[:, target_token, 1:].reshape(-1, side, side), (b1, b2)


# ------------------------------------------------------------------------------ the reference's outputs
def test_mini_vit_matches_the_reference_outputs():
    g = load_golden("vit_rave.npz")
    m = load_golden("vit_mini.npz")
    b = baselines(mini(g))
    x, t = torch.from_numpy(m["x"]), torch.tensor(int(m["target"]))
    for key, kw in (("rave_default", {}), ("rave_nograd", dict(withgrad=False)), ("rave_ablate1", dict(ablate=1)),
                    ("rave_token1", dict(target_token=1)), ("rave_stop0", dict(stop_layer=0))):
        sal, (b1, b2) = b.generate_RAVE(x.clone(), t, device=DEV, **kw)
        assert sal.shape == g[key].shape
        check(f"generate_RAVE/mini/{key}", sal.cpu().numpy(), g[key], 1e-5)
        if key + "_b1" in g:
            check(f"generate_RAVE/mini/{key}/b1", b1.cpu().numpy(), g[key + "_b1"], 1e-5)
            check(f"generate_RAVE/mini/{key}/b2", b2.cpu().numpy(), g[key + "_b2"], 1e-5)
    check("generate_cam_attn/mini/last", b.generate_cam_attn(x.clone(), t, DEV).cpu().numpy(), g["cam_last"], 1e-5)
    check("generate_cam_attn/mini/first", b.generate_cam_attn(x.clone(), t, DEV, layer=0).cpu().numpy(), g["cam_first"], 1e-5)


def test_224_vit_matches_the_reference_outputs():
    g = load_golden("vit_rave.npz")
    b = baselines(vit224(g))
    x, t = torch.from_numpy(g["x224"]), torch.tensor(int(g["target224"]))
    sal, (b1, b2) = b.generate_RAVE(x.clone(), t, device=DEV)
    assert sal.shape == (1, 14, 14)
    check("generate_RAVE/224/default", sal.cpu().numpy(), g["rave224_default"], 1e-5)
    check("generate_RAVE/224/default/b1", b1.cpu().numpy(), g["rave224_default_b1"], 1e-5)
    check("generate_RAVE/224/default/b2", b2.cpu().numpy(), g["rave224_default_b2"], 1e-5)
    sal, _ = b.generate_RAVE(x.clone(), t, withgrad=False, device=DEV, ablate=1)
    check("generate_RAVE/224/nograd_ablate1", sal.cpu().numpy(), g["rave224_nograd_ablate1"], 1e-5)
    check("generate_cam_attn/224", b.generate_cam_attn(x.clone(), t, DEV).cpu().numpy(), g["cam224"], 1e-5)


def test_input_is_not_mutated_and_ablate_is_checked():
    g = load_golden("vit_rave.npz")
    m = load_golden("vit_mini.npz")
    b = baselines(mini(g))
    x = torch.from_numpy(m["x"]).clone()
    b.generate_RAVE(x, 0, device=DEV)
    b.generate_cam_attn(x, 0, DEV)
    assert not x.requires_grad
    with pytest.raises(ValueError):
        b.generate_RAVE(x, 0, device=DEV, ablate=2)
    with pytest.raises(TypeError):
        b.generate_RAVE(x, 0, option='b', device=DEV)


# ------------------------------------------------------------------------------ kernels vs fp64 restatements
def _inputs(L, H, S, D, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.softmax(torch.randn(L, H, S, S, device=DEV, generator=gen) * 2, -1)
    G = torch.randn(L, H, S, S, device=DEV, generator=gen) * 1e-3
    Gb = torch.randn(L, H, S, S, device=DEV, generator=gen) * 1e-2
    streams = [[torch.randn(S, D, device=DEV, generator=gen) * s for _ in range(L)] for s in (1.0, 0.5, 1.2, 0.8)]
    return A, G, Gb, streams


SHAPES = [(12, 12, 197, 768), (1, 1, 17, 40), (2, 3, 50, 64), (1, 16, 257, 96), (2, 1, 257, 33), (2, 16, 17, 768)]


@pytest.mark.parametrize("L,H,S,D", SHAPES)
def test_kernels_against_fp64(L, H, S, D):
    from xai_engine import kernels as K
    A, G, Gb, streams = _inputs(L, H, S, D, 1000 + S + H)
    Ih = K.attn_head_importance(list(A), list(G))
    check(f"K17/{L}x{H}x{S}", Ih.cpu(), ref_head_importance(A, G).cpu(), 2e-6, against="fp64")
    b1, b2 = K.residual_shares(*streams)
    r1, r2 = ref_shares(*streams)
    check(f"K20/{L}x{S}x{D}", torch.cat((b1, b2)).cpu(), torch.cat((r1, r2)).cpu(), 2e-6, against="fp64")
    for withgrad in (0, 1):
        for ablate in (0, 1):
            aug = K.rave_matrices(list(A), Ih, b1, b2, list(Gb) if withgrad else None, ablate)
            want = ref_matrices(A, Ih, b1, b2, Gb if withgrad else None, ablate)
            check(f"K18/{L}x{H}x{S}/g{withgrad}a{ablate}", aug.cpu(), want.cpu(), 2e-6, against="fp64")
            for t in (0, S - 1):
                check(f"K19/{L}x{S}/t{t}/g{withgrad}a{ablate}", K.rollout_row(aug, t).cpu(), ref_row(aug, t).cpu(), 2e-6, against="fp64")
    cam = K.attn_cam(A[:1], G[:1])
    check(f"K21/{H}x{S}", cam[0].cpu(), ref_cam(A[0], G[0]).cpu(), 2e-6, against="fp64")


def test_attn_cam_of_a_constant_map_is_nan_like_the_reference():
    from xai_engine import kernels as K
    A = torch.full((1, 3, 17, 17), 1 / 17, device=DEV)
    G = torch.ones_like(A)
    cam = K.attn_cam(A, G)
    assert torch.isnan(cam).all()
    c = (A[0, :, 0, 1:] * G[0, :, 0, 1:]).mean(0).clamp(min=0)
    assert torch.isnan((c - c.min()) / (c.max() - c.min())).all()


def test_kernel_repeats_are_bit_identical():
    from xai_engine import kernels as K
    A, G, Gb, streams = _inputs(12, 12, 197, 768, 7)
    for f in (lambda: K.attn_head_importance(list(A), list(G)),
              lambda: torch.cat(K.residual_shares(*streams)),
              lambda: K.rave_matrices(list(A), K.attn_head_importance(list(A), list(G)), *K.residual_shares(*streams), list(Gb), 0),
              lambda: K.attn_cam(A[:1], G[:1])):
        assert torch.equal(f(), f())
    aug = K.rave_matrices(list(A), K.attn_head_importance(list(A), list(G)), *K.residual_shares(*streams), None, 0)
    assert torch.equal(K.rollout_row(aug, 0), K.rollout_row(aug, 0))


def test_methods_repeat_bit_identically():
    g = load_golden("vit_rave.npz")
    b = baselines(vit224(g))
    x, t = torch.from_numpy(g["x224"]), int(g["target224"])
    r1, r2 = b.generate_RAVE(x, t, device=DEV), b.generate_RAVE(x, t, device=DEV)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1][0], r2[1][0]) and torch.equal(r1[1][1], r2[1][1])
    assert torch.equal(b.generate_cam_attn(x, t, DEV), b.generate_cam_attn(x, t, DEV))


def test_rave_row_agrees_with_the_mirrors_compute_RAVE():
    """the kernels' M, b1, b2 through the mirror's existing compute_RAVE (torch, full GEMMs) give generate_RAVE's row.  Both are
    fp32 chains of 11 products with different summation orders, so they agree to the 1e-5 bar and not to 1e-6 (3e-6 measured
    on these inputs); what is held tighter is that the kernels are no further from the fp64 product than compute_RAVE is."""
    from xai_engine import kernels as K
    from xai_engine.vit_attr import compute_RAVE
    A, G, Gb, streams = _inputs(12, 12, 197, 768, 11)
    Ih = K.attn_head_importance(list(A), list(G))
    b1, b2 = K.residual_shares(*streams)
    M = (Gb.mean(1) * (A * Ih[:, :, None, None]).max(1)[0]).clamp(0)
    for ablate in (0, 1):
        roll, _ = compute_RAVE([m[None] for m in M], list(b1), list(b2), ablate)
        got = K.rollout_row(K.rave_matrices(list(A), Ih, b1, b2, list(Gb), ablate), 0)
        check(f"K18+K19 vs compute_RAVE/a{ablate}", got[1:].cpu(), roll[0, 0, 1:].cpu(), 1e-5, against="torch")
        roll64, _ = compute_RAVE([m[None].double() for m in M], list(b1.double()), list(b2.double()), ablate)
        truth = roll64[0, 0, 1:].cpu().numpy()
        from conftest import rel_inf
        e_hip, e_torch = rel_inf(got[1:].cpu(), truth), rel_inf(roll[0, 0, 1:].cpu(), truth)
        assert e_hip <= max(2 * e_torch, 1e-6), (e_hip, e_torch)


def test_get_VIT_attr_inflow_is_the_upsampled_rave_map():
    from xai_engine.sweep import get_VIT_attr
    g = load_golden("vit_rave.npz")
    m = load_golden("vit_mini.npz")
    model = mini(g)
    x, t = torch.from_numpy(m["x"]), torch.tensor(int(m["target"]))
    td = {"models": [model, model], "img_hw": 32, "batch_size": 25, "device": DEV, "num_patches": 4, "attr_func": "InFlow"}
    got = get_VIT_attr(x.clone(), None, t, td)
    sal, _ = baselines(model).generate_RAVE(x.clone(), t, device=DEV)
    want = F.interpolate(sal[None].float(), size=(32, 32), mode="bilinear", align_corners=False)[0, 0].abs().cpu().numpy()
    assert got.shape == (32, 32) and got.dtype == np.float32
    check("get_VIT_attr/InFlow", got, want, 1e-6, against="torch")


def test_full_size_vit_b16():
    from xai_engine.zoo import vit_base_patch16_224
    model = vit_base_patch16_224(seed=0).to(DEV)
    b = baselines(model)
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        t = int(model(x.to(DEV)).argmax(1)[0])
    sal, (b1, b2) = b.generate_RAVE(x, t, device=DEV)
    assert sal.shape == (1, 14, 14) and torch.isfinite(sal).all() and (sal >= 0).all()
    assert b1.shape == b2.shape == (12, 2, 197)
    want, (w1, w2) = torch_rave(model, x.to(DEV), t)
    check("generate_RAVE/ViT-B16 vs torch", sal.cpu(), want.detach().cpu(), 1e-5, against="torch")
    check("generate_RAVE/ViT-B16 b1,b2 vs torch", torch.cat((b1, b2)).cpu(), torch.cat((w1, w2)).cpu(), 1e-5, against="torch")
    cam = b.generate_cam_attn(x, t, DEV)
    assert cam.shape == (1, 14, 14) and torch.isfinite(cam).all()
    blk = model.blocks[-1].attn
    check("generate_cam_attn/ViT-B16 vs torch", cam[0].cpu(), ref_cam(blk.get_attention_map()[0].detach(), blk.get_attn_gradients()[0]).reshape(14, 14).cpu(),
          1e-5, against="torch")
