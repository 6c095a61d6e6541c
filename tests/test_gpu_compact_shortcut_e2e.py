"""The compact strided shortcuts and the broadcast head of `prepare.fuse_bn_relu(..., fork_residual=True)` end to end on the MI355X:
logits and input gradients of the prepared classifier against the untouched one, bit for bit under deterministic solvers (what
conftest.py sets), with the counters saying which sites run in the new forms; and the same when every proof is forced to fail, where
the sites must keep MIOpen's and PyTorch's calls and say so."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.fixture()
def P(monkeypatch):
    """prepare.py with fresh decisions and counters (they are process-wide), put back afterwards"""
    from xai_engine import load_library, prepare
    load_library()
    monkeypatch.setattr(prepare, "_PROVEN", {})
    monkeypatch.setattr(prepare, "SITE_COUNTS", {"shortcut_compact": 0, "shortcut_refused": 0, "head_broadcast": 0, "head_refused": 0,
                                                 "reasons": []})
    return prepare


def toy():
    """a stem and four layers of one bottleneck, the last of two, three of them with a stride-2 1x1 shortcut: planes of 10, 5, 3 and
    2 rows at 40 x 40; the second block of layer4 is a plain fused site, so the head's broadcast form applies"""
    from xai_engine.zoo import ResNet
    torch.manual_seed(3)
    m = ResNet((1, 1, 1, 2), num_classes=10, width=8).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(DEV), torch.randn(3, 3, 40, 40, generator=torch.Generator().manual_seed(4)).to(DEV), 3


def resnet50():
    from xai_engine.zoo import resnet50 as make
    return make(seed=0).to(DEV).eval(), torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV), 3


def reference(model, x, targets, grad_out):
    xa = x.clone().requires_grad_(True)
    logits = model(xa)
    scores = logits.gather(1, targets.unsqueeze(1)).squeeze(1)
    (g,) = torch.autograd.grad(scores, xa, grad_out)
    return logits.detach(), scores.detach(), g


def prepared(P, fused, x, targets, grad_out):
    xb = x.clone().requires_grad_(True)
    got = P.target_scores(fused, xb, targets)
    assert got is not None
    scores, logits = got
    (g,) = torch.autograd.grad(scores, xb, grad_out)
    return logits.detach(), scores.detach(), g


@pytest.fixture()
def calls(monkeypatch):
    """how often the new-form kernels are launched: the accepted path is the one that ran, not only the one that was counted"""
    from xai_engine import kernels
    seen = {"stride_gather_cnhw": 0, "bn_relu_fwd_cnhw": 0, "bn_relu_bwd_compact": 0, "bn_relu_bwd_bcast": 0, "compact_gy2": 0,
            "cnhw_g_identity": 0}

    def counted(name):
        inner = getattr(kernels, name)

        def call(*a, **kw):
            seen[name] += 1
            seen["compact_gy2"] += kw.get("gy2_compact") is not None
            seen["cnhw_g_identity"] += bool(kw.get("identity_cnhw")) and name == "bn_relu_bwd_compact"
            return inner(*a, **kw)
        return call
    for name in ("stride_gather_cnhw", "bn_relu_fwd_cnhw", "bn_relu_bwd_compact", "bn_relu_bwd_bcast"):
        monkeypatch.setattr(kernels, name, counted(name))
    return seen


# (model, accepted shortcut sites).  ResNet-50 at 2 x 64 x 64: all three shortcuts (their inputs 256 x 16^2, 512 x 8^2, 1024 x 4^2)
# run as MIOpen's GEMM and the convolution on the view reproduces them; the toy's first shortcut (64 <- 32 channels on 3 x 32 x 10 x 10)
# is run by another MIOpen solver and its proof refuses, the other two are accepted.  The head is plain arithmetic: always accepted.
# Backward launches of the compact entry: in ResNet-50 the block that writes a channel-major g_identity and the block before it that
# takes the compact gy2 are different sites, 2 per shortcut; in the toy layer3's only block is both at once, so 3 for 2 shortcuts.
@pytest.mark.parametrize("make,accepted,compact_backwards", [(toy, 2, 3), (resnet50, 3, 6)])
def test_logits_and_input_gradient_are_the_untouched_models_bit_for_bit(P, calls, make, accepted, compact_backwards):
    assert torch.backends.cudnn.deterministic and not torch.backends.cudnn.benchmark
    model, x, shortcuts = make()
    targets = torch.tensor([1, 1, 7][:x.shape[0]], device=DEV)
    grad_out = torch.tensor([1.0, -2.5, 0.5][:x.shape[0]], device=DEV)
    want = reference(model, x, targets, grad_out)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fused = P.fuse_bn_relu(model, verify=x, fork_residual=True)
        for k in calls:
            calls[k] = 0                                  # (the verify pass has launched them too)
        got = prepared(P, fused, x, targets, grad_out)
        one_pass = dict(calls)
        again = prepared(P, fused, x, targets, grad_out)
    print(make.__name__, P.site_report(), one_pass)
    for a, b, c in zip(want, got, again):
        assert bits(a, b) and bits(b, c)
    assert (want[2] != 0).any()
    c = P.SITE_COUNTS
    # every site is decided exactly once, by its proof (MIOpen runs the smallest shapes with other solvers than its GEMM, and a
    # compact form that does not reproduce them is refused); every refusal has warned and left its reason
    assert c["shortcut_compact"] + c["shortcut_refused"] == shortcuts and c["head_broadcast"] + c["head_refused"] == 1
    assert len(c["reasons"]) == c["shortcut_refused"] + c["head_refused"] == len([w for w in caught if "keeps the PyTorch / MIOpen call" in str(w.message)])
    assert f"{c['shortcut_compact']} strided 1x1 shortcut site(s) on compact" in P.site_report()
    # which sites were accepted, and that the gradient pass compared above really went through them: per accepted shortcut one
    # gather, one channel-major forward, one backward writing a channel-major g_identity and one backward at the block before
    # taking the compact gy2 through the link; the head's gradient through the link into the last block's kernel, once
    assert (c["shortcut_compact"], c["shortcut_refused"], c["head_broadcast"], c["head_refused"]) == (accepted, shortcuts - accepted, 1, 0)
    assert one_pass == {"stride_gather_cnhw": accepted, "bn_relu_fwd_cnhw": accepted, "bn_relu_bwd_compact": compact_backwards,
                        "bn_relu_bwd_bcast": 1, "compact_gy2": accepted, "cnhw_g_identity": accepted}
    # the plain call of the prepared model (no target_scores) is the same classifier
    xb = x.clone().requires_grad_(True)
    logits = fused(xb)
    (g,) = torch.autograd.grad(logits.gather(1, targets.unsqueeze(1)).squeeze(1), xb, grad_out)
    assert bits(logits.detach(), want[0]) and bits(g, want[2])
    with torch.no_grad():
        assert bits(fused(x), want[0])


def test_a_site_whose_proof_fails_keeps_miopens_call_and_says_so(P, calls, monkeypatch):
    model, x, shortcuts = toy()
    targets = torch.tensor([1, 1, 7], device=DEV)
    grad_out = torch.tensor([1.0, -2.5, 0.5], device=DEV)
    want = reference(model, x, targets, grad_out)
    monkeypatch.setattr(P, "_SHORTCUT_CANDIDATES", [("off by a rounding", lambda xv, conv: P._conv_on_view(xv, conv) * 1.0000002)])
    monkeypatch.setattr(P, "_HEAD_CANDIDATES", [("a wrong scale", lambda hw: (0.3, 0.0))])
    with pytest.warns(UserWarning, match="keeps the PyTorch / MIOpen call"):
        fused = P.fuse_bn_relu(model, verify=x, fork_residual=True)
    for k in calls:
        calls[k] = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # decided for good: nothing is proven, or refused, a second time
        got = prepared(P, fused, x, targets, grad_out)
    for a, b in zip(want, got):
        assert bits(a, b)
    assert not any(calls.values())                        # MIOpen's and PyTorch's calls ran, none of the new forms
    c = P.SITE_COUNTS
    assert (c["shortcut_compact"], c["shortcut_refused"], c["head_broadcast"], c["head_refused"]) == (0, shortcuts, 0, 1)
    assert len(c["reasons"]) == shortcuts + 1 and "refused" in P.site_report() and "bit for bit" in P.site_report()
    assert all(v is None for v in P._PROVEN.values())


def test_a_module_hook_sends_the_caller_back_to_the_plain_model_call(P):
    model, x, _ = toy()
    fused = P.fuse_bn_relu(model, fork_residual=True)
    xb = x.clone().requires_grad_(True)
    targets = torch.tensor([1, 1, 7], device=DEV)
    assert P.target_scores(fused, xb, targets) is not None
    for module in (fused, fused.fc, fused.layer4[-1], fused.layer2[0].conv1):
        handle = module.register_forward_hook(lambda m, i, o: None)
        assert P.target_scores(fused, xb, targets) is None
        handle.remove()
    assert P.target_scores(fused, xb, targets) is not None
    with torch.no_grad():
        assert P.target_scores(fused, xb, targets) is None
    assert P.target_scores(model, xb, targets) is None     # not a prepared classifier
