"""The large-plane sites of prepare._fused_block_forward (prepare._conv1x1_wide): one layer2 bottleneck of ResNet-50 at its real
shapes (512 channels on 28 x 28, conv1 128 <- 512, conv3 512 <- 128), batch 50 and the verify batch 2, under deterministic solvers.
conv3's backward-data (gy of 512 channels onto 128) is of an enabled shape class, conv1's (128 onto 512) is not and stays with
MIOpen.  The input gradient through the block is the unpatched block's bit for bit whether the proof accepted the kernel or refused
it; the counters and the module's own record say which of the two happened; a launch count shows that the accepted path is the one
that ran; a walk list that cannot match leaves MIOpen's call for good; a capture of the block with three replays is the eager
result; a caller outside target_scores launches nothing; and the small-plane site (K78) claims nothing here."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.fixture()
def P(monkeypatch):
    """prepare.py with fresh counters of the convolution sites, put back afterwards; the decisions live on the modules, which every
    test builds anew"""
    from xai_engine import load_library, prepare
    load_library()
    monkeypatch.setattr(prepare, "CONV_SITE_COUNTS", {"conv_bwd_kernel": 0, "conv_bwd_refused": 0, "walks": [], "reasons": []})
    monkeypatch.setattr(prepare, "CONV_WIDE_SITE_COUNTS", {"conv_wide_kernel": 0, "conv_wide_refused": 0, "walks": [], "reasons": []})
    return prepare


@pytest.fixture()
def launches(monkeypatch):
    from xai_engine import kernels
    seen = {"n": 0, "small": 0}
    inner, small = kernels.conv1x1_bwd_data_wide, kernels.conv1x1_bwd_data

    def counted(*a, **kw):
        seen["n"] += 1
        return inner(*a, **kw)

    def counted_small(*a, **kw):
        seen["small"] += 1
        return small(*a, **kw)
    monkeypatch.setattr(kernels, "conv1x1_bwd_data_wide", counted)
    monkeypatch.setattr(kernels, "conv1x1_bwd_data", counted_small)
    return seen


def block():
    """layer2.1 of ResNet-50 with seeded weights and running statistics that are not the identity"""
    from xai_engine.zoo import Bottleneck
    torch.manual_seed(7)
    m = torch.nn.Sequential(Bottleneck(512, 128)).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.1)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(DEV)


def inputs(N):
    g = torch.Generator().manual_seed(100 + N)
    return torch.randn(N, 512, 28, 28, generator=g).relu_().to(DEV), torch.randn(N, 512, 28, 28, generator=g).to(DEV)


def input_gradient(model, x, gy, P=None):
    """d<model(x), gy> / dx; with P, as a caller of target_scores runs the blocks: differentiating with respect to the input alone"""
    xa = x.clone().requires_grad_(True)
    before = getattr(P._INPUT_ONLY, "on", False) if P is not None else None
    if P is not None:
        P._INPUT_ONLY.on = True
    try:
        y = model(xa)
    finally:
        if P is not None:
            P._INPUT_ONLY.on = before
    (g,) = torch.autograd.grad(y, xa, gy)
    return y.detach(), g


@pytest.mark.parametrize("N", [50, 2])
def test_the_input_gradient_through_the_site_is_the_unpatched_blocks_and_the_counters_say_what_ran(P, launches, N):
    assert torch.backends.cudnn.deterministic and not torch.backends.cudnn.benchmark
    model = block()
    x, gy = inputs(N)
    want = input_gradient(model, x, gy)
    fused = P.fuse_bn_relu(model)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # a refusal is recorded, not warned
        got = input_gradient(fused, x, gy, P)
        proof_launches = launches["n"]
        launches["n"] = 0
        again = input_gradient(fused, x, gy, P)
    for a, b, c in zip(want, got, again):
        assert bits(a, b) and bits(b, c)
    assert (want[1] != 0).any()
    c = P.CONV_WIDE_SITE_COUNTS
    conv3 = fused[0].conv3
    (decision,) = conv3._xai_bwd_wide_walks.values()      # one running shape, one pair of solver switches: decided once
    print(N, P.site_report(), decision)
    assert c["conv_wide_kernel"] + c["conv_wide_refused"] == 1 and len(c["reasons"]) == c["conv_wide_refused"]
    assert not hasattr(fused[0].conv1, "_xai_bwd_wide_walks")                 # 128 onto 512 rows: not an enabled class, never asked
    assert not hasattr(conv3, "_xai_bwd_walks") and launches["small"] == 0    # the small-plane site claims nothing on 28 x 28
    assert P.CONV_SITE_COUNTS == {"conv_bwd_kernel": 0, "conv_bwd_refused": 0, "walks": [], "reasons": []}
    if decision is None:                                  # refused: MIOpen's call ran, the kernel did not
        assert c["conv_wide_refused"] == 1 and launches["n"] == 0 and proof_launches == len(P._CONV_WIDE_WALKS)
        assert "large planes on the read-once GEMM kernel, 1 refused" in P.site_report() and "bit for bit" in P.site_report()
    else:                                                 # accepted: one launch per gradient pass
        assert c["conv_wide_kernel"] == 1 and launches["n"] == 1 and decision in P._CONV_WIDE_WALKS
        assert proof_launches == P._CONV_WIDE_WALKS.index(decision) + 2       # the walks up to the accepted one, then the pass itself
        assert c["walks"] == [((512, 128), (N, 128, 28, 28), decision)]
        assert "1 1x1 convolution backward-data site(s) on large planes on the read-once GEMM kernel, 0 refused" in P.site_report()
    assert "0 1x1 convolution backward-data site(s) on the folded-batch GEMM kernel, 0 refused" in P.site_report()
    # the report still begins with the sentence of the shortcut and head sites (their counters are process-wide: whatever ran before)
    assert P.site_report().startswith(f"{P.SITE_COUNTS['shortcut_compact']} strided 1x1 shortcut site(s) on compact")
    # a caller that does not say it differentiates with respect to the input alone keeps MIOpen's call
    launches["n"] = 0
    plain = input_gradient(fused, x, gy)
    assert bits(plain[1], want[1]) and launches["n"] == 0


def test_a_site_whose_proof_fails_keeps_miopens_call_for_good_and_records_why(P, launches, monkeypatch):
    model = block()
    x, gy = inputs(2)
    want = input_gradient(model, x, gy)
    monkeypatch.setattr(P, "_CONV_WIDE_WALKS", [(1, 1, 16, 64, 0, 2, 64)])    # a walk no library of this stack uses at this shape
    fused = P.fuse_bn_relu(model)
    got = input_gradient(fused, x, gy, P)
    launches["n"] = 0
    again = input_gradient(fused, x, gy, P)
    assert bits(got[1], want[1]) and bits(again[1], want[1]) and launches["n"] == 0
    c = P.CONV_WIDE_SITE_COUNTS
    assert (c["conv_wide_kernel"], c["conv_wide_refused"]) == (0, 1) and len(c["reasons"]) == 1 and "bit for bit" in c["reasons"][0]
    assert list(fused[0].conv3._xai_bwd_wide_walks.values()) == [None]


def test_a_capture_and_three_replays_of_the_block_are_the_eager_result(P, launches):
    model = block()
    x, gy = inputs(50)
    fused = P.fuse_bn_relu(model)
    want = input_gradient(fused, x, gy, P)                # eager first: the site is decided here, never inside a capture
    decided = dict(fused[0].conv3._xai_bwd_wide_walks)
    xs, gs = x.clone(), gy.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        input_gradient(fused, xs, gs, P)                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    launches["n"] = 0
    with torch.cuda.graph(graph):
        out = input_gradient(fused, xs, gs, P)
    assert launches["n"] == (0 if list(decided.values()) == [None] else 1) and fused[0].conv3._xai_bwd_wide_walks == decided
    other_x, other_g = inputs(51)
    for k in range(3):
        src_x, src_g = (x, gy) if k != 1 else (other_x[:50], other_g[:50])
        xs.copy_(src_x)
        gs.copy_(src_g)
        out[1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        if k != 1:
            assert bits(out[0], want[0]) and bits(out[1], want[1]), k
        else:
            assert not bits(out[1], want[1]) and not bool(out[1].isnan().any())


def test_a_second_derivative_is_refused_and_autocast_keeps_the_module(P, launches):
    model = block()
    x, gy = inputs(2)
    fused = P.fuse_bn_relu(model)
    input_gradient(fused, x, gy, P)                       # decided
    if list(fused[0].conv3._xai_bwd_wide_walks.values()) != [None]:
        conv, walk = fused[0].conv3, list(fused[0].conv3._xai_bwd_wide_walks.values())[0]
        xa = torch.randn(2, 128, 28, 28, device=DEV).requires_grad_(True)
        y = P._conv_wide_function().apply(xa, conv, walk)
        # the backward is a kernel launch, no graph goes through it: a second derivative raises, it is never silently wrong
        (g,) = torch.autograd.grad(y, xa, torch.ones_like(y), create_graph=True)
        assert not g.requires_grad
        with pytest.raises(RuntimeError, match="does not require grad"):
            g.sum().backward()
        seed = torch.ones_like(y).requires_grad_(True)    # a gradient that is itself differentiated with respect to its seed
        (g,) = torch.autograd.grad(y, xa, seed, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()
    launches["n"] = 0
    xa = torch.randn(2, 128, 28, 28, device=DEV).requires_grad_(True)
    P._INPUT_ONLY.on = True
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            y = P._conv1x1_wide(fused[0].conv3, xa)
    finally:
        P._INPUT_ONLY.on = False
    torch.autograd.grad(y, xa, torch.ones_like(y))
    assert y.dtype == torch.float16 and launches["n"] == 0
