"""Which compact forms of the three stride-2 1x1 shortcut convolutions of ResNet-50 reproduce MIOpen's strided call bit for bit under
deterministic solvers, forward and backward-data, at batch 50 and at the verify batch 2: torch.mm(W, Xc), its
transposed form, F.conv2d on the (1, Cin, N*Ho, Wo) view of the compact tensor, and a stride-1 convolution on the compact NCHW
tensor.  Also whether the rest of MIOpen's dense input gradient is +0.  Output: profiles/shortcut_head_probe.txt.
usage: python profiles/experiments/exp_shortcut_forms.py [output file]"""
import sys

import torch
import torch.nn.functional as F

out = open(sys.argv[1] if len(sys.argv) > 1 else "shortcut_head_probe.txt", "w")


def say(*a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


torch.backends.cudnn.deterministic = True
torch.backends.cudnn.benchmark = False
dev = "cuda"


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())
g = torch.Generator(device=dev).manual_seed(1)
for (Cin, Cout, H) in ((256, 512, 56), (512, 1024, 28), (1024, 2048, 14)):
    for N in (50, 2):
        x = torch.randn(N, Cin, H, H, device=dev, generator=g).relu_().requires_grad_(True)
        W = (torch.randn(Cout, Cin, 1, 1, device=dev, generator=g) * 0.05)
        ref = F.conv2d(x, W, stride=2)
        Ho = ref.shape[2]
        gy = torch.randn(ref.shape, device=dev, generator=g)
        (gref,) = torch.autograd.grad(ref, x, gy)
        refc = ref.detach().permute(1, 0, 2, 3).contiguous()
        Xc = x.detach()[:, :, ::2, ::2].permute(1, 0, 2, 3).contiguous()
        W2 = W.view(Cout, Cin)
        X2 = Xc.view(Cin, -1)
        fw = {}
        fw["mm"] = torch.mm(W2, X2).view(Cout, N, Ho, Ho)
        fw["mmT"] = torch.mm(X2.t(), W2.t()).t().contiguous().view(Cout, N, Ho, Ho)
        xv = Xc.view(1, Cin, N * Ho, Ho).requires_grad_(True)
        cv = F.conv2d(xv, W)
        fw["conv_view"] = cv.detach().view(Cout, N, Ho, Ho)
        x4 = Xc.permute(1, 0, 2, 3).contiguous().requires_grad_(True)       # compact NCHW, stride-1 conv
        c4 = F.conv2d(x4, W)
        fw["conv_compact_nchw"] = c4.detach().permute(1, 0, 2, 3).contiguous()
        say("FWD", Cin, Cout, H, N, {k: bits(v, refc) for k, v in fw.items()})
        # backward data
        gc = gy.permute(1, 0, 2, 3).contiguous()
        G2 = gc.view(Cout, -1)
        grefc = gref[:, :, ::2, ::2].permute(1, 0, 2, 3).contiguous()
        dense = torch.zeros_like(gref); dense[:, :, ::2, ::2] = gref[:, :, ::2, ::2]
        bw = {}
        bw["mm"] = torch.mm(W2.t(), G2).view(Cin, N, Ho, Ho)
        bw["mmT"] = torch.mm(G2.t(), W2).t().contiguous().view(Cin, N, Ho, Ho)
        (gv,) = torch.autograd.grad(cv, xv, gc.view(1, Cout, N * Ho, Ho))
        bw["conv_view"] = gv.view(Cin, N, Ho, Ho)
        (g4,) = torch.autograd.grad(c4, x4, gy)
        bw["conv_compact_nchw"] = g4.permute(1, 0, 2, 3).contiguous()
        say("BWD", Cin, Cout, H, N, {k: bits(v, grefc) for k, v in bw.items()}, "rest_is_plus_zero", bits(dense, gref))
        del x, ref, gref, fw, bw
say("preferred blas", torch.backends.cuda.preferred_blas_library())
say("DONE")
