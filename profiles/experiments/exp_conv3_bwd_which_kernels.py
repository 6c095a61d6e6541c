"""MIOpen's forward and backward-data of layer4.0.conv3 (1x1, 2048 <- 512 forward, on 7x7) under deterministic solvers in immediate
mode, batch 50 (backward five times) and batch 2 (seven times), and nothing else: run under a kernel trace it shows which rocBLAS
kernels serve the call, run with MIOpen's logging it shows the solver (profiles/conv3_bwd_rocblas_kernels.txt).
usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python3 profiles/experiments/exp_conv3_bwd_which_kernels.py
       MIOPEN_ENABLE_LOGGING=1 MIOPEN_LOG_LEVEL=6 python3 profiles/experiments/exp_conv3_bwd_which_kernels.py 2>&1 | grep -i solver"""
import torch
import torch.nn.functional as F

torch.backends.cudnn.deterministic = True
torch.backends.cudnn.benchmark = False
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(1)
W = torch.randn(2048, 512, 1, 1, device=dev, generator=g) * 0.05
for N, reps in ((50, 5), (2, 7)):
    x = torch.randn(N, 512, 7, 7, device=dev, generator=g).relu_().requires_grad_(True)
    y = F.conv2d(x, W)
    gy = torch.randn(y.shape, device=dev, generator=g)
    for _ in range(reps):
        torch.autograd.grad(y, x, gy, retain_graph=True)
    torch.cuda.synchronize()
print("DONE")
