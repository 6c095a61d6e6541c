"""captum 0.7.0's GradientShap, as the reference's harness calls it (evaluatePerturbation.py:164-167), restated in plain torch ops on
whatever device the model is on -- the yardstick of tests/test_cpu_gshap.py and tests/test_gpu_gshap.py.  captum is on neither
machine; the flow is restated from its published source (GradientShap -> NoiseTunnel("smoothgrad", draw_baseline_from_distrib) over
InputBaselineXGradient):

  1. stdevs != 0: every row's input gets torch.normal(0, stdevs) noise (rows: x.repeat_interleave(n, 0));
  2. one baseline per row, np.random.choice(N_b, n * B), and one coefficient per row, np.random.uniform(0, 1, n * B) as float32,
     drawn from NumPy's global state in that order;
  3. scaled = alpha * xr + (1 - alpha) * baseline, fp32 products and sum;
  4. the gradient of the raw target logit at every row;
  5. (xr - baseline) * gradient, the mean over an image's n rows;
  6. the harness's map |sum over channels| (:181).

The mean of step 5 is written out in one stated order (from +0, the samples ascending, a true division by n): captum's own
reduction order over the samples is torch's and unpinned.
"""
import numpy as np
import torch


def draw(n_base, n_rows):
    """step 2, the two NumPy calls"""
    idx = np.random.choice(n_base, n_rows)
    alpha = np.float32(np.random.uniform(0.0, 1.0, n_rows))
    return idx, alpha


def interpolants(xr, baselines, idx, alpha):
    """step 3 on tensors of one device: xr (R, ...), baselines (N_b, ...), idx int64 (R,), alpha float32 (R,) -> (R, ...)"""
    a = alpha.view(-1, *([1] * (xr.dim() - 1)))
    return a * xr + (1 - a) * baselines[idx]


def sample_mean(term, n):
    """step 5's mean: term (B * n, ...) -> (B, ...), from +0, samples ascending, a true division (the divisor is a tensor on the
    device: torch turns a division by a Python number into a multiplication by its reciprocal on a GPU)"""
    t = term.view(term.shape[0] // n, n, *term.shape[1:])
    acc = torch.zeros_like(t[:, 0])
    for s in range(n):
        acc = acc + t[:, s]
    return acc / torch.full((), n, dtype=term.dtype, device=term.device)


def gradient_shap(model, x, targets, baselines, n_samples=5, stdevs=0.0, pass_images=None, draws=None):
    """x (B, C, H, W), baselines (N_b, C, H, W), targets (B,) int64, all on the model's device -> attribution (B, C, H, W).
    `pass_images`: images per classifier pass (None: all), so that the classifier sees the batch shapes of the run it is compared
    with; `draws` = (idx, alpha) NumPy arrays instead of step 2."""
    B, n = x.shape[0], int(n_samples)
    dev = x.device
    xr = x.repeat_interleave(n, 0)
    if stdevs != 0.0:
        xr = xr + torch.normal(0, torch.full_like(xr, float(stdevs)))
    idx, alpha = draws if draws is not None else draw(baselines.shape[0], n * B)
    idx = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
    alpha = torch.from_numpy(np.asarray(alpha, dtype=np.float32)).to(dev)
    scaled = interpolants(xr, baselines, idx, alpha)
    t_rows = torch.as_tensor(targets).to(dev).long().reshape(-1).expand(B).repeat_interleave(n).view(-1, 1)
    k = B if pass_images is None else max(1, min(int(pass_images), B))
    grads = []
    for lo in range(0, B, k):
        rows = slice(lo * n, min(lo + k, B) * n)
        xs = scaled[rows].detach().requires_grad_(True)
        out = model(xs)
        (g,) = torch.autograd.grad(out.gather(1, t_rows[rows]).sum(), xs)
        grads.append(g.detach())
    return sample_mean((xr - baselines[idx]) * torch.cat(grads), n)


def harness_map(attr):
    """(C, H, W) attribution of one image -> the (H, W) map of evaluatePerturbation.py:181"""
    return np.abs(np.sum(attr.detach().cpu().numpy(), axis=0))
