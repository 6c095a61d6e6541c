"""fp32 torch restatement of one outer step of the reference's guided_ig_impl (GIGBuilder.py:228-292), for the Guided IG tests.

It is the reference loop written out again (torch fp32 tensors, python-float scalars, torch.quantile), with an iteration cap so
that a test can never hang, and it reports what the tests compare: the x after the step, the attribution it adds, the number of
selections (torch.quantile calls) and the features it moved.

`sum_dtype=torch.float64` takes the two sums of the loop (l1_current, l1_s) in float64 and rounds them to float32, which is K22's
arithmetic (csrc/gig_kernels.hip); every other operation stays the reference's.  The caller sums l1_total the same way (`l1`)."""
import math

import torch


def l1(a, b, sum_dtype=torch.float32):
    """l1_distance of the reference (:164) as a 0-d fp32 tensor, summed in `sum_dtype`."""
    return (a - b).abs().sum(dtype=sum_dtype).float()


def step(x, x_input, x_baseline, grad, step_index, steps, fraction, max_dist, l1_total, cap=64, sum_dtype=torch.float32,
         attr0=None):
    """One step for one image; all tensors fp32 of one shape.  -> (x, attr increment, selections, moved mask).
    With `attr0` (the attribution before the step) the second value is the running total, accumulated in place iteration by
    iteration as the reference's `attr +=` does (:259, :292), not the increment.
    Raises RuntimeError when `cap` selections do not reach the step's target (the reference would loop on)."""
    x = x.clone()
    x_start = x.clone()
    attr = torch.zeros_like(x) if attr0 is None else attr0.clone()
    key = grad.clone()
    alpha = (step_index + 1.0) / steps
    alpha_min = max(alpha - max_dist, 0.0)
    alpha_max = min(alpha + max_dist, 1.0)
    diff = x_input - x_baseline
    x_min = x_baseline + diff * alpha_min
    x_max = x_baseline + diff * alpha_max
    l1_target = l1_total * (1 - (step_index + 1) / steps)
    selections = 0
    gamma = float("inf")
    while gamma > 1.0:
        x_old = x.clone()
        x_alpha = torch.where(diff != 0, (x - x_baseline) / diff, torch.nan)
        x_alpha[torch.isnan(x_alpha)] = alpha_max
        behind = x_alpha < alpha_min
        x[behind] = x_min[behind]
        l1_current = l1(x, x_input, sum_dtype)
        if math.isclose(l1_target, l1_current, rel_tol=1e-9, abs_tol=1e-9):
            attr += (x - x_old) * grad
            break
        if selections == cap:
            raise RuntimeError(f"step {step_index}: {cap} selections did not reach the target")
        key[x == x_max] = float("inf")
        threshold = torch.quantile(key.abs().flatten(), fraction, interpolation="lower")
        s = torch.logical_and(key.abs() <= threshold, key != float("inf"))
        selections += 1
        l1_s = ((x - x_max).abs() * s).sum(dtype=sum_dtype).float()
        gamma = (l1_current - l1_target) / l1_s if l1_s > 0 else float("inf")
        if gamma > 1.0:
            x[s] = x_max[s]
        else:
            assert gamma > 0, gamma
            x[s] = (x + (x_max - x) * gamma)[s]
        attr += (x - x_old) * grad
    return x, attr, selections, x != x_start
