"""NumPy float32 restatement of the reference's AGI (util/attribution_methods/AGI.py:39-115) and of the harness's post-processing
(evaluatePerturbation.py:132-139), for the AGI tests.

The classifier is abstracted away: `attack` asks `oracle(i, x)` for the logits and the two input gradients of forward i at x, so
that the same loop replays recorded values (the fixture's, or the device's own) or runs a live classifier (`torch_oracle`).
Semantics restated: the break before any update when the argmax (torch.max on the CPU: the first NaN, else the first maximum)
is the class; every step from the ORIGINAL image, x = clamp(data + eps * sign(g_adv), 0, 1) with sign(NaN) = sign(+-0) = +0;
c_delta += -g_lab * (x - data) from +0; step_grad = the pairs' c_delta summed in class order from +0."""
import numpy as np
import torch

F32 = np.float32


def torch_argmax(row):
    row = np.asarray(row)
    nan = np.flatnonzero(np.isnan(row))
    return int(nan[0]) if nan.size else int(np.argmax(row))


def sign_step(data, eps, g_adv, g_lab):
    """-> (x, delta), all float32"""
    s = np.where(g_adv > 0, F32(1), np.where(g_adv < 0, F32(-1), F32(0))).astype(F32)
    v = (data + F32(eps) * s).astype(F32)
    x = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
    return x, ((-g_lab) * (x - data)).astype(F32)


def attack(data, cls, eps, max_iter, oracle):
    """One (image, class) attack.  data: (C, H, W) float32.  oracle(i, x) -> (logits, g_adv, g_lab) of forward i.
    -> (list of the x each forward ran on, c_delta, updates, broke)"""
    x = data.copy()
    c = np.zeros_like(data)
    seen = []
    for i in range(max_iter):
        seen.append(x)
        logits, g_adv, g_lab = oracle(i, x)
        if torch_argmax(logits) == cls:
            return seen, c, i, True
        x, d = sign_step(data, eps, np.asarray(g_adv, F32), np.asarray(g_lab, F32))
        c = (c + d).astype(F32)
    return seen, c, max_iter, False


def run(data, classes, init_pred, eps, max_iter, oracle_of):
    """The loop of test over the classes; oracle_of(k) is the oracle of the k-th class's attack.
    -> (per class: (seen, c_delta, updates, broke) or None when skipped, step_grad or None when no update happened)"""
    pairs, total, any_update = [], np.zeros_like(data), False
    for k, cls in enumerate(classes):
        if cls == init_pred:
            pairs.append(None)
            continue
        seen, c, n, broke = attack(data, cls, eps, max_iter, oracle_of(k))
        pairs.append((seen, c, n, broke))
        total = (total + c).astype(F32)
        any_update |= n > 0
    return pairs, (total if any_update else None)


def harness_map(step_grad, q_lo=80, q_hi=99):
    """(C, H, W) -> the normalised (H, W) map of evaluatePerturbation.py:132-138 (NumPy, float32)"""
    hm = np.mean(np.asarray(step_grad, F32), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lo, hi = np.percentile(hm, q_lo), np.percentile(hm, q_hi)
        hm = np.where(hm < lo, lo, hm).astype(F32)
        hm = np.where(hm > hi, hi, hm).astype(F32)
        return ((hm - lo) / (hi - lo)).astype(F32)


def torch_oracle(model, mean, std, init_pred, cls):
    """A live classifier on the CPU behind (x - mean) / std: gradients of softmax[cls] and softmax[init_pred] with respect to x."""
    m = torch.tensor(np.asarray(mean, F32)).view(1, -1, 1, 1)
    s = torch.tensor(np.asarray(std, F32)).view(1, -1, 1, 1)

    def oracle(i, x):
        xs = torch.from_numpy(np.ascontiguousarray(x)[None]).requires_grad_(True)
        logits = model((xs - m) / s)
        p = torch.softmax(logits, dim=1)
        (ga,) = torch.autograd.grad(p[0, cls], xs, retain_graph=True)
        (gl,) = torch.autograd.grad(p[0, init_pred], xs)
        return logits[0].detach().numpy(), ga[0].numpy(), gl[0].numpy()
    return oracle
