"""Regenerate tests/golden/gig.npz and tests/golden/gig_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gig.py

The reference's own GuidedIG().GetMask (util/attribution_methods/GIGBuilder.py:194-310) runs unmodified, on the CPU, with the
reference's call_model_function, for the tiny classifier of tests/helpers.py (seeded weights, stored as w_*):
  (a) keys a_*: a 3x16x16 input, the harness's arguments (evaluatePerturbation.py:114-118: 50 steps, fraction 0.5,
      max_dist 1.0, zero baseline);
  (b) keys b_*: a 3x16x16 input, GetMask's own fraction 0.25 and max_dist 0.02, 40 steps, and a non-zero baseline that equals
      the input on about one feature in eight (the NaN-alpha path) -- inputs on a 1/256 grid and baselines on a 1/16 grid, so
      that x_baseline + (x_input - x_baseline) * 1.0 == x_input exactly and the reference's last step ends;
For (a) and (b), a wrapper around call_model_function logs the x it is called with and the gradient it returns at every step
(<tag>_x[s], <tag>_g[s]; <tag>_x[steps] is the x the reference ends with, the same tensor object, updated in place), and a
counting wrapper around torch.quantile gives the selections of every step (<tag>_iters).  Nothing of the reference is edited.

gig_api.json: parameter names and defaults (inspect.signature) of GuidedIG.GetMask and call_model_function.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XAI_REFERENCE_ROOT")
if not REF or not os.path.isdir(REF):
    sys.exit("make_golden_gig.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from util.attribution_methods import GIGBuilder as GIG  # noqa: E402
from helpers import TinyNet                              # noqa: E402

torch.set_num_threads(4)


def run(model, x, baseline, target, steps, fraction, max_dist):
    xs, gs, iters = [], [], []
    state = {"x": None}
    calls = [0]
    quantile = torch.quantile

    def counting_quantile(*a, **k):
        calls[0] += 1
        return quantile(*a, **k)

    def logged(images, model, device, call_model_args=None, expected_keys=None):
        if xs:
            iters.append(calls[0])
            calls[0] = 0
        state["x"] = images
        xs.append(images.detach().clone())
        out = GIG.call_model_function(images, model, device, call_model_args=call_model_args, expected_keys=expected_keys)
        gs.append(out[GIG.INPUT_OUTPUT_GRADIENTS].detach().clone())
        return out

    torch.quantile = counting_quantile
    try:
        mask = GIG.GuidedIG().GetMask(x, model, "cpu", logged, {"class_idx_str": int(target)}, x_baseline=baseline,
                                      x_steps=steps, fraction=fraction, max_dist=max_dist)
    finally:
        torch.quantile = quantile
    iters.append(calls[0])
    xs.append(state["x"].detach().clone())
    return (mask.detach().numpy(), np.stack([t.numpy() for t in xs]), np.stack([t.numpy() for t in gs]),
            np.array(iters, np.int32))


def main():
    torch.manual_seed(7)
    model = TinyNet().eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(4.0)                     # spread the softmax so that its gradient is not flat
    for p in model.parameters():
        p.requires_grad_(False)
    out = {"w_" + k.replace(".", "_"): v.numpy() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(11)

    def target_of(x):
        with torch.no_grad():
            return int(model(x).argmax(1)[0])

    # (a) harness arguments
    xa = torch.from_numpy(rng.standard_normal((1, 3, 16, 16)).astype(np.float32))
    ta = target_of(xa)
    m, xs, gs, it = run(model, xa, torch.zeros_like(xa), ta, 50, 0.5, 1.0)
    out.update(a_input=xa.numpy(), a_target=np.int64(ta), a_mask=m, a_x=xs, a_g=gs, a_iters=it,
               a_params=np.array([50, 0.5, 1.0]))
    print("(a) target", ta, "selections", int(it.sum()), "max |mask|", float(np.abs(m).max()))

    # (b) GetMask's defaults, non-zero baseline equal to the input on some features
    xb = np.round(rng.standard_normal((1, 3, 16, 16)) * 256).astype(np.float32) / 256
    bb = np.round(rng.standard_normal((1, 3, 16, 16)) * 4).astype(np.float32) / 16
    same = rng.random((1, 3, 16, 16)) < 0.125
    bb[same] = xb[same]
    assert np.array_equal(bb + (xb - bb) * np.float32(1.0), xb)
    xb, bb = torch.from_numpy(xb), torch.from_numpy(bb)
    tb = target_of(xb)
    m, xs, gs, it = run(model, xb, bb, tb, 40, 0.25, 0.02)
    out.update(b_input=xb.numpy(), b_baseline=bb.numpy(), b_target=np.int64(tb), b_mask=m, b_x=xs, b_g=gs, b_iters=it,
               b_params=np.array([40, 0.25, 0.02]))
    print("(b) target", tb, "selections", int(it.sum()), "equal features", int(same.sum()), "max |mask|", float(np.abs(m).max()))
    np.savez_compressed(os.path.join(HERE, "gig.npz"), **out)

    def sig(fn, drop_self):
        params = list(inspect.signature(fn).parameters.values())[1 if drop_self else 0:]
        return [{"name": p.name, "has_default": p.default is not inspect.Parameter.empty,
                 "default": None if p.default is inspect.Parameter.empty else p.default} for p in params]

    api = {"GuidedIG.GetMask": sig(GIG.GuidedIG.GetMask, True), "call_model_function": sig(GIG.call_model_function, False)}
    with open(os.path.join(HERE, "gig_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
    for n in ("gig.npz", "gig_api.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
