"""Regenerate tests/golden/agi.npz and tests/golden/agi_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_agi.py

The reference's own AGI.test (util/attribution_methods/AGI.py:83-115) runs unmodified, on the CPU, for the tiny classifier of
tests/helpers.py (10 classes, seeded weights stored as w_*), behind the reference's AGI.Normalize with the harness's ImageNet
mean and std; the post-processing of evaluatePerturbation.py:132-139 is driven from here.  torchvision, which AGI.py imports but
does not use, is stubbed with inert placeholders.  A wrapper model logs every forward's input and logits, and a hook on the input
logs the two input gradients of each iteration (g_adv, then g_lab); nothing of the reference is edited.

Cases (keys <tag>_*):
  (a) the harness arguments at 16^2: a [0, 1] image, epsilon 0.05, topk 1, selected_ids range(0, 999, 1000), max_iter 20;
  (b) selected_ids [4, 5, 6]: one of them is init_pred (skipped);
  (c) an attack that breaks early: a pair whose argmax reaches its class before max_iter;
  (d) an image given in 0..255 (data in [0, 1]), so that the fgsm step clamps at both bounds;
  (e) selected_ids == [init_pred]: AGI.test returns (0, 0, 0).
Per case: data (the reference's data, after pre_processing), mean, std, classes, params (epsilon, max_iter), init_pred, and per
pair in order the forwards it ran: fx (inputs), fl (logits), fga / fgl (g_adv / g_lab, zeros where the pair broke), pair (class
of each logged forward); adv (step_grad, adv_ex of test) and hm (the normalised map before the harness's abs).
Seeds are searched until no decision can flip between two correct fp32 evaluations: every argmax has a top-two logit margin of
at least 1e-3 and no nonzero g_adv element lies within 1e-5 (relative to its maximum) of zero.

agi_api.json: parameter names and defaults (inspect.signature) of test, pgd_step, fgsm_step, pre_processing and Normalize.
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XAI_REFERENCE_ROOT")
if not REF or not os.path.isdir(REF):
    sys.exit("make_golden_agi.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

if "torchvision" not in sys.modules:                      # AGI.py imports transforms and models and uses neither
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.models": tv.models})

from util.attribution_methods import AGI  # noqa: E402
from helpers import TinyNet                # noqa: E402

torch.set_num_threads(4)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MARGIN, GRAD_GAP = 1e-3, 1e-5


class Logged(torch.nn.Module):
    """Calls `inner` unchanged; logs each forward's input and logits, and the gradients that reach the input."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.log = []

    def forward(self, x):
        out = self.inner(x)
        rec = {"x": x.detach().clone(), "logits": out.detach().clone(), "g": []}
        self.log.append(rec)
        if x.requires_grad:
            x.register_hook(lambda g, rec=rec: rec["g"].append(g.detach().clone()))
        return out


def harness_map(adv):
    """evaluatePerturbation.py:132-138 on adv_ex"""
    hm = adv
    hm = np.mean(hm, axis=0)
    q = np.percentile(hm, 80)
    u = np.percentile(hm, 99)
    hm[hm < q] = q
    hm[hm > u] = u
    return (hm - q) / (u - q)


def run(model, img_hwc, classes, eps=0.05, max_iter=20):
    agi_model = torch.nn.Sequential(AGI.Normalize(MEAN, STD), model)
    logged = Logged(agi_model)
    pred, img, adv = AGI.test(logged, "cpu", img_hwc, eps, 1, classes, max_iter)
    init, rest = logged.log[0], logged.log[1:]
    init_pred = int(init["logits"].argmax(1)[0])
    pair, fx, fl, fga, fgl = [], [], [], [], []
    todo = [c for c in classes if c != init_pred]
    ci, it = 0, 0
    for rec in rest:                                      # forwards of the pairs, in order
        c = todo[ci]
        pair.append(c)
        fx.append(rec["x"][0].numpy())
        fl.append(rec["logits"][0].numpy())
        if rec["g"]:
            assert len(rec["g"]) == 2
            fga.append(rec["g"][0][0].numpy())
            fgl.append(rec["g"][1][0].numpy())
            it += 1
        else:                                             # the break: no gradient, the pair ends
            fga.append(np.zeros_like(fx[-1]))
            fgl.append(np.zeros_like(fx[-1]))
            ci, it = ci + 1, 0
            continue
        if it == max_iter:
            ci, it = ci + 1, 0
    out = {"data": AGI.pre_processing(img_hwc, "cpu").numpy(), "classes": np.array(list(classes), np.int64),
           "params": np.array([eps, max_iter], np.float64), "init_pred": np.int64(init_pred), "init_logits": init["logits"][0].numpy(),
           "pair": np.array(pair, np.int64), "fx": np.array(fx, np.float32).reshape((-1,) + img_hwc.shape[2:] + img_hwc.shape[:2]),
           "fl": np.array(fl, np.float32).reshape(len(pair), init["logits"].shape[1])}
    out["fga"] = np.array(fga, np.float32).reshape(out["fx"].shape)
    out["fgl"] = np.array(fgl, np.float32).reshape(out["fx"].shape)
    if isinstance(adv, int):
        assert pred == 0 and img == 0 and adv == 0
        out["zero"] = np.int64(1)
    else:
        assert pred == init_pred
        out["zero"] = np.int64(0)
        out["adv"] = adv.astype(np.float32)
        out["hm"] = harness_map(adv.copy()).astype(np.float32)
    return out


def safe(o):
    """no argmax within MARGIN of a tie, no nonzero g_adv within GRAD_GAP of zero"""
    logits = np.concatenate([o["init_logits"][None], o["fl"]]) if len(o["fl"]) else o["init_logits"][None]
    top2 = np.sort(logits, axis=1)[:, -2:]
    if (top2[:, 1] - top2[:, 0]).min() < MARGIN:
        return False
    for g in o["fga"]:
        a = np.abs(g)
        if a.max() > 0 and ((a > 0) & (a < GRAD_GAP * a.max())).any():
            return False
    return True


def breaks(o):
    """(updates, broke) per pair"""
    res = []
    for c in np.unique(o["pair"]):
        idx = np.nonzero(o["pair"] == c)[0]
        res.append((int(np.abs(o["fga"][idx]).sum(axis=(1, 2, 3)).astype(bool).sum()), int(np.argmax(o["fl"][idx[-1]])) == c))
    return res


def main():
    torch.manual_seed(7)
    model = TinyNet().eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(4.0)
    for p in model.parameters():
        p.requires_grad_(False)
    out = {"w_" + k.replace(".", "_"): v.numpy() for k, v in model.state_dict().items()}
    out["mean"], out["std"] = np.array(MEAN, np.float32), np.array(STD, np.float32)

    def search(tag, make, ok, tries=400):
        for seed in range(tries):
            rng = np.random.default_rng(1000 * (ord(tag) - 96) + seed)
            img, classes = make(rng)
            o = run(model, img, classes)
            if safe(o) and ok(o):
                out.update({f"{tag}_{k}": v for k, v in o.items()})
                out[f"{tag}_seed"] = np.int64(seed)
                print(f"({tag}) seed {seed}: init_pred {int(o['init_pred'])}, classes {list(classes)}, pairs {breaks(o)}")
                return o
        sys.exit(f"({tag}): no seed in {tries} satisfies the case and the margins")

    hw = 16
    unit = lambda rng: rng.random((hw, hw, 3)).astype(np.float32)            # noqa: E731  a [0, 1] HWC image, as the harness's
    harness_ids = list(range(0, 999, int(1000 / 1)))
    # (a) the harness row: one false class (0), the image must not be predicted as 0
    search("a", lambda rng: (unit(rng), harness_ids), lambda o: not o["zero"])
    # (b) three false classes, init_pred among them
    search("b", lambda rng: (unit(rng), [4, 5, 6]), lambda o: not o["zero"] and int(o["init_pred"]) in (4, 5, 6))
    # (c) a pair that breaks before max_iter
    search("c", lambda rng: (unit(rng), [7, 2]),
           lambda o: not o["zero"] and any(b and 0 < n < 20 for n, b in breaks(o)))
    # (d) an image in 0..255: data in [0, 1], the step clamps at 0 and at 1
    def clamps(o):
        d = o["data"][0]
        moved = o["fx"][1:] if len(o["fx"]) > 1 else o["fx"]
        return not o["zero"] and (moved == 0).any() and (moved == 1).any() and ((d > 0) & (d < 1)).any()
    search("d", lambda rng: (np.round(unit(rng) * 255).astype(np.float32), [1, 8]), clamps)
    # (e) the only selected class is init_pred: (0, 0, 0)
    def own_class(rng):
        img = unit(rng)
        with torch.no_grad():
            x = AGI.pre_processing(img, "cpu")
            c = int(torch.nn.Sequential(AGI.Normalize(MEAN, STD), model)(x).argmax(1)[0])
        return img, [c]
    search("e", own_class, lambda o: bool(o["zero"]))
    np.savez_compressed(os.path.join(HERE, "agi.npz"), **out)

    def sig(fn, drop_self):
        params = list(inspect.signature(fn).parameters.values())[1 if drop_self else 0:]
        return [{"name": p.name, "has_default": p.default is not inspect.Parameter.empty,
                 "default": None if p.default is inspect.Parameter.empty else p.default} for p in params]

    api = {"test": sig(AGI.test, False), "pgd_step": sig(AGI.pgd_step, False), "fgsm_step": sig(AGI.fgsm_step, False),
           "pre_processing": sig(AGI.pre_processing, False), "Normalize.__init__": sig(AGI.Normalize.__init__, True),
           "Normalize.forward": sig(AGI.Normalize.forward, True)}
    with open(os.path.join(HERE, "agi_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
    for n in ("agi.npz", "agi_api.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
