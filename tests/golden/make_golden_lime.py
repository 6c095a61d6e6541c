"""Regenerate tests/golden/lime.npz and tests/golden/lime_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lime.py

The reference's own LimeImageExplainer(random_state=seed).explain_instance and ImageExplanation.get_image_and_mask
(util/attribution_methods/lime/lime_image.py) run unmodified, on the CPU, with limeAttr.batch_predict on the tiny classifier of
ig_small.npz (10 classes, so top_labels=5 holds) and a segmentation_fn that returns stored Voronoi segments.  Its three skimage
imports (lime_image.py:11, wrappers/scikit_image.py:3) are satisfied by empty stub modules in sys.modules: no skimage function
runs when a segmentation_fn is passed and the image has three channels.  sklearn (Ridge, pairwise_distances) is the installed one.

Inputs (tests/lime_restated.seeded_case): in<i>_seg (int16) and in<i>_image (H, W, 3) float32 at 40 x 36 (24 superpixels) and
65 x 63 (70).  Per case <tag>: <tag>_params = [input, num_samples, seed, hide_color (nan = None)], <tag>_data (np.packbits of the
0/1 matrix a wrapper around explainer.base.explain_instance_with_data logged), <tag>_labels (float32, the classifier's
probabilities), <tag>_dist (fp64), <tag>_top (the five labels), per label in that order <tag>_intercept, <tag>_features /
<tag>_weights (local_exp), <tag>_score, <tag>_local_pred (fp64), <tag>_mask (get_image_and_mask(top_labels[0], positive_only=True)),
and <tag>_err = the largest |restatement - reference| over coefficients, intercepts, scores, local predictions, distances.
Every case is held to lime_restated.conditioned(restatement, err) and to equal orders and masks of the reference and the fp64
restatement; a seed that fails is not used.

lime_api.json: parameter names and defaults (inspect.signature) of the public functions and methods.
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
    sys.exit("make_golden_lime.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
sys.dont_write_bytecode = True
for name in ("skimage", "skimage.color", "skimage.segmentation"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["skimage.color"].gray2rgb = None
sys.modules["skimage.segmentation"].felzenszwalb = sys.modules["skimage.segmentation"].slic = sys.modules["skimage.segmentation"].quickshift = None
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from util.attribution_methods.lime import limeAttr, lime_image  # noqa: E402
import lime_restated as R                                        # noqa: E402
from helpers import tiny_from                                    # noqa: E402

# (H, W, Voronoi points, seed, superpixels expected)
INPUTS = [(40, 36, 24, 1, 24), (65, 63, 70, 1, 70)]
# tag: (input, num_samples, random_state seed, hide_color)
CASES = {"a": (0, 200, 11, 0), "b": (0, 200, 12, None), "c": (1, 300, 13, 0), "d": (1, 300, 14, None)}


def run(image, seg, n, seed, hide, model):
    explainer = lime_image.LimeImageExplainer(random_state=seed)
    log = {}
    inner = explainer.base.explain_instance_with_data

    def logged(data, labels, distances, label, num_features, **kw):
        log.update(data=data.copy(), labels=labels.copy(), dist=distances.copy())
        ret = inner(data, labels, distances, label, num_features, **kw)
        log.setdefault("per", []).append((label, ret))
        return ret
    explainer.base.explain_instance_with_data = logged
    exp = explainer.explain_instance(image, limeAttr.batch_predict, model, "cpu", top_labels=5, hide_color=hide, num_samples=n,
                                     segmentation_fn=lambda im: seg.astype(np.int64))
    _, mask = exp.get_image_and_mask(exp.top_labels[0], positive_only=True, hide_rest=False)
    return exp, mask, log


def sig(fn, drop_self):
    params = list(inspect.signature(fn).parameters.values())[1 if drop_self else 0:]
    return [{"name": p.name, "has_default": p.default is not inspect.Parameter.empty,
             "default": None if p.default is inspect.Parameter.empty else (list(p.default) if isinstance(p.default, tuple) else p.default)}
            for p in params]


def main():
    model = tiny_from(np.load(os.path.join(HERE, "ig_small.npz")))
    store = {}
    inputs = []
    for i, (H, W, cells, seed, want_d) in enumerate(INPUTS):
        seg, image = R.seeded_case(H, W, cells, seed)
        assert len(np.unique(seg)) == want_d == int(seg.max()) + 1, (i, len(np.unique(seg)))
        store[f"in{i}_seg"], store[f"in{i}_image"] = seg, image
        inputs.append((seg, image))
    for tag, (i, n, seed, hide) in CASES.items():
        seg, image = inputs[i]
        exp, mask, log = run(image, seg, n, seed, hide, model)
        data, labels = log["data"], log["labels"]
        D = data.shape[1]
        assert labels.dtype == np.float32 and data.shape == (n, D) and set(np.unique(data)) <= {0, 1}
        top = [int(l) for l in exp.top_labels]
        # the reference fits in ascending probability (`for label in top`, lime_image.py:210-213); stored most probable first
        assert [int(l) for l, _ in log["per"]] == top[::-1]
        log["per"] = log["per"][::-1]
        assert exp.score == log["per"][0][1][2] and exp.local_pred == log["per"][0][1][3]          # what is left is the top label's
        feats = np.array([[f for f, _ in ret[1]] for _, ret in log["per"]], np.int16)
        wts = np.array([[w for _, w in ret[1]] for _, ret in log["per"]], np.float64)
        icpt = np.array([ret[0] for _, ret in log["per"]], np.float64)
        score = np.array([ret[2] for _, ret in log["per"]], np.float64)
        pred = np.array([ret[3][0] for _, ret in log["per"]], np.float64)
        mine = R.explain(data, labels[:, top])
        ref_coef = np.zeros_like(mine["coef"])
        for l in range(len(top)):
            ref_coef[l, feats[l]] = wts[l]
        err = max(np.abs(mine["coef"] - ref_coef).max(), np.abs(mine["intercept"] - icpt).max(), np.abs(mine["score"] - score).max(),
                  np.abs(mine["local_pred"] - pred).max(), np.abs(mine["dist"] - log["dist"]).max())
        assert R.conditioned(mine, err), ("ill conditioned", tag, err)
        assert np.array_equal(mine["order"], feats), "the fp64 restatement orders otherwise"
        assert np.array_equal(R.mask_of(seg, mine["order"][0], mine["coef"][0]), mask), "the restated mask left the reference"
        assert np.array_equal(R.top_labels(labels[0], 5), top)
        store.update({f"{tag}_params": np.array([i, n, seed, np.nan if hide is None else hide], np.float64),
                      f"{tag}_data": np.packbits(data.astype(np.uint8), axis=None), f"{tag}_labels": labels,
                      f"{tag}_dist": log["dist"].astype(np.float64), f"{tag}_top": np.array(top, np.int16), f"{tag}_intercept": icpt,
                      f"{tag}_features": feats, f"{tag}_weights": wts, f"{tag}_score": score, f"{tag}_local_pred": pred,
                      f"{tag}_mask": mask.astype(np.int8), f"{tag}_err": np.float64(err)})
        gaps = np.abs(np.diff(np.abs(wts), axis=1)).min()
        print(f"{tag}: N {n} D {D} top {top} chosen {R.chosen_features(feats[0], ref_coef[0])} restatement err {err:.3e} "
              f"smallest |coef| gap {gaps:.3e} score {score.round(4).tolist()}")
    np.savez_compressed(os.path.join(HERE, "lime.npz"), **store)

    api = {"LimeImageExplainer.__init__": sig(lime_image.LimeImageExplainer.__init__, True),
           "LimeImageExplainer.explain_instance": sig(lime_image.LimeImageExplainer.explain_instance, True),
           "ImageExplanation.__init__": sig(lime_image.ImageExplanation.__init__, True),
           "ImageExplanation.get_image_and_mask": sig(lime_image.ImageExplanation.get_image_and_mask, True),
           "get_lime_attr": sig(limeAttr.get_lime_attr, False), "batch_predict": sig(limeAttr.batch_predict, False),
           "make_tensor": sig(limeAttr.make_tensor, False)}
    with open(os.path.join(HERE, "lime_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
    for n in ("lime.npz", "lime_api.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
