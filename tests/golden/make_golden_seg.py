"""Regenerate tests/golden/seg.npz from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_seg.py

XAI_Survey/evaluations/utils/metrices.py is imported unmodified (it needs sklearn only).  evaluateImageNetSeg.py cannot be imported
(transformers, clip, captum), so the source of `eval_batch`, and of the fold inside `evaluate_imagenet_seg` (the initial totals, the
statements of the loop body that update them and the four fh.write calls), is taken out of the file with `ast` at generation time
and executed against metrices' names.  Nothing of that source is written anywhere.

Inputs (tests/seg_restated.seeded_case) are 224 x 224 and rebuilt from seeds, not stored.  Per case <tag>: Res = (x - x.min()) /
(x.max() - x.min()) and ret = Res.mean() by torch on the CPU (:215-217), then the reference's eval_batch(Res, ret, labels):
<tag>_ret, <tag>_correct, <tag>_labeled, <tag>_inter, <tag>_union, <tag>_ap, <tag>_f1 (224 values, one per image row).
Over the case list: fold_numbers (mIoU, pixAcc, mAP, mF1) and fold_lines (the four text lines as bytes).

A case is stored only if no pixel of Res lies in the closed interval between the reference's ret and K44's stated mean
(seg_restated.stated_mean) widened by 4 ulp of ret on each side: then both thresholds cut the map identically.  A seed that fails
is not used.  `cond` is the widest |ret_ref - ret_stated| over the stored cases.
"""
import ast
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("XAI_REFERENCE_ROOT")
if not REF or not os.path.isdir(REF):
    sys.exit("make_golden_seg.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seg_restated as R  # noqa: E402

EVAL = os.path.join(REF, "XAI_Survey", "evaluations")


def _metrices():
    spec = importlib.util.spec_from_file_location("metrices", os.path.join(EVAL, "utils", "metrices.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _compiled(nodes, name):
    return compile(ast.fix_missing_locations(ast.Module(body=list(nodes), type_ignores=[])), name, "exec")


def _targets(node):
    tg = node.targets if isinstance(node, ast.Assign) else [node.target]
    return [n.id for t in tg for n in ast.walk(t) if isinstance(n, ast.Name)]


def _reference_parts():
    tree = ast.parse(open(os.path.join(EVAL, "evaluateImageNetSeg.py")).read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    eval_batch = _compiled([funcs["eval_batch"]], "eval_batch")
    body = funcs["evaluate_imagenet_seg"].body
    init = [n for n in body if isinstance(n, ast.Assign) and all(t.startswith("total_") for t in _targets(n))]
    loop = next(n for n in body if isinstance(n, ast.For))
    keep = ("pixAcc", "IoU", "mIoU", "mAp", "mF1")
    step = [n for n in loop.body if isinstance(n, (ast.Assign, ast.AugAssign)) and
            all(t.startswith("total_") or t in keep for t in _targets(n))]
    writes = [n for n in body if isinstance(n, ast.Expr) and isinstance(n.value, ast.Call) and
              isinstance(n.value.func, ast.Attribute) and n.value.func.attr == "write"]
    assert len(init) == 2 and len(step) == 11 and len(writes) == 4, (len(init), len(step), len(writes))
    return eval_batch, _compiled(init, "fold_init"), _compiled(step, "fold_step"), _compiled(writes, "fold_write")


class _Lines(list):
    def write(self, text):
        self.append(text)


def main():
    metrices = _metrices()
    eval_code, init_code, step_code, write_code = _reference_parts()
    ns = {k: getattr(metrices, k) for k in metrices.__all__}
    ns.update(np=np, torch=torch, warnings=warnings)
    exec(eval_code, ns)
    fold_ns = {"np": np}
    exec(init_code, fold_ns)
    out, cond, tags = {}, 0.0, []
    for kind, seed in R.CASES:
        x, labels = R.seeded_case(kind, seed)
        Res = torch.from_numpy(x).reshape(1, 1, R.HW, R.HW)
        Res = (Res - Res.min()) / (Res.max() - Res.min())
        ret = Res.mean()
        res_np = Res.numpy().copy().reshape(R.HW, R.HW)
        assert np.array_equal(res_np, R.normalize(x), equal_nan=True)
        stated = R.stated_mean(res_np)
        ret_np = np.float32(ret.item())
        if not np.isnan(ret_np):
            lo, hi = min(ret_np, stated), max(ret_np, stated)
            pad = 4 * np.spacing(ret_np)
            if ((res_np >= lo - pad) & (res_np <= hi + pad)).any():
                sys.exit(f"{kind}/{seed}: a pixel lies between the two means; pick another seed")
            cond = max(cond, float(abs(np.float64(ret_np) - np.float64(stated))))
        else:
            assert np.isnan(stated)
        correct, labeled, inter, union, ap, f1, pred, target = ns["eval_batch"](Res, ret, torch.from_numpy(labels)[None])
        tag = f"{kind}{seed}"
        tags.append(tag)
        out.update({f"{tag}_ret": ret_np, f"{tag}_correct": correct, f"{tag}_labeled": labeled, f"{tag}_inter": inter,
                    f"{tag}_union": union, f"{tag}_ap": ap, f"{tag}_f1": f1})
        fold_ns.update(correct=correct, labeled=labeled, inter=inter, union=union, ap=ap, f1=f1)
        exec(step_code, fold_ns)
        print(tag, float(ret_np), float(stated), int(correct), int(labeled), inter, union, ap, float(np.mean(f1)))
    fold_ns["fh"] = _Lines()
    exec(write_code, fold_ns)
    out["fold_numbers"] = np.array([fold_ns["mIoU"], fold_ns["pixAcc"], fold_ns["mAp"], fold_ns["mF1"]], np.float64)
    out["fold_lines"] = np.array([l.encode() for l in fold_ns["fh"]])
    out["cond"] = np.float64(cond)
    out["tags"] = np.array([t.encode() for t in tags])
    np.savez_compressed(os.path.join(HERE, "seg.npz"), **out)
    print("".join(fold_ns["fh"]), "cond", cond)


if __name__ == "__main__":
    main()
