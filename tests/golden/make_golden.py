#!/usr/bin/env python3
"""Generate the golden input/output vectors under tests/golden/ by IMPORTING the
reference (a read-only checkout of the original project, named by XAI_REFERENCE_ROOT) and running it on
small seeded inputs.  The reference itself never travels: only the .npz data does.

Run once, where a checkout of the reference is at hand (no GPU needed):

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

What is pinned (reference file:line in brackets):
  ig_small.npz / ig_224.npz   IG, Left-IG, IDG, IDGI outputs + per-step gradients/logits
                              [util/attribution_methods/saliencyMethods.py:13-181,209-314]
  kern.npz                    gkern(31,31), gkern(11,5), zero-padded blur outputs, auc
                              [util/test_methods/MASTestFunctions.py:11-32]
  perturb_small.npz           32x32 / step 32: salient order, every perturbed image, all
  perturb_patch.npz           five metric classes' return tuples (+ patch_mask branch)
  perturb_224.npz             224x224 / step 224 with per-step image checksums
  perturb_ties.npz            a heavily tied map (ReLU'd, quantised): return tuples + the pixel order the reference's unstable
                              argsort produced here, for the caller-supplied-order path (SURVEY 7 "hard parts": tie order)
                              [MASTestFunctions.py:72-385, RISETestFunctions.py:51-237,
                               AICTestFunctions.py:51-225, PosNegPertFunctions.py:31-175,
                               MonotonicityTest.py:51-213]
  vit_mini.npz                hooked mini-ViT: pixel IG + attention-space IG (Baselines.IG)
                              [VIT_LRP/ViT_ig.py:57-253, VIT_LRP/ViT_explanation_generator.py:139-386]
  cam.npz                     Grad-CAM arithmetic of the reference-owned CAM code (ViT_CX/get_feature_map.py:17-23,
                              ViT_CX/base_cam.py:48-64,129); captum's LayerGradCam itself is absent
  vit_cx.npz                  ViT-CX norm_matrix / cosine similarity / token reshape and causal_score.forward
                              [ViT_CX/ViT_CX.py:22-46, ViT_CX/causal_score.py:17-61]
  tis.npz                     TIS on the mini ViT, every stage except the absent k-means [TIS.py:96-365]
  smoothgrad.npz              seeded smoothGrad("IG", ..., vis=True): mean, total_gradients, noisy_imgs [saliencyMethods.py:184-205]
  sweep_small.npz             the 10-key Counter of run_perturbation, driven exactly like
                              XAI_Survey/evaluations/evaluatePerturbation.py:448-497
  zoo_state_dicts.npz         state-dict key names and tensor shapes of the classifiers the reference's harness instantiates
                              [util/modified_models/resnet.py:430-560 (torchvision layout), VIT_LRP/ViT_ig.py:256-273]
  vit_inflow.npz              InFlow rollout / bidirectional(InFlow=True) on the mini ViT [ViT_explanation_generator.py:48-88,196-240,447-464]
  sweep_counter.npz           five images folded with the reference's `pert_result_counter += ...` (:594-596) and written with its CSV
                              loop (:612-615): keys whose running sum is <= 0 are dropped and re-enter at the end
The only stubs are inert placeholder modules: `cvxopt` (used by the reference only under
special_version=True, which is never exercised) and, for the ViT-CX / TIS files, the third-party modules they
import at module level but never reach on the functions called here (see vitcx_fixture / tis_fixture).
"""
import os
import sys
import types
import hashlib

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XAI_REFERENCE_ROOT")
if not REF or not os.path.isdir(REF):
    sys.exit("make_golden.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
_cv = types.ModuleType("cvxopt")
_cv.matrix = lambda *a, **k: None
_cv.solvers = types.SimpleNamespace(options={}, qp=None)
sys.modules["cvxopt"] = _cv

from util.attribution_methods import saliencyMethods as attr          # noqa: E402
from util.test_methods import MASTestFunctions as MAS                  # noqa: E402
from util.test_methods import RISETestFunctions as RISE                # noqa: E402
from util.test_methods import AICTestFunctions as AIC                  # noqa: E402
from util.test_methods import PosNegPertFunctions as PNP               # noqa: E402
from util.test_methods import MonotonicityTest as MONO                 # noqa: E402
from util import model_utils                                           # noqa: E402

torch.set_num_threads(4)


# ----------------------------------------------------------------------------- models
class TinyNet(nn.Module):
    """Conv(3,8,3,p=1) -> ReLU -> AdaptiveAvgPool(4) -> Flatten -> Linear(128,10)."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, 3, padding=1)
        self.act = nn.ReLU()
        self.pool = nn.AdaptiveAvgPool2d(4)
        self.fc = nn.Linear(128, 10)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.act(self.conv(x))), 1))


def tiny_model(seed):
    g = torch.Generator().manual_seed(seed)
    m = TinyNet().eval()
    with torch.no_grad():
        m.conv.weight.copy_(torch.randn(m.conv.weight.shape, generator=g) * 0.4)
        m.conv.bias.copy_(torch.randn(m.conv.bias.shape, generator=g) * 0.1)
        m.fc.weight.copy_(torch.randn(m.fc.weight.shape, generator=g) * 0.6)
        m.fc.bias.copy_(torch.randn(m.fc.bias.shape, generator=g) * 0.1)
    return m


def weights_of(m):
    return {"w_" + k.replace(".", "_"): v.detach().numpy().copy() for k, v in m.state_dict().items()}


class Recorder(nn.Module):
    """Wraps a model and keeps every batch it was called with."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.seen = []

    def forward(self, x):
        self.seen.append(x.detach().cpu().clone())
        return self.inner(x)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- IG family
def ig_fixture(name, hw, seed):
    model = tiny_model(seed)
    x = randn(seed + 1, 1, 3, hw, hw)
    with torch.no_grad():
        target = model(x).argmax(1)[0]
    base_t = randn(seed + 2, 1, 3, hw, hw) * 0.3
    steps, batch = 50, 25

    rec = {}
    orig = attr.getGradientsParallel

    def spy(inputs, mdl, tc):
        g, s = orig(inputs, mdl, tc)
        rec.setdefault("g", []).append(g.clone())
        rec.setdefault("s", []).append(s.clone())
        return g, s

    out = dict(x=x.numpy(), target=np.int64(target.item()), baseline_tensor=base_t.numpy(),
               steps=np.int64(steps), batch=np.int64(batch), **weights_of(model))

    attr.getGradientsParallel = spy
    try:
        ig = attr.IG(x.clone(), model, steps, batch, 1, 0, "cpu", target)
        out["ig"] = ig.detach().numpy()
        if hw <= 64:
            out["gradients"] = torch.cat(rec["g"]).numpy()
        out["logits"] = torch.cat(rec["s"]).numpy()
        rec.clear()
        lig = attr.IG(x.clone(), model, steps, batch, 0.9, 0, "cpu", target)
        out["lig"] = lig.detach().numpy()
        rec.clear()
        igb = attr.IG(x.clone(), model, steps, 50, 1, base_t.clone(), "cpu", target)
        out["ig_tensor_baseline"] = igb.detach().numpy()
        rec.clear()
        ligb = attr.IG(x.clone(), model, steps, 10, 0.5, 0.25, "cpu", target)
        out["lig_a05_b025"] = ligb.detach().numpy()
        out["lig_a05_b025_logits"] = torch.cat(rec["s"]).numpy()
        rec.clear()
    finally:
        attr.getGradientsParallel = orig

    # quirk: steps % batch_size != 0 -> prints and returns four zeros  [saliencyMethods.py:14-16]
    bad = attr.IG(x.clone(), model, steps, 7, 1, 0, "cpu", target)
    assert bad == (0, 0, 0, 0)

    if hw <= 64:
        slopes, step_size = attr.getSlopes(torch.zeros_like(x), x.clone(), model, steps, batch, "cpu", target)
        out["slopes"] = slopes.numpy()
        out["slope_step"] = np.float64(step_size)
        al, sub = attr.getAlphaParameters(slopes.clone(), steps, step_size)
        out["idg_alphas"] = al.detach().numpy()
        out["idg_substep"] = sub.numpy()
        out["idg"] = attr.IDG(x.clone(), model, steps, batch, 0, "cpu", target).numpy()
        out["idgi"] = attr.IDGI(x.clone(), model, steps, batch, 0, "cpu", target).detach().numpy()
        xg = x.clone()
        out["input_grad"] = attr.input_grad(xg, model, target).numpy()
        pct, logit = model_utils.getPrediction(x.clone(), model, "cpu", -1)
        out["pred_pct"], out["pred_logit"] = np.float32(pct), np.float32(logit)
        out["pred_class"] = np.int64(model_utils.getClass(x.clone(), model, "cpu").item())
        out["pred_class_k2"] = np.int64(model_utils.getClass(x.clone(), model, "cpu", 2).item())
    np.savez(os.path.join(HERE, name), **out)
    print(name, {k: getattr(v, "shape", v) for k, v in out.items() if not k.startswith("w_")})


# ----------------------------------------------------------------------------- kernels
def kern_fixture():
    out = {}
    out["gkern_31_31"] = MAS.gkern(31, 31).numpy()
    out["gkern_11_5"] = MAS.gkern(11, 5).numpy()
    x = randn(11, 1, 3, 96, 96)
    out["blur_x"] = x.numpy()
    out["blur_31_31"] = torch.nn.functional.conv2d(x, MAS.gkern(31, 31), padding=15).numpy()
    out["blur_11_5"] = torch.nn.functional.conv2d(x, MAS.gkern(11, 5), padding=5).numpy()
    x2 = randn(12, 1, 3, 20, 28)           # image smaller than the 31-tap support
    out["blur_small_x"] = x2.numpy()
    out["blur_small_31_31"] = torch.nn.functional.conv2d(x2, MAS.gkern(31, 31), padding=15).numpy()
    curves = np.random.default_rng(5).random((6, 225))
    out["auc_curves"] = curves
    out["auc_values"] = np.array([MAS.auc(c) for c in curves])
    out["auc_linspace"] = np.float64(MAS.auc(np.linspace(0, 1, 225)))
    np.savez(os.path.join(HERE, "kern.npz"), **out)
    print("kern.npz", list(out))


# ----------------------------------------------------------------------------- ins/del
def tie_free_map(seed, hw):
    """|N(0,1)| saliency map with all-distinct float32 values, so that the reference's
    unstable np.argsort [MASTestFunctions.py:209] has exactly one possible answer."""
    rng = np.random.default_rng(seed)
    vals = np.unique(np.abs(rng.standard_normal(2 * hw * hw)).astype(np.float32))
    assert vals.size >= hw * hw
    sal = rng.permutation(vals)[: hw * hw].reshape(hw, hw).astype(np.float32)
    assert len(np.unique(sal)) == sal.size
    return sal


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def perturb_fixture(name, hw, step, seed, max_bs, patch=None, keep_images=True, blur_k=(11, 5), ties=False):
    kern = MAS.gkern(*blur_k)
    blur = lambda t: torch.nn.functional.conv2d(t, kern, padding=blur_k[0] // 2)   # noqa: E731
    # pick the first seed >= `seed` that passes the harness's own usability filter
    # [evaluatePerturbation.py:569]: substrates must score lower and change the class
    while True:
        model = tiny_model(seed)
        x = randn(seed + 1, 1, 3, hw, hw)
        with torch.no_grad():
            p0 = torch.softmax(model(x), 1)[0]
            pb = torch.softmax(model(blur(x)), 1)[0]
            pz = torch.softmax(model(torch.zeros_like(x)), 1)[0]
        t = int(p0.argmax())
        if pb.argmax() != t and pz.argmax() != t and pb[t] < p0[t] and pz[t] < p0[t]:
            break
        seed += 1
    sal = tie_free_map(seed + 2, hw)
    if ties:
        # a ReLU'd, coarsely quantised map (what an up-sampled Grad-CAM looks like): most values tie, and the reference's
        # default np.argsort (unstable, ISA-dependent) decides their order -- recorded below as the order it used HERE
        sal = (np.maximum(np.round((sal - sal.mean()) / sal.std() * 2.0), 0) / 2.0).astype(np.float32)
    HW = hw * hw
    patch_mask = None
    if patch is not None:
        n = hw // patch
        ids = torch.arange(n * n).reshape(n, n)
        patch_mask = ids.repeat_interleave(patch, 0).repeat_interleave(patch, 1)

    out = dict(x=x.numpy(), saliency=sal, step=np.int64(step), max_bs=np.int64(max_bs), seed=np.int64(seed),
               blur_klen=np.int64(blur_k[0]), blur_sig=np.int64(blur_k[1]), **weights_of(model))
    if patch_mask is not None:
        out["patch_mask"] = patch_mask.numpy()

    def run(tag, cls, mode, sub, **kw):
        rec = Recorder(model)
        metric = cls(rec, HW, mode, step, substrate_fn=sub)
        with torch.no_grad():
            res = metric.single_run(x.clone(), sal.copy(), "cpu", patch_mask=patch_mask, max_batch_size=max_bs, **kw)
        for i, r in enumerate(res):
            out[f"{tag}_ret{i}"] = np.asarray(r)
        # batches of step images = every forward call with more than one image, plus 1-image leftovers
        n_pre = {"MAS": 3, "RISE": 2, "AIC": 2, "PNP": 2, "MONO": 2}[tag.split("_")[0]]
        step_batches = rec.seen[n_pre:]
        imgs = torch.cat(step_batches) if step_batches else torch.zeros(0)
        out[f"{tag}_img_sha"] = np.array([_sha(im) for im in imgs])
        out[f"{tag}_img_sum"] = np.array([im.double().sum().item() for im in imgs])
        out[f"{tag}_batch_sizes"] = np.array([b.shape[0] for b in step_batches], dtype=np.int64)
        if keep_images:
            out[f"{tag}_images"] = imgs.numpy()
        return res

    r = run("MAS_ins", MAS.MASMetric, "ins", blur)
    run("MAS_del", MAS.MASMetric, "del", torch.zeros_like)
    run("MAS_lerf", MAS.MASMetric, "lerf", torch.zeros_like)
    run("MAS_morf", MAS.MASMetric, "morf", torch.zeros_like)
    run("RISE_ins", RISE.RISEMetric, "ins", blur)
    run("RISE_del", RISE.RISEMetric, "del", torch.zeros_like)
    run("RISE_lerf", RISE.RISEMetric, "lerf", torch.zeros_like)
    run("AIC_ins", AIC.AICMetric, "ins", blur)
    run("AIC_del", AIC.AICMetric, "del", torch.zeros_like)
    run("PNP_lerf", PNP.PositiveNegativePerturbation, "lerf", torch.zeros_like)
    run("PNP_morf", PNP.PositiveNegativePerturbation, "morf", torch.zeros_like)
    run("MONO_positive", MONO.MonotonicityMetric, "positive", blur)
    run("MONO_negative", MONO.MonotonicityMetric, "negative", torch.zeros_like)
    if patch is None:
        # decision-flip variant of AIC  [AICTestFunctions.py:200-206]
        run("AIC_delflip", AIC.AICMetric, "del", torch.zeros_like, decision_flip=True)
        order = np.flip(np.argsort(sal.reshape(-1, HW), axis=1), axis=-1)
        out["salient_order_desc"] = order.astype(np.int32)
        out["salient_order_asc"] = np.argsort(sal.reshape(-1, HW), axis=1).astype(np.int32)
        if ties:
            stable = np.argsort(sal.reshape(HW), kind="stable")
            out["n_positions_differing_from_the_stable_order"] = np.int64((out["salient_order_asc"][0] != stable).sum())
    out["substrate_blur"] = blur(x).numpy()
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(name, "n_steps+1 =", r[0], "keys:", len(out))


def sweep_fixture():
    """Drive the eight metric objects the way run_perturbation does
    [XAI_Survey/evaluations/evaluatePerturbation.py:448-497] (that file itself cannot be
    imported here: it pulls in clip/captum/torchvision at module import)."""
    from collections import Counter
    hw, seed = 32, 40
    model = tiny_model(seed)
    kern = MAS.gkern(31, 31)
    blur = lambda t: torch.nn.functional.conv2d(t, kern, padding=15)   # noqa: E731
    out = dict(**weights_of(model))
    total = None
    xs, sals = [], []
    for i in range(3):
        x = randn(seed + 10 * i + 1, 1, 3, hw, hw)
        sal = tie_free_map(seed + 10 * i + 2, hw)
        xs.append(x.numpy()); sals.append(sal)
        HW, step, bs, dev = hw * hw, hw, 50, "cpu"
        with torch.no_grad():
            _, MAS_ins, _, _, RISE_ins = MAS.MASMetric(model, HW, 'ins', step, blur).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, MAS_del, _, _, RISE_del = MAS.MASMetric(model, HW, 'del', step, torch.zeros_like).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, AIC_ins = AIC.AICMetric(model, HW, 'ins', step, blur).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, AIC_del = AIC.AICMetric(model, HW, 'del', step, torch.zeros_like).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, LERF = PNP.PositiveNegativePerturbation(model, HW, 'lerf', step, torch.zeros_like).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, MORF = PNP.PositiveNegativePerturbation(model, HW, 'morf', step, torch.zeros_like).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, MONO_pos = MONO.MonotonicityMetric(model, HW, 'positive', step, blur).single_run(x.clone(), sal, dev, max_batch_size=bs)
            _, MONO_neg = MONO.MonotonicityMetric(model, HW, 'negative', step, torch.zeros_like).single_run(x.clone(), sal, dev, max_batch_size=bs)
        c = Counter({"MAS_ins": MAS.auc(MAS_ins), "MAS_del": MAS.auc(MAS_del), "RISE_ins": MAS.auc(RISE_ins),
                     "RISE_del": MAS.auc(RISE_del), "AIC_ins": MAS.auc(AIC_ins), "AIC_del": MAS.auc(AIC_del),
                     "LERF_res": MAS.auc(LERF), "MORF_res": MAS.auc(MORF), "MONO_pos": MONO_pos, "MONO_neg": MONO_neg})
        out[f"counter_{i}"] = np.array([float(c[k]) for k in KEYS])
        total = c if total is None else total + c
    out["x"] = np.concatenate(xs); out["saliency"] = np.stack(sals)
    out["keys"] = np.array(KEYS)
    out["counter_sum"] = np.array([float(total[k]) for k in KEYS])
    np.savez_compressed(os.path.join(HERE, "sweep_small.npz"), **out)
    print("sweep_small.npz", dict(zip(KEYS, out["counter_sum"])))


def _ten_numbers(model, x, sal, hw, blur):
    """One image through the eight metric objects, the statements of run_perturbation [evaluatePerturbation.py:448-497]."""
    from collections import Counter
    HW, step, bs, dev = hw * hw, hw, 50, "cpu"
    z = torch.zeros_like
    with torch.no_grad():
        _, MAS_ins, _, _, RISE_ins = MAS.MASMetric(model, HW, 'ins', step, blur).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, MAS_del, _, _, RISE_del = MAS.MASMetric(model, HW, 'del', step, z).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, AIC_ins = AIC.AICMetric(model, HW, 'ins', step, blur).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, AIC_del = AIC.AICMetric(model, HW, 'del', step, z).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, LERF = PNP.PositiveNegativePerturbation(model, HW, 'lerf', step, z).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, MORF = PNP.PositiveNegativePerturbation(model, HW, 'morf', step, z).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, MONO_pos = MONO.MonotonicityMetric(model, HW, 'positive', step, blur).single_run(x.clone(), sal, dev, max_batch_size=bs)
        _, MONO_neg = MONO.MonotonicityMetric(model, HW, 'negative', step, z).single_run(x.clone(), sal, dev, max_batch_size=bs)
    return Counter({"MAS_ins": MAS.auc(MAS_ins), "MAS_del": MAS.auc(MAS_del), "RISE_ins": MAS.auc(RISE_ins),
                    "RISE_del": MAS.auc(RISE_del), "AIC_ins": MAS.auc(AIC_ins), "AIC_del": MAS.auc(AIC_del),
                    "LERF_res": MAS.auc(LERF), "MORF_res": MAS.auc(MORF), "MONO_pos": MONO_pos, "MONO_neg": MONO_neg})


def counter_fixture():
    """What the reference's image loop does with the per-image Counters [evaluatePerturbation.py:594-596,612-615]: the first
    image's Counter is taken as is, every later one is folded in with `+=` -- collections.Counter.__iadd__, which adds and then
    DELETES every key whose running sum is not > 0 -- and the CSV loop writes the surviving keys in the Counter's own order, so
    a key that was dropped and came back sits at the end and has lost its history.  Five images chosen so that this happens:
    |IG| maps give negative Spearman correlations on this tiny net (images 0, 1, 4), random maps positive ones (2, 3);
    AIC_ins is 0 for four of the five.  Sequence: MONO_pos / MONO_neg / AIC_ins dropped after image 1, MONO_* back after
    image 2, AIC_ins back after image 3.  (evaluatePerturbation.py itself cannot be imported here -- clip / captum /
    torchvision at module import -- so its three statements are driven from this function, on the reference's metric classes
    and the standard library's Counter.)"""
    hw, seed = 32, 40
    model = tiny_model(seed)
    kern = MAS.gkern(31, 31)
    blur = lambda t: torch.nn.functional.conv2d(t, kern, padding=15)   # noqa: E731
    out = dict(**weights_of(model))
    plan = [(0, "absig"), (2, "absig"), (5, "rand"), (1, "rand"), (4, "absig")]
    xs, sals = [], []
    images_used = 0
    for n, (i, kind) in enumerate(plan):
        x = randn(500 + 10 * i + 1, 1, 3, hw, hw)
        if kind == "rand":
            sal = tie_free_map(500 + 10 * i + 2, hw)
        else:
            with torch.no_grad():
                t = model(x).argmax(1)[0]
            sal = np.abs(attr.IG(x.clone(), model, 50, 25, 1, 0, "cpu", t).detach().numpy().sum(0)).astype(np.float32)
            assert len(np.unique(sal)) == sal.size                      # tie-free: the pixel order is the same on every machine
        xs.append(x.numpy()); sals.append(sal)
        c = _ten_numbers(model, x, sal, hw, blur)
        out[f"counter_{n}"] = np.array([float(c[k]) for k in KEYS])
        if images_used == 0:                                            # :593-596
            pert_result_counter = c
        else:
            pert_result_counter += c
        images_used += 1
        out[f"keys_after_{n}"] = np.array(list(pert_result_counter))
        out[f"values_after_{n}"] = np.array([float(pert_result_counter[k]) for k in pert_result_counter])
    rows = [[k, str(pert_result_counter[k] / images_used)] for i, k in enumerate(pert_result_counter)]       # :612-615
    out["x"] = np.concatenate(xs); out["saliency"] = np.stack(sals)
    out["keys"] = np.array(KEYS)
    out["csv_keys"] = np.array([r[0] for r in rows]); out["csv_values"] = np.array([r[1] for r in rows])
    out["images_used"] = np.int64(images_used)
    np.savez_compressed(os.path.join(HERE, "sweep_counter.npz"), **out)
    print("sweep_counter.npz", rows)
    for n in range(len(plan)):
        print("  after image", n, list(out[f"keys_after_{n}"]))


def zoo_fixture():
    """Key names and shapes of the state dicts a `--weights` checkpoint for the reference's classifiers holds: the reference's vendored
    torchvision ResNet definitions (util/modified_models/resnet.py; its `_presets` import needs two inert torchvision.transforms
    names) and its hooked ViT-B/16 (VIT_LRP/ViT_ig.py; the /32 variant lives in ViT_new_timm.py, which needs timm: absent).
    Random initialisation only -- `weights=None` / `pretrained=False`; nothing is fetched."""
    import enum
    tv = types.ModuleType("torchvision"); tvt = types.ModuleType("torchvision.transforms")

    class InterpolationMode(enum.Enum):
        NEAREST = "nearest"; BILINEAR = "bilinear"; BICUBIC = "bicubic"
    tvt.InterpolationMode = InterpolationMode
    tvt.functional = types.SimpleNamespace()
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv); sys.modules.setdefault("torchvision.transforms", tvt)
    from util.modified_models import resnet as ref_resnet
    from util.attribution_methods.VIT_LRP.ViT_ig import vit_base_patch16_224
    out = {}
    makers = {"resnet50": lambda: ref_resnet.resnet50(weights=None), "resnet101": lambda: ref_resnet.resnet101(weights=None),
              "resnet152": lambda: ref_resnet.resnet152(weights=None), "resnext101_64x4d": lambda: ref_resnet.resnext101_64x4d(weights=None),
              "vit_base_patch16_224": lambda: vit_base_patch16_224(pretrained=False)}
    for name, make in makers.items():
        sd = make().state_dict()
        out[name + "_keys"] = np.array(list(sd))
        shapes = np.zeros((len(sd), 4), dtype=np.int64)
        for i, v in enumerate(sd.values()):
            shapes[i, :v.dim()] = list(v.shape)
        out[name + "_shapes"] = shapes
        print(name, len(sd), "entries,", sum(int(v.numel()) for v in sd.values()), "elements")
    np.savez_compressed(os.path.join(HERE, "zoo_state_dicts.npz"), **out)


def vit_fixture():
    """Mini hooked ViT of the reference (ViT_ig.py:161-253; 32x32 image, patch 8, dim 32, depth 2,
    4 heads, 10 classes): pixel-space IG through saliencyMethods.IG and attention-space IG through
    Baselines.IG (ViT_explanation_generator.py:358-386)."""
    from functools import partial
    from util.attribution_methods.VIT_LRP.ViT_ig import VisionTransformer
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import Baselines
    torch.manual_seed(77)
    model = VisionTransformer(img_size=32, patch_size=8, embed_dim=32, depth=2, num_heads=4, num_classes=10, mlp_ratio=4,
                              qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)).eval()
    with torch.no_grad():                       # spread the logits a little (default init is nearly uniform)
        for p in model.parameters():
            p.mul_(3.0)
    x = randn(78, 1, 3, 32, 32)
    with torch.no_grad():
        target = model(x).argmax(1)[0]
    out = dict(x=x.numpy(), target=np.int64(target.item()))
    for k, v in model.state_dict().items():
        out["w_" + k] = v.numpy().copy()
    out["ig"] = attr.IG(x.clone(), model, 50, 25, 1, 0, "cpu", target).detach().numpy()
    b = Baselines(model)
    out["attn_ig"] = b.IG(x.clone(), target, steps=20, device="cpu").detach().numpy()
    out["raw_attn"] = b.generate_raw_attn(x.clone(), "cpu").detach().numpy()
    out["attn_grad"] = b.generate_grad(x.clone(), target, "cpu").detach().numpy()
    out["naive_rollout"] = b.generate_naive_rollout(x.clone())[0].detach().numpy()
    out["rollout"] = b.generate_rollout(x.clone())[0].detach().numpy()
    st, w, fin, last_attn, last_grad = b.generate_transition_attention_maps(x.clone(), target, steps=20, device="cpu")
    out["tam_states"], out["tam_w"], out["tam_final"] = st.detach().numpy(), w.detach().numpy(), fin.detach().numpy()
    out["tam_last_attn"], out["tam_last_grad"] = last_attn.detach().numpy(), last_grad.detach().numpy()
    out["attn_attr"] = b.attn_attr(x.clone(), target, device="cpu").detach().numpy()
    bi, bi_R = b.bidirectional(x.clone(), target, steps=20, start_layer=1, device="cpu")
    out["bi_attr"], out["bi_R"] = bi.detach().numpy(), bi_R.detach().numpy()
    out["bi_mae"] = b.bidirectional(x.clone(), target, steps=20, start_layer=1, mae=True, device="cpu").detach().numpy()
    np.savez(os.path.join(HERE, "vit_mini.npz"), **out)
    print("vit_mini.npz", {k: v.shape for k, v in out.items() if not k.startswith("w_")})


def inflow_fixture():
    """InFlow variants of the attention rollouts (ViT_explanation_generator.py: compute_RAVE :48-88, generate_rollout(InFlow=True)
    :196-240, bidirectional(InFlow=True) :447-464) on the mini ViT of vit_mini.npz.  They read residual-stream accessors
    (`blk.get_input()`, `.get_input_plus_attn()`, `.get_mlp_val()`, `.attn.get_output()`) that only the reference's timm-based twin
    defines (ViT_new_timm.py:223-312; timm is absent here).  The accessors are attached to the reference's ViT_ig blocks with
    torch forward hooks -- norm1's input, attn's output, norm2's input, mlp's output are exactly the tensors the twin saves -- so
    every number below is computed by the reference's own functions, unmodified."""
    from functools import partial
    from util.attribution_methods.VIT_LRP.ViT_ig import VisionTransformer
    from util.attribution_methods.VIT_LRP.ViT_explanation_generator import Baselines
    g = np.load(os.path.join(HERE, "vit_mini.npz"))
    torch.manual_seed(77)
    model = VisionTransformer(img_size=32, patch_size=8, embed_dim=32, depth=2, num_heads=4, num_classes=10, mlp_ratio=4,
                              qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    assert all(np.array_equal(v.numpy(), g["w_" + k]) for k, v in model.state_dict().items())        # the model of vit_mini.npz
    for blk in model.blocks:
        kept = {}
        blk.norm1.register_forward_hook(lambda m, i, o, kept=kept: kept.__setitem__("input", i[0]))
        blk.attn.register_forward_hook(lambda m, i, o, kept=kept: kept.__setitem__("attn_out", o))
        blk.norm2.register_forward_hook(lambda m, i, o, kept=kept: kept.__setitem__("input_plus_attn", i[0]))
        blk.mlp.register_forward_hook(lambda m, i, o, kept=kept: kept.__setitem__("mlp_val", o))
        blk.get_input = lambda kept=kept: kept["input"]
        blk.get_input_plus_attn = lambda kept=kept: kept["input_plus_attn"]
        blk.get_mlp_val = lambda kept=kept: kept["mlp_val"]
        blk.attn.get_output = lambda kept=kept: kept["attn_out"]
    x = torch.from_numpy(g["x"])
    target = torch.tensor(int(g["target"]))
    b = Baselines(model)
    out = {}
    with torch.no_grad():
        roll, mats, layers = b.generate_rollout(x.clone(), InFlow=True)
    out["inflow_rollout"], out["inflow_matrices"], out["inflow_layers"] = roll.detach().numpy(), mats.detach().numpy(), layers.detach().numpy()
    bi, bi_R = b.bidirectional(x.clone(), target, steps=20, start_layer=1, InFlow=True, device="cpu")
    out["inflow_bi_attr"], out["inflow_bi_R"] = bi.detach().numpy(), bi_R.detach().numpy()
    np.savez(os.path.join(HERE, "vit_inflow.npz"), **out)
    print("vit_inflow.npz", {k: v.shape for k, v in out.items()})


def cam_fixture():
    """Grad-CAM arithmetic from the reference-OWNED CAM code (captum itself is absent):
    ViT_CX/get_feature_map.py:17-23 (weights = mean of the gradients over space) and
    ViT_CX/base_cam.py:48-64,129 (weighted channel sum, negatives clamped).  base_cam.py imports cv2 and
    ttach at module level; both are inert stubs here -- the two methods called below are NumPy only."""
    for name in ("cv2", "ttach"):
        sys.modules.setdefault(name, types.ModuleType(name))
    from util.attribution_methods.ViT_CX.get_feature_map import get_feature_map
    from util.attribution_methods.ViT_CX.base_cam import BaseCAM
    rng = np.random.default_rng(90)
    out = {}
    for tag, shape in (("a", (2, 16, 7, 7)), ("b", (1, 256, 7, 7)), ("c", (1, 24, 14, 14))):
        act = rng.standard_normal(shape).astype(np.float32)
        grad = rng.standard_normal(shape).astype(np.float32)
        obj = get_feature_map.__new__(get_feature_map)              # no constructor: it wants a hooked model
        obj.featuremap_and_grads = types.SimpleNamespace(release=lambda: None)   # for BaseCAM.__del__
        w = obj.get_cam_weights(None, None, None, act, grad)
        cam = BaseCAM.get_cam_image(obj, None, None, None, act, grad, eigen_smooth=False)
        clamped = cam.copy()
        clamped[clamped < 0] = 0                                     # base_cam.py:129
        out.update({f"{tag}_act": act, f"{tag}_grad": grad, f"{tag}_weights": w, f"{tag}_cam": cam, f"{tag}_cam_relu": clamped})
    np.savez(os.path.join(HERE, "cam.npz"), **out)
    print("cam.npz", {k: v.shape for k, v in out.items()})


def _inert(*names):
    """Import-time placeholders for third-party modules the reference files import at module level but that the
    functions called here never touch (nothing in them is callable)."""
    for name in names:
        sys.modules.setdefault(name, types.ModuleType(name))
        if "." in name:
            parent, child = name.rsplit(".", 1)
            setattr(sys.modules[parent], child, sys.modules[name])


def vitcx_fixture():
    """ViT-CX pieces that run without torchvision: norm_matrix / get_cos_similar_matrix / reshape_function_vit
    (ViT_CX/ViT_CX.py:22-46) and causal_score.forward (ViT_CX/causal_score.py:17-61) on the CPU with the tiny
    classifier + softmax.  ViT_CX() itself needs torchvision's Resize and is not run.  cv2, ttach, skimage and
    torchvision are inert placeholders (imported at module level there, never called on this path)."""
    _inert("cv2", "ttach", "skimage", "skimage.transform", "torchvision", "torchvision.transforms")
    sys.modules["skimage.transform"].resize = None
    for n in ("Compose", "Normalize", "ToTensor", "Resize"):
        setattr(sys.modules["torchvision.transforms"], n, None)
    from util.attribution_methods.ViT_CX import ViT_CX as VCX
    from util.attribution_methods.ViT_CX.causal_score import causal_score
    out = {}
    tokens = randn(500, 2, 17, 12)
    out["tokens"], out["tokens_reshaped"] = tokens.numpy(), VCX.reshape_function_vit(tokens).contiguous().numpy()
    act = randn(501, 12, 64) * 3 + 1
    out["act"], out["act_norm"] = act.numpy(), VCX.norm_matrix(act).numpy()
    v = VCX.norm_matrix(act)
    v[3] = 0                                                          # a zero row: 0/0 -> NaN -> 0 (:26)
    out["cos_in"], out["cos"] = v.numpy().copy(), VCX.get_cos_similar_matrix(v, v).numpy()
    model = tiny_model(502)
    out.update(weights_of(model))
    soft = nn.Sequential(model, nn.Softmax(dim=1))
    x = randn(503, 1, 3, 32, 32)
    masks = torch.rand(6, 32, 32, generator=torch.Generator().manual_seed(504))
    masks[0, :4] = 0                                                  # some exact zeros / ones like normalised masks have
    masks[1, 5:9] = 1
    class_p = soft(x)[0].detach().numpy()[2]
    torch.manual_seed(505)
    noise = torch.randn([6, 3, 32, 32])                               # the draw causal_score makes first (:27)
    torch.manual_seed(505)
    sal = causal_score(soft, (32, 32), gpu_batch=4, device="cpu")(x, masks, class_p)
    out.update(x=x.numpy(), masks=masks.numpy(), class_p=np.float32(class_p), noise=noise.numpy(), sal=sal.numpy())
    np.savez(os.path.join(HERE, "vit_cx.npz"), **out)
    print("vit_cx.npz", {k: v.shape for k, v in out.items() if not k.startswith("w_")})


def tis_fixture():
    """TIS (util/attribution_methods/TIS.py) on the reference's mini hooked ViT, every stage except the k-means
    (fast_pytorch_kmeans is absent and not even listed in requirements.txt): encoder activations :96-132, binary
    masks :157-190 from given raw masks, token-sampling scores :244-329, saliency :331-365, and the
    input-masking branch :192-242 with the zero baseline.  torchvision.models, timm and fast_pytorch_kmeans are
    inert placeholders (only used in commented-out isinstance checks and in generate_raw_masks)."""
    _inert("torchvision", "torchvision.models", "timm", "timm.models", "timm.models.vision_transformer", "fast_pytorch_kmeans")
    sys.modules["torchvision.models"].VisionTransformer = None
    sys.modules["timm.models.vision_transformer"].VisionTransformer = None
    sys.modules["fast_pytorch_kmeans"].KMeans = None
    from functools import partial
    from util.attribution_methods.TIS import TIS
    from util.attribution_methods.VIT_LRP.ViT_ig import VisionTransformer
    g = np.load(os.path.join(HERE, "vit_mini.npz"))
    model = VisionTransformer(img_size=32, patch_size=8, embed_dim=32, depth=2, num_heads=4, num_classes=10, mlp_ratio=4,
                              qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)).eval()
    model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w_")})
    x = torch.from_numpy(g["x"])
    out = {}
    # (with several ratios the reference can only batch masks of one ratio together: 8 masks, batches of 4)
    for tag, ratio, bs in (("a", 0.5, 3), ("b", [0.25, 0.75], 4)):
        tis = TIS(model, n_masks=8, batch_size=bs, tokens_ratio=ratio, normalise=False)
        with torch.no_grad():
            pred, acts = tis.get_encoder_activations(x)
            raw = randn(600, 8, 16)
            mask_list, idx_list = tis.generate_binary_masks(raw)
            scores = tis.generate_scores(x, int(pred), idx_list)
            sal = tis.generate_saliency(x, scores, mask_list)
            tis.normalise = True
            sal_n = tis.generate_saliency(x, scores, mask_list)
        out.update({f"{tag}_pred": np.int64(pred.item()), f"{tag}_acts": acts.numpy(), f"{tag}_raw": raw.numpy(),
                    f"{tag}_masks": torch.vstack(mask_list).numpy(), f"{tag}_scores": scores.numpy(),
                    f"{tag}_sal": sal.numpy(), f"{tag}_sal_norm": sal_n.numpy()})
        if tag == "a":
            out["a_idx"] = torch.vstack(idx_list).numpy()
            tis.cur_mask_indices = idx_list[:3]
            out["a_masked_zero"] = tis.mask_input(x, baseline="zero").numpy()
    np.savez(os.path.join(HERE, "tis.npz"), **out)
    print("tis.npz", {k: v.shape for k, v in out.items()})


def smoothgrad_fixture():
    """Seeded reference smoothGrad on the tiny net of ig_small.npz [saliencyMethods.py:184-205]: the noise comes from the
    global CPU generator in the reference and in the build alike, so `torch.manual_seed` pins the draw.  vis=True returns
    (mean, total_gradients, noisy_imgs); "IG" is the branch the harness uses (evaluatePerturbation.py:118)."""
    g = np.load(os.path.join(HERE, "ig_small.npz"))
    model = tiny_model(100)
    assert all(np.array_equal(v, g[k]) for k, v in weights_of(model).items())
    x = torch.from_numpy(g["x"])
    target = torch.tensor(int(g["target"]))
    out = {}
    for tag, steps, samples, spread, base in (("a", 10, 3, .15, 0), ("b", 20, 4, .3, 0.1)):
        torch.manual_seed(77)
        mean, total, noisy = attr.smoothGrad("IG", x.clone(), model, steps, base, target, "cpu", sigma_spread=spread, samples=samples, vis=True)
        torch.manual_seed(77)
        only = attr.smoothGrad("IG", x.clone(), model, steps, base, target, "cpu", sigma_spread=spread, samples=samples)
        assert torch.equal(only, mean)
        out.update({f"{tag}_steps": np.int64(steps), f"{tag}_samples": np.int64(samples), f"{tag}_sigma_spread": np.float64(spread),
                    f"{tag}_baseline": np.float64(base), f"{tag}_mean": mean.detach().numpy(), f"{tag}_total_gradients": total.detach().numpy(),
                    f"{tag}_noisy_imgs": noisy.detach().numpy()})
    out["seed"] = np.int64(77)
    np.savez(os.path.join(HERE, "smoothgrad.npz"), **out)
    print("smoothgrad.npz", {k: getattr(v, "shape", v) for k, v in out.items()})


KEYS = ["MAS_ins", "MAS_del", "RISE_ins", "RISE_del", "AIC_ins", "AIC_del", "LERF_res", "MORF_res", "MONO_pos", "MONO_neg"]


if __name__ == "__main__":
    if len(sys.argv) > 1:                                   # python make_golden.py smoothgrad_fixture [...]: only those
        for fn in sys.argv[1:]:
            globals()[fn]()
        raise SystemExit
    ig_fixture("ig_small.npz", 32, 100)
    ig_fixture("ig_224.npz", 224, 200)
    kern_fixture()
    perturb_fixture("perturb_small.npz", 32, 32, 300, 10)          # 32 steps, batches 10,10,10,2
    perturb_fixture("perturb_patch.npz", 32, 32, 310, 50, patch=8)  # 16 patches, batch clamps to n_steps
    perturb_fixture("perturb_224.npz", 224, 224, 320, 50, keep_images=False, blur_k=(31, 31))
    perturb_fixture("perturb_ties.npz", 32, 32, 330, 10, keep_images=False, ties=True)   # tied map: the reference's own (unstable) order recorded
    sweep_fixture()
    counter_fixture()
    zoo_fixture()
    vit_fixture()
    inflow_fixture()
    cam_fixture()
    vitcx_fixture()
    tis_fixture()
    smoothgrad_fixture()
