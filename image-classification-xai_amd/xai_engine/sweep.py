"""Harness counterpart of XAI_Survey/evaluations/evaluatePerturbation.py for the accelerated
methods: attribution dispatch (get_CNN_attr :82-181), the ten perturbation numbers of one image
(run_perturbation :448-497), and the image sweep with its Counter sum / CSV (:499-620), image-
sharded over ranks with one RCCL all-reduce at the end.  The sums are plain sums by default; `reference_counter=True` reproduces
the reference's `Counter +=` fold and CSV loop exactly (keys with a running sum <= 0 vanish, :594-596,:612-615).

`run_perturbation` drives the eight metric objects exactly like the reference.
`PerturbationSweep` computes the same ten numbers from the THREE distinct image sequences the
eight runs contain (insert-blur-descending, delete-zero-descending, delete-zero-ascending;
compare MASTestFunctions.py:137-185, AICTestFunctions.py:94-123, PosNegPertFunctions.py:73-119,
MonotonicityTest.py:93-120): 3 + 3*n_steps classifier passes instead of ~8*(n_steps+3).
"""
import collections
import csv
import os
import time
from collections import Counter

import numpy as np
import torch
from scipy.stats import spearmanr

from . import curves
from . import kernels as K
from .blur import GaussianBlur
from .gradcam import gradcam_saliency
from .guided_ig import guided_ig_batch
from .ig import IG, IDG, abs_channel_sum, getGradientsParallel, hip_device, _logits_of
from .perturb import (AICMetric, MASMetric, MonotonicityMetric, PositiveNegativePerturbation, _Probe, sequence_stats)
from .smooth import smoothGrad
from .streams import LOGIT_RTOL, CapturedCall, ThreadGraphs

KEYS = ("MAS_ins", "MAS_del", "RISE_ins", "RISE_del", "AIC_ins", "AIC_del", "LERF_res", "MORF_res", "MONO_pos", "MONO_neg")
# ("lime" stands in front of "sg": the reference's place for it is between ggc and fa, :168-170, but the tuple's tail and the
# neighbours of "xrai" are pinned by the rows that came before it; "gs", the reference's :164-167 behind ggc, stands behind "lime"
# for the same reason)
CNN_ATTR_FUNCS = ("grad", "inp_x_grad", "ig", "lig", "idg", "gig", "agi", "lime", "gs", "sg", "xrai", "gc", "gbp", "ggc", "fa", "occ")
TRANS_ATTR_FUNCS = ("agi", "lime")   # rows that need the harness's un-normalised [0, 1] image (`trans_img`)
VIT_ATTR_FUNCS = ("attn", "grad", "n_rollout", "rollout", "t_attn", "bi_attn", "attn_ig", "VIT_CX", "TIS", "InFlow")
VIT_TRANS_ATTR_FUNCS = ("MDA",)      # ViT rows that need `trans_img` (and, without skimage, testing_dict["mda_segments"] or "mda_slic": "device")
VIT_LRP_ATTR_FUNCS = ("t_attr",)     # ViT rows of the relevance pass (xai_engine/lrp.py); the segmentation evaluation does not offer them
# the rows of the reference's get_CLIP_attr in its order (:401-437); xai_engine/eclip.py serves METHODS of them and names what the
# others need (REFUSED)
CLIP_ATTR_FUNCS = ("eclip", "eclip_nograd", "eclip_wo", "game", "maskclip", "rollout", "selfattn", "surgery", "m2ib", "lrp")
# the rows of them that xai_engine/clip_attn.py serves on the plain model, when testing_dict["clip_attention_rows"] == "plain" asks for it
CLIP_ATTENTION_ROWS = ("game", "rollout", "lrp")
CLIP_MEAN, CLIP_STD =(0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # generate_emap.py:27


def get_CNN_attr(input_tensor, trans_img, target_class, testing_dict):
    """(H,W) float32 numpy saliency map = |sum over channels| of the attribution
    (reference evaluatePerturbation.py:82-181, the methods on the accelerated path).
    testing_dict["device_maps"] = True (not a reference key): return the same map as a device tensor instead -- no
    device-to-host copy and, above all, no host sync between the attribution and the perturbation sweep of an image, so
    `sweep_images` can keep the GPU queue full (the fused sweep takes device maps as they are)."""
    model = testing_dict["models"][0]
    batch_size = testing_dict["batch_size"]
    img_hw = testing_dict["img_hw"]
    device = testing_dict["device"]
    attr_function = testing_dict["attr_func"]
    steps, baseline = 50, 0
    dev = hip_device(device)
    sal = None                    # a branch leaves either `sal`, the finished (H, W) device map, or `saliency_map`, a (C, H, W) attribution
    if attr_function == "grad":
        x = input_tensor.to(dev).detach().requires_grad_(True)
        saliency_map, _ = getGradientsParallel(x, model, target_class)
    elif attr_function == "inp_x_grad":
        x = input_tensor.to(dev).detach().requires_grad_(True)
        grad, _ = getGradientsParallel(x, model, target_class)
        saliency_map = x.detach().squeeze() * grad
    elif attr_function == "ig":
        saliency_map = IG(input_tensor, model, steps, batch_size, 1, baseline, device, target_class)
    elif attr_function == "lig":
        saliency_map = IG(input_tensor, model, steps, batch_size, .9, baseline, device, target_class)
    elif attr_function == "idg":
        saliency_map = IDG(input_tensor, model, steps, batch_size, baseline, device, target_class)
    elif attr_function == "gig":
        # :114-118: zero baseline, 50 steps, max_dist 1.0, fraction 0.5, the gradient of the softmax probability
        t = target_class.reshape(1) if torch.is_tensor(target_class) else torch.tensor([int(target_class)])
        saliency_map = guided_ig_batch(input_tensor.to(dev), model, t, steps=steps, fraction=0.5, max_dist=1.0, baseline=baseline)[0]
    elif attr_function == "agi":
        # :119-139: epsilon 0.05, topk 1, max_iter 20, selected_ids range(0, 999, 1000) == [0], the reference's Normalize in
        # front of the classifier, the [0, 1] image divided by 255 once more (AGI.py:31), the 80/99 percentile clip
        if trans_img is None:
            raise ValueError("agi: the row needs the harness's un-normalised [0, 1] image (trans_img)")
        from .agi import agi_batch, pre_processing
        from .harness import CNN_MEAN, CNN_STD
        norm = testing_dict.get("normalize", (CNN_MEAN, CNN_STD))
        mean, std = (norm.mean, norm.std) if hasattr(norm, "mean") else norm
        topk = 1
        data = pre_processing(torch.as_tensor(trans_img).permute(1, 2, 0).numpy().astype(np.float32), dev)
        _, init_pred, iters, hm = agi_batch(data, model, list(range(0, 999, int(1000 / topk))), epsilon=0.05, max_iter=20,
                                            normalize=(mean, std), want_map=True)
        if int(iters.max()) == 0:
            # the reference's AGI.test returns (0, 0, 0) and the harness dies in np.mean(0, axis=0) (:133)
            raise ValueError(f"agi: the image predicted as class {int(init_pred[0])} has no attribution: every selected class "
                             "equals its prediction or no attack made an update (the reference crashes here)")
        sal = hm[0]
    elif attr_function == "lime":
        # :168-170 -> limeAttr.py:23-36: the un-normalised [0, 1] image goes to the classifier as it is (no Normalize: the
        # reference's behaviour), quickshift superpixels on the host (skimage; testing_dict["lime_segments"], not a reference key,
        # a callable from the (H, W, C) image to the ids, replaces the segmenter; testing_dict["lime_quickshift"] = "device", not a
        # reference key either, runs the same quickshift on K53-K55 instead of skimage's), 1000 samples, top 5 labels, hide colour 0; the
        # mask of the five most positive superpixels of the top class times ones(3, H, W), |sum over channels| (:181) = K33's 3 / 0
        if trans_img is None:
            raise ValueError("lime: the row needs the harness's un-normalised [0, 1] image (trans_img)")
        from . import lime
        seg_fn = testing_dict.get("lime_segments")
        which = testing_dict.get("lime_quickshift", "skimage")
        if which not in ("skimage", "device"):
            raise ValueError(f"lime: testing_dict['lime_quickshift'] must be 'skimage' or 'device', got {which!r}")
        segmenter = ((lambda im, seed: seg_fn(im)) if seg_fn is not None else
                     lime.device_quickshift_segments if which == "device" else lime.quickshift_segments)
        model.eval()
        sal = lime.lime_batch(torch.as_tensor(trans_img).to(torch.float32)[None].to(dev), model, segmenter, num_samples=1000, top_labels=5,
                              hide_color=0, random_state=testing_dict.get("lime_random_state"))[0]
    elif attr_function == "gs":
        # :164-167: captum's GradientShap(model) with one baseline, torch.randn(1, 3, 224, 224) drawn on the CPU from torch's global
        # generator (here at the harness's img_hw) and then uploaded, so a seeded run draws the reference's baseline; 5 samples,
        # no noise, NumPy's global state for the coefficients; |sum over channels| (:181) straight from K35
        from .gshap import gradient_shap_batch
        baselines = torch.randn(1, 3, img_hw, img_hw)
        sal = gradient_shap_batch(input_tensor.to(dev), model, target_class, baselines.to(dev), n_samples=5, want_attr=False,
                                  want_map=True)[0]
    elif attr_function == "sg":
        saliency_map = smoothGrad("IG", input_tensor, model, 50, baseline, target_class, device)
    elif attr_function == "xrai":
        # :142-146: IG (50 steps, the engine's K1 / K2), max over the channels, Felzenszwalb's six label maps of the image on the
        # host (skimage; testing_dict["xrai_label_maps"], not a reference key, replaces the segmenter), K29 at radius 5, K30;
        # |.| of the one-channel map (:181)
        # testing_dict["xrai_felzenszwalb"] = "device" (not a reference key either) runs the same segmentation on K69-K74 instead of
        # skimage's; an explicit xrai_label_maps wins over it
        from . import xrai
        which = testing_dict.get("xrai_felzenszwalb", "skimage")
        if which not in ("skimage", "device"):
            raise ValueError(f"xrai: testing_dict['xrai_felzenszwalb'] must be 'skimage' or 'device', got {which!r}")
        segmenter = (lambda x_hwc: xrai.device_felzenszwalb_label_maps(x_hwc, device=dev)) if which == "device" else xrai.felzenszwalb_label_maps
        ig = IG(input_tensor, model, steps, batch_size, 1, baseline, device, target_class)
        label_maps = (testing_dict.get("xrai_label_maps") or segmenter)(input_tensor.squeeze().permute(1, 2, 0).cpu())
        sal = xrai.xrai_batch(ig.detach().to(dev)[None], xrai.pack_segments(label_maps, dilation_rad=5, device=dev))[0].abs()
    elif attr_function == "gc":
        # |cam_up + cam_up + cam_up| fused into the up-sample kernel (scale 3, abs); with testing_dict["capture_gradcam"] the
        # launch-bound one-image pass is one replay of the calling thread's hipGraph (gradcam._PASSES)
        sal = gradcam_saliency(model, model.layer4, input_tensor.to(dev), target_class, (img_hw, img_hw),
                               graphs=bool(testing_dict.get("capture_gradcam")))[0]
    elif attr_function in ("gbp", "ggc"):
        # :154-163: captum's GuidedBackprop / GuidedGradCam(model, model.layer4) on models[1] (:84; the reference's copy without
        # in-place ReLUs -- a fused classifier needs none), then |sum over channels| (:181) straight from K28
        from .guided import guided_backprop_batch
        models = testing_dict["models"]
        guided_model = models[1] if len(models) > 1 else models[0]
        sal = guided_backprop_batch(input_tensor.to(dev), guided_model, target_class,
                                    layer=guided_model.layer4 if attr_function == "ggc" else None, want_attr=False, want_map=True)[0]
    elif attr_function in ("fa", "occ"):
        # :171-176: captum's FeatureAblation over the 14 x 14 patch mask (:94-97) / Occlusion with window (3, 64, 64), stride 32;
        # resize(downsize(.)) and |sum over channels| (:92-95, :181) come from K27's 14 x 14 samples and the up-sample kernel
        from . import ablation
        x = input_tensor.to(dev)
        if attr_function == "fa":
            # the id plane is uploaded once per stream: its upload and its readers must be ordered on one stream
            key = (img_hw, tuple(x.shape), str(dev), torch.cuda.current_stream(dev).cuda_stream)
            cache = testing_dict.setdefault("_fa_masks", {})
            if key not in cache:
                cache[key] = ablation.prepare_mask(ablation.harness_patch_mask(img_hw), x.shape, dev)
            sal = ablation.feature_ablation_batch(x, model, target_class, cache[key], want_map=ablation.NUM_PATCHES, attribution=False)[0]
        else:
            sal = ablation.occlusion_batch(x, model, target_class, ablation.OCC_WINDOW, ablation.OCC_STRIDE,
                                           want_map=ablation.NUM_PATCHES, attribution=False)[0]
    else:
        print("Model-attribution mismatch, please use --help.")
        raise SystemExit
    device_maps = testing_dict.get("device_maps")
    if sal is None and not device_maps:
        return np.abs(np.sum(saliency_map.detach().cpu().numpy(), axis=0))       # the reference's expression, on the host
    if sal is None:               # (a + b) + c per pixel: bit-identical to the host expression
        m = saliency_map.detach()
        sal = abs_channel_sum(m) if m.shape[0] == 3 else m.sum(0).abs()
    return sal if device_maps else sal.cpu().numpy()


def vit_patch_map(input_tensor, target_class, testing_dict):
    """The (1, p, p) patch-grid map of the attention-space rows of get_VIT_attr, on the device and before any resize; None for a
    row that has no patch grid (VIT_CX, MDA) or that the table does not know.  Shared with segeval, whose resize takes no abs."""
    from .vit_attr import Baselines
    model = testing_dict["models"][0]
    attr_function = testing_dict["attr_func"]
    dev = hip_device(testing_dict["device"])
    explainer = Baselines(model)
    x = input_tensor.to(dev)
    if attr_function == "attn":
        sal = explainer.generate_raw_attn(x, dev)
    elif attr_function == "grad":
        sal = explainer.generate_grad(x, target_class, dev)
    elif attr_function == "n_rollout":
        sal, _, _ = explainer.generate_naive_rollout(x)
    elif attr_function == "rollout":
        sal, _, _ = explainer.generate_rollout(x)
    elif attr_function == "t_attn":
        _, _, sal, _, _ = explainer.generate_transition_attention_maps(x, target_class, start_layer=0, device=dev)
    elif attr_function == "bi_attn":
        sal, _ = explainer.bidirectional(x, target_class, device=dev)
    elif attr_function == "attn_ig":
        sal = explainer.IG(x, target_class, device=dev)
    elif attr_function == "TIS":
        from .tis import TIS
        # :236-239 (n_masks is the class default, 1024, in the reference; the key exists for models with fewer channels).
        # testing_dict["tis_kmeans"] = "device" (not a reference key) runs the k-means on K58-K61 instead of the torch loop; TIS
        # refuses any other value.
        sal = TIS(model, n_masks=testing_dict.get("tis_n_masks", 1024), batch_size=64,
                  kmeans=testing_dict.get("tis_kmeans", "torch"))(x, class_idx=target_class)[None]
    elif attr_function == "InFlow":
        # :240-242 passes option='b', which generate_RAVE does not take (a TypeError in the reference too): dropped here
        sal, _ = explainer.generate_RAVE(x, target_class, device=dev)
    elif attr_function == "t_attr":
        # :228-230: LRP(models[1]).generate_LRP(x, target, method="transformer_attribution", start_layer=0); the reference's
        # models[1] is its relprop twin of models[0] with the same weights, here the pass runs on models[0] itself
        from .lrp import LRP
        sal = LRP(model, graphs=True).generate_LRP(x, target_class, method="transformer_attribution", start_layer=0, device=dev)
    else:
        return None
    return sal.detach().float().contiguous()


def get_VIT_attr(input_tensor, trans_img, target_class, testing_dict):
    """(H,W) float32 numpy saliency map of a hooked ViT for the attention-space methods on the accelerated
    path (reference evaluatePerturbation.py:192-370): patch map (1,p,p) -> bilinear up-sample to the image
    (torchvision Resize(antialias=True) == plain bilinear when up-sampling) -> abs, the last two fused in
    xai_bilinear_up_f32.  "attn_ig" (Baselines.IG) is commented out in the reference's table (:276-278) and
    offered here because it is the config-4 method."""
    from .vit_attr import Baselines
    model = testing_dict["models"][0]
    img_hw = testing_dict["img_hw"]
    device = testing_dict["device"]
    attr_function = testing_dict["attr_func"]
    dev = hip_device(device)
    sal = vit_patch_map(input_tensor, target_class, testing_dict)
    if sal is not None:
        # sal is the (1, p, p) patch grid of an img_hw-pixel input, p = img_hw / patch size: no axis shrinks, plain bilinear is the reference's resize
        return K.bilinear_up(sal, img_hw, img_hw, scale=1.0, take_abs=True)[0].cpu().numpy()
    explainer = Baselines(model)
    x = input_tensor.to(dev)
    if attr_function == "VIT_CX":
        # :231-235: ViT-CX map of the top-1 class (the reference does not pass target_class), min-max normalised, times
        # ones(H,W,3), then |sum over the 3 copies| = 3 * normalised map.  The reference passes gpu_batch=1; the batch only
        # groups the 2N masked forwards, 50 is ViT_CX's own default.  testing_dict["vit_cx_clustering"] = "device" (not a reference
        # key) runs the complete-linkage clustering on K56 / K57 instead of scikit-learn's host call: the same labels.
        from .vit_cx import ViT_CX
        result, _ = ViT_CX(model, x, model.blocks[-1].norm1, device=device, gpu_batch=testing_dict.get("vit_cx_batch", 50),
                           return_feature_map=False, clustering=testing_dict.get("vit_cx_clustering", "sklearn"))
        result = result.reshape(img_hw, img_hw)
        result = (result - result.min()) / (result.max() - result.min())
        return (result * 3.0).abs().numpy()
    elif attr_function == "MDA":
        # :243-263: the growing-kernel blur search, Baselines.bidirectional resized to the image and times ones(3), MDA with
        # num_patches ** 2 segments and max_batch_size 5, the map of its first return value (:181 |sum over channels|).
        # testing_dict["mda_segments"] (not a reference key): the (img_hw, img_hw) label map to use instead of skimage's SLIC;
        # testing_dict["mda_slic"] = "device" (not a reference key either) runs the same SLIC on K65-K68 instead of skimage's
        from .blur import blur_until_unconfident
        from .mda import MDA
        which = testing_dict.get("mda_slic", "skimage")
        if which not in ("skimage", "device"):
            raise ValueError(f"MDA: testing_dict['mda_slic'] must be 'skimage' or 'device', got {which!r}")
        if trans_img is None and testing_dict.get("mda_segments") is None:
            raise ValueError("MDA: the row needs the harness's un-normalised [0, 1] image (trans_img) for SLIC, or mda_segments")
        blur, _, _, _ = blur_until_unconfident(model, input_tensor, target_class, dev)
        bi_attn, _ = explainer.bidirectional(x, target_class, device=dev)
        bi_attn = K.resize_bilinear(bi_attn.detach().float().contiguous(), img_hw, img_hw)[0].cpu().numpy()[:, :, None] * np.ones((img_hw, img_hw, 3))
        mda, _, _ = MDA(trans_img, input_tensor.cpu(), bi_attn, testing_dict["num_patches"] ** 2, blur, model, device, img_hw, max_batch_size=5,
                        segments=testing_dict.get("mda_segments") if testing_dict.get("mda_segments") is not None else which)
        return np.abs(np.sum(mda, axis=2)).astype(np.float32)
    else:
        print("Model-attribution mismatch, please use --help.")
        raise SystemExit


def clip_keepsize_input(trans_img, patch=(16, 16)):
    """The reference's `imgprocess_keepsize(to_pil_image(trans_img))` (evaluatePerturbation.py:394-395, generate_emap.py:29-37) for a
    (3, H, W) image in [0, 1] whose H and W are multiples of `patch` (its default 16 x 16, whatever the model's patch is): the
    bicubic resize to the nearest multiples is then the identity, and what is left is the 8-bit round trip (to_pil_image:
    `mul(255).byte()`, which truncates; ToTensor: `/ 255`) and CLIP's Normalize.  -> (1, 3, H, W) fp32.  Any other size needs PIL's
    bicubic resize: NotImplementedError."""
    if trans_img.dim() != 3 or trans_img.shape[0] != 3:
        raise ValueError(f"trans_img must be (3, H, W), got {tuple(trans_img.shape)}")
    H, W = trans_img.shape[1:]
    if H % patch[0] or W % patch[1]:
        raise NotImplementedError(f"clip_keepsize_input: a {H} x {W} image is not a multiple of {patch[0]} x {patch[1]}; the reference "
                                  "resizes it with PIL's bicubic filter, which is not restated here")
    x = trans_img.detach().to("cpu", torch.float32).mul(255).byte().to(torch.float32).div(255)
    mean, std = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (CLIP_MEAN, CLIP_STD))
    return x.sub(mean).div(std).unsqueeze(0)


def _class_text(testing_dict, target_class):
    """The (1, E) row of testing_dict["embeddings"] for the class, not normalised yet: the reference re-encodes "a photo of a <class>",
    the very text that row was made from, so no tokeniser is needed"""
    emb = testing_dict["embeddings"]
    return emb.reshape(-1, emb.shape[-1])[int(target_class)][None]


def _plain_attention_rows(td, clipmodel, target_class):
    from . import clip_attn
    txt = torch.nn.functional.normalize(_class_text(td, target_class), dim=-1)
    return lambda x: clip_attn.attention_rows_batch(clipmodel, x, txt, td["attr_func"], img_hw=td["img_hw"])


def _plain_surgery(td, clipmodel, target_class):
    from . import surgery
    context = td.get("surgery_text_features")
    if context is None:
        raise ValueError("get_CLIP_attr: clip_surgery='plain' needs testing_dict['surgery_text_features'], the (T - 1, E) text "
                         "features of the context classes (59 prompt-ensembled class names in the reference's harness)")
    row = _class_text(td, target_class)
    if not isinstance(context, torch.Tensor) or context.dim() != 2 or context.shape[1] != row.shape[1]:
        raise ValueError(f"get_CLIP_attr: surgery_text_features must be a (T - 1, {row.shape[1]}) tensor")
    txt = torch.nn.functional.normalize(torch.cat([row.float(), context.to(row.device).float()]), dim=-1)
    return lambda x: surgery.surgery_batch(clipmodel, x, txt, img_hw=td["img_hw"])


def _plain_m2ib(td, clipmodel, target_class):
    from . import m2ib
    table = td.get("m2ib_text_features")
    if table is None:
        raise ValueError("get_CLIP_attr: clip_m2ib='plain' needs testing_dict['m2ib_text_features'], the (n_classes, E) table of "
                         "the M2IB wrapper's text features (m2ib.wrapper_text_features of each class's token ids; they are not "
                         "encode_text's, so `embeddings` does not serve)")
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != clipmodel.visual.proj.shape[1]:
        raise ValueError(f"get_CLIP_attr: m2ib_text_features must be a (n_classes, {clipmodel.visual.proj.shape[1]}) tensor")
    return lambda x: m2ib.m2ib_batch(clipmodel, x, table[int(target_class)], img_hw=td["img_hw"],
                                     noise=td.get("m2ib_noise", "device"), seed=td.get("m2ib_seed"))


# (the key of testing_dict that asks for it, the rows the key governs, what builds the row's text operand and returns the call):
# the rows the reference runs on further model objects and this engine serves on models[0], in closed form, on request
CLIP_PLAIN_ROWS = (("clip_attention_rows", CLIP_ATTENTION_ROWS, _plain_attention_rows),
                   ("clip_surgery", ("surgery",), _plain_surgery),
                   ("clip_m2ib", ("m2ib",), _plain_m2ib))


def get_CLIP_attr(trans_img, target_class, testing_dict):
    """(H,W) float32 numpy saliency map of a row of the reference's get_CLIP_attr (evaluatePerturbation.py:373-445); with
    testing_dict["device_maps"] the map stays a device tensor.  eclip, eclip_wo, eclip_nograd, maskclip and selfattn
    (xai_engine/eclip.py) are served on testing_dict["models"][0] with the text normalize(testing_dict["embeddings"][target_class]).
    game, rollout, lrp, surgery and m2ib run on further model objects in the reference: NotImplementedError naming the model,
    unless the key of CLIP_PLAIN_ROWS that governs the row is "plain"; then the row is served on models[0] in closed form
    (xai_engine/clip_attn.py, surgery.py, m2ib.py say why that is the same map), for an input_resolution-square image.  A key's
    other values are None and "modified" (the default); anything else: ValueError.  surgery also needs
    testing_dict["surgery_text_features"], the (T - 1, E) features of its context classes (the reference also prompt-ensembles the caption
    over its 85 templates: a caller who wants that passes an `embeddings` table made that way), and m2ib
    testing_dict["m2ib_text_features"], the (n_classes, E) table of m2ib.wrapper_text_features, with the optional "m2ib_noise" and
    "m2ib_seed" of m2ib_batch."""
    from . import eclip
    attr_function = testing_dict["attr_func"]

    def result(maps):
        return maps[0] if testing_dict.get("device_maps") else maps[0].cpu().numpy()
    for key, rows, serve in CLIP_PLAIN_ROWS:
        asked = testing_dict.get(key)
        if asked not in (None, "modified", "plain"):
            raise ValueError(f"get_CLIP_attr: {key} must be 'plain' or 'modified' (the default), got {asked!r}")
        if asked == "plain" and attr_function in rows:
            clipmodel = testing_dict["models"][0]
            call = serve(testing_dict, clipmodel, target_class)
            res = int(clipmodel.visual.input_resolution)
            if tuple(trans_img.shape[1:]) != (res, res):
                raise NotImplementedError(f"get_CLIP_attr: the row {attr_function!r} takes the reference's preprocess(img); a "
                                          f"{trans_img.shape[1]} x {trans_img.shape[2]} image is not the model's {res} x {res}, and PIL's "
                                          "bicubic resize is not restated here")
            return result(call(clip_keepsize_input(trans_img, (1, 1))))
    if attr_function in eclip.REFUSED:
        raise NotImplementedError(f"get_CLIP_attr: the row {attr_function!r} needs {eclip.REFUSED[attr_function]}, which this engine "
                                  "does not build")
    if attr_function not in eclip.METHODS:
        print("Model-attribution mismatch, please use --help.")
        raise SystemExit
    clipmodel = testing_dict["models"][0]
    txt = torch.nn.functional.normalize(_class_text(testing_dict, target_class), dim=-1)
    ksize = clipmodel.visual.conv1.kernel_size
    if trans_img.shape[1] % ksize[0] or trans_img.shape[2] % ksize[1]:
        raise NotImplementedError(f"get_CLIP_attr: a {trans_img.shape[1]} x {trans_img.shape[2]} image is not a multiple of the model's "
                                  f"patch size {tuple(ksize)}")
    return result(eclip.eclip_batch(clipmodel, clip_keepsize_input(trans_img), txt, attr_function, img_hw=testing_dict["img_hw"]))


def run_perturbation(input_tensor, attribution, testing_dict, CLIP_test_info=None, blur=None):
    """Eight single_run calls, ten numbers -- call for call the reference's run_perturbation
    (evaluatePerturbation.py:448-497); the blur substrate runs on the device."""
    img_hw = testing_dict["img_hw"]
    step_size = img_hw
    model = testing_dict["models"][0]
    batch_size = testing_dict["batch_size"]
    device = testing_dict["device"]
    HW = img_hw * img_hw
    blur = blur if blur is not None else GaussianBlur(31, 31, device)
    z = torch.zeros_like
    kw = dict(max_batch_size=batch_size, CLIP_test_info=CLIP_test_info)
    _, MAS_ins, _, _, RISE_ins = MASMetric(model, HW, 'ins', step_size, blur).single_run(input_tensor, attribution, device, **kw)
    _, MAS_del, _, _, RISE_del = MASMetric(model, HW, 'del', step_size, z).single_run(input_tensor, attribution, device, **kw)
    _, AIC_ins = AICMetric(model, HW, 'ins', step_size, blur).single_run(input_tensor, attribution, device, **kw)
    _, AIC_del = AICMetric(model, HW, 'del', step_size, z).single_run(input_tensor, attribution, device, **kw)
    _, LERF_res = PositiveNegativePerturbation(model, HW, 'lerf', step_size, z).single_run(input_tensor, attribution, device, **kw)
    _, MORF_res = PositiveNegativePerturbation(model, HW, 'morf', step_size, z).single_run(input_tensor, attribution, device, **kw)
    _, MONO_pos = MonotonicityMetric(model, HW, 'positive', step_size, blur).single_run(input_tensor, attribution, device, **kw)
    _, MONO_neg = MonotonicityMetric(model, HW, 'negative', step_size, z).single_run(input_tensor, attribution, device, **kw)
    auc = curves.auc
    return Counter({"MAS_ins": auc(MAS_ins), "MAS_del": auc(MAS_del), "RISE_ins": auc(RISE_ins), "RISE_del": auc(RISE_del),
                    "AIC_ins": auc(AIC_ins), "AIC_del": auc(AIC_del), "LERF_res": auc(LERF_res), "MORF_res": auc(MORF_res),
                    "MONO_pos": MONO_pos, "MONO_neg": MONO_neg})


FORWARD_COUNTS = {"replayed": 0, "eager": 0, "captures": 0, "captures_refused": 0}
_FORWARDS = ThreadGraphs(limit=6)


class _CapturedForward(CapturedCall):
    """The classifier's forward pass for a batch of b step images on a static input buffer `x` (K6 writes the step images into it),
    replayed as ONE hipGraph by the stream worker that captured it (streams.CapturedCall; with one host thread per stream the ~250
    launches of every forward batch are otherwise enqueued under one interpreter lock)."""

    def __init__(self, model, b, img_shape, dev):
        super().__init__(FORWARD_COUNTS, (LOGIT_RTOL,))
        self.model = model
        self.x = torch.zeros((b,) + tuple(img_shape), dtype=torch.float32, device=dev)

    def step(self):
        with torch.no_grad():
            return (_logits_of(self.model(self.x)),)


class PerturbationSweep:
    """The same ten numbers from three device-resident sequences (see module docstring)."""

    def __init__(self, model, img_hw, device, step_size=None, batch_size=50, klen=31, ksig=31):
        self.model = model
        self.dev = hip_device(device)
        self.img_hw = img_hw
        self.HW = img_hw * img_hw
        self.step_size = step_size or img_hw
        self.batch_size = batch_size
        self.blur = GaussianBlur(klen, ksig, self.dev)

    def _stats(self, images, target, out=None, offset=0):
        with torch.no_grad():
            return _Probe(_logits_of(self.model(images)).detach(), target, out, offset)

    def _captured(self, b, img_shape):
        """this thread's graph of a b-image forward, or None once its capture has been refused"""
        cf = _FORWARDS.get(self.model, self.dev, (b, tuple(img_shape)), lambda: _CapturedForward(self.model, b, img_shape, self.dev))
        return None if cf.refused else cf

    def launch(self, input_tensor, attribution, graphs=False):
        """Queue the whole device part of one image (probes, ranking, three sequences) and an asynchronous
        copy of the curves into pinned host memory; returns a handle for `finish`.  Nothing here waits for the
        GPU, so the next image can be queued (or the previous one finished) while this one runs.
        `attribution`: (H,W) float32 NumPy array or device tensor (a device tensor avoids the upload).
        `graphs` (stream workers only, sweep_images): replay the forward passes of the step batches from this thread's hipGraphs."""
        dev = self.dev
        n_steps, step, batches = curves.step_plan(self.HW, self.step_size, self.batch_size)
        if input_tensor.is_cuda:
            img = input_tensor.to(dev, torch.float32).contiguous()
        else:
            img = input_tensor.to(torch.float32).contiguous().pin_memory().to(dev, non_blocking=True)
        blurred = self.blur(img)
        zeros = torch.zeros_like(img)
        orig = self._stats(img, None)
        target = orig.argmax
        pb = self._stats(blurred, target)
        pz = self._stats(zeros, target)
        if torch.is_tensor(attribution) and attribution.is_cuda:
            sal = attribution.to(dev, torch.float32).reshape(1, self.HW).contiguous()
        else:
            host_sal = torch.as_tensor(np.ascontiguousarray(attribution, dtype=np.float32)).reshape(1, self.HW)
            sal = host_sal.pin_memory().to(dev, non_blocking=True)
        order, rk = K.rank(sal)
        f_desc = K.flip_steps(rk[0], True, step)
        f_asc = K.flip_steps(rk[0], False, step)
        seg_d, total = K.segment_sums(sal[0], order[0], True, step, n_steps)
        img_shape = tuple(img.shape[1:])

        def slot_for(b):
            cf = self._captured(b, img_shape) if graphs else None
            return None if cf is None else cf.x

        def stats(images, tgt, out=None, offset=0):
            cf = self._captured(images.shape[0], img_shape) if graphs else None
            if cf is None or images.data_ptr() != cf.x.data_ptr():
                FORWARD_COUNTS["eager"] += 1
                return self._stats(images, tgt, out, offset)
            return _Probe(cf.run()[0], tgt, out, offset)      # the step images are in cf.x already (K6 wrote them there)

        ins = sequence_stats(stats, blurred[0], img[0], f_desc, n_steps, batches, target, pb, slot_for)
        dele = sequence_stats(stats, img[0], zeros[0], f_desc, n_steps, batches, target, orig, slot_for)
        lerf = sequence_stats(stats, img[0], zeros[0], f_asc, n_steps, batches, target, orig, slot_for)
        packed = torch.cat([ins[0], ins[2].float(), dele[0], dele[2].float(), lerf[0], seg_d, total,
                            orig.p, pb.p, pz.p, pb.argmax.float(), pz.argmax.float(), target.float()])
        host = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        return (n_steps, host, done, packed)          # `packed` is kept alive until the copy has happened

    def finish(self, handle, return_curves=False):
        """Wait for `launch`'s copy and do the 225-point curve arithmetic on the host."""
        n_steps, host_t, done, _ = handle
        done.synchronize()
        host = host_t.numpy().astype(np.float64)
        n1 = n_steps + 1
        r_ins, a_ins, r_del, a_del, r_lerf = (host[i * n1:(i + 1) * n1] for i in range(5))
        seg = host[5 * n1:5 * n1 + n_steps].astype(np.float32)
        tot = np.float32(host[5 * n1 + n_steps])
        o_p, b_p, z_p, b_cls, z_cls, tgt = host[5 * n1 + n_steps + 1:]

        norm_ins = curves.monotone_normalise(r_ins, b_p, o_p, falling=False)
        norm_del = curves.monotone_normalise(r_del, z_p, o_p, falling=True)
        mas_ins = curves.mas_correct(norm_ins, curves.density_curve(seg, tot, True), 'ins')
        mas_del = curves.mas_correct(norm_del, curves.density_curve(seg, tot, False), 'del')
        aic_i = (a_ins == tgt).astype(np.float64)
        aic_d = (a_del == tgt).astype(np.float64)
        aic_i[0], aic_d[0] = float(b_cls == tgt), 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            aic_ins = curves.monotone_normalise(aic_i, float(b_cls == tgt), 1, falling=False)
            aic_del = curves.monotone_normalise(aic_d, float(z_cls == tgt), 1, falling=True)
        auc = curves.auc
        out = Counter({"MAS_ins": auc(mas_ins), "MAS_del": auc(mas_del), "RISE_ins": auc(norm_ins), "RISE_del": auc(norm_del),
                       "AIC_ins": auc(aic_ins), "AIC_del": auc(aic_del), "LERF_res": auc(r_lerf), "MORF_res": auc(r_del),
                       "MONO_pos": spearmanr(np.linspace(0, 1, n1), r_ins).correlation,
                       "MONO_neg": spearmanr(np.linspace(1, 0, n1), r_del).correlation})
        if return_curves:
            return out, dict(ins=r_ins, dele=r_del, lerf=r_lerf, mas_ins=mas_ins, mas_del=mas_del)
        return out

    def run(self, input_tensor, attribution, return_curves=False):
        return self.finish(self.launch(input_tensor, attribution), return_curves)


# ------------------------------------------------------------------------------ image sweep, sharded over ranks
def shard_indices(n_items, rank, world):
    """Round-robin ownership: item i belongs to rank i % world (deterministic, order-preserving)."""
    return list(range(rank, n_items, world))


def reduce_counters(local_sum, n_local, device=None, group=None, world=None, attr_seconds=None):
    """One all-reduce(SUM) of [10 metric sums, images used, seconds in attribution] in fp64 (96 bytes) -> global Counter, count
    (and the summed seconds when `attr_seconds` is given).  `world=1` (a caller that did not shard) skips the collective even
    inside an initialised job."""
    import torch.distributed as dist
    vec = torch.tensor([float(local_sum.get(k, 0.0)) for k in KEYS] + [float(n_local), float(attr_seconds or 0.0)], dtype=torch.float64)
    if world != 1 and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == "nccl":
            vec = vec.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
        vec = vec.cpu()
    out = (Counter({k: float(vec[i]) for i, k in enumerate(KEYS)}), int(round(float(vec[len(KEYS)]))))
    return out if attr_seconds is None else out + (float(vec[len(KEYS) + 1]),)


def replay_reference_counter(rows):
    """The reference's running Counter over per-image results in FILE ORDER (evaluatePerturbation.py:593-596): the first image's
    Counter is taken as it is, every later one is folded in with `+=` -- collections.Counter.__iadd__ adds and then deletes every
    key whose running sum is not > 0 (a zero AIC sum, a negative Spearman sum, a NaN), and a deleted key that comes back starts from
    nothing and sits at the end.  rows: iterable of 10-vectors in KEYS order.  Uses the standard library's Counter itself, so the
    semantics are the reference's by construction (pinned by tests/golden/sweep_counter.npz)."""
    total = None
    for r in rows:
        c = Counter({k: float(v) for k, v in zip(KEYS, r)})
        if total is None:
            total = c
        else:
            total += c
    return total if total is not None else Counter()


def gather_rows(local_rows, n_items, device=None, group=None, world=None, attr_seconds=0.0):
    """All ranks' per-image 10-vectors as one (n_items, 10) fp64 matrix plus a used-flag column, by ONE all-reduce(SUM) of the
    zero-padded (n_items + 1, 11) matrix (every image is owned by exactly one rank, so the rows are disjoint; 88 B x images --
    88 KB for the 1000-image sweep; the extra row carries the seconds in attribution).  local_rows: {global index: 10-vector}.
    -> (rows (n_items, 10) float64, used (n_items,) bool, summed attribution seconds)."""
    import torch.distributed as dist
    mat = torch.zeros((n_items + 1, len(KEYS) + 1), dtype=torch.float64)
    for i, r in local_rows.items():
        mat[int(i), :len(KEYS)] = torch.as_tensor(np.asarray(r, dtype=np.float64))
        mat[int(i), len(KEYS)] = 1.0
    mat[n_items, 0] = float(attr_seconds)
    if world != 1 and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == "nccl":
            mat = mat.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(mat, op=dist.ReduceOp.SUM, group=group)
        mat = mat.cpu()
    m = mat.numpy()
    return m[:n_items, :len(KEYS)].copy(), m[:n_items, len(KEYS)] > 0.5, float(m[n_items, 0])


def sweep_identity(**facts):
    """Stable string describing WHAT a checkpointed sweep computes (attribution method, model, weights, flow, image
    list ...): the facts as sorted `key=value` pairs, long values hashed.  A checkpoint resumes only under the same string."""
    import hashlib

    def short(v):
        v = str(v)
        return v if len(v) <= 40 else "sha256:" + hashlib.sha256(v.encode()).hexdigest()[:24]
    return ";".join(f"{k}={short(facts[k])}" for k in sorted(facts))


def model_fingerprint(model, max_tensors=8):
    """Cheap fingerprint of a classifier's weights: class name, parameter count and the sums of its first and last
    few tensors (enough to tell two checkpoints of one architecture apart without hashing 100 MB)."""
    tensors = list(model.state_dict().items())
    picked = tensors[:max_tensors // 2] + tensors[-(max_tensors // 2):]
    parts = [type(model).__name__, str(sum(int(t.numel()) for _, t in tensors))]
    parts += [f"{k}:{float(t.double().sum()):.10e}" for k, t in picked]
    return "|".join(parts)


class CheckpointMismatch(RuntimeError):
    pass


class SweepState:
    """Per-rank running sums of a sharded sweep, checkpointed so that a crash does not lose the run (the
    reference writes its CSV once at the very end, evaluatePerturbation.py:612).  One small JSON file per
    rank, replaced atomically.  It is only valid for the same (n_items, rank, world) split AND the same
    `identity` (see sweep_identity): resuming somebody else's sums into this run's CSV is refused loudly."""

    def __init__(self, n_items, rank, world, identity=""):
        self.n_items, self.rank, self.world, self.identity = n_items, rank, world, identity
        self.sums = {k: 0.0 for k in KEYS}
        self.used = 0            # images folded into `sums`
        self.next_pos = 0        # position in this rank's shard list
        self.attr_time = 0.0
        self.rows = {}           # reference_counter mode: {global image index: that image's ten numbers}

    @staticmethod
    def path_for(prefix, rank, world):
        return f"{prefix}.rank{rank}of{world}.json"

    def save(self, prefix):
        import json
        path = self.path_for(prefix, self.rank, self.world)
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(dict(n_items=self.n_items, rank=self.rank, world=self.world, identity=self.identity, sums=self.sums,
                           used=self.used, next_pos=self.next_pos, attr_time=self.attr_time,
                           rows={str(i): [float(v) for v in r] for i, r in self.rows.items()}), f)
        os.replace(tmp, path)

    @classmethod
    def load_or_new(cls, prefix, n_items, rank, world, identity=""):
        import json
        st = cls(n_items, rank, world, identity)
        path = cls.path_for(prefix, rank, world) if prefix else None
        if path and os.path.exists(path):
            d = json.load(open(path))
            split = (d.get("n_items"), d.get("rank"), d.get("world"))
            if split != (n_items, rank, world) or d.get("identity", "") != identity or set(d.get("sums", {})) != set(KEYS):
                raise CheckpointMismatch(
                    f"{path} belongs to a different sweep and is not resumed: it holds (n_items, rank, world) = {split}, "
                    f"identity '{d.get('identity', '')}'; this run is {(n_items, rank, world)}, identity '{identity}'. "
                    "Use another --checkpoint prefix or delete the file.")
            st.sums = {k: float(d["sums"][k]) for k in KEYS}
            st.used, st.next_pos, st.attr_time = int(d["used"]), int(d["next_pos"]), float(d["attr_time"])
            st.rows = {int(i): [float(v) for v in r] for i, r in d.get("rows", {}).items()}
        return st


def sweep_images(images, model, device, attr_fn, img_hw=224, batch_size=50, fused=True, rank=0, world=1, testing_dict=None,
                 checkpoint=None, checkpoint_every=25, identity=None, streams=1, reference_counter=False, kind=None, graphs=True,
                 extra=False):
    """Attribution + ten perturbation numbers for every image this rank owns; returns the
    globally reduced (Counter of sums, images used, seconds in attribution).
    images: sequence of (1,C,H,W) CPU/device tensors (already selected -- the order-dependent
    filters of evaluatePerturbation.py:520-576 must run as a deterministic pre-pass so that the
    1-GPU and N-GPU runs see the same list).  attr_fn(x, target) -> (H,W) float32 numpy map.
    `checkpoint`: path prefix; every `checkpoint_every` images the rank's running sums are saved and an
    interrupted sweep with the same split and the same `identity` resumes after the last saved image; a checkpoint
    of another split or identity raises CheckpointMismatch.  `identity`: string from `sweep_identity(...)` naming
    what the caller's attr_fn / image list are (the harness passes attr_func, model name, file-name hash, ...); the
    flow (fused / eight runs), geometry and a fingerprint of the classifier's weights are always added here.
    `reference_counter`: fold the per-image results the way the reference does (`replay_reference_counter`: Counter `+=` in file
    order, keys with a running sum <= 0 dropped) instead of plain sums.  The fold is order-dependent, so every rank keeps its
    images' ten numbers, ONE all-reduce of the zero-padded (images, 11) matrix hands every rank all of them (`gather_rows`), and
    the replay runs over them in file order -- the same Counter for every world size.  The Counter returned then holds only
    the surviving keys, in the reference's order; `write_csv(..., reference_counter=True)` writes exactly those rows.
    `streams` > 1 (fused flow): consecutive images are queued round-robin on that many HIP streams, each driven by its own host
    thread (xai_engine/streams.py; `attr_fn` and the image access then run on those threads, in no particular order) --
    attribution, ranking and the three step sequences of one image form a serial chain of mostly small or low-occupancy launches,
    so the chains of `streams` images overlap on the chip.  Only for classifiers whose forward keeps no per-pass state ON THE MODEL:
    the hooked ViT saves attention maps / gradients / block outputs on its modules and TIS / ViT-CX hang hooks on it, so concurrent
    passes through one such model would read each other's tensors -- use `streams=1` there (the harness does).
    `graphs` (with `streams` > 1): every stream worker replays the forward passes of its step batches as hipGraphs it captured itself
    (`_CapturedForward`, a streams.CapturedCall; three threads enqueueing ~250 launches per batch under one interpreter lock are
    otherwise the limit).
    Every image still runs the same kernels on the same shapes and the per-image Counters are folded in image order, so the sums are
    bit-identical to `streams=1` (tests/test_gpu_configs.py::test_classifier_passes_on_several_streams_are_bit_identical_to_one_stream).
    The third return value, seconds in attribution, is measured with HIP events on the image's stream when the map stays on the
    device (the reference times a finished attribution, evaluatePerturbation.py:581-590; the host clock around an asynchronous
    launch would only see the enqueue).
    `extra`: images[i] is a pair (x, extra_i) and the attribution is attr_fn(x, target, extra_i) (the harness passes the
    un-normalised image and its file name to the rows that need them, TRANS_ATTR_FUNCS)."""
    dev = hip_device(device)
    sweep = PerturbationSweep(model, img_hw, dev, batch_size=batch_size) if fused else None
    td = testing_dict or {"models": [model], "img_hw": img_hw, "batch_size": batch_size, "device": str(dev)}
    blur = GaussianBlur(31, 31, dev)
    mine = shard_indices(len(images), rank, world)
    ident = ""
    if checkpoint:
        ident = sweep_identity(caller=identity or "", fused=fused, img_hw=img_hw, batch_size=batch_size, model=model_fingerprint(model))
    st = SweepState.load_or_new(checkpoint, len(images), rank, world, ident)

    def fold(c, pos):
        for k in KEYS:                                   # plain sums: see DESIGN.md on the reference's Counter `+=`
            st.sums[k] += float(c[k])
        if reference_counter:
            st.rows[mine[pos]] = [float(c[k]) for k in KEYS]
        st.used += 1
        st.next_pos = pos + 1
        if checkpoint and (st.next_pos % checkpoint_every == 0 or st.next_pos == len(mine)):
            st.save(checkpoint)

    from .streams import on_worker
    n_streams = max(1, int(streams)) if (fused and not on_worker()) else 1      # (called from a stream worker: this thread is the stream)
    ws = None
    if n_streams > 1:
        from .streams import workers, join, first_alone
        ws = workers(dev, n_streams)                     # one host thread per stream (streams.py)
        # the first image of a kind of sweep on each worker runs alone (streams.first_alone); `kind` names what attr_fn does (the
        # harness passes the method name), by default the function object itself
        kind = ("sweep", id(model), kind if kind is not None else id(attr_fn), img_hw, batch_size, bool(graphs))
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))     # weights, blur taps: whatever the caller's stream has queued so far
    pending = collections.deque()                        # (future or result, pos) of the images whose device work is in flight
    failed = None

    def device_part(pos):
        """Everything of one image that runs on the device, queued on the current stream of the calling thread:
        -> (handle for `finish` or the finished Counter, attribution timer or None)."""
        x, ext = images[mine[pos]] if extra else (images[mine[pos]], None)
        if ws is not None:
            torch.cuda.current_stream(dev).wait_event(ready)
        if fused and not x.is_cuda:
            # one upload through pinned memory, queued behind the previous image's work: a pageable .to(dev) blocks the
            # host until the stream has drained, which would undo the pipelining
            x = x.to(torch.float32).contiguous().pin_memory().to(dev, non_blocking=True)
        with torch.no_grad():
            target = _logits_of(model(x.to(dev))).argmax(1)[0]
        timer = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        t0 = time.time()
        timer[0].record(torch.cuda.current_stream(dev))
        sal = attr_fn(x, target, ext) if extra else attr_fn(x, target)
        timer[1].record(torch.cuda.current_stream(dev))
        host_seconds = None
        if not (torch.is_tensor(sal) and sal.is_cuda):
            host_seconds = time.time() - t0              # a host map: attr_fn has waited for the device itself
            timer = None
        if fused:
            return sweep.launch(x, sal, graphs=graphs and ws is not None), timer, host_seconds
        if timer is not None:
            timer[1].synchronize()
            host_seconds, timer = timer[0].elapsed_time(timer[1]) * 1e-3, None
        return run_perturbation(x.cpu(), sal, td, blur=blur), timer, host_seconds

    def finish_oldest():
        job, pos = pending.popleft()
        out, timer, host_seconds = job.result() if ws is not None else job
        c = sweep.finish(out) if fused else out
        if timer is not None:                            # the events lie before `done` on the same stream: complete by now
            st.attr_time += timer[0].elapsed_time(timer[1]) * 1e-3
        if host_seconds is not None:
            st.attr_time += host_seconds
        fold(c, pos)

    try:
        for pos in range(st.next_pos, len(mine)):
            # `n_streams` images deep: queue this image's device work (on its stream's worker thread), then do the oldest image's
            # host arithmetic while the device runs
            pending.append((first_alone(ws[pos % n_streams], kind, lambda pos=pos: device_part(pos)) if ws is not None else device_part(pos), pos))
            while len(pending) > (n_streams if fused else 0):
                finish_oldest()
    except BaseException as e:
        failed = e
        raise
    finally:
        while pending:                                   # also on an exception: the queued images are complete work, keep them
            try:
                finish_oldest()
            except Exception:
                if failed is None:                       # nothing else went wrong: this IS the error
                    raise
                break                                    # a device error already in flight makes the fold fail too: report the original
        if ws is not None:
            join(dev, ws)
    if reference_counter:
        if len(st.rows) != st.used:
            raise CheckpointMismatch("this checkpoint was written without reference_counter: it holds sums only, not the per-image "
                                     "numbers the reference's order-dependent fold needs; start again with another --checkpoint prefix")
        rows, flags, attr_seconds = gather_rows(st.rows, len(images), dev, world=world, attr_seconds=st.attr_time)
        return replay_reference_counter(rows[flags]), int(flags.sum()), attr_seconds
    return reduce_counters(st.sums, st.used, dev, world=world, attr_seconds=st.attr_time)


def write_csv(path, counter_sum, images_used, attr_time, total_time, reference_counter=False):
    """rows `key,mean` for the metrics + the two runtime rows (reference :606-618).
    Default: always the ten keys in KEYS order, plain sums / images, and a last row `Fold,plain sums` that says so.
    `reference_counter=True`: `counter_sum` is the Counter of `sweep_images(..., reference_counter=True)` and the file is the reference's,
    row for row (:612-618) -- only the keys that survived its `+=`, in the Counter's own order, then the two runtime rows."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        w = csv.writer(f)
        for k in (counter_sum if reference_counter else KEYS):
            w.writerow([k, str(counter_sum[k] / images_used)])
        w.writerow(["Attr Avg Runtime", str(attr_time / images_used)])
        w.writerow(["Total Runtime", str(total_time)])
        if not reference_counter:                        # (nothing in the reference reads these files back; the row tells the two folds apart)
            w.writerow(["Fold", "plain sums"])
