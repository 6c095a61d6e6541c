"""Command line of the segmentation-evaluation counterpart -- the reference's flags
(XAI_Survey/evaluations/evaluateImageNetSeg.py:680-701: --model --image_count --attr_func --cuda_num --dataset_path) plus what an
offline box needs (weights from a local file, output folder, the number of maps scored per launch).

    python -m xai_engine.evaluate_imagenet_seg --model R50 --attr_func gc --image_count 1000 \
        --dataset_path /data/gtsegs_ijcv.mat --weights r50.pt

--dataset_path is gtsegs_ijcv.mat (read with h5py) or an .npz file with the keys img_<i> (uint8 HWC) and gt_<i> (uint8 HW).
The rows t_attr, MDA_dense and the CLIP models are refused by name (segeval.REFUSED).
"""
import argparse

import torch

from . import segeval
from .evaluate_perturbation import MODELS
from .sweep import CNN_ATTR_FUNCS, VIT_ATTR_FUNCS, VIT_TRANS_ATTR_FUNCS


def build_parser():
    p = argparse.ArgumentParser("")
    p.add_argument("--model", type=str, default="R101", help="Classifier to use: " + ", ".join(MODELS))
    p.add_argument("--image_count", type=int, default=-1, help="How many images to test with. -1 indicates all images")
    p.add_argument("--attr_func", type=str, default="ig", help="attr to use: R50/R101/R152/RNXT: {" + ", ".join(CNN_ATTR_FUNCS) +
                   "}, VIT16/VIT32: {" + ", ".join(VIT_ATTR_FUNCS + VIT_TRANS_ATTR_FUNCS) + "}")
    p.add_argument("--cuda_num", type=int, default=0, help="The number of the GPU you want to use.")
    p.add_argument("--dataset_path", type=str, default="../../../gtsegs_ijcv.mat", help="The path to your dataset input")
    p.add_argument("--weights", type=str, default=None, help="state_dict file for the chosen architecture")
    p.add_argument("--out_dir", type=str, default="seg_test_results")
    p.add_argument("--batch", type=int, default=32, help="maps scored by one K44 / K45 launch pair and one read-back")
    return p


def main(argv=None):
    args, _ = build_parser().parse_known_args(argv)
    if args.model not in MODELS:
        raise SystemExit(f"unknown --model {args.model}; choose from {sorted(MODELS)}")
    if args.attr_func in segeval.REFUSED:
        raise SystemExit(f"--attr_func {args.attr_func} is not served: {segeval.REFUSED[args.attr_func]}")
    is_vit = "VIT" in args.model
    if args.attr_func not in (VIT_ATTR_FUNCS + VIT_TRANS_ATTR_FUNCS if is_vit else CNN_ATTR_FUNCS):
        print("Model-attribution mismatch, please use --help.")
        raise SystemExit(1)
    device = torch.device("cuda", args.cuda_num)
    torch.cuda.set_device(device)
    ctor, batch_size, norm, num_patches = MODELS[args.model]
    model = ctor()
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    reader = segeval.NpzSegmentation if args.dataset_path.endswith(".npz") else segeval.MatSegmentation
    ds = reader(args.dataset_path)
    count = len(ds) if args.image_count == -1 else min(args.image_count, len(ds))
    testing_dict = {"models": [model, model], "segmentation_dataloader": ds.loader(count), "normalize": norm, "img_hw": 224,
                    "image_count": count, "num_patches": num_patches, "batch_size": batch_size, "attr_func": args.attr_func,
                    "model_name": args.model, "device": str(device)}
    miou, pix_acc, m_ap, m_f1 = segeval.evaluate_imagenet_seg(testing_dict, out_dir=args.out_dir, batch=args.batch)
    print(f"{args.model} pixAcc {args.attr_func}: {pix_acc:.4f}, mIoU: {miou:.4f}, mAP: {m_ap:.4f}, mF1: {m_f1:.4f}")


if __name__ == "__main__":
    main()
