"""Command line of the sanity-test counterpart -- the reference's flags (XAI_Survey/evaluations/evaluateSanity.py:636-660:
--image_count --model --attr_func --cuda_num --dataset_path) plus what an offline box needs (weights from a local file, class-map
path, output folder).

    python -m xai_engine.evaluate_sanity --model R50 --attr_func gc --image_count 1000 \
        --dataset_path /data/ImageNet/val --class_map /data/correctly_classified_R50.txt --weights r50.pt

The randomised copy is a second instance of the architecture with the same weights, passed through sanity.randomize_CNN_model /
randomize_VIT_model (:521, :539).  CLIP models are not built.
"""
import argparse

import torch

from . import sanity
from .evaluate_perturbation import MODELS
from .sweep import CNN_ATTR_FUNCS, VIT_ATTR_FUNCS, VIT_LRP_ATTR_FUNCS, VIT_TRANS_ATTR_FUNCS


def build_parser():
    p = argparse.ArgumentParser("")
    p.add_argument("--image_count", type=int, default=1000, help="How many images to test with.")
    p.add_argument("--model", type=str, default="R101", help="Classifier to use: " + ", ".join(MODELS))
    p.add_argument("--attr_func", type=str, default="ig", help="attr to use: R50/R101/R152/RNXT: {" + ", ".join(CNN_ATTR_FUNCS) +
                   "}, VIT16/VIT32: {" + ", ".join(VIT_ATTR_FUNCS + VIT_LRP_ATTR_FUNCS + VIT_TRANS_ATTR_FUNCS) + "}")
    p.add_argument("--cuda_num", type=int, default=0, help="The number of the GPU you want to use.")
    p.add_argument("--dataset_path", type=str, default="../../../ImageNet", help="The path to your dataset input")
    p.add_argument("--class_map", type=str, default=None, help="correctly_classified_<MODEL>.txt (optional)")
    p.add_argument("--weights", type=str, default=None, help="state_dict file for the chosen architecture")
    p.add_argument("--out_dir", type=str, default="sanity_test_results")
    p.add_argument("--reference_counter", action="store_true", help="fold the images' results exactly like the reference's "
                   "`sanity_result_counter += ...` (evaluateSanity.py:485-488: a key whose running sum is <= 0 or NaN is dropped) and "
                   "write only the surviving CSV rows.  Default: plain sums, always three rows")
    return p


def _instance(ctor, weights, device):
    model = ctor()
    if weights:
        model.load_state_dict(torch.load(weights, map_location="cpu", weights_only=True))
    return model.to(device).eval()


def main(argv=None):
    args, _ = build_parser().parse_known_args(argv)
    if args.model not in MODELS:
        raise SystemExit(f"unknown --model {args.model}; choose from {sorted(MODELS)}")
    is_vit = "VIT" in args.model
    if args.attr_func not in (VIT_ATTR_FUNCS + VIT_LRP_ATTR_FUNCS + VIT_TRANS_ATTR_FUNCS if is_vit else CNN_ATTR_FUNCS):
        print("Model-attribution mismatch, please use --help.")
        raise SystemExit(1)
    device = torch.device("cuda", args.cuda_num)
    torch.cuda.set_device(device)
    ctor, batch_size, norm, num_patches = MODELS[args.model]
    model = _instance(ctor, args.weights, device)
    model_rand = (sanity.randomize_VIT_model if is_vit else sanity.randomize_CNN_model)(_instance(ctor, args.weights, device))
    for m in (model, model_rand):
        for p in m.parameters():
            p.requires_grad_(False)
    testing_dict = {"models": [model, model, model_rand, model_rand], "imagenet_dataset": args.dataset_path, "normalize": norm,
                    "img_hw": 224, "batch_size": batch_size, "attr_func": args.attr_func, "model_name": args.model,
                    "image_count": args.image_count, "device": str(device), "class_map_path": args.class_map,
                    "num_patches": num_patches}
    total, used, _ = sanity.evaluate_sanity(testing_dict, out_dir=args.out_dir, reference_counter=args.reference_counter)
    fold = "reference Counter += (keys with a running sum <= 0 dropped)" if args.reference_counter else "plain sums"
    print(f"{used} images; {fold}; means: " + ", ".join(f"{k}={total[k] / max(used, 1):.6f}" for k in total))


if __name__ == "__main__":
    main()
