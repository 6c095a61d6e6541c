"""Command line of the harness counterpart for the CLIP models of the reference's table
(XAI_Survey/evaluations/evaluatePerturbation.py:660-677, `--model CLIP16 | CLIP32`): the flags of xai_engine.evaluate_perturbation
plus the two a CLIP run needs.  A module of its own: evaluate_perturbation's MODELS is also the table of the sanity and the
segmentation CLIs, which do not serve CLIP, and all three refuse a CLIP model by name.

    python -m xai_engine.evaluate_clip --model CLIP16 --attr_func eclip --image_count 1000 \
        --dataset_path /data/ImageNet/val --weights clip_b16.pt --text_embeddings embeddings_b16.pt

`--weights` takes the state_dict of `clip.load(...)` (OpenAI's parameter names); without it the weights are seeded and random.
`--text_embeddings` takes a (classes, E) tensor, row c the text embedding of "a photo of a <class c>" (the reference's
testing_dict["embeddings"]); without it the embeddings are seeded and random too.  The served rows are eclip, eclip_wo, eclip_nograd,
maskclip and selfattn (xai_engine/eclip.py).  game, rollout and lrp are refused by default, naming the second model object the
reference runs them on; `--clip_attention_rows plain` serves them in closed form on the plain model (xai_engine/clip_attn.py), which
is exact because that second model has plain CLIP's weights and forward and the rows read only its attention probabilities and their
gradients.  surgery is refused by default too, naming the third model object; `--clip_surgery plain` serves it in closed form on the
plain model in fp32 (xai_engine/surgery.py), with `--surgery_text_features`, a (T - 1, E) tensor of the context classes' text
features (the reference's 59 prompt-ensembled class names; without it seeded and random, like `--text_embeddings`).  m2ib is refused
by default as well, naming the fourth model object; `--clip_m2ib plain` serves it in closed form on the plain model in the model's
dtype (xai_engine/m2ib.py), with `--m2ib_text_features`, the (classes, E) table of the M2IB wrapper's text features
(m2ib.wrapper_text_features; without it seeded and random), and `--m2ib_noise device|host`.
"""
import torch

from . import dist as xd
from . import evaluate_perturbation, harness
from .sweep import CLIP_ATTR_FUNCS
from .zoo import clip_vit_b16, clip_vit_b32, convert_weights_fp16

CLIP_MODELS = {
    # name: (constructor, batch size, normalisation, num_patches), as evaluate_perturbation.MODELS
    "CLIP16": (clip_vit_b16, 25, (harness.CLIP_MEAN, harness.CLIP_STD), 14),
    "CLIP32": (clip_vit_b32, 50, (harness.CLIP_MEAN, harness.CLIP_STD), 7),
}


def build_parser():
    p = evaluate_perturbation.build_parser()
    p.set_defaults(model="CLIP16", attr_func="eclip")
    p.add_argument("--text_embeddings", type=str, default=None, help="a (classes, E) tensor saved with torch.save; default: seeded random")
    p.add_argument("--clip_fp32", action="store_true", help="run the model in fp32; default: OpenAI's mixed fp16, as the reference's "
                   "clip.load gives on a GPU")
    p.add_argument("--clip_attention_rows", choices=("modified", "plain"), default="modified",
                   help="game, rollout and lrp: 'modified' refuses them (the reference runs them on a second, hooked model object); "
                   "'plain' computes them in closed form on the plain model")
    p.add_argument("--clip_surgery", choices=("modified", "plain"), default="modified",
                   help="surgery: 'modified' refuses it (the reference runs it on a third model object, the CLIP Surgery class); "
                   "'plain' computes it in closed form on the plain model, in fp32")
    p.add_argument("--surgery_text_features", type=str, default=None,
                   help="a (T - 1, E) tensor saved with torch.save, the text features of surgery's context classes; default: 59 seeded "
                   "random rows")
    p.add_argument("--clip_m2ib", choices=("modified", "plain"), default="modified",
                   help="m2ib: 'modified' refuses it (the reference runs it on a fourth model object, the M2IB wrapper); 'plain' "
                   "computes it in closed form on the plain model, in the model's dtype")
    p.add_argument("--m2ib_text_features", type=str, default=None,
                   help="a (classes, E) tensor saved with torch.save, the M2IB wrapper's text feature of each class "
                   "(m2ib.wrapper_text_features); default: seeded random rows")
    p.add_argument("--m2ib_noise", choices=("device", "host"), default="device",
                   help="m2ib: where the bottleneck's noise is drawn; 'host' draws from torch's CPU generator in the reference's order")
    return p


def main(argv=None):
    args, _ = build_parser().parse_known_args(argv)
    if args.model not in CLIP_MODELS:
        raise SystemExit(f"unknown --model {args.model}; choose from {sorted(CLIP_MODELS)}")
    if args.attr_func not in CLIP_ATTR_FUNCS:
        print("Model-attribution mismatch, please use --help.")
        raise SystemExit(1)
    rank, world, device = xd.init_from_env()
    if world == 1:
        device = torch.device("cuda", args.cuda_num)
        torch.cuda.set_device(device)
    ctor, batch_size, norm, num_patches = CLIP_MODELS[args.model]
    model = ctor()
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
    if not args.clip_fp32:
        convert_weights_fp16(model)
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    embed = model.visual.output_dim
    if args.text_embeddings:
        emb = torch.load(args.text_embeddings, map_location="cpu", weights_only=True)
    else:
        emb = torch.randn(1000, embed, generator=torch.Generator().manual_seed(0))
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.shape[1] != embed:
        raise SystemExit(f"--text_embeddings must hold a (classes, {embed}) tensor")
    if args.surgery_text_features:
        context = torch.load(args.surgery_text_features, map_location="cpu", weights_only=True)
    else:
        context = torch.randn(59, embed, generator=torch.Generator().manual_seed(1))
    if not torch.is_tensor(context) or context.dim() != 2 or context.shape[1] != embed:
        raise SystemExit(f"--surgery_text_features must hold a (T - 1, {embed}) tensor")
    if args.m2ib_text_features:
        m2ib_table = torch.load(args.m2ib_text_features, map_location="cpu", weights_only=True)
    else:
        m2ib_table = torch.randn(emb.shape[0], embed, generator=torch.Generator().manual_seed(2))
    if not torch.is_tensor(m2ib_table) or m2ib_table.dim() != 2 or m2ib_table.shape[1] != embed:
        raise SystemExit(f"--m2ib_text_features must hold a (classes, {embed}) tensor")
    testing_dict = {"models": [model], "imagenet_dataset": args.dataset_path, "normalize": norm, "img_hw": 224,
                    "batch_size": args.batch_size or batch_size, "attr_func": args.attr_func, "model_name": args.model,
                    "image_count": args.image_count, "device": str(device), "class_map_path": args.class_map,
                    "weights_path": args.weights or "", "num_patches": num_patches,
                    "embeddings": emb.to(device=device, dtype=model.dtype), "num_classes": emb.shape[0],
                    "clip_attention_rows": args.clip_attention_rows, "clip_surgery": args.clip_surgery,
                    "surgery_text_features": context.to(device=device, dtype=torch.float32),
                    "clip_m2ib": args.clip_m2ib, "m2ib_text_features": m2ib_table.to(device=device, dtype=model.dtype),
                    "m2ib_noise": args.m2ib_noise}
    total, used, _ = harness.evaluate_perturbation(testing_dict, rank=rank, world=world, out_dir=args.out_dir,
                                                     reference_counter=args.reference_counter)
    if rank == 0:
        print(f"{used} images; means: " + ", ".join(f"{k}={total[k] / max(used, 1):.6f}" for k in total))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
