#!/usr/bin/env python3
"""Guided Backprop (`gbp`) and Guided Grad-CAM (`ggc`) on ResNet-50 at 224^2 with the harness's arguments; writes
profiles/r08_guided.txt.  Three steps, each a process of its own with its own time limit, chained with &&:

    timeout -k 10 600 python profiles/bench_guided.py rates --json OUT/guided_rates.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/guided_prof -o guided -- \\
        python profiles/bench_guided.py kernels && \\
    python profiles/bench_guided.py report --json OUT/guided_rates.json --trace OUT/guided_prof --out profiles/r08_guided.txt

rates    attributions/s (wall clock around synchronised calls, warmed) of the harness's one-image call and of
         guided_backprop_batch at B = 32, replayed from the hipGraph and eager, on the fused (fork_residual) and the unfused
         classifier; the yardstick is captum's flow restated in the same process (tests/guided_restated.py: backward-pre-hooks for
         gbp, two forwards and two backwards for ggc, the map on the host); next to them the existing `grad` row, which moves the
         same bytes.  Parity configuration: cudnn.deterministic, benchmark off.
kernels  the guided instantiations of the two fused backward kernels alternating with their unguided twins on the same tensors,
         and K28 at a size past the Infinity Cache, a few launches each, for a rocprofv3 --kernel-trace run (no counters).
report   no device: the two results as one text file."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
HBM_PEAK = 8.0e12
MASK_SHAPE = (32, 256, 56, 56)           # layer1's block output at B = 32: 102.8 MB per tensor
STEM_SHAPE = (32, 64, 112, 112)          # the stem activation at B = 32
K28_B = 512                              # 512 x 3 x 224 x 224: 308 MB in, past the 256 MiB Infinity Cache
LAUNCHES = 6                             # per kernel; the first of each is dropped as warm-up


def timed(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def rates(args):
    import torch
    import guided_restated as R
    from xai_engine import guided
    from xai_engine.prepare import fuse_bn_relu
    from xai_engine.sweep import get_CNN_attr
    from xai_engine.zoo import resnet50
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    model = resnet50(seed=0).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    fused = fuse_bn_relu(model, fork_residual=True)
    x = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        t = model(x).argmax(1)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model": "resnet50 seed 0", "deterministic": True}

    def rel_inf(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max())

    restated = {"gbp": lambda xs, ts: R.guided_backprop(model, xs, ts), "ggc": lambda xs, ts: R.guided_gradcam(model, model.layer4, xs, ts)}
    for name in ("gbp", "ggc"):
        flow = restated[name]
        R.harness_map(flow(x[:1], t[:1])[0])                                       # warm
        s1 = timed(lambda: R.harness_map(flow(x[1:2], t[1:2])[0]), 10)
        flow(x, t)
        s32 = timed(lambda: flow(x, t), 3)
        res[f"{name}.captum_flow"] = {"one_image_s": s1, "one_image_attr_per_s": 1 / s1, "batch32_s": s32, "batch32_attr_per_s": 32 / s32}
    for label, m in (("fused", fused), ("unfused", model)):
        td = {"models": [m, m], "img_hw": 224, "batch_size": 50, "device": DEV, "device_maps": True}
        row = dict(td, attr_func="grad")
        get_CNN_attr(x[:1], None, t[0], row)
        s = timed(lambda: get_CNN_attr(x[:1], None, t[0], row), 20)
        res[f"grad.{label}"] = {"harness_one_image_s": s, "harness_one_image_attr_per_s": 1 / s}
        for name in ("gbp", "ggc"):
            layer = m.layer4 if name == "ggc" else None
            row = dict(td, attr_func=name)
            for _ in range(3):                                                      # eager warm-up, capture, proof, first replays
                get_CNN_attr(x[:1], None, t[0], row)
            one = timed(lambda: get_CNN_attr(x[:1], None, t[0], row), 20)
            kw = dict(layer=layer, want_attr=False, want_map=True)
            guided.guided_backprop_batch(x[:1], m, t[:1], graphs=False, **kw)
            one_eager = timed(lambda: guided.guided_backprop_batch(x[:1], m, t[:1], graphs=False, **kw), 10)
            for _ in range(2):
                guided.guided_backprop_batch(x, m, t, graphs=True, **kw)
            b32 = timed(lambda: guided.guided_backprop_batch(x, m, t, graphs=True, **kw), 3)
            guided.guided_backprop_batch(x, m, t, graphs=False, **kw)
            b32_eager = timed(lambda: guided.guided_backprop_batch(x, m, t, graphs=False, **kw), 3)
            got = guided.guided_backprop_batch(x[2:3], m, t[2:3], layer=layer, graphs=False)
            flow_s = res[f"{name}.captum_flow"]
            res[f"{name}.{label}"] = {
                "harness_one_image_s": one, "harness_one_image_attr_per_s": 1 / one, "one_image_eager_s": one_eager,
                "one_image_eager_attr_per_s": 1 / one_eager, "batch32_s": b32, "batch32_attr_per_s": 32 / b32, "batch32_eager_s": b32_eager,
                "batch32_eager_attr_per_s": 32 / b32_eager, "one_image_over_captum_flow": flow_s["one_image_s"] / one,
                "batch32_over_captum_flow": flow_s["batch32_s"] / b32, "engine_vs_captum_flow_rel_inf": rel_inf(got, restated[name](x[2:3], t[2:3]))}
    res["graph_counts"] = dict(guided.GUIDED_COUNTS)
    for k, v in res.items():
        print(f"{k:24s} {json.dumps(v) if isinstance(v, dict) else v}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)


def kernels(args):
    import torch
    from xai_engine import kernels as K
    from xai_engine.prepare import BN_VARIANT
    gen = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)      # noqa: E731
    Cc = MASK_SHAPE[1]
    w, b, mean, var = torch.rand(Cc, device=DEV) + 0.5, rnd(Cc), rnd(Cc), torch.rand(Cc, device=DEV) + 0.5
    xm, idt, gy, gy2 = rnd(*MASK_SHAPE), rnd(*MASK_SHAPE), rnd(*MASK_SHAPE), rnd(*MASK_SHAPE)
    _, mask = K.bn_relu_fwd_mask(xm, idt, w, b, mean, var, 1e-5, BN_VARIANT)
    del xm, idt
    for _ in range(LAUNCHES):
        for guided in (False, True):
            K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, BN_VARIANT, want_identity=True, gy2=gy2, guided=guided)
    del gy, gy2
    Cs = STEM_SHAPE[1]
    ws, bs, ms, vs = torch.rand(Cs, device=DEV) + 0.5, rnd(Cs), rnd(Cs), torch.rand(Cs, device=DEV) + 0.5
    y, code = K.bn_relu_maxpool_fwd_code(rnd(*STEM_SHAPE), ws, bs, ms, vs, 1e-5, BN_VARIANT, 3, 2, 1)
    g1, g2 = rnd(*y.shape), rnd(*y.shape)
    for _ in range(LAUNCHES):
        for guided in (False, True):
            K.bn_relu_maxpool_bwd(g1, code, ws, vs, 1e-5, BN_VARIANT, STEM_SHAPE[2], STEM_SHAPE[3], 3, 2, 1, gy2=g2, guided=guided)
    grad, cam = rnd(K28_B, 3, 224, 224), rnd(K28_B, 7, 7).relu()
    attr, out = torch.empty_like(grad), torch.empty(K28_B, 224, 224, device=DEV)
    for _ in range(LAUNCHES):
        K.guided_map(grad, cam, want_attr=True, want_map=True, attr=attr, map=out)
    torch.cuda.synchronize()
    for _ in range(LAUNCHES):                                         # the harness's form: the map only
        K.guided_map(grad, cam, want_attr=False, want_map=True, map=out)
    torch.cuda.synchronize()
    print("kernels done")


def _launch_times(trace_dir):
    """{kernel name: [duration in us per launch, in launch order]} from rocprofv3's kernel trace"""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out = {}
    for _, name, us in sorted(rows):
        out.setdefault(name, []).append(us)
    return out


def report(args):
    res = json.load(open(args.json))
    times = _launch_times(args.trace)
    n_mask = MASK_SHAPE[0] * MASK_SHAPE[1] * MASK_SHAPE[2] * MASK_SHAPE[3]
    n_stem_in = STEM_SHAPE[0] * STEM_SHAPE[1] * STEM_SHAPE[2] * STEM_SHAPE[3]
    n_stem_out = n_stem_in // 4
    n28 = K28_B * 3 * 224 * 224
    lines = ["# python profiles/bench_guided.py rates | kernels (under rocprofv3 --kernel-trace --stats) | report, on one MI355X; ResNet-50 (seed 0)",
             "# at 224^2, harness arguments (gbp: GuidedBackprop; ggc: GuidedGradCam on layer4); parity mode: cudnn.deterministic, benchmark off;",
             "# rates: one process, wall clock around synchronised calls, every shape warmed first"]
    for k, v in res.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                lines.append(f"{k + '.' + kk:52s} {vv}")
        else:
            lines.append(f"{k:52s} {v}")
    lines += ["# captum_flow: tests/guided_restated.py on the unfused classifier in the same process -- hooks on every nn.ReLU for gbp; for ggc",
              "#   a plain forward + backward to layer4 and a guided forward + backward, then the product; one_image includes the host map (:181)",
              "# harness_one_image: get_CNN_attr(..., 'gbp' | 'ggc') with device_maps -- one hipGraph replay of forward + guided backward",
              "#   (+ Grad-CAM reduction) + K28, map only; one_image_eager / batch32_eager: the same pass with graphs=False",
              "# grad: the existing row (getGradientsParallel, eager) on the same classifier: a guided pass moves the same bytes",
              "",
              "# rocprofv3 --kernel-trace --stats -- python profiles/bench_guided.py kernels   (a run of its own, no counters); us per launch,",
              f"# {LAUNCHES} launches each, guided and unguided alternating on the same tensors, the first launch of each dropped"]

    def pick(sub):
        hit = [n for n in times if all(s in n for s in sub)]
        if len(hit) != 1:
            raise SystemExit(f"kernel {sub}: {len(hit)} matches in the trace: {hit}")
        return times[hit[0]]

    def stat(label, us, nbytes):
        us = us[1:]
        avg = sum(us) / len(us)
        lines.append(f"{label:44s} " + " ".join(f"{u:.1f}" for u in us) + f"   avg {avg:.1f}  -> {nbytes / avg / 1e6:.2f} TB/s = "
                     f"{nbytes / avg * 1e6 / HBM_PEAK:.2f} of the 8 TB/s peak ({nbytes / 1e6:.0f} MB)")
        return avg
    mask_bytes = 4 * n_mask * 4 + n_mask // 8                                      # gy, gy2 in; gx, g_identity out; the gate bits
    a = stat("bn_relu_bwd_mask_kernel<true, true, false>", pick(("bn_relu_bwd_mask_kernel<true, true, false>",)), mask_bytes)
    g = stat("bn_relu_bwd_mask_kernel<true, true, true>   (guided)", pick(("bn_relu_bwd_mask_kernel<true, true, true>",)), mask_bytes)
    lines.append(f"guided / unguided                            {g / a:.3f}")
    stem_bytes = 2 * n_stem_out * 4 + n_stem_out + n_stem_in * 4                    # gy, gy2, codes in; gx out
    a = stat("bn_relu_maxpool_bwd_kernel<2, false>", pick(("bn_relu_maxpool_bwd_kernel<2, false>",)), stem_bytes)
    g = stat("bn_relu_maxpool_bwd_kernel<2, true>         (guided)", pick(("bn_relu_maxpool_bwd_kernel<2, true>",)), stem_bytes)
    lines.append(f"guided / unguided                            {g / a:.3f}")
    k28 = pick(("guided_map_kernel<true>",))
    stat(f"guided_map_kernel<true> (K28) attr + map, B = {K28_B}", k28[:LAUNCHES], 2 * n28 * 4 + n28 // 3 * 4)
    stat(f"guided_map_kernel<true> (K28) map only,   B = {K28_B}", k28[LAUNCHES:], n28 * 4 + n28 // 3 * 4)
    lines.append("# bytes are the algorithm's (every tensor once; the 7 x 7 cam is 100 KB and stays in L2); README's K6 / K26 on 472 MB written:")
    lines.append("# 5.34 / 5.00 TB/s = 0.67 / 0.62 of peak (profiles/r07_ablation.txt)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["rates", "kernels", "report"])
    ap.add_argument("--json", help="rates: written; report: read")
    ap.add_argument("--trace", help="report: the directory rocprofv3 wrote into")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_guided.txt"))
    args = ap.parse_args()
    if (args.step != "kernels" and not args.json) or (args.step == "report" and not args.trace):
        ap.error("rates needs --json, report needs --json and --trace")
    {"rates": rates, "kernels": kernels, "report": report}[args.step](args)


if __name__ == "__main__":
    main()
