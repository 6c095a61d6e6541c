#!/usr/bin/env python3
"""GradientShap (`gs`) on ResNet-50 at 224^2 with the harness's arguments; writes profiles/r11_gshap.txt.  Three steps, each a
process of its own with its own time limit, chained with &&:

    timeout -k 10 600 python profiles/bench_gshap.py rates --json OUT/gshap_rates.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/gshap_prof -o gshap -- \\
        python profiles/bench_gshap.py kernels && \\
    python profiles/bench_gshap.py report --json OUT/gshap_rates.json --trace OUT/gshap_prof --out profiles/r11_gshap.txt

rates    attributions/s (wall clock around synchronised calls, warmed) of the harness's one-image row and of gradient_shap_batch at
         B = 32 (160 rows, in passes of 8 images), replayed from the hipGraph and eager, on the fused (fork_residual) classifier; the
         yardstick is captum's flow restated in the same process (tests/gshap_restated.py: torch element-wise ops, the map on the
         host) on the unfused classifier.  Parity configuration: cudnn.deterministic, benchmark off.
kernels  K34 and K35 at a size past the Infinity Cache, alternating with K1 / K2 on the same bytes, a few launches each, for a
         rocprofv3 --kernel-trace run (no counters).
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
KB, KN = 128, 5                          # 640 rows x 3 x 224 x 224: 385 MB of interpolants / gradients, past the 256 MiB Infinity Cache
LAUNCHES = 6                             # per kernel; the first of each is dropped as warm-up
PASS_IMAGES = 8                          # 40 rows per classifier pass at B = 32


def timed(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def rates(args):
    import numpy as np
    import torch
    import gshap_restated as R
    from xai_engine import gshap
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
    base = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        t = model(x).argmax(1)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model": "resnet50 seed 0", "deterministic": True,
           "n_samples": 5, "pass_images_at_B32": PASS_IMAGES}

    def flow(xs, ts, k=None):
        return R.gradient_shap(model, xs, ts, base, n_samples=5, pass_images=k)
    R.harness_map(flow(x[:1], t[:1])[0])                                           # warm
    s1 = timed(lambda: R.harness_map(flow(x[1:2], t[1:2])[0]), 10)
    flow(x, t, PASS_IMAGES)
    s32 = timed(lambda: flow(x, t, PASS_IMAGES), 3)
    res["gs.captum_flow"] = {"one_image_s": s1, "one_image_attr_per_s": 1 / s1, "batch32_s": s32, "batch32_attr_per_s": 32 / s32}
    td = {"models": [fused], "img_hw": 224, "batch_size": 50, "device": DEV, "device_maps": True, "attr_func": "gs"}
    for _ in range(3):                                                              # eager warm-up, capture, proof, first replays
        get_CNN_attr(x[:1], None, t[0], td)
    one = timed(lambda: get_CNN_attr(x[:1], None, t[0], td), 20)
    kw = dict(n_samples=5, want_attr=False, want_map=True)
    gshap.gradient_shap_batch(x[:1], fused, t[:1], base, graphs=False, **kw)
    one_eager = timed(lambda: gshap.gradient_shap_batch(x[:1], fused, t[:1], base, graphs=False, **kw), 10)
    for _ in range(2):
        gshap.gradient_shap_batch(x, fused, t, base, pass_images=PASS_IMAGES, **kw)
    b32 = timed(lambda: gshap.gradient_shap_batch(x, fused, t, base, pass_images=PASS_IMAGES, **kw), 3)
    gshap.gradient_shap_batch(x, fused, t, base, pass_images=PASS_IMAGES, graphs=False, **kw)
    b32_eager = timed(lambda: gshap.gradient_shap_batch(x, fused, t, base, pass_images=PASS_IMAGES, graphs=False, **kw), 3)
    draws = (np.zeros(5, np.int64), np.linspace(0.1, 0.9, 5).astype(np.float32))
    got = gshap.gradient_shap_batch(x[2:3], fused, t[2:3], base, draws=draws)
    want = R.gradient_shap(model, x[2:3], t[2:3], base, draws=draws)
    cf = res["gs.captum_flow"]
    res["gs.fused"] = {"harness_one_image_s": one, "harness_one_image_attr_per_s": 1 / one, "one_image_eager_s": one_eager,
                       "one_image_eager_attr_per_s": 1 / one_eager, "batch32_s": b32, "batch32_attr_per_s": 32 / b32,
                       "batch32_eager_s": b32_eager, "batch32_eager_attr_per_s": 32 / b32_eager,
                       "one_image_over_captum_flow": cf["one_image_s"] / one, "batch32_over_captum_flow": cf["batch32_s"] / b32,
                       "engine_vs_captum_flow_rel_inf": float((got.double() - want.double()).abs().max() / want.double().abs().max())}
    res["graph_counts"] = dict(gshap.GSHAP_COUNTS)
    for k, v in res.items():
        print(f"{k:24s} {json.dumps(v) if isinstance(v, dict) else v}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)


def kernels(args):
    import torch
    from xai_engine import kernels as K
    gen = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)      # noqa: E731
    x, base1, baseB = rnd(KB, 3, 224, 224), rnd(1, 3, 224, 224), rnd(KB, 3, 224, 224)
    alpha = torch.rand(KB * KN, device=DEV, generator=gen)
    idx = torch.zeros(KB * KN, dtype=torch.int64, device=DEV)
    out = torch.empty(KB * KN, 3, 224, 224, device=DEV)
    for _ in range(LAUNCHES):
        K.gshap_scale(x, base1, alpha, idx, KN, out=out)                           # K34
        K.ig_interp(x, baseB, alpha[:KN].contiguous(), out=out.view(KB, KN, 3, 224, 224))        # K1 on the same bytes
    torch.cuda.synchronize()
    grads = out.normal_(generator=gen)
    attr, m = torch.empty(KB, 3, 224, 224, device=DEV), torch.empty(KB, 224, 224, device=DEV)
    for _ in range(LAUNCHES):
        K.gshap_finish(grads, x, base1, idx, KN, want_attr=True, want_map=True, attr=attr, map=m)    # K35
        K.ig_accum(grads.view(KB, KN, 3, 224, 224), x, baseB, want_abs=True)                         # K2 on the same bytes
    torch.cuda.synchronize()
    for _ in range(LAUNCHES):                                                       # the harness's form: the map only
        K.gshap_finish(grads, x, base1, idx, KN, want_attr=False, want_map=True, map=m)
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
    n_rows = KB * KN * 3 * 224 * 224
    n_img = KB * 3 * 224 * 224
    lines = ["# python profiles/bench_gshap.py rates | kernels (under rocprofv3 --kernel-trace --stats) | report, on one MI355X; ResNet-50 (seed 0)",
             "# at 224^2, harness arguments (gs: GradientShap, one randn baseline, 5 samples, no noise); parity mode: cudnn.deterministic,",
             "# benchmark off; rates: one process, wall clock around synchronised calls, every shape warmed first"]
    for k, v in res.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                lines.append(f"{k + '.' + kk:52s} {vv}")
        else:
            lines.append(f"{k:52s} {v}")
    lines += ["# captum_flow: tests/gshap_restated.py on the unfused classifier in the same process -- torch element-wise ops in front of and",
              "#   behind one forward + backward, the coefficients uploaded from the host per call; one_image includes the host map (:181)",
              "# harness_one_image: get_CNN_attr(..., 'gs') with device_maps -- the baseline drawn on the CPU and uploaded, then one hipGraph",
              "#   replay of K34 + forward + gather + backward + K35, map only; *_eager: the same pass with graphs=False",
              "",
              "# rocprofv3 --kernel-trace --stats -- python profiles/bench_gshap.py kernels   (a run of its own, no counters); us per launch,",
              f"# {LAUNCHES} launches each, alternating with K1 / K2 on the same tensors, the first launch of each dropped"]

    def pick(sub):
        hit = [n for n in times if all(s in n for s in sub)]
        if len(hit) != 1:
            raise SystemExit(f"kernel {sub}: {len(hit)} matches in the trace: {hit}")
        return times[hit[0]]

    def stat(label, us, nbytes):
        us = us[1:]
        avg = sum(us) / len(us)
        lines.append(f"{label:52s} " + " ".join(f"{u:.1f}" for u in us) + f"   avg {avg:.1f}  -> {nbytes / avg / 1e6:.2f} TB/s = "
                     f"{nbytes / avg * 1e6 / HBM_PEAK:.2f} of the 8 TB/s peak ({nbytes / 1e6:.0f} MB)")
        return avg
    # algorithmic bytes: every tensor once (K34 / K35 re-read x and the one baseline per sample from L2)
    stat(f"gshap_scale_kernel<4> (K34), {KB * KN} rows", pick(("gshap_scale_kernel<4>",)), (n_rows + n_img) * 4 + n_img // KB * 4)
    stat("K1 ig_interp on the same bytes", pick(("ig_interp",)), (n_rows + 2 * n_img) * 4)
    k35 = pick(("gshap_finish_kernel<4>",))
    stat(f"gshap_finish_kernel<4> (K35) attr + map, B = {KB}", k35[:LAUNCHES], (n_rows + 2 * n_img + n_img // 3) * 4 + n_img // KB * 4)
    stat(f"gshap_finish_kernel<4> (K35) map only,   B = {KB}", k35[LAUNCHES:], (n_rows + n_img + n_img // 3) * 4 + n_img // KB * 4)
    stat("K2 ig_accum (attr + |sum_c|) on the same bytes", pick(("ig_accum",)), (n_rows + 3 * n_img + n_img // 3) * 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["rates", "kernels", "report"])
    ap.add_argument("--json", help="rates: written; report: read")
    ap.add_argument("--trace", help="report: the directory rocprofv3 wrote into")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_gshap.txt"))
    args = ap.parse_args()
    if (args.step != "kernels" and not args.json) or (args.step == "report" and not args.trace):
        ap.error("rates needs --json, report needs --json and --trace")
    {"rates": rates, "kernels": kernels, "report": report}[args.step](args)


if __name__ == "__main__":
    main()
