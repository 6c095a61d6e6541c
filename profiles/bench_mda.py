#!/usr/bin/env python3
"""MDA (`--attr_func MDA`) on ViT-B/16 at 224^2 with 196 patches; writes profiles/r12_mda.txt.  Three steps, each a process of its
own with its own time limit, chained with &&:

    timeout -k 10 1100 python profiles/bench_mda.py rates --json OUT/mda_rates.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/mda_prof -o mda -- \\
        python profiles/bench_mda.py kernels && \\
    python profiles/bench_mda.py report --json OUT/mda_rates.json --trace OUT/mda_prof --out profiles/r12_mda.txt

rates    seconds per attribution (wall clock around synchronised calls, warmed) of the harness row get_VIT_attr(..., "MDA") with a
         14 x 14 grid as `mda_segments` (skimage's SLIC is not a dependency of the engine), against the reference's flow restated in
         the same process (tests/mda_restated.py: every candidate image built on the host, uploaded five at a time, the scores read
         back) behind the same blur search and bi_attn map.  Parity configuration: cudnn.deterministic, benchmark off.
kernels  K36 at 28 rows x 3 x 224 x 224 x 32 images (past the Infinity Cache), alternating with K26 on the same bytes, a few
         launches each, for a rocprofv3 --kernel-trace run (no counters).
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
sys.path.insert(0, ROOT)

DEV = "cuda:0"
HBM_PEAK = 8.0e12
KB, KL = 32, 28                          # 896 rows x 3 x 224 x 224: 539 MB of candidate images, past the 256 MiB Infinity Cache
LAUNCHES = 6                             # per kernel; the first of each is dropped as warm-up


def rates(args):
    import numpy as np
    import torch
    import mda_restated as R
    from xai_engine import kernels as K
    from xai_engine import mda
    from xai_engine.blur import blur_until_unconfident
    from xai_engine.sweep import get_VIT_attr
    from xai_engine.vit_attr import Baselines
    from xai_engine.zoo import vit_base_patch16_224
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    model = vit_base_patch16_224().to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        t = model(x.to(DEV)).argmax(1)[0].cpu()
    seg = R.grid_labels(224, 14)
    td = {"models": [model, model], "img_hw": 224, "batch_size": 25, "device": DEV, "num_patches": 14, "attr_func": "MDA", "mda_segments": seg}
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model": "vit_base_patch16_224, seeded random weights",
           "deterministic": True, "segments": 196, "sub_search_width": mda.subsearch_len(196), "poll_interval": mda.POLL_INTERVAL}

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    first, _ = sync_time(lambda: get_VIT_attr(x.clone(), None, t, td))               # eager warm-up, capture, proof
    before = dict(mda.MDA_COUNTS)
    row, got = sync_time(lambda: get_VIT_attr(x.clone(), None, t, td))
    res["mda.engine"] = {"first_call_s": first, "harness_row_s": row, "counts_of_the_timed_call": {k: mda.MDA_COUNTS[k] - before[k] for k in before}}

    def flow():
        blur, _, _, _ = blur_until_unconfident(model, x, t, DEV)
        bi, _ = Baselines(model).bidirectional(x.to(DEV), t, device=torch.device(DEV))
        bi = K.resize_bilinear(bi.detach().float().contiguous(), 224, 224)[0].cpu().numpy()[:, :, None] * np.ones((224, 224, 3))
        m, _, _ = R.MDA(None, x, bi, 196, blur, model, DEV, 224, max_batch_size=5, segments=seg, metric=R.engine_metric(model, 224))
        return np.abs(np.sum(m, axis=2)).astype(np.float32)
    ref_s, want = sync_time(flow)
    res["mda.reference_flow"] = {"harness_row_s": ref_s}
    res["mda.engine"]["over_reference_flow"] = ref_s / row
    res["mda.engine"]["engine_vs_reference_flow_rel_inf"] = float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30))
    for k, v in res.items():
        print(f"{k:24s} {json.dumps(v) if isinstance(v, dict) else v}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)


def kernels(args):
    import torch
    from xai_engine import kernels as K
    gen = torch.Generator(device=DEV).manual_seed(0)
    start, finish = torch.randn(KB, 3, 224, 224, device=DEV, generator=gen), torch.randn(KB, 3, 224, 224, device=DEV, generator=gen)
    seg = torch.randint(0, 196, (KB, 224, 224), device=DEV, dtype=torch.int32, generator=gen)
    cand = torch.stack([torch.randperm(196, device=DEV, generator=gen)[:KL] for _ in range(KB)]).to(torch.int32)
    out = torch.empty(KB * KL, 3, 224, 224, device=DEV)
    for _ in range(LAUNCHES):
        K.mda_compose(start, finish, seg, cand, out=out)                              # K36
        K.ablate_features(start, seg[0], 0, KL, finish[0], 0, KB * KL, out=out)                   # K26 on the same bytes (ids shared)
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
    lines = ["# python profiles/bench_mda.py rates | kernels (under rocprofv3 --kernel-trace --stats) | report, on one MI355X; ViT-B/16 (seeded",
             "# random weights) at 224^2, 196 grid segments, harness arguments (MDA, max_batch_size 5); parity mode: cudnn.deterministic,",
             "# benchmark off; rates: one process, wall clock around synchronised calls, one timed call each after a warming first call"]
    for k, v in res.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                lines.append(f"{k + '.' + kk:52s} {vv}")
        else:
            lines.append(f"{k:52s} {v}")
    lines += ["# reference_flow: tests/mda_restated.py in the same process -- every candidate image built on the host, uploaded five at a",
              "#   time, the scores read back, behind the same blur search and bi_attn map and with the engine's MASMetric",
              "",
              "# rocprofv3 --kernel-trace --stats -- python profiles/bench_mda.py kernels   (a run of its own, no counters); us per launch,",
              f"# {LAUNCHES} launches each, alternating with K26 on the same tensors, the first launch of each dropped"]

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
    n_out, n_img = KB * KL * 3 * 224 * 224, KB * 3 * 224 * 224
    stat(f"mda_compose_kernel<4> (K36), {KB} x {KL} rows", pick(("mda_compose_kernel<4>",)), (n_out + 2 * n_img + n_img // 3) * 4)
    stat("K26 ablate_kernel on the same bytes", pick(("ablate_kernel<4",)), (n_out + n_img + n_img // 3) * 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["rates", "kernels", "report"])
    ap.add_argument("--json", help="rates: written; report: read")
    ap.add_argument("--trace", help="report: the directory rocprofv3 wrote into")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_mda.txt"))
    args = ap.parse_args()
    if (args.step != "kernels" and not args.json) or (args.step == "report" and not args.trace):
        ap.error("rates needs --json, report needs --json and --trace")
    {"rates": rates, "kernels": kernels, "report": report}[args.step](args)


if __name__ == "__main__":
    main()
