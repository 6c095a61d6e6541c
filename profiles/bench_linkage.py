#!/usr/bin/env python3
"""Device complete linkage (K56-K57) for ViT-CX at D = 768 and D = 1024: K56 at each width of its one workgroup and K57 alone, the
whole device step (three launches, the one read-back, the host heapq cut) against the host step it replaces (the `.cpu()` copy of the
matrix and scikit-learn's AgglomerativeClustering.fit) in the same process, and the whole ViT_CX call on ViT-B/16 (seed 0, random
weights) both ways.
    python profiles/bench_linkage.py [--out profiles/r17_linkage.txt]
Kernel times are device events around `REPS` back-to-back launches after a warm-up, the median of `ROUNDS` such windows and their
spread, the kernels alternating inside a round.  Step and call times are a host clock around calls that end in a device synchronise,
median of `ROUNDS`.  There is no CPU fallback: no device, no numbers."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import torch  # noqa: E402
from xai_engine import kernels as K  # noqa: E402
from xai_engine import linkage as L  # noqa: E402
from xai_engine import vit_cx  # noqa: E402

DEV = "cuda:0"
REPS, ROUNDS = 5, 7
THRESHOLD = 0.1


def masks_like(D, P=196, groups=48, seed=0):
    """(D, P) non-negative rows around `groups` prototypes, so that the threshold 0.1 leaves tens of clusters as on a real ViT"""
    g = torch.Generator().manual_seed(seed)
    proto = torch.rand(groups, P, generator=g)
    rows = proto[torch.randint(0, groups, (D,), generator=g)] + 0.35 * torch.rand(D, P, generator=g)
    return rows.to(DEV)


def event_ms(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def windows(fns):
    """{name: fn} -> {name: (median ms, min ms, max ms)} over ROUNDS rounds, the functions alternating inside a round"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            got[k].append(event_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def wall(fn, reps=ROUNDS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_linkage.txt"))
    ap.add_argument("--no_vit", action="store_true", help="the clustering step only, no ViT-B/16 calls")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_linkage.py: no HIP device; nothing is measured without one")
    import scipy
    import sklearn
    from sklearn.cluster import AgglomerativeClustering
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, scikit-learn {sklearn.__version__}, scipy {scipy.__version__}, "
             f"{os.cpu_count()} host CPUs visible",
             f"kernel times: device events around {REPS} back-to-back launches, median [min .. max] of {ROUNDS} windows, the kernels alternating",
             f"step times: host clock around a call that ends in a device synchronise, median [min .. max] of {ROUNDS} calls; threshold {THRESHOLD}"]
    for D in (768, 1024):
        mask = masks_like(D)
        distance = (1 - vit_cx.get_cos_similar_matrix(mask, mask)).contiguous()
        m = D - 1
        ws = K.linkage_workspace(distance)
        out = torch.empty(3 * m + 4, dtype=torch.int32, device=DEV)
        children, heights, info = out[:2 * m], out[2 * m:3 * m].view(torch.float32), out[3 * m:]

        def host_step():
            c = AgglomerativeClustering(n_clusters=None, distance_threshold=THRESHOLD, metric="precomputed", linkage="complete")
            c.fit(distance.cpu())
            return c.labels_
        want = host_step()
        got_labels, n_clusters, _, _ = L.agglomerative_labels(distance, THRESHOLD)
        stats = L.linkage_device(distance)[2]
        lines.append(f"D = {D}: {n_clusters} clusters; K56 made {stats[1]} row scans and {stats[2]} pushes for {stats[3]} merges; labels equal to "
                     f"scikit-learn's: {bool(np.array_equal(want, got_labels))}")
        fns = {f"K56 copy + chain, {w:4d} lanes": (lambda w=w: K.linkage_complete(distance, ws, info, w)) for w in (64, 256, 1024)}
        fns["K57 sort + relabel"] = lambda: K.linkage_sort_relabel(D, ws, children, heights, info)
        for k, (med, lo, hi) in windows(fns).items():
            lines.append(f"  {k:34s} {med:9.4f} ms [{lo:.4f} .. {hi:.4f}]")
        for k, fn in (("device step (K56 + K57 + read-back + heapq cut)", lambda: L.agglomerative_labels(distance, THRESHOLD)),
                      ("  of which the host cut alone", None),
                      ("host step (.cpu() + AgglomerativeClustering.fit)", host_step),
                      ("  of which the .cpu() copy alone", lambda: distance.cpu())):
            if fn is None:
                c, h = L.complete_linkage(distance)
                t0 = time.perf_counter()
                for _ in range(ROUNDS):
                    L.hc_cut(c, h, THRESHOLD)
                lines.append(f"  {k:50s} {(time.perf_counter() - t0) / ROUNDS * 1e3:9.3f} ms")
                continue
            med, lo, hi = wall(fn)
            lines.append(f"  {k:50s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]")

    if not args.no_vit:
        from xai_engine.zoo import vit_base_patch16_224
        vit = vit_base_patch16_224(seed=0).to(DEV)
        x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(6))
        layer = vit.blocks[-1].norm1
        maps = {}
        lines.append("ViT_CX on ViT-B/16 (seed 0, random weights), one 3 x 224 x 224 image, device noise, gpu_batch 50, no feature-map download:")
        for which in vit_cx.CLUSTERINGS:
            def call(which=which):
                torch.manual_seed(6)
                return vit_cx.ViT_CX(vit, x, layer, device=DEV, device_noise=True, return_feature_map=False, clustering=which)[0]
            maps[which] = call()
            med, lo, hi = wall(call, 5)
            lines.append(f"  clustering = {which:8s} {med:9.2f} ms [{lo:.2f} .. {hi:.2f}]")
        lines.append(f"  maps equal: {bool(torch.equal(maps['sklearn'], maps['device']))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
