#!/usr/bin/env python3
"""Device k-means (K58-K61) for TIS at (n, d, k) = (9216, 196, 1024) and (9216, 49, 1024): one iteration of the device loop against
one iteration of the torch loop it can replace (the body of xai_engine/tis.py kmeans_centroids, its `float(err)` included) in the same
process, K59 and K60 + K61 alone, and on the encoder activations of ViT-B/16 (seed 0, random weights, one synthetic image) the
iterations both loops run and the whole TIS call with each setting.
    python profiles/bench_kmeans.py [--out profiles/r18_kmeans.txt]
Kernel times are device events around `REPS` back-to-back launches after a warm-up, the median of `ROUNDS` such windows and their
spread, the candidates alternating inside a round.  The torch iteration ends in a host read, so it and the whole calls are a host clock
around calls that end in a device synchronise, median of `ROUNDS`.  There is no CPU fallback: no device, no numbers."""
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
from xai_engine import kmeans as M  # noqa: E402
from xai_engine import tis  # noqa: E402

DEV = "cuda:0"
REPS, ROUNDS = 5, 7
NEVER = 1 << 30                     # a max_iter the windows never reach; with tol = -1 the loop never stops


def mixture(n, d, components=64, seed=0):
    """(n, d) fp32: `components` Gaussian centres of spread 1, noise 0.1"""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(components, d, generator=g)
    return (centres[torch.randint(0, components, (n,), generator=g)] + 0.1 * torch.randn(n, d, generator=g)).to(DEV).contiguous()


def torch_iteration(points, c, x_sq, n_clusters):
    """the body of tis.kmeans_centroids' loop, word for word -> (new centroids, err as the Python float the loop reads)"""
    n = points.shape[0]
    sim = 2 * points @ c.T - x_sq - (c * c).sum(1)[None]
    closest = sim.argmax(1)
    onehot = torch.zeros((n_clusters, n), dtype=points.dtype, device=points.device)
    onehot[closest, torch.arange(n, device=points.device)] = 1
    new = onehot @ points / onehot.sum(-1)[:, None]
    new[new != new] = 0
    err = (new - c).pow(2).sum()
    return new, float(err)


def torch_loop(points, first, max_iter=100, tol=1e-4):
    """tis.kmeans_centroids from given initial points -> (centroids, iterations run, last err)"""
    c = points[first].clone()
    x_sq = (points * points).sum(1, keepdim=True)
    for it in range(max_iter):
        c, err = torch_iteration(points, c, x_sq, len(first))
        if err <= tol:
            break
    return c, it + 1, err


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_kmeans.txt"))
    ap.add_argument("--no_vit", action="store_true", help="the k-means step only, no ViT-B/16 calls")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_kmeans.py: no HIP device; nothing is measured without one")
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {os.cpu_count()} host CPUs visible",
             f"kernel times: device events around {REPS} back-to-back launches, median [min .. max] of {ROUNDS} windows, the candidates alternating",
             f"torch iteration and whole calls: host clock around calls that end in a device synchronise, median [min .. max] of {ROUNDS}"]
    k = 1024
    for n, d in ((9216, 196), (9216, 49)):
        points = mixture(n, d)
        first = torch.from_numpy(np.random.RandomState(0).choice(n, size=[k], replace=False)).to(DEV)
        got, info = M.kmeans_device(points, k, first=first, return_info=True)
        want, t_iters, t_err = torch_loop(points, first)
        lines.append(f"(n, d, k) = ({n}, {d}, {k}), a 64-component mixture: the device loop runs {info['iterations']} iterations (err {info['err']:.3e}), "
                     f"the torch loop {t_iters} (err {t_err:.3e}); centroids max |difference| {float((got - want).abs().max()):.3e}")
        ws = K.kmeans_workspace(points, k)
        C = torch.empty((k, d), dtype=torch.float32, device=DEV)
        assign = torch.empty(n, dtype=torch.int32, device=DEV)
        counts = torch.empty(k, dtype=torch.int32, device=DEV)
        state = torch.empty(K.KMEANS_STATE_WORDS, dtype=torch.int32, device=DEV)
        K.kmeans_init(points, first, C, ws, state)
        fns = {"K58 init (xx, gather, cc)": lambda: K.kmeans_init(points, first, C, ws, state),
               "K59 assign": lambda: K.kmeans_assign(points, C, assign, ws, state),
               "K60 + K61 update": lambda: K.kmeans_update(points, C, assign, counts, ws, state, NEVER, -1.0),
               "one iteration (K59, K60, K61)": lambda: K.kmeans_iterate(points, C, assign, counts, ws, state, NEVER, -1.0, 1),
               "8 iterations in one call, per iteration": lambda: K.kmeans_iterate(points, C, assign, counts, ws, state, NEVER, -1.0, 8)}
        for name, (med, lo, hi) in windows(fns).items():
            per = 8 if name.startswith("8 ") else 1
            lines.append(f"  {name:42s} {med / per:9.4f} ms [{lo / per:.4f} .. {hi / per:.4f}]")
        assert int(state[1]) == 0                       # the timed launches were live ones: the loop had not stopped
        x_sq = (points * points).sum(1, keepdim=True)
        c0 = points[first].clone()
        med, lo, hi = wall(lambda: torch_iteration(points, c0, x_sq, k))
        lines.append(f"  {'torch iteration (with its float(err))':42s} {med:9.4f} ms [{lo:.4f} .. {hi:.4f}]")
        for name, fn in (("kmeans_device, whole call", lambda: M.kmeans_device(points, k, first=first)),
                         ("torch loop, whole call", lambda: torch_loop(points, first))):
            med, lo, hi = wall(fn)
            lines.append(f"  {name:42s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]")

    if not args.no_vit:
        from xai_engine.zoo import vit_base_patch16_224
        vit = vit_base_patch16_224(seed=0).to(DEV)
        x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(DEV)
        with torch.no_grad():
            _, acts = tis.TIS(vit).get_encoder_activations(x)
        channels = acts.squeeze(0)[1:].T.contiguous().float()
        n, d = channels.shape
        first = torch.from_numpy(np.random.RandomState(0).choice(n, size=[k], replace=False)).to(DEV)
        got, info = M.kmeans_device(channels, k, first=first, return_info=True)
        want, t_iters, t_err = torch_loop(channels, first)
        lines.append(f"encoder activations of ViT-B/16 (seed 0, random weights), one synthetic 3 x 224 x 224 image: channels ({n}, {d}), k = {k}")
        lines.append(f"  the device loop runs {info['iterations']} iterations (err {info['err']:.3e}), the torch loop {t_iters} (err {t_err:.3e}); "
                     f"empty clusters {int((info['counts'] == 0).sum())}; centroids max |difference| {float((got - want).abs().max()):.3e}")
        for name, fn in (("kmeans_device, whole call", lambda: M.kmeans_device(channels, k, first=first)),
                         ("torch loop, whole call", lambda: torch_loop(channels, first))):
            med, lo, hi = wall(fn)
            lines.append(f"  {name:42s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]")
        lines.append("  TIS(vit, n_masks=1024, batch_size=64)(x), the harness's call:")
        for which in tis.KMEANS:
            def call(which=which):
                np.random.seed(6)
                return tis.TIS(vit, n_masks=k, batch_size=64, kmeans=which)(x)
            med, lo, hi = wall(call, 5)
            lines.append(f"    kmeans = {which:8s} {med:9.2f} ms [{lo:.2f} .. {hi:.2f}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
