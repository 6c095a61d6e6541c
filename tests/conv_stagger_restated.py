"""The staggered start of a K loop (csrc/xai_conv_walk.h: xai_stagger_plan, xai_stagger_first, xai_stagger_block) restated in Python,
and the sum it orders, for tests/test_cpu_conv_wide.py (which holds the planner to the restatement on the host) and
tests/test_gpu_conv1x1_bwd_wide_edges.py (which holds K81 to the emulation and K80 and K81 to the bound).

A stagger is (depth, tile, axis, n, stride).  The K loop runs iters = K / depth iterations of depth / 16 K-blocks each.  shift is the
largest s >= 0 with 4 * depth * 2^s <= stride (0 if there is none); su is n halved until su << shift <= iters or su <= 1; mask = su - 1
(0 for su = 0), and shift counts as 0 where mask is 0.  The output at `at` along the axis lies in tile w = at // tile and starts at
iteration ((w & mask) << shift), goes up to the last iteration, wraps, and ends with the iteration before its first.

The bound is conv_walk_restated.bound's for one partial sum of all K terms: the start only moves roundings around inside the
chain."""
import numpy as np

import conv_walk_restated as R

COLUMNS, ROWS = 0, 1


def plan(K, depth, tile, axis, n, stride):
    """-> (blocks, per_iter, tile, axis, mask, shift), or None where the planner refuses"""
    if K < 16 or depth < 16 or depth % 16 or K % depth or tile < 16 or tile % 16:
        return None
    if axis not in (COLUMNS, ROWS) or n < 0 or n & (n - 1) or stride < 0:
        return None
    iters = K // depth
    shift = 0
    while 4 * depth * 2 ** (shift + 1) <= stride:
        shift += 1
    su = n
    while su > 1 and iters < su << shift:
        su //= 2
    mask = su - 1 if su >= 1 else 0
    return (K // 16, depth // 16, tile, axis, mask, shift if mask else 0)


def chain(p, at):
    """the K-blocks of the output at `at` along the axis, in the order in which they are added"""
    blocks, per_iter, tile, _, mask, shift = p
    first = (((at // tile) & mask) << shift) * per_iter
    return [(first + t) % blocks for t in range(blocks)]


def emulate(gy, w, grouping, from_zero, p):
    """gy (K, P), w (K, C) fp32 -> gx (C, P) fp32, every fma rounded once (as conv_walk_restated.emulate), the chain per tile"""
    C, P = w.shape[1], gy.shape[1]
    gd, wd = gy.astype(np.float64), w.astype(np.float64)
    out = np.zeros((C, P), np.float32)
    extent = C if p[3] == ROWS else P
    for lo in range(0, extent, 16):                         # 16 | tile: one chain per 16 outputs along the axis
        rows, cols = (slice(lo, lo + 16), slice(None)) if p[3] == ROWS else (slice(None), slice(lo, lo + 16))
        acc = np.zeros_like(out[rows, cols])
        for b in chain(p, lo):
            for m in range(4):
                for q in range(4):
                    k = b * 16 + R.k_of(grouping, m, q)
                    acc = (acc.astype(np.float64) + wd[k][rows, None] * gd[k][None, cols]).astype(np.float32)
        out[rows, cols] = (np.zeros_like(acc) + acc) if from_zero else acc
    return out


def bound(K, abs_sum):
    return R.bound(K, 1, R.CONTIGUOUS, R.ASCENDING, abs_sum)
