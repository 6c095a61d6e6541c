"""The K-walk of csrc/xai_conv_walk.h restated in Python, and the forward-error bound of a sum walked by it, for
tests/test_cpu_conv_walk.py (which holds the planner to the restatement on the host) and tests/test_gpu_conv1x1_bwd_edges.py
(which holds K78 and K79 to the bound).

A walk is (splits S, membership, grouping, order, from_zero).  K is cut into nb = K / 16 blocks; q, r = divmod(nb, S); partial sum s
owns q + (s < r) blocks, contiguous (s*q + min(s, r) onwards) or round robin (s, s + S, ...); the partial sums are added ascending
or descending, starting from the first of them or from +0.

The bound.  Per output element, partial sum s is the fmaf chain acc <- fma(a_k, b_k, acc) from +0 over its n_s = 16 * count_s terms
in some order: one rounding per fma, each term passing through at most n_s of them.  The partial sums are then added one after the other: S - 1 roundings (adding the first to +0 is exact).  A term therefore
carries at most n_max + S - 1 factors (1 + d), |d| <= u = 2^-24, with n_max = 16 * max_s count_s, and by Higham's Lemma 3.1
    |computed - exact| <= gamma(n_max + S - 1) * sum_k |gy_k| |w_k|,        gamma(n) = n u / (1 - n u).
The grouping and the order move roundings around inside that count and do not enter.  The fp64 sum the tests compare with has
an error of its own of at most gamma64(K) * sum_k |gy_k| |w_k| with u64 = 2^-53, which `bound` adds."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
BLOCK = 16
MAX_SPLITS = 32
CONTIGUOUS, ROUND_ROBIN = 0, 1
CONSECUTIVE, STRIDE4 = 0, 1
ASCENDING, DESCENDING = 0, 1


def parts(K, S, membership, order):
    """[[block, ...] per partial sum, in adding order]"""
    nb = K // BLOCK
    q, r = divmod(nb, S)
    out = []
    for s in range(S):
        count = q + (s < r)
        if membership == CONTIGUOUS:
            first = s * q + min(s, r)
            out.append(list(range(first, first + count)))
        else:
            out.append([s + t * S for t in range(count)])
    return out[::-1] if order == DESCENDING else out


def k_of(grouping, m, q):
    return m + 4 * q if grouping == STRIDE4 else 4 * m + q


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def bound(K, S, membership, order, abs_sum):
    """abs_sum: sum_k |gy_k| |w_k| per output element (fp64) -> the largest |computed - fp64 sum| the walk allows"""
    n_max = BLOCK * max(len(p) for p in parts(K, S, membership, order))
    return (gamma(n_max + S - 1) + gamma(K, U64)) * abs_sum


def emulate(gy, w, walk):
    """gy (K, P), w (K, C) fp32 -> gx (C, P) fp32 by the walk, every fma rounded once (the product of two fp32 is exact in fp64; the
    fp64 sum is rounded to fp32 -- a second rounding that matters only on a tie of the first, which random data does not meet)"""
    S, membership, grouping, order, from_zero = walk
    K = gy.shape[0]
    gd, wd = gy.astype(np.float64), w.astype(np.float64)
    total = None
    for blocks in parts(K, S, membership, order):
        acc = np.zeros((w.shape[1], gy.shape[1]), np.float32)
        for b in blocks:
            for m in range(4):
                for q in range(4):
                    k = b * BLOCK + k_of(grouping, m, q)
                    acc = (acc.astype(np.float64) + wd[k][:, None] * gd[k][None, :]).astype(np.float32)
        if total is None:
            total = (np.zeros_like(acc) + acc) if from_zero else acc
        else:
            total = (total + acc).astype(np.float32)
    return total
