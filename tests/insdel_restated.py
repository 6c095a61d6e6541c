"""K8 (csrc/rank_kernels.hip), the flip-step map, K6, K10 and K9 (csrc/perturb_kernels.hip) restated on the host in numpy, with
the host code's launch plans, the scratch layout, a derived bound and the cases of the edge tests.  tests/test_cpu_insdel.py
checks all of it without a GPU, tests/test_gpu_insdel_edges.py holds the kernels to it.

What the kernel files promise and this module restates:
    K8    key = 0xFFFFFFFF for any NaN, -0.0 folded onto +0.0, then the sign flip; order = stable ascending argsort of the keys,
          rank its inverse; pass p (8-bit digit p of the key) is an identity pass exactly when every key of the map shares it
    flip  flip[p] = (descending ? hw - 1 - rank[p] : rank[p]) / step_size
    K6    out[k][c][p] = flip[p] <= first_step + k ? finish[c][p] : start[c][p], a move of bits
    K10   seg[t]: lane l adds elements lo + l, lo + l + 64, ... in sequence from +0, then a 6-level xor butterfly (offsets 32 .. 1);
          total: 1024 lanes with stride 1024, the butterfly per wave, the 16 wave partials padded with zeros to 64, the butterfly
          again -- every sum rounded to fp32 (-ffp-contract=off, no atomics)
    K9    p = exp(z - m) / sum, entropy = -sum p log2 p (0 * -inf kept as NaN), argmax = the first NaN, else the first maximum"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24                                 # unit roundoff of fp32
TILE, BINS, BLOCK, WAVE = 1024, 256, 256, 64
INT32_MAX = 2 ** 31 - 1


def bits(a):
    """fp32 values of uint32 bit patterns."""
    return np.ascontiguousarray(a, np.uint32).view(F32)


# ---- K8 --------------------------------------------------------------------------------------------------------------------------

def sort_key(sal):
    u = np.ascontiguousarray(sal, F32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)             # either sign, any payload
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)             # -0.0 ties with +0.0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(nan, np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def rank_expect(sal):
    """-> order, rank (int32) and flags (4,) uint32 of one map."""
    key = sort_key(np.ravel(sal))
    order = np.argsort(key, kind="stable").astype(np.int32)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size, dtype=np.int32)
    flags = np.array([int((((key >> np.uint32(8 * p)) & np.uint32(255)) == ((key[0] >> np.uint32(8 * p)) & np.uint32(255))).all())
                      for p in range(4)], np.uint32)
    return order, rank, flags


# the scratch layout, from the comment above front_words in rank_kernels.hip: front = [n_seg][8] identity flags (4 used), then
# [n_seg][4][tiles][256] histograms; behind it per map key0 key1 idx0 idx1 (hw words each) and offs [tiles][256]
def tiles_of(hw):
    return -(-hw // TILE)


def front_words(n_seg, n_tiles):
    return n_seg * (8 + 4 * BINS * n_tiles)


def seg_words(hw, n_tiles):
    return 4 * hw + BINS * n_tiles


def workspace_bytes(n_seg, hw):
    nt = tiles_of(hw)
    return (front_words(n_seg, nt) + n_seg * seg_words(hw, nt)) * 4


def flag_words(ws_words, seg):
    """The four identity flags of segment `seg` in a workspace read back as uint32 words: ws[seg * 8 + pass]."""
    return np.asarray(ws_words[seg * 8:seg * 8 + 4], np.uint32)


def zero_fill_strided(n_seg, hw):
    """Share of the front words that rank_zero_kernel reaches through its grid stride (a grid of at most 1024 x 256 lanes)."""
    fw = front_words(n_seg, tiles_of(hw))
    return max(0, fw - 1024 * BLOCK) / fw


RANK_HW = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 7169, 8192, 8193, 16389)
PATTERNS = tuple(tuple((n >> (3 - p)) & 1 for p in range(4)) for n in range(16))       # (flag of pass 0, .., pass 3)
# top key bytes whose floats are finite whatever the lower bytes hold: 0x00 and 0xFF reach inf / NaN, 0x7F reaches -0.0
TOP_BYTES = np.array(list(range(0x01, 0x7F)) + list(range(0x80, 0xFF)), np.uint32)


def key_to_bits(key):
    key = np.asarray(key, np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)


def pattern_map(hw, flags, rng):
    """A finite map of hw >= 2 values whose pass p is an identity pass exactly where flags[p]: an identity byte is one value, a
    real byte takes 2, 5 or up to 256 values placed at random over the whole map (its two ends always differ)."""
    assert hw >= 2
    key = np.zeros(hw, np.uint32)
    for p in range(4):
        allowed = TOP_BYTES if p == 3 else np.arange(256, dtype=np.uint32)
        if flags[p]:
            b = np.full(hw, rng.choice(allowed), np.uint32)
        else:
            vals = rng.choice(allowed, size=(2, 5, 256)[int(rng.integers(3))] if p < 3 else (2, 5, 200)[int(rng.integers(3))], replace=False)
            b = rng.choice(vals, size=hw).astype(np.uint32)
            b[0], b[-1] = max(vals[:2]), min(vals[:2])          # the last key sorts before the first: out of a last tile of one
        key |= b << np.uint32(8 * p)
    return bits(key_to_bits(key))


SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC0DEAD, 0xFF812345,          # NaNs: both signs, payloads
                     0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32)
N_NAN = 6


def _zeros(hw, rng):
    return np.zeros(hw, F32)


def _last_smaller(hw, rng):
    m = np.full(hw, 1.0, F32)
    m[-1] = 0.5
    return m


def _zero_one(hw, rng):
    return rng.integers(0, 2, hw).astype(F32)


def _small_int(hw, rng):
    return rng.integers(0, 10, hw).astype(F32)


def _one_two(hw, rng):
    return bits(np.uint32(0x3F800000) | rng.integers(0, 1 << 23, hw).astype(np.uint32))


def _quarters(hw, rng):
    m = bits(np.uint32(0x40800000) | (rng.integers(0, 16, hw).astype(np.uint32) << np.uint32(19)))
    if hw >= 2:
        m[0], m[-1] = 4.0, 7.75
    return m


def _ascending(hw, rng):
    return np.sort(rng.standard_normal(hw).astype(F32))


def _descending_ties(hw, rng):
    return np.sort(np.round(rng.standard_normal(hw) * 4).astype(F32) / F32(4))[::-1].copy()


def _mostly_equal(hw, rng):
    m = np.full(hw, 0.25, F32)
    loose = rng.random(hw) < 0.1
    m[loose] = rng.standard_normal(int(loose.sum())).astype(F32)
    return m


def _specials(hw, rng):
    m = rng.standard_normal(hw).astype(F32)
    u = m.view(np.uint32)
    sp = SPECIALS[rng.permutation(len(SPECIALS))]
    if hw <= len(sp):
        u[:] = sp[:hw]
    else:                                                   # the two ends, and twice over at random places
        where = np.concatenate([[0, hw - 1], rng.choice(np.arange(1, hw - 1), size=min(hw - 2, 2 * len(sp) - 2), replace=False)])
        u[where] = np.resize(sp, where.size)
    return m


FAMILIES = {"zeros": _zeros, "last_smaller": _last_smaller, "zero_one": _zero_one, "small_int": _small_int, "one_two": _one_two,
            "quarters": _quarters, "ascending": _ascending, "descending_ties": _descending_ties, "mostly_equal": _mostly_equal,
            "specials": _specials}


def pattern_name(flags):
    return "p" + "".join(map(str, flags))


def rank_case(hw, seed=0):
    """-> names, maps (n_seg, hw): the named families and, for hw >= 2, the 16 pattern maps -- the segments of one K8 call."""
    names, maps = [], []
    for k, (name, make) in enumerate(FAMILIES.items()):
        names.append(name)
        maps.append(make(hw, np.random.default_rng([8, hw, seed, k])))
    if hw >= 2:
        for k, flags in enumerate(PATTERNS):
            names.append(pattern_name(flags))
            maps.append(pattern_map(hw, flags, np.random.default_rng([88, hw, seed, k])))
    return names, np.stack(maps).astype(F32)


STRIDED_CALL = (64, 16389)       # (n_seg, hw): 17 tiles, a last tile of 5 keys, a front of 1 114 624 words of which 76 % are strided


def strided_case():
    n_seg, hw = STRIDED_CALL
    maps = np.concatenate([rank_case(hw, seed)[1] for seed in range(1, 4)])
    return maps[:n_seg]


# ---- flip ------------------------------------------------------------------------------------------------------------------------

FLIP_HW = (1, 255, 256, 257)


def flip_of(rank, descending, step):
    rank = np.asarray(rank, np.int64)
    pos = rank.size - 1 - rank if descending else rank
    return (pos // step).astype(np.int32)


# ---- K6 --------------------------------------------------------------------------------------------------------------------------

HBM_BYTES = 64 << 20


def perturb_plan(C, hw, n_batch, aligned=True):
    """xai_perturb_batch_f32's launch: vec (the float4 flavour), per (step images per chunk), chunks (grid y), zdim (grid z)."""
    vec = hw % 4 == 0 and aligned
    tiles = -(-hw // (BLOCK * (4 if vec else 1)))
    zdim = 1
    if n_batch * C * hw * 4 >= HBM_BYTES and C <= 64:
        per, zdim = (2 if n_batch >= 2 else 1), C
    else:
        c0 = min(n_batch, max(1, -(-2048 // tiles)))
        per = -(-n_batch // c0)
    return vec, per, -(-n_batch // per), zdim


def images(start, finish, flip, first, n):
    """(n, C, hw) int32 words: image k holds finish where flip <= first + k, else start."""
    s = np.ascontiguousarray(start, F32).view(np.int32)
    f = np.ascontiguousarray(finish, F32).view(np.int32)
    t = (first + np.arange(n, dtype=np.int64))[:, None, None]
    return np.where(np.asarray(flip, np.int64)[None, None, :] <= t, f[None], s[None])


def k6_values(C, hw, seed):
    """start, finish (C, hw): N(0, 1) with NaNs of distinct payloads, +-0.0, +-inf and denormals among them, no word of start
    equal to the word of finish at its place."""
    rng = np.random.default_rng([6, C, hw, seed])
    out = []
    for side in range(2):
        m = rng.standard_normal((C, hw)).astype(F32)
        u = m.view(np.uint32).ravel()
        n = min(u.size, 3 * len(SPECIALS))
        where = rng.choice(u.size, size=n, replace=False)
        u[where] = np.resize(SPECIALS, n) + np.uint32(side) * np.where(np.resize(np.arange(len(SPECIALS)), n) < N_NAN, np.uint32(0x100), np.uint32(0))
        out.append(m)
    same = out[0].view(np.uint32) == out[1].view(np.uint32)
    out[1].view(np.uint32)[same] ^= np.uint32(0x00400001)
    return out[0], out[1]


def k6_flip(hw, first, n, seed):
    """flip (hw,) int32: every step of the batch, the steps around it, -1, 0, values beyond the last step and INT32_MAX."""
    rng = np.random.default_rng([66, hw, first, n, seed])
    f = rng.integers(max(-1, first - 2), first + n + 2, hw).astype(np.int32)
    must = np.array([-1, 0, first, first + n - 1, first + n, first + n + 1000, INT32_MAX, first + n // 2], np.int32)
    where = rng.choice(hw, size=min(hw, must.size), replace=False)
    f[where] = must[:where.size]
    return f


# (C, hw, n_batch, first_step) -> what it is there for; the plan of each is pinned in tests/test_cpu_insdel.py
K6_SMALL = (
    (3, 4, 1, 0), (3, 4, 2049, 0),                # one float4 lane; n_batch > 2048 on one tile: per = 2, a last chunk of one
    (3, 5, 1, 0), (3, 5, 2049, 3),                # the scalar flavour of the same
    (3, 3000, 1009, 5),                           # 3 tiles, c0 = 683: a prime n_batch, per = 2, a last chunk of one, first_step > 0
    (2, 1021, 13, 7),                             # hw and n_batch prime, scalar, per = 1
    (1, 2048 * 256 + 1, 3, 0),                    # scalar with 2049 tiles: ceil(2048 / tiles) = 1, one chunk of all three
    (1, 2047 * 256, 3, 1),                        # scalar (misaligned below) with 2047 tiles: c0 = 2, per = 2
)
K6_HBM = (
    (4, 4096, 1024, 0),                           # exactly 64 MiB: one channel per lane, per = 2
    (4, 4096, 1023, 2),                           # one image smaller: all channels per lane
    (64, 1024, 256, 0),                           # 64 MiB at C = 64: the HBM branch
    (65, 1024, 256, 0),                           # C = 65: not
    (4, 4096, 1025, 1),                           # the HBM branch with an odd n_batch: a last chunk of one
    (3, 4099, 1365, 0),                           # the HBM branch with the scalar flavour (hw odd), odd n_batch
)
K6_REFUSED = (1, 132, 131071)                     # 69 205 488 bytes: HBM branch, per = 2, 65 536 chunks


# ---- K10 -------------------------------------------------------------------------------------------------------------------------

K10_CASES = ((1, 1, 1), (99, 7, 15), (1000, 1, 1000), (1024, 64, 16), (1025, 64, 17), (2500, 63, 40), (5000, 65, 77), (50176, 224, 224),
             (3000, 3000, 1))                      # (hw, step_size, n_steps)


def k10_map(hw, seed=0):
    """|values| in [0.5, 2] with random signs: one element is orders of magnitude above segment_bound."""
    rng = np.random.default_rng([10, hw, seed])
    return (rng.uniform(0.5, 2.0, hw) * rng.choice([-1.0, 1.0], hw)).astype(F32)


def butterfly(v):
    """wave_sum: v += v[lane ^ off] for off = 32 .. 1 over the last axis (64 lanes), each sum rounded to fp32; lane 0's value."""
    v = np.asarray(v, F32)
    lane = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ off]).astype(F32)
    return v[..., 0]


def lane_partials(vals, lanes):
    """Lane l of `lanes` adds vals[l], vals[l + lanes], ... in sequence from +0.  (Padding with +0 changes nothing: an
    accumulator that started at +0 is never -0.)"""
    vals = np.asarray(vals, F32)
    rows = -(-vals.size // lanes)
    m = np.zeros(rows * lanes, F32)
    m[:vals.size] = vals
    acc = np.zeros(lanes, F32)
    for r in m.reshape(rows, lanes):
        acc = (acc + r).astype(F32)
    return acc


def segment_indices(order, descending, step, n_steps):
    """The elements of sal each segment adds, in the kernel's order of i: order[hw - 1 - i] for a descending call."""
    order = np.asarray(order, np.int64)
    walk = order[::-1] if descending else order
    return [walk[t * step:min((t + 1) * step, order.size)] for t in range(n_steps)]


def segment_sums32(sal, order, descending, step, n_steps):
    """-> seg (n_steps,) fp32, total fp32: K10 in its own order of additions."""
    sal = np.asarray(sal, F32).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        seg = np.array([butterfly(lane_partials(sal[idx], WAVE)) for idx in segment_indices(order, descending, step, n_steps)], F32)
        waves = butterfly(lane_partials(sal, 1024).reshape(16, WAVE))
        total = butterfly(np.concatenate([waves, np.zeros(WAVE - 16, F32)]))
    return seg, F32(total)


def gamma(d):
    return d * U32 / (1 - d * U32)


def segment_bound(sal, idx, total=False):
    """|fp32 tree - exact sum| <= gamma_d * sum |x| over the n elements sal[idx], gamma_d = d u / (1 - d u), u = 2^-24.

    Every fp32 addition returns (a + b)(1 + e) with |e| <= u, so the computed sum is sum x_i (1 + t_i) with
    (1 - u)^k <= 1 + t_i <= (1 + u)^k, k the number of additions x_i passes through, and |t_i| <= gamma_k (Higham, Accuracy
    and Stability of Numerical Algorithms, lemma 3.1).  In a segment an element joins its lane's accumulator (ceil(n / 64)
    additions at most in that lane, the first onto +0 exact) and then rides through the 6 levels of the butterfly:
    d = ceil(n / 64) + 6.  In the total it joins one of 1024 lanes (ceil(n / 1024) additions), rides the 6 levels of its
    wave's butterfly and the 6 levels of the butterfly over the wave partials (the padding zeros add exactly):
    d = ceil(n / 1024) + 12.  Nothing is fitted; both count one addition more than the worst path has."""
    x = np.asarray(sal, F32).ravel()[np.asarray(idx, np.int64)]
    n = x.size
    d = -(-n // 1024) + 12 if total else -(-n // WAVE) + 6
    return gamma(d) * math.fsum(abs(float(v)) for v in x)


def exact_sum(sal, idx):
    return math.fsum(float(v) for v in np.asarray(sal, F32).ravel()[np.asarray(idx, np.int64)])


# ---- K9 --------------------------------------------------------------------------------------------------------------------------

K9_K = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
K9_B = (1, 3, 4, 5, 9)
K9_SCALES = (0.5, 3.0, 30.0)
# Tolerances of the value comparisons, rel_inf against softmax_expect: twice the largest error measured on an MI355X over all of
# K9_K x K9_B -- 7.3179e-08 for p, 2.1017e-07 for the entropy (profiles/insdel_edges_parity.json; tests/test_cpu_insdel.py ties
# these figures to that file) -- rounded down, far below the 1e-5 bar.
K9_TOL = {"p": 1.4635e-07, "entropy": 4.2032e-07}


def argmax_rule(row):
    row = np.asarray(row)
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def softmax_expect(z, target):
    """z (B, K) fp32, target an int or (B,) ints (< 0: the row's argmax; >= K: NaN) -> p (B,), entropy in bits (B,), argmax (B,),
    in fp64 from the fp32 logits."""
    z32 = np.asarray(z, F32)
    B, K = z32.shape
    am = np.array([argmax_rule(r) for r in z32], np.int32)
    z = z32.astype(F64)
    tgt = np.broadcast_to(np.asarray(target, np.int64), (B,)).copy()
    tgt[tgt < 0] = am[tgt < 0]
    with np.errstate(all="ignore"):
        e = np.exp(z - z[np.arange(B), am][:, None])
        p = e / e.sum(axis=1, keepdims=True)
        ent = -(p * np.log2(p)).sum(axis=1)
    pt = np.where(tgt < K, p[np.arange(B), np.minimum(tgt, K - 1)], np.nan)
    return pt, ent, am


def k9_logits(B, K, seed=0):
    """N(0, 1) clipped to +-1.3, row r scaled by K9_SCALES[r % 3]: z - max stays above -78, so exp(z - max) is a normal fp32
    number in every row (below -87 it leaves the normal range, p reaches 0 and the fp32 entropy is NaN where fp64 has a value:
    the rule the special rows pin, not a value to compare)."""
    rng = np.random.default_rng([9, B, K, seed])
    z = np.clip(rng.standard_normal((B, K)), -1.3, 1.3)
    return (z * np.array(K9_SCALES)[np.arange(B) % 3][:, None]).astype(F32)


def k9_special_rows(K=200):
    """name -> (row, argmax): the NaN and tie rows of the GPU test."""
    rng = np.random.default_rng([99, K])
    base = lambda: rng.standard_normal(K).astype(F32)               # noqa: E731
    rows = {}
    r = base(); r[70] = np.nan; r[131] = np.nan                     # lane 6 holds index 70, lane 3 the later 131
    rows["nan_70_131"] = (r, 70)
    r = base(); r[131] = np.nan; r[5] = 99.0
    rows["nan_beats_max"] = (r, 131)
    r = base(); r[17] = r[17 + 64] = 9.0                            # the same lane, two rounds
    rows["tie_j_j64"] = (r, 17)
    r = base(); r[65] = r[2] = 9.0                                  # lane 1 holds the later index
    rows["tie_65_2"] = (r, 2)
    r = base(); r[130] = r[3] = r[67] = 9.0
    rows["tie_three"] = (r, 3)
    rows["all_neg_inf"] = (np.full(K, -np.inf, F32), 0)
    r = base(); r[40] = np.inf; r[100] = np.inf
    rows["two_pos_inf"] = (r, 40)
    r = base(); r[::3] = -np.inf
    rows["some_neg_inf"] = (r, argmax_rule(r))
    r = base(); r[150] = 300.0
    rows["saturated"] = (r, 150)
    rows["constant"] = (np.full(K, 1.5, F32), 0)
    return rows


def ledger_names():
    return sorted(f"insdel_edges/softmax_{what}/K{K}" for what in ("p", "entropy") for K in K9_K)
