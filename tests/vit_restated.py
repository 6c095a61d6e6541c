"""K17-K21 (csrc/vit_kernels.hip: head_importance_tiles_kernel + head_importance_finish_kernel, rave_matrices_kernel,
rollout_row_kernel, residual_shares_kernel, attn_cam_kernel) restated in NumPy, for tests/test_cpu_vit.py (which proves the
restatements on the host) and tests/test_gpu_vit_edges.py (which holds the kernels to them).

Per kernel: the kernel's own arithmetic in the kernel's own order, every operation rounded to fp32 (`*_fp32`: the kernel must
return these BITS); the definition in float64 from the fp32 inputs (`*64`); a derived element-wise bound on the distance between
the two (`*_bound`); the cells at which the launch geometry changes; seeded inputs (`normal_case`), integer inputs on which every
order of addition is exact (`exact_case`, K17 / K19 / K21) and the degenerate values the reference defines (the named makers at
the end).  The file is built with -ffp-contract=off, so every a * b + c written in C++ rounds twice; only the MFMA of K17 fuses.

NaN: the reference's torch.max / clamp / min / F.normalize carry a NaN to their result, C's fmaxf / fminf return the other operand.
The kernels follow the REFERENCE (max_nan, relu_nan and the NaN flag of K21 in vit_kernels.hip), and so do the restatements:
np.maximum / np.minimum / ndarray.min / .max all propagate."""
from collections import namedtuple

import numpy as np

from insdel_restated import butterfly
from maskers_restated import fma32

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                      # unit roundoff of fp32
WAVE = 64
TILE, K17_WAVES = 32, 4             # kTile, kK17Waves
ROLL_WAVES = 16                     # kRollWaves
CAM_THREADS = 1024                  # kCamThreads
K17_MAX_LH, K17_MAX_S = 4096, 4096
K19_LDS_CAP = 160 * 1024
# v_mfma_f32_32x32x2_f32 adds the products of its two k to the accumulator as a chain of fused multiply-adds; this is the order
# of the two inside one instruction (k0 + 0 first).  With the k-steps ascending the whole tile is one fmaf chain, k = 0 .. S-1.
MFMA_K_ORDER = (0, 1)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): a product of n factors (1 + d_i)^(+-1), |d_i| <= u, is 1 + t with |t| <= gamma_n."""
    return n * U / (1.0 - n * U)


def lane_sum(x):
    """Sum over the last axis as a wave does it: lane l adds x[l], x[l + 64], ... ascending from +0, then the xor butterfly.
    Lanes past the end keep +0 (padding with +0 changes nothing: an accumulator that started at +0 is never -0)."""
    x = np.asarray(x, F32)
    n = x.shape[-1]
    rows = -(-n // WAVE)
    pad = np.zeros(x.shape[:-1] + (rows * WAVE,), F32)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (rows, WAVE))
    acc = np.zeros(x.shape[:-1] + (WAVE,), F32)
    for r in range(rows):
        acc = acc + pad[..., r, :]
    assert acc.dtype == F32
    return butterfly(acc)


def lane_rows(n):
    """additions of lane_sum on the longest path: ceil(n / 64) in the lane, 6 in the butterfly"""
    return -(-n // WAVE) + 6


def relu_nan(x):
    """relu_nan of vit_kernels.hip: NaN stays, everything not above 0 becomes +0.0 (torch.clamp(min=0))"""
    return np.where(np.isnan(x), x, np.where(x > 0, x, F32(0))).astype(F32)


# ---- geometry --------------------------------------------------------------------------------------------------------------------

def k17_tiles(S):
    t = -(-S // TILE)
    return t * t


def k17_workspace_bytes(L, H, S):
    return 0 if min(L, H, S) <= 0 else 4 * L * H * k17_tiles(S)


def k17_grid(L, H, S):
    """-> (workgroups per block-head, idle waves of the last one)"""
    wgs = -(-k17_tiles(S) // K17_WAVES)
    return wgs, wgs * K17_WAVES - k17_tiles(S)


def k19_lds_bytes(S):
    return (ROLL_WAVES + 1) * S * 4


K19_MAX_S = K19_LDS_CAP // ((ROLL_WAVES + 1) * 4)        # 2409


def k19_kc(S):
    return -(-S // ROLL_WAVES)


# ---- K17 -------------------------------------------------------------------------------------------------------------------------

def head_importance_parts_fp32(A, G, k_descending=False, sum_before_abs=False):
    """A, G (L, H, S, S) -> the K17 workspace (L * H, tiles): per 32 x 32 tile of A_h^T G_h the accumulator is the fmaf chain
    acc = fma(A[k][i], G[k][j], acc) over k ascending from 0 (rows / columns / k past S are exact zeros and leave it unchanged);
    lane (half, j) adds |acc[i][j]| over registers r = 0 .. 15 from +0, i = 8 (r / 4) + 4 half + r % 4; then the butterfly.
    A plane that holds a NaN gives NaN partials (every product chain of the plane meets it in some tile; see nan_gradient_case)."""
    A, G = np.asarray(A, F32), np.asarray(G, F32)
    L, H, S, _ = A.shape
    A, G = A.reshape(L * H, S, S), G.reshape(L * H, S, S)
    bad = np.isnan(A).any(axis=(1, 2)) | np.isnan(G).any(axis=(1, 2))
    assert np.isfinite(A[~bad]).all() and np.isfinite(G[~bad]).all()
    A, G = np.where(bad[:, None, None], F32(0), A), np.where(bad[:, None, None], F32(0), G)
    nt = -(-S // TILE)
    ks = [k0 + kk for k0 in range(0, S + 1, 2) for kk in MFMA_K_ORDER if k0 + kk < S]
    acc = np.zeros((L * H, S, S), F32)
    for k in (ks[::-1] if k_descending else ks):
        acc = fma32(A[:, k, :, None], G[:, k, None, :], acc)
    full = np.zeros((L * H, nt * TILE, nt * TILE), F32)
    full[:, :S, :S] = acc if sum_before_abs else np.abs(acc)
    tiles = full.reshape(L * H, nt, TILE, nt, TILE).transpose(0, 1, 3, 2, 4)      # (LH, ti, tj, i, j)
    lanes = np.zeros((L * H, nt, nt, 2, TILE), F32)                                # lane = 32 half + j
    for r in range(16):
        for half in (0, 1):
            lanes[..., half, :] = lanes[..., half, :] + tiles[..., 8 * (r // 4) + 4 * half + r % 4, :]
    part = butterfly(lanes.reshape(L * H, nt * nt, WAVE))
    if sum_before_abs:
        part = np.abs(part)
    part[bad] = np.nan
    return part


def head_importance_finish_fp32(part, L, H, S):
    """(L * H, tiles) -> Ih (L, H): tile partials from +0 in tile order, / (float(S) * float(S)), the head total from +0 in h
    order, a true division"""
    part = np.asarray(part, F32)
    s = np.zeros(L * H, F32)
    for t in range(part.shape[1]):
        s = s + part[:, t]
    mean = (s / (F32(S) * F32(S))).reshape(L, H)
    tot = np.zeros(L, F32)
    for h in range(H):
        tot = tot + mean[:, h]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = mean / tot[:, None]
    assert out.dtype == F32
    return out


def head_importance_fp32(A, G, **mutant):
    A = np.asarray(A, F32)
    L, H, S, _ = A.shape
    return head_importance_finish_fp32(head_importance_parts_fp32(A, G, **mutant), L, H, S)


def head_importance64(A, G):
    A, G = np.asarray(A, F64), np.asarray(G, F64)
    m = np.abs(np.einsum("lhki,lhkj->lhij", A, G)).mean(axis=(2, 3))
    return m / m.sum(axis=1, keepdims=True)


def head_importance_bound(A, G):
    """(L, H): |head_importance_fp32 - head_importance64| <= this, for finite data.

    Entry.  acc_ij is an fmaf chain of S steps: acc^ = sum_k a_ki g_kj (1 + t), |t| <= gamma_S, so |acc^ - acc| <= gamma_S P_ij
    with P = |A|^T |G|.  Mean.  |acc^_ij| then passes 16 additions in the lane (the first to 0 counted all the same), 6 in the
    butterfly, tiles additions in the finish kernel and one division by the exact S^2: n2 = 16 + 6 + tiles + 1 more factors, all on
    non-negative terms.  |m^ - m| <= (gamma_S (1 + gamma_n2) + gamma_n2) mean(P) <= gamma_(S + n2) mean(P) =: e   (|acc| <= P).
    Total.  tot^ = sum_h m^_h (1 + t_H): |tot^ - tot| <= (1 + gamma_H) sum_h e_h + gamma_H tot =: E.
    Quotient.  |m^ / tot^ - m / tot| = |(m^ - m) tot - m (tot^ - tot)| / (tot tot^) <= (e tot + m E) / (tot (tot - E)), and the
    division adds one rounding of the result.  tot <= E (a block whose products cancel to rounding level) gives an infinite bound."""
    A, G = np.asarray(A, F64), np.asarray(G, F64)
    L, H, S, _ = A.shape
    n2 = 16 + 6 + k17_tiles(S) + 1
    P = np.einsum("lhki,lhkj->lhij", np.abs(A), np.abs(G)).mean(axis=(2, 3))
    m = np.abs(np.einsum("lhki,lhkj->lhij", A, G)).mean(axis=(2, 3))
    tot = m.sum(axis=1, keepdims=True)
    e = gamma(S + n2) * P
    E = (1 + gamma(H)) * e.sum(axis=1, keepdims=True) + gamma(H) * tot
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(tot > E, (e * tot + m * E) / (tot * (tot - E)), np.inf)
        return b + U * (m / tot + b)


# ---- K20 -------------------------------------------------------------------------------------------------------------------------

def residual_shares_fp32(xs, ats, rs, ms, squared=False):
    """four (L, S, D) streams -> b1, b2 (L, 2, S): per token the lane sum of fl(x * x), sqrtf, d = max(q0 + q1, 1e-12) (NaN
    carried), true divisions"""
    q = []
    with np.errstate(invalid="ignore"):
        for x in (xs, ats, rs, ms):
            x = np.asarray(x, F32)
            s = lane_sum(x * x)
            q.append(s if squared else np.sqrt(s))
        out = []
        for a, b in ((q[0], q[1]), (q[2], q[3])):
            d = np.maximum(a + b, F32(1e-12))
            out.append(np.stack((a / d, b / d), axis=1))
    assert out[0].dtype == F32 and out[1].dtype == F32
    return out[0], out[1]


def residual_shares64(xs, ats, rs, ms):
    q = [np.sqrt((np.asarray(x, F64) ** 2).sum(axis=-1)) for x in (xs, ats, rs, ms)]
    out = []
    for a, b in ((q[0], q[1]), (q[2], q[3])):
        d = np.maximum(a + b, 1e-12)
        out.append(np.stack((a / d, b / d), axis=1))
    return out[0], out[1]


def residual_shares_bound(xs, ats, rs, ms):
    """-> bounds for b1, b2.  A sum of squares carries n = 1 (the product) + ceil(D / 64) + 6 roundings on non-negative terms:
    s^ = s (1 + t_n); sqrtf halves that and adds one: q^ = q (1 + t), |t| <= gamma_(n + 1).  d^ = (q0^ + q1^)(1 + d) = d (1 +
    t_(n + 2)); the quotient (1 + t_(n + 1)) / (1 + t_(n + 2)) (1 + d): |share^ - share| <= gamma_(2 n + 4) share.  A token whose
    two norms are 0 is 0 / 1e-12 = 0 in both (bound 0); squares of these magnitudes do not underflow."""
    D = np.asarray(xs).shape[-1]
    n = 1 + lane_rows(D)
    b1, b2 = residual_shares64(xs, ats, rs, ms)
    return gamma(2 * n + 4) * b1, gamma(2 * n + 4) * b2


# ---- K18 -------------------------------------------------------------------------------------------------------------------------

def rave_matrices_fp32(A, Ih, b1, b2, Gb=None, ablate=0, diag_first=False, max_from_zero=False, ratio_raw=False):
    """A, Gb (L, H, S, S), Ih (L, H), b1, b2 (L, 2, S) -> aug (L, S, S), rave_matrices_kernel line for line.  The keyword
    mutants are for tests/test_cpu_vit.py."""
    A, Ih, b1, b2 = (np.asarray(x, F32) for x in (A, Ih, b1, b2))
    L, H, S, _ = A.shape
    with np.errstate(all="ignore"):
        if max_from_zero:
            m = np.zeros((L, S, S), F32)
            first = 0
        else:
            m = A[:, 0] * Ih[:, 0, None, None]
            first = 1
        for h in range(first, H):
            m = np.maximum(m, A[:, h] * Ih[:, h, None, None])          # the max over heads starts from head 0; NaN carried
        if Gb is not None:
            Gb = np.asarray(Gb, F32)
            g = np.zeros((L, S, S), F32)
            for h in range(H):
                g = g + Gb[:, h]
            m = relu_nan((g / F32(H)) * m)
        eye = np.eye(S, dtype=bool)[None]
        if diag_first:
            r = np.where(eye, m + b1[:, 0, None, :], m) * b1[:, 1, None, :]
        else:
            r = m * b1[:, 1, None, :]
            r = np.where(eye, r + b1[:, 0, None, :], r)                  # the diagonal add comes after the b1 product
        if ablate == 0:
            q = b2[:, 1] / b2[:, 0]
            qs = np.maximum(lane_sum(np.abs(q)), F32(1e-12))
            ratio = q if ratio_raw else q / qs[:, None]
            r = r * (ratio * b2[:, 1] + b2[:, 0])[:, None, :]            # two roundings inside the bracket
        rs = lane_sum(r)
        out = r / rs[..., None]
    assert out.dtype == F32
    return out


def _rave_unnormalised64(A, Ih, b1, b2, Gb, ablate):
    A, Ih, b1, b2 = (np.asarray(x, F64) for x in (A, Ih, b1, b2))
    M = (A * Ih[:, :, None, None]).max(axis=1)
    if Gb is not None:
        M = np.maximum(np.asarray(Gb, F64).mean(axis=1) * M, 0.0)
    r = M * b1[:, 1, None, :]
    r = r + np.eye(A.shape[-1])[None] * b1[:, 0, None, :]
    d = None
    if ablate == 0:
        with np.errstate(all="ignore"):
            q = b2[:, 1] / b2[:, 0]
            ratio = q / np.maximum(np.abs(q).sum(axis=-1, keepdims=True), 1e-12)
            d = ratio * b2[:, 1] + b2[:, 0]
        r = r * d[:, None, :]
    return M, r, d


def rave_matrices64(A, Ih, b1, b2, Gb=None, ablate=0):
    with np.errstate(all="ignore"):
        r = _rave_unnormalised64(A, Ih, b1, b2, Gb, ablate)[1]
        return r / r.sum(axis=-1, keepdims=True)


def rave_matrices_bound(A, Ih, b1, b2, Gb=None, ablate=0):
    """(L, S, S): |rave_matrices_fp32 - rave_matrices64| <= this, for finite data with A, Ih, b1, b2 >= 0 and sum |q| > 1e-11.

    M.  Each A_h ih_h rounds once and max is exact: |m^ - m| <= u m.  With the gradient, g^ / H m^ is sum_h Gb_h m / H with
    H additions, the division, the product and m's own rounding on every term: |x^ - x| <= gamma_(H + 3) mean_h |Gb_h| m =: eM;
    the clamp is 1-Lipschitz.  Without it eM = u m.
    r.  r^ = fl(M^ b1) : e_r = eM b1 (1 + u) + u |M b1|; on the diagonal one more addition: e_r += u (|r| + e_r).
    Column scale (ablate 0).  q = b2[1] / b2[0] rounds once; sum |q| carries n = 1 + ceil(S / 64) + 6 roundings on non-negative
    terms, so ratio = q / qs is relative gamma_(n + 2) (the clamp at 1e-12 is not active); ratio b2[1] (+ 1) + b2[0] (+ 1) on
    non-negative terms: d^ = d (1 + t_(n + 4)); the product r d adds one: e_rd = e_r d (1 + gamma_(n + 5)) + gamma_(n + 5) |r| d.
    Row sum.  rs^ = sum_j rd^_j (1 + t_w), w = ceil(S / 64) + 6: E = (1 + gamma_w) sum_j e_rd_j + gamma_w sum_j |rd_j|.
    Quotient.  As in head_importance_bound: (e_rd |rs| + |rd| E) / (|rs| (|rs| - E)), plus one rounding of the result."""
    A64, Ih64, b164, b264 = (np.asarray(x, F64) for x in (A, Ih, b1, b2))
    L, H, S, _ = A64.shape
    assert (A64 >= 0).all() and (Ih64 >= 0).all() and (b164 >= 0).all() and (b264 >= 0).all()
    M, r, d = _rave_unnormalised64(A, Ih, b1, b2, Gb, ablate)
    m = (A64 * Ih64[:, :, None, None]).max(axis=1)
    eM = gamma(H + 3) * np.abs(np.asarray(Gb, F64)).mean(axis=1) * m if Gb is not None else U * m
    r0 = M * b164[:, 1, None, :]
    e_r = eM * b164[:, 1, None, :] * (1 + U) + U * np.abs(r0)
    eye = np.eye(S)[None]
    r1 = r0 + eye * b164[:, 0, None, :]
    e_r = e_r + eye * U * (np.abs(r1) + e_r)
    if ablate == 0:
        q = b264[:, 1] / b264[:, 0]
        assert np.isfinite(q).all() and (np.abs(q).sum(axis=-1) > 1e-11).all()
        n = 1 + lane_rows(S)
        e_r = e_r * d[:, None, :] * (1 + gamma(n + 5)) + gamma(n + 5) * np.abs(r1) * d[:, None, :]
    w = lane_rows(S)
    rs = r.sum(axis=-1, keepdims=True)
    E = (1 + gamma(w)) * e_r.sum(axis=-1, keepdims=True) + gamma(w) * np.abs(r).sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(np.abs(rs) > E, (e_r * np.abs(rs) + np.abs(r) * E) / (np.abs(rs) * (np.abs(rs) - E)), np.inf)
        return b + U * (np.abs(r / rs) + b)


def row_sum_bound(S):
    """|sum_j aug[i][j] - 1| (the sum taken exactly) for non-negative rows: out_j = rd_j / rs^ (1 + d_j) and rs^ = sum_j rd_j
    (1 + t_w), w = ceil(S / 64) + 6, so the sum is (1 + d) / (1 + t_w): within gamma_(w + 2) of 1."""
    return gamma(lane_rows(S) + 2)


# ---- K19 -------------------------------------------------------------------------------------------------------------------------

def rollout_row_fp32(aug, t, reverse_waves=False, kc_floor=False, forward_chain=False, image0_only=False):
    """aug (n, L, S, S) -> (n, S): v = aug[L-1][t], then v <- v . aug[l] for l = L-2 .. 0.  Wave w adds fl(v[k] * M[k][j]) for k in
    [w kc, min(S, (w + 1) kc)) ascending from +0, kc = ceil(S / 16); the 16 partial rows are added in wave order from +0 (an empty
    range adds +0.0, so a -0.0 becomes +0.0).  With L = 1 the row is copied."""
    aug = np.asarray(aug, F32)
    if image0_only:
        aug = np.broadcast_to(aug[:1], aug.shape)
    n, L, S, _ = aug.shape
    order = list(range(L)) if forward_chain else list(range(L - 1, -1, -1))
    v = aug[:, order[0], t, :].copy()
    kc = S // ROLL_WAVES if kc_floor else k19_kc(S)
    waves = range(ROLL_WAVES - 1, -1, -1) if reverse_waves else range(ROLL_WAVES)
    with np.errstate(all="ignore"):
        for l in order[1:]:
            M = aug[:, l]
            total = np.zeros((n, S), F32)
            for w in waves:
                part = np.zeros((n, S), F32)
                for k in range(w * kc, min(S, w * kc + kc)):
                    part = part + v[:, k:k + 1] * M[:, k, :]
                total = total + part
            v = total
    assert v.dtype == F32
    return v


def rollout_row64(aug, t):
    aug = np.asarray(aug, F32)
    n, L, S, _ = aug.shape
    v = aug[:, L - 1, t, :].astype(F64)
    for l in range(L - 2, -1, -1):
        v = np.einsum("nk,nkj->nj", v, aug[:, l].astype(F64))
    return v


def rollout_row_bound(aug, t):
    """(n, S).  One product: v'^_j = sum_k v^_k M_kj (1 + t), |t| <= gamma_c with c = 1 (the product) + kc (the wave's additions)
    + 16 (the partials): |v'^ - v'| <= (1 + gamma_c) (e . |M|)_j + gamma_c (|v| . |M|)_j, e the error v arrived with (0 for the
    copied row)."""
    aug = np.asarray(aug, F32)
    n, L, S, _ = aug.shape
    c = 1 + k19_kc(S) + ROLL_WAVES
    v = aug[:, L - 1, t, :].astype(F64)
    e = np.zeros_like(v)
    for l in range(L - 2, -1, -1):
        M = aug[:, l].astype(F64)
        absM = np.abs(M)
        e = (1 + gamma(c)) * np.einsum("nk,nkj->nj", e, absM) + gamma(c) * np.einsum("nk,nkj->nj", np.abs(v), absM)
        v = np.einsum("nk,nkj->nj", v, M)
    return e


# ---- K21 -------------------------------------------------------------------------------------------------------------------------

def attn_cam_fp32(A, G, column_p=False, clamp_before_mean=False, image0_only=False):
    """A, G (n, H, S, S) -> (n, S - 1): s = sum_h fl(A[h][0][1 + p] * G[h][0][1 + p]) from +0 in h order, c = clamp(s / float(H)),
    lo / hi over the image (NaN if any c is), (c - lo) / (hi - lo)"""
    A, G = np.asarray(A, F32), np.asarray(G, F32)
    if image0_only:
        A, G = np.broadcast_to(A[:1], A.shape), np.broadcast_to(G[:1], G.shape)
    n, H, S, _ = A.shape
    cols = slice(0, S - 1) if column_p else slice(1, S)
    a, g = A[:, :, 0, cols], G[:, :, 0, cols]
    with np.errstate(all="ignore"):
        s = np.zeros((n, S - 1), F32)
        for h in range(H):
            s = s + (relu_nan(a[:, h] * g[:, h]) if clamp_before_mean else a[:, h] * g[:, h])
        c = relu_nan(s / F32(H))
        lo, hi = c.min(axis=1, keepdims=True), c.max(axis=1, keepdims=True)
        out = (c - lo) / (hi - lo)
    assert out.dtype == F32
    return out


def attn_cam64(A, G):
    A, G = np.asarray(A, F64), np.asarray(G, F64)
    c = np.maximum((A[:, :, 0, 1:] * G[:, :, 0, 1:]).mean(axis=1), 0.0)
    lo, hi = c.min(axis=1, keepdims=True), c.max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return (c - lo) / (hi - lo)


def attn_cam_bound(A, G):
    """(n, S - 1).  c^_p = sum_h A G (1 + t_(H + 2)) / H (product, H additions, division; the clamp is 1-Lipschitz): e_p =
    gamma_(H + 2) mean_h |A G|.  min and max are exact on the perturbed values, so lo and hi move by at most E = max_p e_p.
    N = c - lo: e_N = e_p + E + u (N + e_p + E).  D = hi - lo: e_D = 2 E + u (D + 2 E).  The quotient's condition:
    |N^ / D^ - N / D| <= (e_N D + N e_D) / (D (D - e_D)), plus one rounding; D <= e_D (a map that is constant to rounding level)
    gives an infinite bound."""
    A, G = np.asarray(A, F64), np.asarray(G, F64)
    H = A.shape[1]
    p = A[:, :, 0, 1:] * G[:, :, 0, 1:]
    c = np.maximum(p.mean(axis=1), 0.0)
    e = gamma(H + 2) * np.abs(p).mean(axis=1)
    E = e.max(axis=1, keepdims=True)
    lo, hi = c.min(axis=1, keepdims=True), c.max(axis=1, keepdims=True)
    N, D = c - lo, hi - lo
    eN = e + E + U * (N + e + E)
    eD = 2 * E + U * (D + 2 * E)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D > eD, (eN * D + N * eD) / (D * (D - eD)) * (1 + U) + U * N / D, np.inf)


# ---- cells -----------------------------------------------------------------------------------------------------------------------

K17 = namedtuple("K17", "L H S")
K18 = namedtuple("K18", "L H S withgrad ablate")
K19 = namedtuple("K19", "n_img L S t")
K20 = namedtuple("K20", "L S D")
K21 = namedtuple("K21", "n_img H S")

K17_SECOND_TRIP = K17(41, 25, 2)                # L * H = 1025: thread 0 of the finish kernel takes a second cell
K17_CAP = K17(1, 4096, 1)
K19_OVER_64K = K19(1, 2, 1000, 0)               # 68 000 B of LDS
K19_CAP = K19(1, 2, 2409, 2408)                 # 163 812 B of 163 840
K21_SECOND_TRIP_S = 1026                        # P = 1025


def k17_cells():
    """S: one entry; the odd S = 1 and even S = 2 (one k-step, its kh = 1 half empty or not); inside a tile (17, 31: odd, the last k
    has only the kh = 0 half); one full tile (32); 33 = four tiles, the last workgroup full; 63 / 64 (4 tiles) and 65 (9 tiles: the
    last workgroup has 3 idle waves).  (L, H) = (1, 1) and (2, 3): blockIdx.y over blocks and heads."""
    cells = [K17(L, H, S) for S in (1, 2, 17, 31, 32, 33, 63, 64, 65) for L, H in ((1, 1), (2, 3))]
    return cells + [K17_SECOND_TRIP, K17_CAP]


def k18_cells():
    """S at both sides of the 4-rows-per-workgroup seam (3, 4, 5) and of the 64-lane stride (63, 64, 65, and 130: a third trip)"""
    return [K18(L, H, S, g, a) for S in (1, 3, 4, 5, 63, 64, 65, 130) for H in (1, 2, 5) for g in (0, 1) for a in (0, 1) for L in (1, 2)]


def k19_cells():
    """S < 16: kc = 1 and waves S .. 15 add empty sums; 15 / 16 / 17 change kc from 1 to 2; 64 / 65 the lane stride; L = 1 copies
    the row; then the two cells above 64 KiB of LDS"""
    cells = []
    for S in (1, 15, 16, 17, 64, 65, 197):
        for n in (1, 3):
            for L in (1, 2, 4):
                for t in sorted({0, S // 2, S - 1}):
                    cells.append(K19(n, L, S, t))
    return cells + [K19_OVER_64K, K19_CAP]


def k20_cells():
    return [K20(L, S, D) for S in (1, 3, 4, 5) for D in (1, 63, 64, 65, 769) for L in (1, 2)]


def k21_cells():
    """S = 2: one token (0 / 0); 1025 / 1026: P = 1024 / 1025, the second trip of the 1024 threads; 1090 ends it inside a wave"""
    return [K21(n, H, S) for S in (2, 3, 65, 1025, 1026, 1090) for n in (1, 3) for H in (1, 3)]


def cell_name(cell):
    return type(cell).__name__ + "_" + "x".join(str(v) for v in cell)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

STREAM_SCALES = (1.0, 0.5, 1.2, 0.8)            # input, attention output, input + attention, MLP output
K18_D = 8                                       # width of the token streams that give a K18 cell its b1, b2


def _softmax_rows(rng, shape):
    x = rng.standard_normal(shape, dtype=F32) * F32(2)
    x = np.exp(x - x.max(axis=-1, keepdims=True))
    return (x / x.sum(axis=-1, keepdims=True)).astype(F32)


def _streams(rng, L, S, D):
    return tuple((rng.standard_normal((L, S, D), dtype=F32) * F32(s)).astype(F32) for s in STREAM_SCALES)


def normal_case(cell):
    """-> dict of the kernel's inputs: softmax rows for A (and K19's matrices), N(0, 1e-3) for G, N(0, 1e-2) for Gb, N(0, 1) token
    streams at the four scales; K18's Ih is a seeded point of the simplex and its b1, b2 are residual_shares_fp32 of such streams."""
    rng = np.random.default_rng([17, "K17 K18 K19 K20 K21".split().index(type(cell).__name__)] + [int(v) for v in cell])
    if isinstance(cell, K17):
        shape = (cell.L, cell.H, cell.S, cell.S)
        return {"A": _softmax_rows(rng, shape), "G": (rng.standard_normal(shape, dtype=F32) * F32(1e-3)).astype(F32)}
    if isinstance(cell, K18):
        shape = (cell.L, cell.H, cell.S, cell.S)
        ih = rng.random((cell.L, cell.H), dtype=F32) + F32(0.1)
        b1, b2 = residual_shares_fp32(*_streams(rng, cell.L, cell.S, K18_D))
        return {"A": _softmax_rows(rng, shape), "Ih": (ih / ih.sum(axis=1, keepdims=True)).astype(F32), "b1": b1, "b2": b2,
                "Gb": (rng.standard_normal(shape, dtype=F32) * F32(1e-2)).astype(F32) if cell.withgrad else None, "ablate": cell.ablate}
    if isinstance(cell, K19):
        return {"aug": _softmax_rows(rng, (cell.n_img, cell.L, cell.S, cell.S)), "t": cell.t}
    if isinstance(cell, K20):
        return dict(zip(("xs", "ats", "rs", "ms"), _streams(rng, cell.L, cell.S, cell.D)))
    if isinstance(cell, K21):
        shape = (cell.n_img, cell.H, cell.S, cell.S)
        A, G = _softmax_rows(rng, shape), (rng.standard_normal(shape, dtype=F32) * F32(1e-3)).astype(F32)
        # an image none of whose head means is positive (one time in four with two tokens) would be 0 / 0, which is
        # degenerate_cam_case's business: its gradients are negated
        dull = (A[:, :, 0, 1:].astype(F64) * G[:, :, 0, 1:]).mean(axis=1).max(axis=1) <= 0
        G[dull] = -G[dull]
        return {"A": A, "G": G}
    raise TypeError(cell)


def exact_case(cell):
    """Integer-valued fp32 inputs on which every partial sum is an integer below 2^24 (asserted here), so that any order of
    addition is exact, and int64 results that do not come from the restatement.

    K17: A in [1, 3], G in +-[1, 3] -> "part" (L * H, tiles) int64 tile sums of |A^T G| and "total" (L, H); Ih itself is two
         divisions away (finish_from_int).
    K19: at most 3 entries of +-1, +-2 per matrix row (|v| grows by at most 6 per product) -> "row" (n, S) int64.
    K21: c = sum_h A G / H is a chosen integer in [-8, 16] with 16 and a negative value present where P >= 2 (the last head has
         A = 1 and the G that makes the sum H c), so lo = 0, hi = 16 and out = max(c, 0) / 16 exactly -> "numer" int64, "denom";
         everything but row 0, columns 1 .. S-1 holds 1000, which no result can absorb.  P = 1 is 0 / 0."""
    rng = np.random.default_rng([19] + [int(v) for v in cell])
    if isinstance(cell, K17):
        L, H, S = cell
        A = rng.integers(1, 4, (L, H, S, S))
        G = rng.integers(1, 4, (L, H, S, S)) * rng.choice((-1, 1), (L, H, S, S))
        prod = np.abs(np.einsum("lhki,lhkj->lhij", A, G))
        nt = -(-S // TILE)
        full = np.zeros((L * H, nt * TILE, nt * TILE), np.int64)
        full[:, :S, :S] = prod.reshape(L * H, S, S)
        part = full.reshape(L * H, nt, TILE, nt, TILE).sum(axis=(2, 4)).reshape(L * H, nt * nt)
        total = part.sum(axis=1).reshape(L, H)
        assert total.max() < 2 ** 24 and (total.sum(axis=1) > 0).all() and 9 * S < 2 ** 24
        return {"A": A.astype(F32), "G": G.astype(F32), "part": part, "total": total}
    if isinstance(cell, K19):
        n, L, S, t = cell
        aug = np.zeros((n, L, S, S), np.int64)
        idx = rng.integers(0, S, (n, L, S, 3))
        val = rng.integers(1, 3, (n, L, S, 3)) * rng.choice((-1, 1), (n, L, S, 3))
        np.put_along_axis(aug, idx, val, axis=-1)
        v, mag = aug[:, L - 1, t], np.abs(aug[:, L - 1, t])
        for l in range(L - 2, -1, -1):
            v, mag = np.einsum("nk,nkj->nj", v, aug[:, l]), np.einsum("nk,nkj->nj", mag, np.abs(aug[:, l]))
        assert mag.max(initial=0) < 2 ** 24
        return {"aug": aug.astype(F32), "t": t, "row": v}
    if isinstance(cell, K21):
        n, H, S = cell
        P = S - 1
        c = rng.integers(-8, 17, (n, P))
        if P >= 2:
            where = np.stack([rng.permutation(P)[:2] for _ in range(n)])
            np.put_along_axis(c, where, np.array([[16, -3]] * n), axis=1)
        a = rng.integers(-3, 4, (n, H, P))
        g = rng.integers(-3, 4, (n, H, P))
        a[:, H - 1] = 1
        g[:, H - 1] = H * c - (a[:, :H - 1] * g[:, :H - 1]).sum(axis=1)
        assert ((a * g).sum(axis=1) == H * c).all() and np.abs(a * g).sum(axis=1).max() < 2 ** 24
        A, G = np.full((n, H, S, S), 1000, np.int64), np.full((n, H, S, S), 1000, np.int64)
        A[:, :, 0, 1:], G[:, :, 0, 1:] = a, g
        return {"A": A.astype(F32), "G": G.astype(F32), "numer": np.maximum(c, 0), "denom": 16 if P >= 2 else 0}
    raise TypeError(cell)


def finish_from_int(total, S):
    """K17's Ih from the int64 totals (exact as fp32): / S^2, the head total in h order, the division -- no tile arithmetic"""
    L, H = total.shape
    return head_importance_finish_fp32(total.astype(F32).reshape(L * H, 1), L, H, S)


# ---- degenerate values the reference defines -------------------------------------------------------------------------------------

DEGENERATE_K18 = K18(2, 3, 5, 1, 0)
DEGENERATE_K21 = K21(3, 3, 6)


def zero_tokens_case():
    """K20: token 1 of block 0 is zero in the input and the attention output, token 2 in input + attention and the MLP output:
    both norms 0, F.normalize's clamp gives 0 / 1e-12 = +0.0 for both shares"""
    d = normal_case(K20(2, 4, 65))
    d["xs"][0, 1] = d["ats"][0, 1] = 0
    d["rs"][0, 2] = d["ms"][0, 2] = 0
    return d


def zero_resid_share_case(mlp_share):
    """K18: b2[0][0][2] = 0 with b2[0][1][2] = mlp_share: q = 1 / 0 = inf (mlp_share 1, a zero resid_1 token) or 0 / 0 = NaN
    (mlp_share 0, what zero_tokens_case's token 2 gives).  The reference's ratio is then NaN in that column (inf / inf) or in all
    (NaN sum), every row of block 0 sums to NaN; block 1 is untouched."""
    d = normal_case(DEGENERATE_K18)
    d["b2"][0, 0, 2], d["b2"][0, 1, 2] = 0, mlp_share
    return d


def zero_masked_row_case():
    """K18: the Gb means of row 3 of block 1 are all negative: the clamp leaves +0.0 and only the diagonal term is left: e_3"""
    d = normal_case(DEGENERATE_K18)
    d["Gb"][1, :, 3, :] = -np.abs(d["Gb"][1, :, 3, :])
    return d


def all_negative_gb_case():
    """K18: every Gb mean of block 0 is negative: the block is the identity, and its zeros are +0.0"""
    d = normal_case(DEGENERATE_K18)
    d["Gb"][0] = -np.abs(d["Gb"][0])
    return d


def negative_importance_case():
    """K18 with Ih of block 0 negated (no K17 output is, but the kernel is a function of any Ih): every product A ih is
    negative there, which is what tells a max started from head 0 from one started from 0"""
    d = normal_case(K18(2, 3, 5, 0, 1))
    d["Ih"][0] = -d["Ih"][0]
    return d


def nan_gradient_case(kernel):
    """One NaN in a gradient.  K17: in G of block 1, head 0 -> Ih[1] is NaN in every head, Ih[0] is untouched.  K18: in Gb[0][1][2][3]
    -> the reference's clamp keeps it, row 2 of block 0 sums to NaN.  K21: in G[1][0][0][2] -> image 1 is NaN everywhere (clamp,
    min and max all carry it); images 0 and 2 are untouched."""
    if kernel == "K17":
        d = normal_case(K17(2, 3, 33))
        d["G"][1, 0, 4, 7] = np.nan
    elif kernel == "K18":
        d = normal_case(DEGENERATE_K18)
        d["Gb"][0, 1, 2, 3] = np.nan
    else:
        d = normal_case(DEGENERATE_K21)
        d["G"][1, 0, 0, 2] = np.nan
    return d


def degenerate_cam_case(kind):
    """K21: image 0 all <= 0 ("nonpositive": c = +0.0 everywhere, 0 / 0) or one positive constant ("constant"); images 1, 2 normal"""
    d = normal_case(DEGENERATE_K21)
    if kind == "nonpositive":
        d["G"][0] = -np.abs(d["G"][0])
    else:
        d["A"][0], d["G"][0] = F32(0.25), F32(0.5)
    return d


def ledger_names():
    """the rows tests/test_gpu_vit_edges.py leaves in its ledger (profiles/vit_edges_parity.json): per comparison the error in the
    project's norm at the bar and, under /bound, the largest |error| / derived bound at 1.0"""
    names = [f"vit_edges/{cell_name(c)}" for c in k17_cells() + k18_cells() + k19_cells() + k20_cells() + k21_cells()
             if not (isinstance(c, K21) and c.S == 2)]
    names += [f"vit_edges/{cell_name(c)}/b2" for c in k20_cells()]
    names = names + [n + "/bound" for n in names]
    names += [f"vit_edges/{cell_name(c)}/offdiag/bound" for c in k18_cells() if c.S > 1]
    names += [f"vit_edges/{cell_name(c)}/rowsum/bound" for c in k18_cells()]
    return sorted(names)
