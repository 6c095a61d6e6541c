"""tests/vit_restated.py (K17-K21, csrc/vit_kernels.hip) proved on the host: every fp32 restatement lies inside its derived bound
around the fp64 definition at every cell of the matrix; the fp64 definitions are the fp64 torch restatements of
tests/test_gpu_vit_rave.py; integer data gives the int64 results; the degenerate values give the NaN / inf / zero pattern of the
reference's own torch expressions run in fp32; and the cells tell each mutant of the restatement from the restatement.

NaN: where C's fmaxf / fminf would drop a NaN and torch.max / clamp / min / F.normalize carry it, the restatement -- and since
this file exists the kernels -- follow torch: generate_RAVE and generate_cam_attn are torch expressions in the reference, so an
attribution that is NaN there has to be NaN here and not a finite map made of the remaining entries."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_restated as R
from test_cpu_cam import inside
from test_gpu_vit_rave import ref_cam, ref_head_importance, ref_matrices, ref_row, ref_shares

F32 = np.float32


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close64(mine, torchs, what):
    """`*64` against the fp64 torch restatement: 1e-12 of each entry, plus 1e-15 of the largest for the entries that are sums of
    cancelling terms"""
    want = torchs.numpy() if isinstance(torchs, torch.Tensor) else np.asarray(torchs)
    assert mine.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(mine), np.isnan(want), err_msg=str(what))
    ok = ~np.isnan(want)
    scale = np.abs(want[ok]).max(initial=0.0)
    assert (np.abs(mine[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]) + 1e-15 * scale).all(), what


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return bool((a.view(np.int32) != b.view(np.int32)).any())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def held_to_cam64(got, want, bound):
    """K21's fraction of the bound.  An image whose clamped map is constant is 0 / 0 in fp64 and must be NaN in fp32 too, whole;
    every other image has a finite bound."""
    nan = np.isnan(want)
    assert (nan.all(axis=1) | ~nan.any(axis=1)).all()
    np.testing.assert_array_equal(np.isnan(got), nan)
    assert np.isfinite(bound[~nan]).all()
    return inside(got[~nan], want[~nan], bound[~nan]) if (~nan).any() else 0.0


# ---- every cell: fp32 inside the bound around fp64, fp64 equal to torch's ---------------------------------------------------------

@pytest.mark.parametrize("cell", R.k17_cells(), ids=R.cell_name)
def test_k17_restatement_cell(cell):
    d = R.normal_case(cell)
    want = R.head_importance64(**d)
    assert inside(R.head_importance_fp32(**d), want, R.head_importance_bound(**d)) <= 1.0
    close64(want, ref_head_importance(tt(d["A"]), tt(d["G"])), cell)
    e = R.exact_case(cell)
    part = R.head_importance_parts_fp32(e["A"], e["G"])
    np.testing.assert_array_equal(part, np.rint(part))
    np.testing.assert_array_equal(part.astype(np.int64), e["part"])
    assert bits_equal(R.head_importance_fp32(e["A"], e["G"]), R.finish_from_int(e["total"], cell.S))


@pytest.mark.parametrize("cell", R.k18_cells(), ids=R.cell_name)
def test_k18_restatement_cell(cell):
    d = R.normal_case(cell)
    got, want, bound = R.rave_matrices_fp32(**d), R.rave_matrices64(**d), R.rave_matrices_bound(**d)
    assert np.isfinite(bound).all() and inside(got, want, bound) <= 1.0
    assert np.abs(got.astype(np.float64).sum(axis=-1) - 1).max() <= R.row_sum_bound(cell.S)
    close64(want, ref_matrices(tt(d["A"]), tt(d["Ih"]), tt(d["b1"]), tt(d["b2"]), None if d["Gb"] is None else tt(d["Gb"]), cell.ablate), cell)


@pytest.mark.parametrize("cell", R.k19_cells(), ids=R.cell_name)
def test_k19_restatement_cell(cell):
    d = R.normal_case(cell)
    want = R.rollout_row64(**d)
    assert inside(R.rollout_row_fp32(**d), want, R.rollout_row_bound(**d)) <= 1.0
    close64(want, torch.stack([ref_row(tt(a), cell.t) for a in d["aug"]]), cell)
    e = R.exact_case(cell)
    got = R.rollout_row_fp32(e["aug"], e["t"])
    np.testing.assert_array_equal(got, np.rint(got))
    np.testing.assert_array_equal(got.astype(np.int64), e["row"])
    assert not np.signbit(got[got == 0]).any() or cell.L == 1, "a zero of a product is +0.0"


@pytest.mark.parametrize("cell", R.k20_cells(), ids=R.cell_name)
def test_k20_restatement_cell(cell):
    d = R.normal_case(cell)
    got, want, bound = R.residual_shares_fp32(**d), R.residual_shares64(**d), R.residual_shares_bound(**d)
    refs = ref_shares(*(list(tt(d[k])) for k in ("xs", "ats", "rs", "ms")))
    for g, w, b, r in zip(got, want, bound, refs):
        assert inside(g, w, b) <= 1.0
        close64(w, r, cell)


@pytest.mark.parametrize("cell", R.k21_cells(), ids=R.cell_name)
def test_k21_restatement_cell(cell):
    d = R.normal_case(cell)
    got, want = R.attn_cam_fp32(**d), R.attn_cam64(**d)
    close64(want, torch.stack([ref_cam(tt(a), tt(g)) for a, g in zip(d["A"], d["G"])]), cell)
    e = R.exact_case(cell)
    out = R.attn_cam_fp32(e["A"], e["G"])
    if cell.S == 2:
        assert np.isnan(got).all() and np.isnan(want).all() and np.isnan(out).all()
        return
    assert held_to_cam64(got, want, R.attn_cam_bound(**d)) <= 1.0
    scaled = out * F32(e["denom"])
    np.testing.assert_array_equal(scaled, np.rint(scaled))
    np.testing.assert_array_equal(scaled.astype(np.int64), e["numer"])


# ---- degenerate values: the reference's torch expressions in fp32 ----------------------------------------------------------------

def pattern(x):
    """per entry: 1 NaN, 2 +inf, 3 -inf, 4 +0.0, 5 -0.0, 0 any other number"""
    x = np.asarray(x, F32)
    p = np.zeros(x.shape, np.int8)
    p[np.isnan(x)] = 1
    p[x == np.inf] = 2
    p[x == -np.inf] = 3
    p[(x == 0) & ~np.signbit(x)] = 4
    p[(x == 0) & np.signbit(x)] = 5
    return p


# the lines of ref_head_importance, ref_shares, ref_matrices and ref_cam (tests/test_gpu_vit_rave.py; the same expressions as
# torch_rave there and compute_RAVE in xai_engine/vit_attr.py) without their .double(): what the reference computes, in fp32
def torch32_head_importance(A, G):
    m = (tt(A).transpose(-1, -2) @ tt(G)).abs().mean((-1, -2))
    return (m / m.sum(1, keepdim=True)).numpy()


def torch32_shares(xs, ats, rs, ms):
    def pair(a, b):
        return F.normalize(torch.stack((tt(a).norm(dim=-1), tt(b).norm(dim=-1))), p=1, dim=0)
    return (torch.stack([pair(a, b) for a, b in zip(xs, ats)]).numpy(), torch.stack([pair(a, b) for a, b in zip(rs, ms)]).numpy())


def torch32_matrices(A, Ih, b1, b2, Gb, ablate):
    A, Ih, b1, b2 = tt(A), tt(Ih), tt(b1), tt(b2)
    M = (A * Ih[:, :, None, None]).amax(1)
    if Gb is not None:
        M = (tt(Gb).mean(1) * M).clamp(min=0)
    r = M * b1[:, 1, None, :] + torch.diag_embed(b1[:, 0])
    if ablate == 0:
        ratio = F.normalize(b2[:, 1] / b2[:, 0], p=1, dim=-1)
        r = r @ torch.diag_embed(ratio * b2[:, 1] + b2[:, 0])
    return (r / r.sum(-1, keepdim=True)).numpy()


def torch32_cam(A, G):
    out = []
    for a, g in zip(tt(A), tt(G)):
        c = (a[:, 0, 1:] * g[:, 0, 1:]).mean(0).clamp(min=0)
        out.append((c - c.min()) / (c.max() - c.min()))
    return torch.stack(out).numpy()


RESTATED = {"K17": lambda d: R.head_importance_fp32(**d), "K18": lambda d: R.rave_matrices_fp32(**d), "K20": lambda d: np.stack(R.residual_shares_fp32(**d)),
            "K21": lambda d: R.attn_cam_fp32(**d)}
REFERENCE32 = {"K17": lambda d: torch32_head_importance(**d), "K18": lambda d: torch32_matrices(**d), "K20": lambda d: np.stack(torch32_shares(**d)),
               "K21": lambda d: torch32_cam(**d)}
EYE5 = np.where(np.eye(5) == 1, 0, 4)


def degenerate_cases():
    """name -> (kernel, its inputs, what must be true of the pattern of the result: 1 NaN, 4 +0.0, 0 a number)"""
    return {
        "zero_tokens": ("K20", R.zero_tokens_case(), lambda p: (p[0, 0, :, 1] == 4).all() and (p[1, 0, :, 2] == 4).all() and (p == 4).sum() == 4),
        "zero_resid_share_inf": ("K18", R.zero_resid_share_case(1.0), lambda p: (p[0] == 1).all() and (p[1] != 1).all()),
        "zero_resid_share_nan": ("K18", R.zero_resid_share_case(0.0), lambda p: (p[0] == 1).all() and (p[1] != 1).all()),
        "zero_masked_row": ("K18", R.zero_masked_row_case(), lambda p: (p[1, 3] == EYE5[3]).all() and not (p == 1).any()),
        "all_negative_gb": ("K18", R.all_negative_gb_case(), lambda p: (p[0] == EYE5).all()),
        "nan_gradient_K17": ("K17", R.nan_gradient_case("K17"), lambda p: (p[1] == 1).all() and (p[0] == 0).all()),
        "nan_gradient_K18": ("K18", R.nan_gradient_case("K18"), lambda p: (p[0, 2] == 1).all() and (p == 1).sum() == 5),
        "nan_gradient_K21": ("K21", R.nan_gradient_case("K21"), lambda p: (p[1] == 1).all() and (p[[0, 2]] != 1).all()),
        "cam_nonpositive": ("K21", R.degenerate_cam_case("nonpositive"), lambda p: (p[0] == 1).all() and (p[[1, 2]] != 1).all()),
        "cam_constant": ("K21", R.degenerate_cam_case("constant"), lambda p: (p[0] == 1).all() and (p[[1, 2]] != 1).all()),
    }


DEGENERATE = ("zero_tokens", "zero_resid_share_inf", "zero_resid_share_nan", "zero_masked_row", "all_negative_gb", "nan_gradient_K17",
              "nan_gradient_K18", "nan_gradient_K21", "cam_nonpositive", "cam_constant")


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_values_have_the_pattern_of_the_reference(name):
    """Which entries are NaN, inf, +0.0, -0.0 or numbers: the restatement against the reference's torch expressions in fp32 on this
    CPU, entry for entry, and the property the case was built for.  The numbers themselves agree to fp32 rounding (1e-5 of the
    largest)."""
    kernel, d, holds = degenerate_cases()[name]
    got, ref = RESTATED[kernel](d), REFERENCE32[kernel](d)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(pattern(got), pattern(ref), err_msg=name)
    assert holds(pattern(got)), (name, pattern(got))
    num = pattern(ref) == 0
    if num.any():
        assert np.abs(got[num].astype(np.float64) - ref[num]).max() <= 1e-5 * np.abs(ref[num]).max()


def test_degenerate_case_list_is_complete():
    assert set(degenerate_cases()) == set(DEGENERATE)


# ---- the cells discriminate ------------------------------------------------------------------------------------------------------

def _k17(**m):
    return lambda d: R.head_importance_fp32(d["A"], d["G"], **m)


def _k18(**m):
    return lambda d: R.rave_matrices_fp32(**d, **m)


def _k19(**m):
    return lambda d: R.rollout_row_fp32(d["aug"], d["t"], **m)


# mutant -> (the cell, or the named case, that tells it from the restatement; restatement; mutant)
MUTANTS = {
    "K17 k descending": (R.K17(2, 3, 65), _k17(), _k17(k_descending=True)),
    "K17 partials summed before abs": (R.K17(2, 3, 33), _k17(), _k17(sum_before_abs=True)),
    "K18 diagonal added before the b1 product": (R.K18(2, 2, 5, 1, 0), _k18(), _k18(diag_first=True)),
    "K18 max over heads started from 0": ("negative_importance_case", _k18(), _k18(max_from_zero=True)),
    "K18 ratio not divided by qs": (R.K18(2, 2, 5, 0, 0), _k18(), _k18(ratio_raw=True)),
    "K19 partials in reverse wave order": (R.K19(1, 2, 65, 0), _k19(), _k19(reverse_waves=True)),
    "K19 kc = S // 16": (R.K19(1, 2, 17, 0), _k19(), _k19(kc_floor=True)),
    "K19 aug[0] @ ... @ aug[L-1]": (R.K19(1, 2, 16, 8), _k19(), _k19(forward_chain=True)),
    "K20 shares from squared norms": (R.K20(1, 3, 65), lambda d: np.stack(R.residual_shares_fp32(**d)),
                                      lambda d: np.stack(R.residual_shares_fp32(**d, squared=True))),
    "K21 column p instead of 1 + p": (R.K21(1, 3, 65), lambda d: R.attn_cam_fp32(**d), lambda d: R.attn_cam_fp32(**d, column_p=True)),
    "K21 mean after the clamp": (R.K21(1, 3, 65), lambda d: R.attn_cam_fp32(**d), lambda d: R.attn_cam_fp32(**d, clamp_before_mean=True)),
    "K19 image 1 reads image 0": (R.K19(3, 2, 16, 0), _k19(), _k19(image0_only=True)),
    "K21 image 1 reads image 0": (R.K21(3, 1, 65), lambda d: R.attn_cam_fp32(**d), lambda d: R.attn_cam_fp32(**d, image0_only=True)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_named_cell_tells_the_mutant_from_the_restatement(mutant):
    """... and that cell is in the matrix both test files run (or is one of the named cases the GPU file holds bit for bit)"""
    cell, good, bad = MUTANTS[mutant]
    if isinstance(cell, str):
        d = getattr(R, cell)()
    else:
        assert cell in R.k17_cells() + R.k18_cells() + R.k19_cells() + R.k20_cells() + R.k21_cells(), cell
        d = R.normal_case(cell)
    assert bits_differ(good(d), bad(d)), (mutant, cell)
    if "image 1" in mutant:
        assert bits_equal(good(d)[0], bad(d)[0]) and bits_differ(good(d)[1], bad(d)[1])


def test_one_k_order_inside_an_mfma_changes_bits_too():
    """MFMA_K_ORDER is a named constant because the cells can tell its two values apart"""
    d = R.normal_case(R.K17(2, 3, 65))
    want = R.head_importance_parts_fp32(d["A"], d["G"])
    old = R.MFMA_K_ORDER
    try:
        R.MFMA_K_ORDER = (1, 0)
        assert bits_differ(want, R.head_importance_parts_fp32(d["A"], d["G"]))
    finally:
        R.MFMA_K_ORDER = old


# ---- geometry --------------------------------------------------------------------------------------------------------------------

def _library():
    try:
        import xai_engine
        return xai_engine._lib.load()
    except Exception:       # not built, or not loadable on a machine without the HIP runtime: the closed forms stand alone
        return None


def test_geometry_helpers():
    assert [R.k17_tiles(S) for S in (1, 31, 32, 33, 64, 65, 4096)] == [1, 1, 1, 4, 4, 9, 128 * 128]
    assert [R.k17_grid(1, 1, S) for S in (1, 32, 33, 64, 65)] == [(1, 3), (1, 3), (1, 0), (1, 0), (3, 3)]
    assert R.k17_workspace_bytes(41, 25, 2) == 4 * 1025 and R.k17_workspace_bytes(2, 3, 65) == 4 * 6 * 9 and R.k17_workspace_bytes(0, 1, 1) == 0
    assert R.k19_lds_bytes(257) == 17476 and R.k19_lds_bytes(1000) == 68000 > 64 * 1024
    assert R.K19_MAX_S == 2409 and R.k19_lds_bytes(2409) == 163812 <= R.K19_LDS_CAP < R.k19_lds_bytes(2410)
    assert [R.k19_kc(S) for S in (1, 15, 16, 17, 197, 2409)] == [1, 1, 1, 2, 13, 151]
    lib = _library()
    if lib is not None:
        for c in R.k17_cells() + [R.K17(0, 1, 1), R.K17(12, 12, 197)]:
            assert lib.xai_attn_head_importance_workspace_bytes(c.L, c.H, c.S) == R.k17_workspace_bytes(*c), c
