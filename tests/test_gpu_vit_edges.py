"""K17-K21 (csrc/vit_kernels.hip) on the MI355X against tests/vit_restated.py at their edges.

Every kernel is called through the C ABI and held bit for bit to its fp32 restatement on seeded data; K17, K19 and K21 also element
for element to int64 results on integer data that is exact in any order; the same output lies inside the derived bound around the
fp64 definition (the fraction goes to the ledger at 1.0) and inside the project's 1e-5.  Every output and the K17 workspace live
between guard words that must come back untouched, every input is read back after the call, the blocks behind the pointer tables
are separate allocations made in shuffled order, and one cell per kernel places every buffer one float past a 16-byte boundary.
The degenerate values have the NaN / inf / +0.0 pattern of the reference's torch expressions in fp32 (tests/test_cpu_vit.py)."""
import numpy as np
import pytest
import torch

import vit_restated as R
from conftest import BAR, check
from test_cpu_cam import inside
from test_cpu_vit import REFERENCE32, RESTATED, degenerate_cases, held_to_cam64, pattern
from test_gpu_masker_edges import In, Out, call, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGAINST = "fp64 restatement"
F32 = np.float32
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3

# the cell of each kernel that is also run with every buffer 4 bytes past a 16-byte boundary
OFF_CELLS = {R.K17(2, 3, 33), R.K18(2, 2, 65, 1, 0), R.K19(3, 2, 17, 8), R.K20(2, 5, 65), R.K21(3, 3, 65)}


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    return __import__("xai_engine")._lib.load()


class Blocks:
    """The blocks of a per-block operand (L, ...) as L separate device buffers, allocated in a shuffled order, and the device
    table of their pointers"""

    def __init__(self, a, off=0, seed=0):
        order = np.random.default_rng([23, seed, len(a)]).permutation(len(a))
        self.ins = [None] * len(a)
        for l in order:
            self.ins[l] = In(a[l], off)
        self.tab = In(np.array([i.ptr for i in self.ins], np.int64))
        self.ptr = self.tab.ptr

    def unchanged(self):
        self.tab.unchanged()
        for i in self.ins:
            i.unchanged()


def f32(words, shape):
    return words.view(F32).reshape(shape).copy()


def held(name, got, want, bound):
    """inside the derived bound around fp64 (the fraction to the ledger at 1.0) and inside the project's bar"""
    ratio = inside(got, want, bound)
    print(f"{name}: {ratio:.4f} of the derived bound")
    check(name + "/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
    check(name, got, want, BAR, against=AGAINST)


# ---- runners ---------------------------------------------------------------------------------------------------------------------

def run_k17(K, lib, A, G, off=0):
    """-> Ih (L, H), the workspace (L * H, tiles)"""
    L, H, S, _ = A.shape
    nbytes = lib.xai_attn_head_importance_workspace_bytes(L, H, S)
    assert nbytes == R.k17_workspace_bytes(L, H, S)
    a, g, out, ws = Blocks(A, off, 1), Blocks(G, off, 2), Out(L * H, off), Out(nbytes // 4, off)
    call(K, "xai_attn_head_importance_f32", a.ptr, g.ptr, L, H, S, out.ptr, ws.ptr, nbytes)
    got, part = f32(out.get(), (L, H)), f32(ws.get(), (L * H, R.k17_tiles(S)))
    a.unchanged(), g.unchanged()
    return got, part


def run_k18(K, A, Ih, b1, b2, Gb, ablate, off=0):
    L, H, S, _ = A.shape
    a, gb = Blocks(A, off, 3), (Blocks(Gb, off, 4) if Gb is not None else None)
    ih, s1, s2, out = In(Ih, off), In(b1, off), In(b2, off), Out(L * S * S, off)
    call(K, "xai_rave_matrices_f32", a.ptr, gb.ptr if gb else None, ih.ptr, s1.ptr, s2.ptr, L, H, S, int(ablate), out.ptr)
    got = f32(out.get(), (L, S, S))
    for i in (a, ih, s1, s2) + ((gb,) if gb else ()):
        i.unchanged()
    return got


def run_k19(K, aug, t, off=0):
    n, L, S, _ = aug.shape
    a, out = In(aug, off), Out(n * S, off)
    call(K, "xai_rollout_row_f32", a.ptr, n, L, S, int(t), out.ptr)
    got = f32(out.get(), (n, S))
    a.unchanged()
    return got


def run_k20(K, xs, ats, rs, ms, off=0):
    L, S, D = xs.shape
    groups = [Blocks(x, off, 5 + i) for i, x in enumerate((xs, ats, rs, ms))]
    tab = In(np.array([g.ins[l].ptr for l in range(L) for g in groups], np.int64))
    o1, o2 = Out(L * 2 * S, off), Out(L * 2 * S, off)
    call(K, "xai_residual_shares_f32", tab.ptr, L, S, D, o1.ptr, o2.ptr)
    got = f32(o1.get(), (L, 2, S)), f32(o2.get(), (L, 2, S))
    tab.unchanged()
    for g in groups:
        g.unchanged()
    return got


def run_k21(K, A, G, off=0):
    n, H, S, _ = A.shape
    a, g, out = In(A, off), In(G, off), Out(n * (S - 1), off)
    call(K, "xai_attn_cam_f32", a.ptr, g.ptr, n, H, S, out.ptr)
    got = f32(out.get(), (n, S - 1))
    a.unchanged(), g.unchanged()
    return got


def offsets(cell):
    return (0, 1) if cell in OFF_CELLS else (0,)


def test_every_kernel_has_its_misaligned_cell():
    cells = R.k17_cells() + R.k18_cells() + R.k19_cells() + R.k20_cells() + R.k21_cells()
    assert OFF_CELLS <= set(cells) and {type(c) for c in OFF_CELLS} == {R.K17, R.K18, R.K19, R.K20, R.K21}


# ---- the cells -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", R.k17_cells(), ids=R.cell_name)
def test_head_importance_cell(K, lib, cell):
    """Integer data: the workspace holds the int64 tile sums of |A^T G| and Ih is two divisions away from their totals, whatever
    the order inside a tile.  N(0, 1e-3) gradients: the workspace and Ih have the bits of the fmaf chain in ascending k."""
    name = f"vit_edges/{R.cell_name(cell)}"
    e, d = R.exact_case(cell), R.normal_case(cell)
    for off in offsets(cell):
        got, part = run_k17(K, lib, e["A"], e["G"], off)
        assert (part == np.rint(part)).all(), "integer data came back with a fraction"
        np.testing.assert_array_equal(part.astype(np.int64), e["part"])
        same_bits(got, R.finish_from_int(e["total"], cell.S), (name, "integer data", off))
        got, part = run_k17(K, lib, d["A"], d["G"], off)
        same_bits(part, R.head_importance_parts_fp32(**d), (name, "workspace", off))
        same_bits(got, R.head_importance_fp32(**d), (name, off))
    held(name, got, R.head_importance64(**d), R.head_importance_bound(**d))


@pytest.mark.parametrize("cell", R.k18_cells(), ids=R.cell_name)
def test_rave_matrices_cell(K, cell):
    """... and so that the small entries count too: the off-diagonal entries alone, each against its own bound, and every row
    sum within its bound of 1"""
    name = f"vit_edges/{R.cell_name(cell)}"
    d = R.normal_case(cell)
    for off in offsets(cell):
        got = run_k18(K, off=off, **d)
        same_bits(got, R.rave_matrices_fp32(**d), (name, off))
    want, bound = R.rave_matrices64(**d), R.rave_matrices_bound(**d)
    held(name, got, want, bound)
    offdiag = np.broadcast_to(~np.eye(cell.S, dtype=bool), got.shape)
    if offdiag.any():
        assert (np.abs(got.astype(np.float64) - want)[offdiag] <= bound[offdiag]).all()
        check(name + "/offdiag/bound", inside(got[offdiag], want[offdiag], bound[offdiag]), 0, 1.0, against=AGAINST, absolute=True)
    rows = np.abs(got.astype(np.float64).sum(axis=-1) - 1).max() / R.row_sum_bound(cell.S)
    check(name + "/rowsum/bound", rows, 0, 1.0, against="1", absolute=True)


@pytest.mark.parametrize("cell", R.k19_cells(), ids=R.cell_name)
def test_rollout_row_cell(K, cell):
    """With three images, one call equals the three single-image calls.  The last two cells ask for 68 000 and 163 812 bytes of
    dynamic LDS."""
    name = f"vit_edges/{R.cell_name(cell)}"
    e, d = R.exact_case(cell), R.normal_case(cell)
    for off in offsets(cell):
        got = run_k19(K, e["aug"], e["t"], off)
        assert (got == np.rint(got)).all(), "integer data came back with a fraction"
        np.testing.assert_array_equal(got.astype(np.int64), e["row"])
        got = run_k19(K, d["aug"], d["t"], off)
        same_bits(got, R.rollout_row_fp32(**d), (name, off))
    held(name, got, R.rollout_row64(**d), R.rollout_row_bound(**d))
    if cell.n_img > 1:
        for i in range(cell.n_img):
            same_bits(run_k19(K, d["aug"][i:i + 1], d["t"]), got[i], (name, "image", i, "alone"))


@pytest.mark.parametrize("cell", R.k20_cells(), ids=R.cell_name)
def test_residual_shares_cell(K, cell):
    name = f"vit_edges/{R.cell_name(cell)}"
    d = R.normal_case(cell)
    for off in offsets(cell):
        got = run_k20(K, off=off, **d)
        for g, w, which in zip(got, R.residual_shares_fp32(**d), ("b1", "b2")):
            same_bits(g, w, (name, which, off))
    for g, w, b, tag in zip(got, R.residual_shares64(**d), R.residual_shares_bound(**d), ("", "/b2")):
        held(name + tag, g, w, b)


@pytest.mark.parametrize("cell", R.k21_cells(), ids=R.cell_name)
def test_attn_cam_cell(K, cell):
    """Integer data: 16 * out is max(c, 0) as an integer.  One token (S = 2) is 0 / 0.  With three images, one call equals the
    three single-image calls."""
    name = f"vit_edges/{R.cell_name(cell)}"
    e, d = R.exact_case(cell), R.normal_case(cell)
    for off in offsets(cell):
        got = run_k21(K, e["A"], e["G"], off)
        if cell.S == 2:
            assert np.isnan(got).all()
        else:
            scaled = got * F32(e["denom"])
            assert (scaled == np.rint(scaled)).all(), "integer data came back with a fraction"
            np.testing.assert_array_equal(scaled.astype(np.int64), e["numer"])
        got = run_k21(K, d["A"], d["G"], off)
        same_bits(got, R.attn_cam_fp32(**d), (name, off))
    if cell.n_img > 1:
        for i in range(cell.n_img):
            same_bits(run_k21(K, d["A"][i:i + 1], d["G"][i:i + 1]), got[i], (name, "image", i, "alone"))
    if cell.S == 2:
        assert np.isnan(got).all()
        return
    want = R.attn_cam64(**d)
    ratio = held_to_cam64(got, want, R.attn_cam_bound(**d))
    print(f"{name}: {ratio:.4f} of the derived bound")
    check(name + "/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
    ok = ~np.isnan(want)
    check(name, got[ok], want[ok], BAR, against=AGAINST)


# ---- degenerate values -----------------------------------------------------------------------------------------------------------

def run_case(K, lib, kernel, d):
    if kernel == "K17":
        return run_k17(K, lib, d["A"], d["G"])[0]
    if kernel == "K18":
        return run_k18(K, **d)
    if kernel == "K20":
        return np.stack(run_k20(K, **d))
    return run_k21(K, d["A"], d["G"])


@pytest.mark.parametrize("name", list(degenerate_cases()))
def test_degenerate_values_have_the_pattern_of_the_reference(K, lib, name):
    """NaN, inf, +0.0 and -0.0 where the reference's torch expressions have them in fp32 on the CPU (a NaN gradient gives a NaN row,
    block or image there: torch's clamp, max and min carry it, and so do the kernels), and the bits of the restatement everywhere"""
    kernel, d, holds = degenerate_cases()[name]
    got = run_case(K, lib, kernel, d)
    np.testing.assert_array_equal(pattern(got), pattern(REFERENCE32[kernel](d)), err_msg=name)
    assert holds(pattern(got)), name
    same_bits(got, RESTATED[kernel](d), name)


def test_rave_matrices_take_the_max_over_heads_from_head_0(K):
    d = R.negative_importance_case()
    same_bits(run_k18(K, **d), R.rave_matrices_fp32(**d), "negative Ih")


# ---- repeats ---------------------------------------------------------------------------------------------------------------------

def test_second_trip_cells_repeat_bit_identically(K, lib):
    d = R.normal_case(R.K17_SECOND_TRIP)
    first = run_k17(K, lib, d["A"], d["G"])
    for _ in range(2):
        again = run_k17(K, lib, d["A"], d["G"])
        same_bits(again[0], first[0], "K17 Ih")
        same_bits(again[1], first[1], "K17 workspace")
    d = R.normal_case(R.K21(3, 3, R.K21_SECOND_TRIP_S))
    first = run_k21(K, d["A"], d["G"])
    for _ in range(2):
        same_bits(run_k21(K, d["A"], d["G"]), first, "K21")


# ---- refusals: no launch ---------------------------------------------------------------------------------------------------------

def zeros(n):
    return torch.zeros(n, dtype=torch.float32, device=DEV)


def test_head_importance_refuses_without_writing(lib):
    """A workspace one byte short or absent, L * H = 4097, S = 4097.  Every buffer has the size the extents ask for."""
    for (L, H, S), short, null, code in (((2, 3, 33), 1, False, E_SHAPE), ((2, 3, 33), 0, True, E_NULL), ((1, 4097, 1), 0, False, E_UNSUPPORTED),
                                         ((1, 1, 4097), 0, False, E_UNSUPPORTED)):
        blocks = [(zeros(H * S * S), zeros(H * S * S)) for _ in range(L)]
        atab = In(np.array([a.data_ptr() for a, _ in blocks], np.int64))
        gtab = In(np.array([g.data_ptr() for _, g in blocks], np.int64))
        nbytes = lib.xai_attn_head_importance_workspace_bytes(L, H, S)
        assert nbytes == R.k17_workspace_bytes(L, H, S)
        out, ws = Out(L * H), Out(nbytes // 4)
        got = lib.xai_attn_head_importance_f32(atab.ptr, gtab.ptr, L, H, S, out.ptr, None if null else ws.ptr, nbytes - short, None)
        assert got == code, ((L, H, S), short, null, got)
        assert out.untouched() and ws.untouched()
        del blocks


def test_rave_matrices_refuse_an_unknown_ablation(lib):
    d = R.normal_case(R.K18(1, 2, 5, 0, 0))
    a, ih, b1, b2, out = Blocks(d["A"]), In(d["Ih"]), In(d["b1"]), In(d["b2"]), Out(25)
    assert lib.xai_rave_matrices_f32(a.ptr, None, ih.ptr, b1.ptr, b2.ptr, 1, 2, 5, 2, out.ptr, None) == E_SHAPE
    assert out.untouched()


def test_rollout_row_refuses_beyond_the_lds_cap_and_a_token_past_the_end(lib):
    S = R.K19_MAX_S + 1
    assert R.k19_lds_bytes(S) > R.K19_LDS_CAP
    aug, out = zeros(S * S), Out(S)
    assert lib.xai_rollout_row_f32(aug.data_ptr(), 1, 1, S, 0, out.ptr, None) == E_UNSUPPORTED
    assert out.untouched()
    aug, out = zeros(2 * 17 * 17), Out(17)
    assert lib.xai_rollout_row_f32(aug.data_ptr(), 1, 2, 17, 17, out.ptr, None) == E_SHAPE
    assert out.untouched()


def test_attn_cam_refuses_a_single_token(lib):
    a, g, out = zeros(3), zeros(3), Out(4)
    assert lib.xai_attn_cam_f32(a.data_ptr(), g.data_ptr(), 1, 3, 1, out.ptr, None) == E_SHAPE
    assert out.untouched()
