"""K11-K14 and K16 (csrc/masker_kernels.hip: up_rownorm_kernel<true | false>, rownorm_kernel<true | false>,
cluster_sum_kernel<true | false>, causal_apply_kernel / _v4, masked_sums_kernel<4 | 1>) on the MI355X against
tests/maskers_restated.py at their edges, bit for bit.

Every output lives between two runs of guard words (a NaN pattern) that must come back untouched, at a 16-byte boundary or one
float past it; every input is read back and compared after the call (the in-place K12 call apart); results are compared through
int32 views, NaNs by position.  The data of a cell differs from row to row, map to map and mask to mask.  Which instantiation
ran is read from a profiler trace where a pointer's alignment decides it."""
import numpy as np
import pytest
import torch

import maskers_restated as R
from conftest import check
from test_cpu_maskers import BAR, restated_against_oracle
from test_gpu_blur_edges import kernels_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                      # words on either side of an output
POISON = 0x7FC0DEAD             # a quiet NaN no kernel here produces
UNSUPPORTED = -3


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    return __import__("xai_engine")._lib.load()


class Out:
    """n words for a kernel to write, `off` words past a 16-byte boundary, inside a buffer of POISON words."""

    def __init__(self, n, off=0, fill=None):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.full((GUARD + off + n + GUARD,), POISON, dtype=torch.int32, device=DEV)
        self.t = self.buf[self.lo:self.lo + n]
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.int32).ravel()))
        self.ptr = self.t.data_ptr()
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (4 * off) % 16

    def get(self):
        """The n words as int32, after the guards are seen untouched."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == POISON).all(), "words before the output were written"
        assert (b[self.lo + self.n:] == POISON).all(), "words behind the output were written"
        return b[self.lo:self.lo + self.n]

    def untouched(self):
        return bool((self.get() == POISON).all())


class In:
    """An input on the device, `off` words past a 16-byte boundary; unchanged() compares it with what was put there."""

    def __init__(self, a, off=0):
        self.words = np.ascontiguousarray(a).view(np.int32).ravel()
        self.buf = torch.zeros(off + self.words.size + 4, dtype=torch.int32, device=DEV)
        self.t = self.buf[off:off + self.words.size]
        self.t.copy_(torch.from_numpy(self.words))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == (4 * off) % 16

    def unchanged(self):
        np.testing.assert_array_equal(self.t.cpu().numpy(), self.words, err_msg="an input was written")


def same_bits(got, want, what):
    got = np.ascontiguousarray(got).view(np.int32).ravel()
    want = np.ascontiguousarray(want, np.float32).ravel()
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got.view(np.float32)), nan, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(got[~nan], want.view(np.int32)[~nan], err_msg=str(what))


def call(K, name, *args):
    K._call(name, torch.device(DEV), *args)


def flavour(names, kernel, true="true", false="false"):
    """Which instantiation of `kernel` is among the names (demangled or in the Itanium mangling); exactly one launch of it."""
    mine = [n for n in names if kernel in n and "up_" + kernel not in n]
    assert len(mine) == 1, names
    for value, arg in ((True, true), (False, false)):
        tag = ("Lb1" if arg == "true" else "Lb0" if arg == "false" else f"Li{arg}")
        if f"{kernel}<{arg}>" in mine[0] or f"{kernel}I{tag}EE" in mine[0]:
            return value
    raise AssertionError(names)


# ---- K11 -----------------------------------------------------------------------------------------------------------------------

def run_k11(K, cell, fmap, off=0):
    Rn, h, w, H, W = cell
    src, out = In(fmap), Out(Rn * H * W, off)
    call(K, "xai_up_rownorm_f32", src.ptr, Rn, h, w, H, W, out.ptr)
    got = out.get()
    src.unchanged()
    return got


@pytest.mark.parametrize("cell", R.K11_CELLS, ids=R.k11_name)
def test_up_rownorm_cell_has_the_bits_of_the_restatement(K, lib, cell):
    """N(0, 1) maps, and integer maps on the dyadic cells (exact in any order).  The one-pixel maps come back all NaN (0/0, as
    in the reference), the identity cell equals K12 on the input, the cell that shrinks along H is refused with nothing
    written, and the cell at all three LDS limits -- 16 416 B static and 49 152 B dynamic, 65 568 B in one workgroup --
    launches (status 0) and is held to the same bits."""
    Rn, h, w, H, W = cell
    if R.k11_refuses(cell):
        src, out = In(R.k11_maps(cell)), Out(Rn * H * W)
        assert lib.xai_up_rownorm_f32(src.ptr, Rn, h, w, H, W, out.ptr, None) == UNSUPPORTED
        assert out.untouched()
        return
    for kind in ("normal", "integer") if R.k11_is_dyadic(cell) else ("normal",):
        fmap = R.k11_maps(cell, kind)
        got = run_k11(K, cell, fmap)
        same_bits(got, R.up_rownorm(fmap, H, W), (cell, kind))
        if R.k11_is_constant(cell):
            assert np.isnan(got.view(np.float32)).all()
        if (h, w) == (H, W):
            flat = torch.from_numpy(fmap.reshape(Rn, h * w)).to(DEV)
            same_bits(got, K.rownorm(flat).cpu().numpy(), (cell, kind, "K12 on the input"))


def test_restatement_against_the_oracle_on_this_machine():
    """The ledger rows of this file: every kernel comparison here is bit for bit, so what is measured is the restatement against
    oracle.vit_cx with this machine's torch, one row per K11 cell that runs (tests/test_cpu_maskers.py reads the file)."""
    for cell in R.K11_CELLS:
        if not R.k11_refuses(cell):
            check(R.ledger_name(cell), restated_against_oracle(cell)[0], 0, BAR, against="oracle.vit_cx", absolute=True)


@pytest.mark.parametrize("cell", R.K11_ALIGNMENT_CELLS, ids=R.k11_name)
def test_up_rownorm_one_float_off_runs_the_scalar_form_with_the_same_bits(K, cell):
    Rn, h, w, H, W = cell
    fmap = R.k11_maps(cell)
    want = R.up_rownorm(fmap, H, W)
    got, names = kernels_of(lambda: run_k11(K, cell, fmap))
    assert flavour(names, "up_rownorm_kernel") is True, names
    same_bits(got, want, (cell, "aligned"))
    got, names = kernels_of(lambda: run_k11(K, cell, fmap, off=1))
    assert flavour(names, "up_rownorm_kernel") is False, names
    same_bits(got, want, (cell, "out 4 bytes off"))


def test_up_rownorm_is_invariant_under_powers_of_two(K):
    """A map times 2^60 and times 2^-60 gives the bits of the map: every product, sum and quotient scales exactly."""
    cell = (3, 14, 14, 28, 28)
    fmap = R.k11_maps(cell)
    want = R.up_rownorm(fmap, 28, 28)
    for e in (60, -60):
        scaled = (fmap * np.float32(2.0 ** e)).astype(np.float32)
        assert np.array_equal(scaled.astype(np.float64), fmap.astype(np.float64) * 2.0 ** e)
        same_bits(R.up_rownorm(scaled, 28, 28), want, ("restatement", e))
        same_bits(run_k11(K, cell, scaled), want, ("K11", e))


@pytest.mark.parametrize("why", list(R.K11_REFUSED))
def test_up_rownorm_refuses_without_writing(lib, why):
    """Beyond each LDS limit by one, and -- new -- a target smaller than the source in either axis, where the reference's
    antialiased resize is not the two-tap formula."""
    Rn, h, w, H, W = R.K11_REFUSED[why]
    src, out = In(np.arange(Rn * h * w, dtype=np.float32)), Out(Rn * H * W)
    assert lib.xai_up_rownorm_f32(src.ptr, Rn, h, w, H, W, out.ptr, None) == UNSUPPORTED, why
    assert out.untouched()


# ---- K12 -----------------------------------------------------------------------------------------------------------------------

def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def k12_seams_of(Rn, P):
    slices = R.k12_slices(Rn, P, cu_count())
    return sorted(set(R.k12_seams(P, slices, False)[0] + (R.k12_seams(P, slices, True)[0] if P % 4 == 0 else [])))


def test_rownorm_matrix_reaches_slices_seams_and_the_cap_on_this_device():
    got = {c: R.k12_slices(*c, cu_count()) for c in R.K12_CELLS}
    assert any(s > 1 and c[0] % 8 for c, s in got.items()), got
    assert any(s == R.K12_MAX_SLICES for s in got.values()), got
    short = [c for c, s in got.items() if s > 1 and R.k12_seams(c[1], s, c[1] % 4 == 0)[1] < R.k12_seams(c[1], s, c[1] % 4 == 0)[2]]
    assert any(c[1] % 4 == 0 for c in short) and any(c[1] % 4 for c in short), got
    assert any(got[c] == R.K12_MAX_SLICES for c in short), got
    assert got[(600, 2052)] == 1 and 600 > 2 * cu_count()


@pytest.mark.parametrize("cell", R.K12_CELLS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_rownorm_three_ways_has_the_bits_of_the_restatement(K, cell):
    """Out of place (several slices per row), in place (one slice), and with x one float off where P % 4 == 0 (the scalar
    form at a float4 length): the same bits, over rounds of data that put each row's min and max at the first and last
    element, inside the last float4 and on both sides of every slice seam; one row with +-inf (all NaN), one with -0.0."""
    Rn, P = cell
    seams = k12_seams_of(Rn, P)
    for rnd in range(R.k12_rounds(Rn, P, seams)):
        x = R.k12_rows(Rn, P, seams, rnd)
        want = R.rownorm(x)
        if P == 1:
            assert np.isnan(want).all()

        def out_of_place(off):
            xin, out = In(x, off), Out(Rn * P)
            call(K, "xai_rownorm_f32", xin.ptr, Rn, P, out.ptr)
            got = out.get()
            xin.unchanged()
            return got

        if rnd == 0:
            got, names = kernels_of(lambda: out_of_place(0))
            assert flavour(names, "rownorm_kernel") is (P % 4 == 0), names
        else:
            got = out_of_place(0)
        same_bits(got, want, (cell, rnd, "out of place"))
        io = Out(Rn * P, fill=x)
        call(K, "xai_rownorm_f32", io.ptr, Rn, P, io.ptr)
        same_bits(io.get(), want, (cell, rnd, "in place"))
        if P % 4 == 0:
            if rnd == 0:
                got, names = kernels_of(lambda: out_of_place(1))
                assert flavour(names, "rownorm_kernel") is False, names
            else:
                got = out_of_place(1)
            same_bits(got, want, (cell, rnd, "x 4 bytes off"))


# ---- K13 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,off", [(p, 0) for p in R.K13_PS] + [(1028, 1)], ids=lambda v: str(v))
def test_cluster_sum_has_the_bits_of_the_sequential_sums(K, P, off):
    """12 rows of magnitudes 1e8 / 1 / -1e8 ..., so the order of addition decides the bits; a singleton, a scattered majority, a
    pair, and an empty cluster that must come back as +0.0."""
    rows = R.k13_rows(P)
    n_k = len(R.K13_OFFS) - 1

    def run():
        rin, mem, offs, out = In(rows, off), In(R.K13_MEMBERS), In(R.K13_OFFS), Out(n_k * P)
        call(K, "xai_cluster_sum_f32", rin.ptr, mem.ptr, offs.ptr, n_k, P, out.ptr)
        got = out.get()
        for i in (rin, mem, offs):
            i.unchanged()
        return got

    got, names = kernels_of(run)
    assert flavour(names, "cluster_sum_kernel") is (P % 4 == 0 and off == 0), names
    same_bits(got, R.cluster_sum(rows, R.K13_MEMBERS, R.K13_OFFS), (P, off))
    assert (got.reshape(n_k, P)[1] == 0).all(), "the empty cluster is +0.0"


# ---- K14 -----------------------------------------------------------------------------------------------------------------------

def run_k14(K, cell, case, scale, offs=(0, 0, 0, 0)):
    N, C, HW = cell
    x, m, noise = (In(a, o) for a, o in zip(case, offs))
    out = Out(2 * N * C * HW, offs[3])
    call(K, "xai_causal_apply_f32", x.ptr, m.ptr, noise.ptr, N, C, HW, float(scale), out.ptr)
    got = out.get()
    for i in (x, m, noise):
        i.unchanged()
    return got


@pytest.mark.parametrize("cell", R.K14_CELLS, ids=lambda c: "x".join(map(str, c)))
def test_causal_apply_has_the_bits_of_the_restatement(K, cell):
    """Masks with exact 0, exact 1 and values outside [0, 1]; noise scales 0.1, 0 and -0.25.  tests/test_cpu_maskers.py shows
    that every case with a non-zero scale holds elements a contracted multiply-add would change."""
    case = R.k14_case(cell)
    for scale in R.K14_SCALES:
        same_bits(run_k14(K, cell, case, scale), R.causal_stack(*case, scale), (cell, scale))


@pytest.mark.parametrize("which", range(5), ids=["aligned", "x", "masks", "noise", "stack"])
def test_causal_apply_with_one_pointer_off_runs_the_scalar_form(K, which):
    cell = R.K14_MISALIGNED_CELL
    case = R.k14_case(cell)
    offs = tuple(int(i == which - 1) for i in range(4))
    got, names = kernels_of(lambda: run_k14(K, cell, case, 0.1, offs))
    mine = [n for n in names if "causal_apply_kernel" in n]
    assert len(mine) == 1 and ("causal_apply_kernel_v4" in mine[0]) == (which == 0), names
    same_bits(got, R.causal_stack(*case, 0.1), (cell, offs))


# ---- K16 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,off", [(p, 0) for p in R.K16_PS] + [(1028, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("N", R.K16_NS)
def test_masked_sums_has_the_bits_of_the_sequential_sums(K, N, P, off):
    """N at both sides of the 8-row unroll, once and twice; P at the float4 form, the scalar form, and the scalar form at a
    float4 length (rows one float off)."""
    rows, w = R.k16_case(N, P)

    def run():
        rin, win, ow, op = In(rows, off), In(w), Out(P), Out(P)
        call(K, "xai_masked_sums_f32", rin.ptr, win.ptr, N, P, ow.ptr, op.ptr)
        got = ow.get(), op.get()
        rin.unchanged()
        win.unchanged()
        return got

    (gw, gp), names = kernels_of(run)
    assert flavour(names, "masked_sums_kernel", "4", "1") is (P % 4 == 0 and off == 0), names
    ww, wp = R.masked_sums(rows, w)
    same_bits(gw, ww, (N, P, off, "weighted"))
    same_bits(gp, wp, (N, P, off, "plain"))


# ---- argument checks: no launch ------------------------------------------------------------------------------------------------

def test_grid_limits_are_refused_without_a_launch(lib):
    """The y (K13, K14) and row (K12) grid dimension stops at 65 535: one more is XAI_E_UNSUPPORTED, and nothing is written."""
    a, b, c, out = In(np.ones(8, np.float32)), In(np.ones(8, np.float32)), In(np.zeros(8, np.int32)), Out(8)
    assert lib.xai_causal_apply_f32(a.ptr, b.ptr, a.ptr, 65536, 1, 1, 0.1, out.ptr, None) == UNSUPPORTED
    assert lib.xai_cluster_sum_f32(a.ptr, c.ptr, c.ptr, 65536, 1, out.ptr, None) == UNSUPPORTED
    assert lib.xai_rownorm_f32(a.ptr, 65536, 1, out.ptr, None) == UNSUPPORTED
    assert out.untouched()
    for i in (a, b, c):
        i.unchanged()
