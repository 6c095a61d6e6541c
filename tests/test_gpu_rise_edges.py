"""K4 / K5 (csrc/rise_kernels.hip: rise_apply_kernel, rise_apply_kernel_v4, rise_apply_kernel_s8<NT, C3>, rise_accum_kernel,
rise_accum_kernel_s8) on the MI355X against tests/rise_restated.py at their edges.

K4 is held bit for bit to mask32 (taps in fp64 rounded once, a fixed four-term fp32 blend, the clip) and to the exact fp32
product image * mask, through every kernel that can take a call; K5 bit for bit to the sequential fp64 sum where the launch plan
has one slice, and inside the derived bound where slices merge by atomics.  Every output lives between guard words that must
come back untouched, every input is read back after the call, and which kernel ran is read from a profiler trace.  Behind
every K5 input lie 16 masks' worth of in-range filler with NaN scores: a slice that reads past n_masks shows as NaN."""
import numpy as np
import pytest
import torch

import rise_restated as R
from conftest import check, rel_inf
from test_cpu_rise import restated_against_oracle
from test_gpu_blur_edges import kernels_of
from test_gpu_masker_edges import In, Out, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGAINST = "fp64 restatement"
SHAPE, UNSUPPORTED = -2, -3


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    return __import__("xai_engine")._lib.load()


class Bytes:
    """uint8 input on the device, `off` bytes past a 16-byte boundary."""

    def __init__(self, a, off=0):
        self.host = np.ascontiguousarray(a, np.uint8).ravel()
        self.buf = torch.zeros(16 + off + self.host.size + 16, dtype=torch.uint8, device=DEV)
        self.t = self.buf[16 + off:16 + off + self.host.size]
        self.t.copy_(torch.from_numpy(self.host))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == off % 16

    def unchanged(self):
        np.testing.assert_array_equal(self.t.cpu().numpy(), self.host, err_msg="the grids were written")


def apply_ran(names):
    """Which K4 kernel is among the launched ones (exactly one): ("s8", NT, C3), ("v4",) or ("scalar",)."""
    mine = [n for n in names if "rise_apply_kernel" in n]
    assert len(mine) == 1, names
    if "rise_apply_kernel_s8" in mine[0]:
        for nt in (False, True):
            for c3 in (False, True):
                if (f"rise_apply_kernel_s8<{str(nt).lower()},{str(c3).lower()}>" in mine[0]
                        or f"rise_apply_kernel_s8ILb{int(nt)}ELb{int(c3)}EE" in mine[0]):
                    return ("s8", nt, c3)
        raise AssertionError(names)
    return ("v4",) if "rise_apply_kernel_v4" in mine[0] else ("scalar",)


def accum_ran(names):
    mine = [n for n in names if "rise_accum_kernel" in n]
    assert len(mine) == 1, names
    return "s8" if "rise_accum_kernel_s8" in mine[0] else "generic"


def run_k4(K, grid, shifts, cell, image, masked, masks, off=0, grid_off=0):
    """-> (masked (n, C, H, W) or None, masks (n, H, W) or None) as fp32 arrays; `off`: image and outputs that many floats past a
    16-byte boundary; grid_off: the grids that many bytes past one."""
    n, s = grid.shape[:2]
    C, H, W = image.shape
    g, sh, im = Bytes(grid, grid_off), In(shifts), In(image, off)
    om = Out(n * C * H * W, off) if masked else None
    ok = Out(n * H * W, off) if masks else None
    K._call("xai_rise_apply_f32", torch.device(DEV), g.ptr, sh.ptr, n, s, int(cell[0]), int(cell[1]), im.ptr, C, H, W,
            om.ptr if om else None, ok.ptr if ok else None)
    got = (om.get().view(np.float32).reshape(n, C, H, W) if om else None, ok.get().view(np.float32).reshape(n, H, W) if ok else None)
    g.unchanged(), sh.unchanged(), im.unchanged()
    return got


def expect_k4(grid, shifts, cell, image):
    C, H, W = image.shape
    m = R.masks32(grid, shifts, cell, H, W)
    return (image[None] * m[:, None]).astype(np.float32), m


def padded(grid, shifts, scores):
    """PAD_MASKS more masks behind the inputs: all-one grids at shift 0 with NaN scores."""
    n, s = grid.shape[:2]
    return (np.concatenate([grid, np.ones((R.PAD_MASKS, s, s), np.uint8)]),
            np.concatenate([shifts, np.zeros((R.PAD_MASKS, 2), np.int32)]),
            np.concatenate([scores, np.full(R.PAD_MASKS, np.nan, np.float32)]))


def run_k5(K, grid, shifts, scores, cell, H, W, scale, kernel, acc0=None):
    """xai_rise_accum_f64 on n masks (the inputs padded behind them); kernel "generic" at s == 8 puts the grids one byte off.
    -> acc (H, W) float64.  The kernel that ran is checked."""
    n, s = grid.shape[:2]
    gp, shp, scp = padded(grid, shifts, scores)
    grid_off = 1 if (s == 8 and kernel == "generic") else 0

    def go():
        g, sh, sc = Bytes(gp, grid_off), In(shp), In(scp)
        acc = Out(2 * H * W, fill=np.zeros((H, W), np.float64) if acc0 is None else np.asarray(acc0, np.float64))
        K._call("xai_rise_accum_f64", torch.device(DEV), g.ptr, sh.ptr, sc.ptr, n, s, int(cell[0]), int(cell[1]), H, W, float(scale), acc.ptr)
        got = acc.get().view(np.float64).reshape(H, W).copy()
        g.unchanged(), sh.unchanged(), sc.unchanged()
        return got

    got, names = kernels_of(go)
    assert accum_ran(names) == kernel, names
    return got


def same_bits64(got, want, what):
    np.testing.assert_array_equal(np.ascontiguousarray(got, np.float64).view(np.int64), np.ascontiguousarray(want, np.float64).view(np.int64),
                                  err_msg=str(what))


# ---- K4 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell3", R.K4_CELLS, ids=R.k4_name)
def test_apply_cell_has_the_bits_of_the_restatement(K, cell3):
    """60 masks per cell -- all-zero, all-one, single ones at the corners and the centre, a single zero, a checkerboard and
    random grids, each at the four extreme shifts and a random one -- with C in {1, 3, 4} and masked only, masks only and both:
    masks == mask32 and masked == image * mask32 through int32 views.  The kernel that ran is the one apply_path names."""
    H, W, s = cell3
    grid, shifts, cell = R.k4_case(cell3)
    path = R.apply_path(s, W)
    for C in R.K4_CHANNELS:
        image = R.k4_image(C, H, W)
        want_masked, want_masks = expect_k4(grid, shifts, cell, image)
        (masked, masks), names = kernels_of(lambda: run_k4(K, grid, shifts, cell, image, True, True))
        assert apply_ran(names) == (("s8", False, C == 3) if path == "s8" else (path,)), names
        same_bits(masks, want_masks, (cell3, C, "masks, both"))
        same_bits(masked, want_masked, (cell3, C, "masked, both"))
        same_bits(run_k4(K, grid, shifts, cell, image, True, False)[0], want_masked, (cell3, C, "masked only"))
        same_bits(run_k4(K, grid, shifts, cell, image, False, True)[1], want_masks, (cell3, C, "masks only"))
    assert (want_masks[:R.N_SHIFTS].view(np.int32) == 0).all() and (want_masks[R.N_SHIFTS:2 * R.N_SHIFTS] == 1).all()


def test_restatement_against_the_oracle_on_this_machine():
    """The mask rows of the ledger: every K4 comparison here is bit for bit, so what is measured is the restatement against
    oracle.rise with this machine's scipy, one row per K4 cell (tests/test_cpu_rise.py reads the file)."""
    for cell3 in R.K4_CELLS:
        check(R.mask_ledger_name(cell3), restated_against_oracle(cell3), 0, R.ORACLE_BOUND, against="oracle.rise", absolute=True)


@pytest.mark.parametrize("cell3", [c for c in R.K4_CELLS if c[1] % 4 == 0], ids=R.k4_name)
def test_every_apply_route_gives_the_same_bits(K, cell3):
    """The same call through every kernel that can take it: image and outputs one float off run the scalar kernel at
    W % 4 == 0; at s == 8 the grids one byte off run _v4 instead of _s8.  All routes equal mask32 bit for bit."""
    H, W, s = cell3
    grid, shifts, cell = R.k4_case(cell3)
    image = R.k4_image(3, H, W)
    want_masked, want_masks = expect_k4(grid, shifts, cell, image)
    routes = [(0, 0, R.apply_path(s, W)), (1, 0, "scalar")] + ([(0, 1, "v4"), (1, 1, "scalar")] if s == 8 else [])
    assert [r[2] for r in routes] == [R.apply_path(s, W, aligned16=not off, grid_aligned8=not goff) for off, goff, _ in routes]
    for off, goff, path in routes:
        (masked, masks), names = kernels_of(lambda: run_k4(K, grid, shifts, cell, image, True, True, off=off, grid_off=goff))
        assert apply_ran(names)[0] == path, (names, off, goff)
        same_bits(masks, want_masks, (cell3, off, goff, "masks"))
        same_bits(masked, want_masked, (cell3, off, goff, "masked"))


@pytest.mark.parametrize("C", [3, 4])
def test_non_temporal_instantiations_have_the_bits_of_the_restatement(K, C):
    """The smallest batch whose masked images and masks together pass 128 MiB at 64 x 64: rise_apply_kernel_s8<true, C == 3>,
    every mask and masked image compared with mask32, in chunks."""
    H = W = 64
    n = R.NT_BYTES // (H * W * 4 * (C + 1)) + 1
    assert R.apply_flavour(n, C, H, W, True, True) == (True, C == 3) and not R.apply_flavour(n - 1, C, H, W, True, True)[0]
    rng = np.random.default_rng([7, C])
    pool, _, cell = R.k4_case((H, W, 8))
    grid = pool[rng.integers(0, len(pool), n)]
    shifts = np.stack([rng.integers(0, cell[0], n), rng.integers(0, cell[1], n)], axis=1).astype(np.int32)
    image = R.k4_image(C, H, W)
    (masked, masks), names = kernels_of(lambda: run_k4(K, grid, shifts, cell, image, True, True))
    assert apply_ran(names) == ("s8", True, C == 3), names
    for lo in range(0, n, 512):
        want_masked, want_masks = expect_k4(grid[lo:lo + 512], shifts[lo:lo + 512], cell, image)
        same_bits(masks[lo:lo + 512], want_masks, (C, lo, "masks"))
        same_bits(masked[lo:lo + 512], want_masked, (C, lo, "masked"))


def test_apply_limits(K, lib):
    """65 535 masks (the y extent of the launch grid) at 8 x 8 are exact; 65 536 masks and s = 65 are XAI_E_UNSUPPORTED, a crop
    outside the up-sampled grid is XAI_E_SHAPE, and none of the three writes anything."""
    rng = np.random.default_rng(9)
    pool = (rng.random((97, 8, 8)) < 0.5).astype(np.uint8)
    pool[0], pool[1] = 0, 1
    grid = pool[np.arange(R.MAX_MASKS) % 97]
    shifts = np.zeros((R.MAX_MASKS, 2), np.int32)
    image = R.k4_image(1, 8, 8)
    masks = run_k4(K, grid, shifts, (1, 1), image, False, True)[1]
    same_bits(masks, R.masks32(grid, shifts, (1, 1), 8, 8), "65535 masks")
    g, sh, im, out = Bytes(np.ones(65 * 65, np.uint8)), In(np.zeros(8, np.int32)), In(image), Out(81)
    call = lambda n, s, ch, cw, H, W: lib.xai_rise_apply_f32(g.ptr, sh.ptr, n, s, ch, cw, im.ptr, 1, H, W, None, out.ptr, None)   # noqa: E731
    assert call(R.MAX_MASKS + 1, 8, 1, 1, 8, 8) == UNSUPPORTED
    assert call(1, R.MAX_S + 1, 1, 1, 8, 8) == UNSUPPORTED
    assert call(1, 8, 1, 1, 10, 8) == SHAPE and call(1, 8, 1, 1, 8, 10) == SHAPE          # H + cell - 1 > (s + 1) * cell
    assert out.untouched()
    assert call(1, 8, 1, 1, 9, 9) == 0                                                    # ... and the largest crop that fits does run
    same_bits(out.get(), np.ones(81, np.float32), "9 x 9 of an all-one grid")


def test_apply_refusals_write_nothing(lib):
    g, sh, im, out = Bytes(np.ones(65 * 65, np.uint8)), In(np.zeros(8, np.int32)), In(np.ones(64, np.float32)), Out(64)
    for n, s, H in ((R.MAX_MASKS + 1, 8, 8), (1, R.MAX_S + 1, 8), (1, 8, 10)):
        assert lib.xai_rise_apply_f32(g.ptr, sh.ptr, n, s, 1, 1, im.ptr, 1, H, 8, out.ptr, out.ptr, None) < 0
    assert out.untouched()


# ---- K5 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell4", R.K5_ONE_SLICE, ids=lambda c: "x".join(map(str, c)))
def test_accumulate_with_one_slice_has_the_bits_of_the_sequential_sum(K, cell4):
    """accum_plan says one slice: the kernel adds in ascending n into one fp64 register and adds acc once -- accum64 bit for bit,
    from both kernels at s == 8, with acc zero and with acc carried in."""
    H, W, s, n = cell4
    assert R.accum_plan(n, H, W)["slices"] == 1
    grid, shifts, scores, cell, scale = R.k5_case(cell4)
    carried = np.random.default_rng(3).standard_normal((H, W))
    for kernel in R.k5_kernels(cell4):
        same_bits64(run_k5(K, grid, shifts, scores, cell, H, W, scale, kernel), R.accum64(grid, shifts, scores, cell, H, W, scale), (cell4, kernel))
        same_bits64(run_k5(K, grid, shifts, scores, cell, H, W, scale, kernel, acc0=carried),
                    R.accum64(grid, shifts, scores, cell, H, W, scale, acc0=carried), (cell4, kernel, "carried"))


@pytest.mark.parametrize("cell4,kernel", R.bounded_rows(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_accumulate_with_slices_and_rounds_is_inside_the_derived_bound(K, cell4, kernel):
    """Several slices (merged by fp64 atomics in any order) and / or several staging rounds: |K5 - accum64| / accum_bound goes to
    the ledger per cell and kernel (profiles/rise_edges_parity.json, tied by tests/test_cpu_rise.py); 1.0 is the derived
    condition, not a measured slack.  Where the magnitude is 0 (every mask 0 at the pixel) the result is exactly 0; a plan of one
    slice is held to accum64's bits as well.  The 512 x 512 cells are compared on ten pixel rows (every pixel of them is covered
    by test_integer_scores_on_all_one_grids_are_exact)."""
    H, W, s, n = cell4
    grid, shifts, scores, cell, scale = R.k5_case(cell4)
    stage = R.accum_stage(s, cell, kernel)
    plan = R.accum_plan(n, H, W, stage)
    assert stage >= 1 and (plan["slices"] > 1 or plan["rounds"] > 1)
    rows = list(R.LONG_ROWS) if cell4 in R.K5_LONG else None
    got = run_k5(K, grid, shifts, scores, cell, H, W, scale, kernel)
    assert np.isfinite(got).all(), "a slice read past n_masks, or a mask outside [0, 1]"
    got = got if rows is None else got[rows]
    want = R.accum64(grid, shifts, scores, cell, H, W, scale, rows=rows)
    bound = R.accum_bound(n, R.accum_magnitude(grid, shifts, scores, cell, H, W, scale, rows=rows))
    err = np.abs(got - want)
    assert (err[bound == 0] == 0).all()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{R.accum_ledger_name(cell4, kernel)}: {ratio:.4f}  plan {plan}")
    check(R.accum_ledger_name(cell4, kernel), ratio, 0, 1.0, against=AGAINST, absolute=True)
    if plan["slices"] == 1:
        same_bits64(got, want, (cell4, kernel))


@pytest.mark.parametrize("cell4", [(32, 32, 8, 513), (30, 45, 7, 513), (64, 128, 64, 40)] + list(R.K5_LONG), ids=lambda c: "x".join(map(str, c)))
def test_integer_scores_on_all_one_grids_are_exact(K, cell4):
    """Every mask is exactly 1.0 and every score an integer: each partial sum is an integer below 2^53 and scale a power of two,
    so any order of addition returns sum(scores) * scale at every pixel -- a mask left out, read twice or taken from behind
    n_masks shows everywhere."""
    H, W, s, n = cell4
    _, shifts, _, cell, _ = R.k5_case(cell4)
    scores = np.random.default_rng([6, n]).integers(-50, 51, n).astype(np.float32)
    grid = np.ones((n, s, s), np.uint8)
    want = np.full((H, W), float(scores.astype(np.int64).sum()) * 0.25)
    for kernel in R.k5_kernels(cell4):
        same_bits64(run_k5(K, grid, shifts, scores, cell, H, W, 0.25, kernel), want, (cell4, kernel))


@pytest.mark.parametrize("cell4", [(30, 45, 8, 130), (30, 45, 7, 130)], ids=lambda c: "x".join(map(str, c)))
def test_an_infinite_score_gives_nan_where_its_mask_is_zero_and_inf_elsewhere(K, cell4):
    """As preds * masks does in the reference: inf * 0 is NaN, inf * m is inf for m > 0, and neither is lost in a later sum."""
    H, W, s, n = cell4
    grid, shifts, scores, cell, scale = R.k5_case(cell4)
    k = n // 2 + 3                                              # in the second of three slices
    assert R.accum_plan(n, H, W)["slices"] == 3 and R.accum_plan(n, H, W)["per_slice"] <= k < 2 * R.accum_plan(n, H, W)["per_slice"]
    scores = scores.copy()
    scores[k] = np.inf
    m = R.mask32(grid[k], shifts[k], cell, H, W)
    assert (m == 0).any() and (m > 0).any()
    for kernel in R.k5_kernels(cell4):
        got = run_k5(K, grid, shifts, scores, cell, H, W, scale, kernel)
        np.testing.assert_array_equal(np.isnan(got), m == 0, err_msg=str((cell4, kernel)))
        assert (got[m > 0] == np.inf).all(), (cell4, kernel)


def test_accumulate_limits(lib):
    """s = 65, and s = 64 on 2560 x 2560 (62 400 B of tap tables leave no room for one 4 116-byte mask), are XAI_E_UNSUPPORTED; a
    crop outside the up-sampled grid is XAI_E_SHAPE; acc is not written."""
    g, sh, sc, acc = Bytes(np.ones(65 * 65, np.uint8)), In(np.zeros(8, np.int32)), In(np.ones(8, np.float32)), Out(2 * 2560 * 2560)
    assert R.accum_stage(64, R.cell_of(2560, 2560, 64)) == 0
    assert lib.xai_rise_accum_f64(g.ptr, sh.ptr, sc.ptr, 1, 65, 1, 1, 8, 8, 1.0, acc.ptr, None) == UNSUPPORTED
    assert lib.xai_rise_accum_f64(g.ptr, sh.ptr, sc.ptr, 1, 64, 40, 40, 2560, 2560, 1.0, acc.ptr, None) == UNSUPPORTED
    assert lib.xai_rise_accum_f64(g.ptr, sh.ptr, sc.ptr, 1, 8, 1, 1, 10, 8, 1.0, acc.ptr, None) == SHAPE
    assert acc.untouched()


def test_rise_with_s_16_equals_the_oracle(K):
    """rise(..., s = 16) on 64 x 64 with the tiny classifier of test_rise_full_rise_vs_oracle: the last call, K5 at s = 16, used
    to be refused after every masked batch had been built and scored."""
    from oracle import rise as orise
    from xai_engine.rise import rise
    H = W = 64
    N, s, p1 = 120, 16, 0.5
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(2),
                              torch.nn.Flatten(), torch.nn.Linear(16, 5)).to(DEV).eval()
    image = torch.randn(1, 3, H, W)
    score = lambda b: torch.softmax(net(b), 1)[:, 2]          # noqa: E731
    grid, shifts, cell = orise.draw_grid_and_shifts((H, W), N, s, p1, np.random.RandomState(9))
    got = rise(None, image, None, DEV, N=N, s=s, p1=p1, score_fn=score, masks=(grid.astype(np.uint8), shifts, cell))

    def score_np(b):
        with torch.no_grad():
            return score(torch.from_numpy(b).to(DEV)).cpu().numpy()
    want = orise.rise(score_np, image.numpy(), N, s, p1, grid, shifts, cell)
    assert rel_inf(got.cpu().numpy(), want) <= 1e-5            # tests/test_gpu_kernels.py's TOL
