"""tests/rise_restated.py checked on the host before a kernel is held to it: the fp32 restatement of the RISE mask against the
oracle's scipy up-sampling and its fp64 formula inside a derived bound, the clip and the support of single grid cells exactly,
the sequential fp64 accumulation against its own error analysis, the host's dispatch and launch plans on hand-worked cases,
the completeness of the matrix, and the ledger of tests/test_gpu_rise_edges.py from an MI355X."""
import json
import os

import numpy as np
import pytest

import rise_restated as R
from conftest import ROOT, check
from oracle import rise as orise

S_SWEEP = (1, 2, 3, 7, 8, 11, 16, 17, 31, 64)


def restated_against_oracle(cell3):
    """max |upsampled32 - oracle.rise.upsample_grid| over every distinct grid of the cell (the whole up-sampling: every crop)."""
    H, W, s = cell3
    grid, _, cell = R.k4_case(cell3)
    up = np.array(cell) * (s + 1)
    worst = 0.0
    for g in np.unique(grid.reshape(len(grid), -1), axis=0).reshape(-1, s, s):
        want = orise.upsample_grid(g.astype(np.float32), up)
        assert want.dtype == np.float32
        worst = max(worst, float(np.abs(R.upsampled32(g, cell).astype(np.float64) - want).max()))
    return worst


@pytest.mark.parametrize("cell3", R.K4_CELLS, ids=R.k4_name)
def test_restatement_is_the_oracle_within_the_derived_bound(cell3):
    """Every (s, H, W) of the matrix, every grid family: scipy's zoom (fp64 inside, fp32 out) and the fp64 formula the oracle
    spells out, both within ORACLE_BOUND = 8.5 * 2^-24 (derived in rise_restated.py) -- not the 1e-6 of the older tests."""
    H, W, s = cell3
    err = restated_against_oracle(cell3)
    print(f"{R.mask_ledger_name(cell3)}: {err:.3e} (bound {R.ORACLE_BOUND:.3e})")
    check(R.mask_ledger_name(cell3), err, 0, R.ORACLE_BOUND, against="oracle.rise", absolute=True)
    grid, _, cell = R.k4_case(cell3)
    up = np.array(cell) * (s + 1)
    for g in grid[::R.N_SHIFTS]:
        formula = orise.upsample_grid_formula(g.astype(np.float32), up)
        assert np.abs(R.upsampled32(g, cell).astype(np.float64) - formula).max() <= R.ORACLE_BOUND


def test_the_bound_is_not_slack_by_orders_of_magnitude():
    """Over s in {1, 2, 3, 7, 8, 11, 16, 17, 31, 64} and cells 1 .. 7 the worst |restatement - oracle| is one ulp of 1 (2^-23):
    the bound of 4.25 ulp could not hide a wrong tap or a term left out, which move a mask by a weight."""
    worst = 0.0
    for s in S_SWEEP:
        for cell in ((1, 1), (3, 4), (7, 5)) if s < 31 else ((1, 2),):
            for f in ("one", "hole", "checker", "p0.5"):
                g = R.family_grid(f, s)
                want = orise.upsample_grid(g.astype(np.float32), np.array(cell) * (s + 1))
                worst = max(worst, float(np.abs(R.upsampled32(g, cell).astype(np.float64) - want).max()))
    print(f"worst |restatement - oracle| = {worst:.3e}")
    assert 0 < worst <= R.ORACLE_BOUND and R.ORACLE_BOUND < 5 * 2.0 ** -23 < 1e-6


def test_taps_are_the_oracles_taps_rounded_once():
    for n_in, n_out in ((1, 10), (2, 15), (7, 40), (8, 9), (8, 252), (17, 54), (64, 130)):
        i0, i1, t = R.taps(n_in, n_out)
        o0, o1, ot = orise.taps_1d(n_in, n_out)
        np.testing.assert_array_equal(i0, o0)
        np.testing.assert_array_equal(i1, np.maximum(o1, 0))
        np.testing.assert_array_equal(t.view(np.int32), ot.astype(np.float32).view(np.int32))
        assert i0.min() >= 0 and i0.max() == n_in - 1 and i1.min() >= 0 and i1.max() <= n_in - 1 and (t >= 0).all() and (t < 1).all()
    assert (R.taps(1, 10)[1] == 0).all()                                        # n_in == 1: the neighbour is clamped


def test_constant_grids_are_exact_and_the_clip_is_what_makes_them_so():
    """All ones -> exactly 1.0, all zeros -> exactly +0.0, at every s of the sweep; the raw four-term blend of an all-one grid is
    1 - 2^-24 or 1 + 2^-23 at some pixels, so without the clip to the grid's own [min, max] this fails."""
    off = 0
    for s in S_SWEEP:
        cell = (3, 5) if s < 31 else (1, 2)
        one, zero = R.upsampled32(np.ones((s, s), np.uint8), cell), R.upsampled32(np.zeros((s, s), np.uint8), cell)
        assert (one.view(np.int32) == np.float32(1).view(np.int32)).all(), s
        assert (zero.view(np.int32) == 0).all(), s
        raw = R.raw_blend32(np.ones((s, s), np.uint8), cell)
        assert np.abs(raw.astype(np.float64) - 1).max() <= 2.0 ** -23
        off += int((raw != 1).sum())
        hole = R.upsampled32(R.family_grid("hole", s), cell)
        assert hole.max() <= 1 and hole.min() >= 0
    assert off > 0, "no all-one grid needs the clip: the test could not see it dropped"


@pytest.mark.parametrize("s", [2, 3, 7, 8, 17])
def test_impulses_have_exactly_the_support_of_their_taps(s):
    """One 1 at (0, s - 1), and one at (s - 1, 0): the mask is non-zero exactly where a row tap touches the row and a column tap
    the column (a tap touches with weight 1 - t > 0 always, with weight t only when t > 0); the two supports differ, so rows
    and columns swapped show."""
    cell = (3, 4)
    r0, r1, tr = R.taps(s, (s + 1) * cell[0])
    c0, c1, tc = R.taps(s, (s + 1) * cell[1])
    rows = lambda k: (r0 == k) | ((r1 == k) & (tr > 0))          # noqa: E731
    cols = lambda k: (c0 == k) | ((c1 == k) & (tc > 0))          # noqa: E731
    a = R.upsampled32(R.family_grid("impulse0e", s), cell)
    b = R.upsampled32(R.family_grid("impulsee0", s), cell)
    np.testing.assert_array_equal(a != 0, np.outer(rows(0), cols(s - 1)))
    np.testing.assert_array_equal(b != 0, np.outer(rows(s - 1), cols(0)))
    assert not np.array_equal(a, b) and (s == 2 or not np.array_equal(a != 0, b != 0))     # s == 2: every tap touches both
    ay, ax = np.unravel_index(a.argmax(), a.shape)
    assert a.max() <= 1 and (a.min() == 0 or s == 2) and ay < cell[0] and ax >= a.shape[1] - cell[1]     # the peak sits in the corner cell


def test_accum64_is_a_sequential_fp64_sum_and_lies_where_its_analysis_says():
    grid, shifts, scores, cell, scale = R.k5_case((30, 45, 7, 130))
    got = R.accum64(grid, shifts, scores, cell, 30, 45, scale)
    masks = R.masks32(grid, shifts, cell, 30, 45)
    acc = np.zeros((30, 45))
    for n in range(130):
        acc = acc + np.float64(scores[n]) * masks[n].astype(np.float64)
    np.testing.assert_array_equal(got, acc * scale)
    exact = np.array([[np.sum([np.longdouble(scores[n]) * np.longdouble(masks[n, y, x]) for n in range(130)]) for x in range(45)]
                      for y in range(30)]) * np.longdouble(scale)
    mag = R.accum_magnitude(grid, shifts, scores, cell, 30, 45, scale)
    assert (np.abs(got - exact).astype(np.float64) <= R.accum_bound(130, mag)).all()
    carried = np.random.default_rng(1).standard_normal((30, 45))
    np.testing.assert_array_equal(R.accum64(grid, shifts, scores, cell, 30, 45, scale, acc0=carried), carried + got)
    np.testing.assert_array_equal(R.accum64(grid, shifts, scores, cell, 30, 45, scale, rows=[0, 29]), got[[0, 29]])
    # against the oracle's masks the difference is the masks' (ORACLE_BOUND each), not the summation's
    want = (scores.reshape(-1, 1).astype(np.float64) * orise.masks_from(grid.astype(np.float32), shifts, (30, 45), np.array(cell))
            .reshape(130, -1)).sum(0).reshape(30, 45) * scale
    assert np.abs(got - want).max() <= R.ORACLE_BOUND * scale * np.abs(scores).sum() + R.accum_bound(130, mag).max()


@pytest.mark.parametrize("cell4,kernel", R.bounded_rows(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_the_stated_accumulate_bound_covers_the_rigorous_one_on_every_bounded_cell(cell4, kernel):
    """accum_bound is (n + 2) u of the magnitude, the error of one sum in any order; the difference of two sums can be twice that
    on adversarial data.  running_error is rigorous for the cell's own data and slice plan, and is below accum_bound at every
    pixel compared: on these inputs the stated condition is one a correct kernel meets."""
    H, W, s, n = cell4
    grid, shifts, scores, cell, scale = R.k5_case(cell4)
    plan = R.accum_plan(n, H, W, R.accum_stage(s, cell, kernel))
    rows = R.LONG_ROWS if cell4 in R.K5_LONG else None
    mag = R.accum_magnitude(grid, shifts, scores, cell, H, W, scale, rows=rows)
    rig = R.running_error(grid, shifts, scores, cell, H, W, scale, plan, rows=rows)
    assert (rig <= R.accum_bound(n, mag)).all(), float((rig / np.maximum(R.accum_bound(n, mag), 1e-300)).max())
    assert (mag > 0).any()


def test_plans_and_dispatch_on_hand_worked_cases():
    """The issue's LDS table for the generic accumulate kernel, now as masks staged per round; slices and rounds; the apply
    kernel chosen from s, W and the alignments."""
    lds = lambda s, H: (s + 1) * 2 * -(-H // s) * 12 + 256 * (20 + s * s)                    # noqa: E731
    assert (lds(14, 224), lds(15, 64), lds(15, 224), lds(16, 32)) == (61056, 64640, 68480, 71472)
    assert R.accum_stage(14, R.cell_of(224, 224, 14)) == 256 and R.accum_stage(15, R.cell_of(64, 64, 15)) == 256
    assert R.accum_stage(15, R.cell_of(224, 224, 15)) == (65536 - 5760) // 245 == 243
    assert R.accum_stage(16, R.cell_of(32, 32, 16)) == (65536 - 816) // 276 == 234
    assert R.accum_stage(64, R.cell_of(64, 128, 64)) == (65536 - 2340) // 4116 == 15
    assert R.accum_stage(8, (28, 28)) == 256 and R.accum_stage(8, (28, 28), "generic") == 256
    assert all(R.accum_stage(s, R.cell_of(224, 224, s)) >= 14 for s in range(1, 65))             # every s K4 accepts, at 224 x 224
    assert R.accum_stage(64, R.cell_of(2560, 2560, 64)) == 0                                      # 62 400 B of taps: not one mask
    assert R.accum_plan(40, 224, 224) == {"slices": 1, "per_slice": 40, "last_slice": 40, "rounds": 1, "last_round": 40, "stage": 256}
    assert R.accum_plan(120, 64, 64)["slices"] == 2
    p = R.accum_plan(8000, 224, 224)
    assert (p["slices"], p["per_slice"], p["last_slice"], p["rounds"], p["last_round"]) == (11, 728, 720, 3, 208)
    p = R.accum_plan(514, 512, 512)
    assert (p["slices"], p["per_slice"], p["rounds"], p["last_round"]) == (2, 257, 2, 1)
    p = R.accum_plan(130, 32, 32)
    assert (p["slices"], p["per_slice"], p["last_slice"]) == (3, 44, 42)
    assert R.accum_plan(40, 64, 128, 15)["rounds"] == 3 and R.accum_plan(40, 64, 128, 15)["last_round"] == 10
    assert R.apply_path(8, 224) == "s8" and R.apply_path(8, 224, grid_aligned8=False) == "v4"
    assert R.apply_path(8, 224, aligned16=False) == "scalar" and R.apply_path(8, 45) == "scalar" and R.apply_path(7, 224) == "v4"
    assert R.apply_flavour(240, 3, 224, 224, True, False) == (True, True) and R.apply_flavour(80, 3, 224, 224, True, True) == (False, True)
    assert R.apply_flavour(2049, 4, 64, 64, True, False) == (True, False) and R.apply_flavour(2048, 4, 64, 64, True, False) == (False, False)


def test_the_matrix_reaches_what_it_says():
    paths = {c: R.apply_path(c[2], c[1]) for c in R.K4_CELLS}
    assert set(paths.values()) == {"s8", "v4", "scalar"}
    assert any(p == "scalar" and c[2] == 8 for c, p in paths.items()) and any(p == "scalar" and c[2] != 8 for c, p in paths.items())
    assert {R.apply_flavour(60, C, 32, 32, True, True) for C in R.K4_CHANNELS} == {(False, True), (False, False)}   # C3, NT = false
    assert {1, 17, 64} <= {c[2] for c in R.K4_CELLS} and any(c[0] < c[2] for c in R.K4_CELLS)
    assert any(c[0] * c[1] == 4 * R.BLOCK for c in R.K4_CELLS if paths[c] == "s8")                     # exactly one workgroup
    assert any(c[0] * c[1] < R.BLOCK for c in R.K4_CELLS) and any((c[0] * c[1]) % (4 * R.BLOCK) and c[0] * c[1] > 4 * R.BLOCK for c in R.K4_CELLS)
    last = [R.reaches_last_row(c) for c in R.K4_CELLS]
    assert any(r for r, _ in last) and any(c for _, c in last)
    assert not any(r or c for cell3, (r, c) in zip(R.K4_CELLS, last) if cell3 not in R.K4_CELL_OVERRIDE)   # never with ceil(H / s)
    for cell3 in R.K4_CELLS:
        H, W, s = cell3
        grid, shifts, cell = R.k4_case(cell3)
        assert H + cell[0] - 1 <= (s + 1) * cell[0] and W + cell[1] - 1 <= (s + 1) * cell[1]
        assert len(grid) == len(R.GRID_FAMILIES) * R.N_SHIFTS and (shifts >= 0).all() and (shifts < np.array(cell)).all()
        ext = {tuple(x) for x in shifts[:4].tolist()}
        assert ext == {(a, b) for a in (0, cell[0] - 1) for b in (0, cell[1] - 1)}
        assert not grid[:5].any() and grid[5:10].all() and grid[10:35].reshape(25, -1).sum(1).tolist() == [1] * 25
    # the NT instantiations: the smallest batch over 128 MiB at 64 x 64, C = 3 and C = 4, masked and masks together
    for C in (3, 4):
        n = R.NT_BYTES // (64 * 64 * 4 * (C + 1)) + 1
        assert R.apply_flavour(n, C, 64, 64, True, True) == (True, C == 3) and R.apply_flavour(n - 1, C, 64, 64, True, True)[0] is False
    # accumulate plans, on both kernels
    for kernel in ("s8", "generic"):
        cells = [c for c in R.K5_ONE_SLICE + R.K5_BOUNDED + R.K5_LONG + R.K5_LARGE_S if kernel in R.k5_kernels(c)]
        plans = [R.accum_plan(c[3], c[0], c[1], R.accum_stage(c[2], R.cell_of(*c[:3]), kernel)) for c in cells]
        assert any(p["slices"] == 1 for p in plans)
        assert any(p["slices"] > 1 and p["last_slice"] < p["per_slice"] for p in plans)
        assert any(p["slices"] > 1 and p["per_slice"] > 256 and p["last_round"] == 1 for p in plans)
    assert all(R.accum_plan(c[3], c[0], c[1])["slices"] == 1 and c[3] <= 64 for c in R.K5_ONE_SLICE)
    large = [R.accum_plan(c[3], c[0], c[1], R.accum_stage(c[2], R.cell_of(*c[:3]))) for c in R.K5_LARGE_S]
    assert all(p["stage"] < 256 for p in large) and any(p["rounds"] > 1 for p in large) and any(p["slices"] > 1 for p in large)
    assert {c[2] for c in R.K5_LARGE_S} == {15, 16, 17, 33, 64}
    for c in R.K5_BOUNDED + R.K5_LONG + R.K5_LARGE_S:                           # what an over-reading last slice would reach is padded
        p = R.accum_plan(c[3], c[0], c[1])
        assert p["slices"] * p["per_slice"] - c[3] < R.PAD_MASKS


def test_rise_edge_ledger_is_complete_and_inside_its_conditions():
    """profiles/rise_edges_parity.json is the ledger tests/test_gpu_rise_edges.py wrote on an MI355X
    (XAI_PARITY_REPORT=profiles/rise_edges_parity.json python -m pytest tests/test_gpu_rise_edges.py -m gpu -q): the run passed;
    every bit-for-bit comparison leaves no row, so it holds one row per K4 cell (the restatement against the oracle with that
    machine's scipy, at ORACLE_BOUND) and one per bounded K5 cell and kernel (|K5 - accum64| / accum_bound, at 1.0)."""
    led = json.load(open(os.path.join(ROOT, "profiles", "rise_edges_parity.json")))
    assert led["meta"]["exitstatus"] == 0 and led["meta"]["device"] != "cpu"
    rows = [r for r in led["comparisons"] if r["name"].startswith("rise_edges/")]
    assert sorted(r["name"] for r in rows) == R.ledger_names()
    for r in rows:
        if r["name"].startswith("rise_edges/mask_vs_oracle/"):
            assert r["tol"] == R.ORACLE_BOUND and r["norm"] == "abs" and r["against"] == "oracle.rise", r
        else:
            assert r["tol"] == 1.0 and r["norm"] == "abs" and r["against"] == "fp64 restatement", r
        assert 0.0 <= r["measured"] <= r["tol"], r
