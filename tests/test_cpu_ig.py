"""tests/ig_restated.py checked on the host before a kernel is held to it: the fp32 restatements of the accumulate and IDGI
kernels against the oracle and the reference-made golden vectors, the cutoff against the reference's lines restated with torch's
CPU ops, fp32 inside the derived bounds around fp64 on every cell, the exact cases' own conditions, the launch choices of the
matrix at 256 CUs from the index arithmetic, what the bit comparisons of sumsq can tell apart, and the ledger of
tests/test_gpu_ig_edges.py from an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import ig_restated as R
from conftest import BAR, ROOT, load_golden, rel_inf
from oracle import ig as oig

F32 = np.float32
CUS = 256                   # MI355X


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def inside(got, want, bound):
    """largest |got - want| / bound; where the bound is 0 the two must be equal"""
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def cell_case(cell, cus=CUS):
    """-> the keyword arguments of accum_fp32 / accum64 / accum_bound for a cell of the matrix, on N(0, 1) data"""
    n_img = R.n_img_of(cell, cus)
    d = R.normal_accum_case(n_img, cell.n_steps, cell.C, cell.hw)
    return {"grads": d["grads"], "n_use": R.cell_n_use(cell, n_img), "x": d["x"], "base": d["base"] if cell.base == "tensor" else R.SCALAR_BASE,
            "w1": d["w1"] if cell.weights >= 1 else None, "w2": d["w2"] if cell.weights == 2 else None}


def held_to_fp64(got, case):
    """-> (fraction of accum_bound for out, for abs); both restatement and kernel output go through this"""
    o64, a64, _ = R.accum64(**case)
    bo, ba = R.accum_bound(**case)
    return inside(got[0], o64, bo), inside(got[1], a64, ba), o64, a64


# ---- restatements against the oracle and the golden vectors ------------------------------------------------------------------------

def test_accum_fp32_is_the_oracle_and_the_golden_vectors():
    """tests/golden/ig_small.npz holds the reference's own gradients, logits, IG and Left-IG maps (alpha_star 0.9, baseline 0):
    accum_fp32 on those gradients is inside BAR of the maps, and inside the derived bound of oracle.ig.accumulate (both lie
    within accum_bound of accum64, so within twice that of each other)."""
    g = load_golden("ig_small.npz")
    grads, x = g["gradients"].reshape(1, 50, 3, -1), g["x"].reshape(1, 3, -1)
    n_lig = R.cutoff(g["logits"], 0.9)
    assert n_lig == oig.left_cutoff(g["logits"], 0.9) and 1 < n_lig < 50
    for key, n_use in (("ig", 50), ("lig", n_lig)):
        out, out_abs = R.accum_fp32(grads, n_use, x, 0.0)
        assert rel_inf(out.reshape(3, 32, 32), g[key]) <= BAR
        orc = oig.accumulate(g["gradients"], n_use, g["x"][0], np.zeros_like(g["x"][0]))
        bound = R.accum_bound(grads, n_use, x, 0.0)[0]
        o64 = R.accum64(grads, n_use, x, 0.0)[0]
        assert inside(out, o64, bound) <= 1.0 and inside(orc.reshape(out.shape), o64, bound) <= 1.0
        assert inside(out, orc.reshape(out.shape).astype(np.float64), 2 * bound) <= 1.0
        np.testing.assert_array_equal(bits(out_abs), bits(np.abs((out[:, 0] + out[:, 1]) + out[:, 2])))


def test_idgi_fp32_is_the_golden_vector():
    g = load_golden("ig_small.npz")
    grads = g["gradients"].reshape(50, -1)
    sq = R.sumsq_fp32(grads)
    assert inside(sq, R.sumsq64(grads), R.sumsq_bound(grads)) <= 1.0
    got = R.idgi_fp32(grads, g["logits"], sq)
    assert rel_inf(got.reshape(3, 32, 32), g["idgi"]) <= BAR
    assert inside(got, R.idgi64(grads, g["logits"], sq)[0], R.idgi_bound(grads, g["logits"], sq)) <= 1.0


def test_accum_fp32_on_a_case_small_enough_to_follow_by_hand():
    d = R.normal_accum_case(1, 3, 2, 1, seed=7)
    g, x, b, w1, w2 = d["grads"][0, :, :, 0], d["x"][0, :, 0], d["base"][0, :, 0], d["w1"][0], d["w2"][0]
    out, out_abs = R.accum_fp32(d["grads"], 2, d["x"], d["base"])
    want = ((g[0] + g[1]) / F32(2)) * (x - b)
    np.testing.assert_array_equal(bits(out[0, :, 0]), bits(want))
    np.testing.assert_array_equal(bits(out_abs[0, 0]), bits(np.abs(want[0] + want[1])))
    out, _ = R.accum_fp32(d["grads"], 2, d["x"], 0.5, w1=d["w1"], w2=d["w2"])
    want = (((g[0] * w1[0]) * w2[0] + (g[1] * w1[1]) * w2[1]) / F32(3)) * (x - F32(0.5))           # the divisor stays n_steps
    np.testing.assert_array_equal(bits(out[0, :, 0]), bits(want))
    for n_use, clamped in ((0, 1), (-3, 1), (8, 3)):
        np.testing.assert_array_equal(bits(R.accum_fp32(d["grads"], n_use, d["x"], 0.0)[0]), bits(R.accum_fp32(d["grads"], clamped, d["x"], 0.0)[0]))
    acc = R.accum_add_fp32(d["grads"][0].reshape(3, 2), np.zeros(2, F32))
    np.testing.assert_array_equal(bits(acc), bits((g[0] + g[1]) + g[2]))
    np.testing.assert_array_equal(bits(R.finish_fp32(acc.reshape(1, 2, 1), 3, d["x"], d["base"])[0]), bits(R.accum_fp32(d["grads"], None, d["x"], d["base"])[0]))


# ---- the cutoff --------------------------------------------------------------------------------------------------------------------

def reference_lines(logits, alpha_star):
    """saliencyMethods.py:48-67 of the reference, restated with torch's CPU ops"""
    logits = torch.from_numpy(np.ascontiguousarray(logits, F32))
    cutoff_perc = torch.max(logits) * alpha_star
    if alpha_star == 1:
        return logits.shape[0]
    steps = torch.where(logits > cutoff_perc)[0]
    cutoff_step = int(steps[0]) if len(steps) != 0 else 1
    return 1 if cutoff_step == 0 else cutoff_step


@pytest.mark.parametrize("alpha", R.CUTOFF_ALPHAS + (R.NO_HIT_ALPHA,))
def test_cutoff_is_the_reference_on_every_planted_row(alpha):
    seen = {}
    for n in R.CUTOFF_STEPS:
        labels, rows = R.cutoff_rows(n, alpha)
        assert len(set(labels)) == len(labels)
        for label, row in zip(labels, rows):
            got = R.cutoff(row, alpha)
            assert got == reference_lines(row, alpha), (n, label)
            if alpha != 1.0:
                assert got == oig.left_cutoff(row, alpha), (n, label)
            assert 1 <= got <= n
            seen[(n, label)] = got
    if alpha == 1.0:
        assert all(v == n for (n, _), v in seen.items())
        return
    # the rows say what their labels say
    assert seen[(200, "hit_at_0")] == 1 and seen[(200, "hit_at_1")] == 1 and seen[(200, "hit_at_63")] == 63 and seen[(200, "hit_at_64")] == 64
    assert seen[(200, "hit_at_199")] == 199 and seen[(65, "hit_at_64")] == 64 and seen[(1, "hit_at_0")] == 1 and seen[(2, "hit_at_1")] == 1
    assert seen[(200, "hits_65_70")] == 65 and seen[(200, "hits_70_129")] == 70 and seen[(128, "hits_63_64")] == 63
    for n in (63, 200):
        assert {seen[(n, k)] for k in ("all_equal", "negative_max", "zero_max", "all_minus_inf", "nan_before_hit", "nan_after_hit", "nan_at_0")} == {1}
        assert seen[(n, "equal_to_thr_first")] == n - 2 and seen[(n, "several_maxima")] == n // 2
        # ... and without the NaN the same rows give a later step: dropping the NaN, as fmaxf does, is visible
        labels, rows = R.cutoff_rows(n, alpha)
        for k in ("nan_before_hit", "nan_after_hit", "nan_at_0"):
            row = rows[labels.index(k)]
            assert R.cutoff(np.where(np.isnan(row), F32(1), row), alpha) == n - 2


def test_threshold_is_an_fp32_product_and_strict():
    row = np.full(8, 1, F32)
    row[7], row[3], row[5] = 8, 4, np.nextafter(F32(4), F32(9))
    assert R.cutoff(row, 0.5) == 5
    thr = F32(F32(8) * F32(0.9))
    assert float(thr) != 8 * 0.9                      # the fp64 product is another number: a row sitting on fl32(thr) tells them apart
    row[3], row[5] = thr, np.nextafter(thr, F32(9))
    assert R.cutoff(row, 0.9) == 5 == reference_lines(row, 0.9)


# ---- fp32 inside the bound around fp64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", R.accum_cells(), ids=R.accum_name)
def test_accum_fp32_is_inside_the_derived_bound_around_accum64(cell):
    case = cell_case(cell)
    got = R.accum_fp32(**case)
    r_out, r_abs, o64, a64 = held_to_fp64(got, case)
    print(f"{cell.name}: out {r_out:.4f}, abs {r_abs:.4f} of the bound; rel_inf {rel_inf(got[0], o64):.2e} / {rel_inf(got[1], a64):.2e}")
    assert r_out <= 1.0 and r_abs <= 1.0 and rel_inf(got[0], o64) <= BAR and rel_inf(got[1], a64) <= BAR


@pytest.mark.parametrize("cell", R.SUMSQ_CELLS, ids=R.sumsq_name)
def test_sumsq_fp32_is_inside_the_derived_bound_around_sumsq64(cell):
    rows = R.sumsq_case(cell)
    for aligned in (True, False):
        got, want = R.sumsq_fp32(rows, aligned), R.sumsq64(rows)
        ratio = inside(got, want, R.sumsq_bound(rows, aligned))
        print(f"{R.sumsq_name(cell)} aligned={aligned}: {ratio:.4f} of the bound (n = {R.sumsq_chain(cell[1], R.sumsq_is_vector(cell[1], aligned))})")
        assert ratio <= 1.0 and rel_inf(got, want) <= BAR
    ints = R.sumsq_case(cell, integer=True)
    want = (ints.astype(np.int64) ** 2).sum(axis=1)
    assert want.max() < 2 ** 24
    for aligned in (True, False):
        np.testing.assert_array_equal(R.sumsq_fp32(ints, aligned).astype(np.int64), want)


@pytest.mark.parametrize("cell", R.IDGI_CELLS + (R.IDGI_CHAINED,), ids=R.idgi_name)
def test_idgi_fp32_is_inside_the_derived_bound_around_idgi64(cell):
    g, lg = R.idgi_case(cell)
    sq = R.sumsq_fp32(g)
    got, want = R.idgi_fp32(g, lg, sq), R.idgi64(g, lg, sq)[0]
    ratio = inside(got, want, R.idgi_bound(g, lg, sq))
    print(f"{R.idgi_name(cell)}: {ratio:.4f} of the bound (n = {R.idgi_chain(cell[0])}), rel_inf {rel_inf(got, want):.2e}")
    assert ratio <= 1.0 and rel_inf(got, want) <= BAR
    assert cell[0] < 3 or (np.diff(lg) < 0).any() and (np.diff(lg) > 0).any()


def test_a_zero_gradient_step_is_nan_everywhere_as_in_the_reference():
    g, lg = R.idgi_case(R.IDGI_ZERO_STEP, zero_step=2)
    sq = R.sumsq_fp32(g)
    assert sq[2] == 0 and (sq[[0, 1, 3]] > 0).all()
    assert np.isnan(R.idgi_fp32(g, lg, sq)).all()
    acc = np.zeros(g.shape[1], F32)
    with np.errstate(invalid="ignore"):
        for i in range(g.shape[0] - 1):                      # oracle.ig.idgi's loop
            sqi = g[i] * g[i]
            acc += sqi * (lg[i + 1] - lg[i]) / sqi.sum(dtype=F32)
    assert np.isnan(acc).all()


# ---- exact cases -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.PER_KERNEL)
def test_exact_accum_cases_meet_their_conditions_and_come_back_as_integers(name):
    cell = next(c for c in R.accum_cells() if c.name == name)
    n_img = R.n_img_of(cell, CUS)
    n_use = R.cell_n_use(cell, n_img)
    grads, x, base, out, out_abs = R.exact_accum_case(n_img, cell.n_steps, cell.C, cell.hw, n_use)
    assert R.exact_accum_case_holds(grads, x, base, out, out_abs, n_use)
    got = R.accum_fp32(grads, n_use, x, base)
    assert (got[0] == np.rint(got[0])).all()
    np.testing.assert_array_equal(got[0].astype(np.int64), out)
    np.testing.assert_array_equal(got[1].astype(np.int64), out_abs)
    if (np.asarray(n_use) < cell.n_steps).any():             # one step too many shows at every pixel of the image concerned
        late = R.accum_fp32(grads, np.asarray(n_use) + 1, x, base)[0]
        i = int(np.argmax(np.asarray(n_use) < cell.n_steps))
        assert (np.abs(late[i]) > 2 ** 16)[x[i] != base[i]].all()


# ---- the matrix --------------------------------------------------------------------------------------------------------------------

def test_accum_kernel_for_on_hand_worked_cases():
    L = R.accum_kernel_for
    assert L(32, 3, 224 * 224, True, False, 256) == ("ig_accum_stream_kernel", (256, 4, 1, 3, False), 512, 784)         # the benchmark
    assert L(2048, 3, 512, True, False, 256)[1][:3] == (256, 4, 1) and L(2047, 3, 512, True, True, 256) == ("ig_accum_stream_kernel", (64, 1, 5, 3, True), 4094, 64)
    assert L(1, 1, 4, True, False, 256) == ("ig_accum_stream_kernel", (64, 1, 5, 1, False), 1, 1)
    assert L(3, 3, 72, True, False, 256)[2:] == (1, 54) and L(3, 3, 260, True, False, 256)[2:] == (4, 49)
    assert L(1, 3, 256, False, False, 256) == ("ig_accum_kernel", (1, False), None, None) == L(1, 3, 197, True, False, 256)
    assert L(1, 2, 64, True, True, 256) == ("ig_accum_kernel", (4, True), None, None) and L(1, 2, 64, False, True, 256)[1] == (1, True)
    assert R.spellings("ig_accum_stream_kernel", (256, 4, 1, 3, False)) == ("ig_accum_stream_kernel<256,4,1,3,false>", "ig_accum_stream_kernelILi256ELi4ELi1ELi3ELb0EE")
    assert R.spellings("ig_accum_kernel", (4, True)) == ("ig_accum_kernel<4,true>", "ig_accum_kernelILi4ELb1EE")
    assert R.ran(["void(anonymousnamespace)::ig_accum_kernel<4,true>(floatconst*)", "Memcpy"], L(1, 2, 64, True, True, 256))
    assert not R.ran(["ig_accum_kernel<4,true>", "ig_accum_kernel<1,true>"], L(1, 2, 64, True, True, 256))
    assert not R.ran(["ig_accum_kernel<1,true>"], L(1, 2, 64, True, True, 256))


def test_the_matrix_reaches_every_kernel_and_flavour_at_256_cus():
    cells = R.accum_cells()
    by_name = {c.name: c for c in cells}
    assert len(by_name) == len(cells) and all(n in by_name for n in R.PER_KERNEL)
    launches = {c.name: R.cell_launch(c, CUS) for c in cells}
    chosen = {(l.kernel, l.args) for l in launches.values()}
    want = {("ig_accum_stream_kernel", shape + (C, w)) for shape in ((256, 4, 1), (64, 1, 5)) for C in (3, 1) for w in (False, True)}
    want |= {("ig_accum_kernel", (W, w)) for W in (4, 1) for w in (False, True)}
    assert want == chosen, want ^ chosen                    # all twelve instantiations ig_accum_impl can launch
    assert {launches[n][:2] for n in R.PER_KERNEL} == {("ig_accum_stream_kernel", (64, 1, 5, 3, False)), ("ig_accum_stream_kernel", (256, 4, 1, 3, False)),
                                                       ("ig_accum_kernel", (4, False)), ("ig_accum_kernel", (1, False))}
    # every kernel with a scalar and with a tensor baseline, and with w1 alone and w1 with w2
    for kernel in {(l.kernel, l.args[:-1]) for l in launches.values()}:
        mine = [c for c in cells if (launches[c.name].kernel, launches[c.name].args[:-1]) == kernel]
        assert {c.base for c in mine} == {"scalar", "tensor"}, kernel
        assert {1, 2} <= {c.weights for c in mine} or kernel[0].endswith("stream_kernel") and kernel[1][-1] == 1, kernel             # (C = 1: one of the two)
    # the small stream cells: every n_use around the 5-step unroll, on the device and from the host
    small = [c for c in cells if c.name.startswith("small_")]
    assert len(small) == 48 and all(launches[c.name].args[:3] == (64, 1, 5) for c in small)
    assert {u for c in small if c.mode == "dev" for u in c.n_use} == set(R.SMALL_USE) == {c.n_use for c in small if c.mode == "host"}
    assert {launches[c.name].grid for c in small if c.hw == 4} == {1} and launches["small_C3_hw72_B3_dev"].per == 54      # a last workgroup partly idle
    assert launches["small_C3_hw256_B3_dev"][2:] == (3, 64) and launches["small_C1_hw260_B3_none"][2:] == (4, 49)        # 65 items per image: workgroups straddle images
    # ig_accum_kernel<4>: both sides of the 8-step unroll
    v4 = [c for c in cells if c.name.startswith("v4_")]
    assert len(v4) == 20 and all(launches[c.name][:2] == ("ig_accum_kernel", (4, False)) for c in v4)
    # the misaligned cells: one operand each, all fall back to the scalar kernel
    off = [c for c in cells if c.off]
    assert [c.off for c in off] == list(R.OPERANDS) and all(launches[c.name][:2] == ("ig_accum_kernel", (1, False)) for c in off)
    assert R.accum_kernel_for(2, 3, 256, True, False, CUS).args == (64, 1, 5, 3, False)
    # the big cells, from the index arithmetic
    over, under, two = by_name["big_C3_over"], by_name["big_C3_under"], by_name["big_C1_two_rounds"]
    lo, lu, lt = launches[over.name], launches[under.name], launches[two.name]
    assert lo.args == (256, 4, 1, 3, False) and lu.args == (64, 1, 5, 3, False) and lt.args == (256, 4, 1, 1, False)
    assert R.n_img_of(over, CUS) * 128 - CUS * 1024 == 128 and CUS * 1024 - R.n_img_of(under, CUS) * 128 == 128          # one image either side
    assert lo.per == 513 and lo.per % 1024 != 0 and lt.per == 1025 > 1024
    assert R.n_img_of(two, CUS) * 128 == 512 * 1025                                                                          # every workgroup: one full round and one item
    for cell, launch in ((over, lo), (two, lt), (by_name["weighted_big_w1"], launches["weighted_big_w1"])):
        n_img = R.n_img_of(cell, CUS)
        nu = R.clamp_n_use(R.cell_n_use(cell, n_img), n_img, cell.n_steps)
        ragged = idle = 0
        for wg in (0, 1, launch.grid // 2, launch.grid - 1):
            rounds = R.stream_lanes(n_img, cell.hw, nu, launch, wg)
            for live, held in rounds:
                ragged += int(((held.max(axis=1) != held.min(axis=1)) & (live.sum(axis=1) >= 2)).sum())
                idle += int((~live).sum())
            if cell is two:
                assert len(rounds) == 2 and rounds[0][0].all() and rounds[1][0].sum() == 1
            if cell is over and wg == 0:
                assert len(rounds) == 1 and (rounds[0][0].sum(axis=1) >= 2).all()
        assert ragged > 0 and idle > 0, cell.name
    # 256 items of a lane's four lie 2 images apart at hw = 512: every lane of the big C = 3 cell holds several images
    assert 256 // (R.BIG_HW // 4) == 2
    assert len(set(R.ledger_names())) == len(R.ledger_names())


def test_store_and_stream_cells_reach_both_forms():
    cells = R.store_cells(CUS)
    assert {R.store_kernel_for(n, s == 0, d == 0) for n, s, d in cells} == {"store_stream_kernel", "store_stream_scalar_kernel"}
    trip = CUS * 8 * 256
    assert any(n // 4 > trip and R.store_kernel_for(n, s == 0, d == 0) == "store_stream_kernel" for n, s, d in cells)
    assert any(n > trip and R.store_kernel_for(n, s == 0, d == 0) == "store_stream_scalar_kernel" for n, s, d in cells)
    assert [R.store_kernel_for(4096, s == 0, d == 0) for s, d in ((0, 0), (1, 0), (0, 1))] == ["store_stream_kernel"] + ["store_stream_scalar_kernel"] * 2
    w = R.store_payload(1024).view(F32)
    assert np.isnan(w).any() and (R.store_payload(1024) == -2 ** 31).any() and ((np.abs(w) < 2.0 ** -126) & (w != 0)).any()
    assert {b for b, *_ in R.ADD_CELLS} == set(R.ADD_BATCHES) and {n for _, n, *_ in R.ADD_CELLS} >= set(R.ADD_ELEMS)


def test_sumsq_order_is_visible_in_the_bits():
    """What a norm cannot see and the bit comparison can: the kernel's tree differs from a left-to-right fp32 sum, and its
    vector form from its scalar form on the same row."""
    differs = forms = 0
    for cell in R.SUMSQ_CELLS:
        rows = R.sumsq_case(cell)
        plain = np.zeros(cell[0], F32)
        for v in rows.T:
            plain = plain + v * v
        differs += int((bits(R.sumsq_fp32(rows)) != bits(plain)).any())
        forms += int(R.sumsq_is_vector(cell[1], True) and (bits(R.sumsq_fp32(rows, True)) != bits(R.sumsq_fp32(rows, False))).any())
    assert differs >= 1 and forms >= 1
    rows = R.sumsq_case((3, 4096, 1))
    assert not R.sumsq_is_vector(4096, False) and (bits(R.sumsq_fp32(rows, True)) != bits(R.sumsq_fp32(rows, False))).any()
    assert [R.sumsq_trips(n, True) for n in (4, 4096, 4100, 150528)] == [4, 4, 8, 148] and [R.sumsq_trips(n, False) for n in (1, 1024, 4097, 150528)] == [1, 1, 5, 147]
    # 150528 = 36 * 4096 + 3072: threads below 768 make 37 trips, the others 36
    assert 150528 - 36 * 4096 == 4 * 768


# ---- the ledger --------------------------------------------------------------------------------------------------------------------

def test_ig_edge_ledger_is_complete_and_inside_its_conditions():
    """profiles/ig_edges_parity.json is the ledger tests/test_gpu_ig_edges.py wrote on an MI355X
    (XAI_PARITY_REPORT=profiles/ig_edges_parity.json python -m pytest tests/test_gpu_ig_edges.py -m gpu -q -x): the run passed,
    in deterministic mode; bit-for-bit and int64 comparisons leave no row, so it holds per cell the kernel's distance from the
    fp64 definition in the project's norm at the 1e-5 bar and, under /bound, as a fraction of the derived bound at 1.0."""
    led = json.load(open(os.path.join(ROOT, "profiles", "ig_edges_parity.json")))
    assert led["meta"]["exitstatus"] == 0 and led["meta"]["deterministic"] is True and led["meta"]["device"] != "cpu"
    rows = [r for r in led["comparisons"] if r["name"].startswith("ig_edges/")]
    assert sorted(r["name"] for r in rows) == R.ledger_names()
    for r in rows:
        if r["name"].endswith("/bound"):
            assert r["tol"] == 1.0 and r["norm"] == "abs", r
        else:
            assert r["tol"] == BAR and r["norm"] == "rel_inf", r
        assert 0.0 <= r["measured"] <= r["tol"], r
