"""tests/maskers_restated.py checked on the host before a kernel is held to it: the K11 restatement against the oracle
(torch's antialiased resize and the reference's norm_matrix) over the whole matrix, its dyadic cells against rationals, K11's
reciprocal-and-FMA division against the IEEE quotient on an adversarial set, the K14 / K16 cases against what a bit comparison
needs to see a contracted multiply-add, the K12 / K13 inputs against their own conditions, and the ledger of
tests/test_gpu_masker_edges.py from an MI355X."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import maskers_restated as R
from conftest import ROOT, check
from oracle import vit_cx as ocx

BAR = 4e-6            # tests/test_gpu_fuzz.py's bar for K11 against the oracle, times amp


def restated_against_oracle(cell):
    """-> (max err / amp over the rows the oracle defines, the rows it does not: 0/0).  amp as in tests/test_gpu_fuzz.py: the
    last-bit differences of two up-samples are amplified by |v|max / (max - min) of the row."""
    Rn, h, w, H, W = cell
    fmap = R.k11_maps(cell)
    up_ref = ocx.resize_maps(fmap, H, W).reshape(Rn, H * W)
    ref = ocx.norm_matrix(up_ref)
    ok = np.isfinite(ref).all(axis=1)
    span = up_ref.max(axis=1) - up_ref.min(axis=1)
    amp = np.maximum(1.0, np.abs(up_ref).max(axis=1) / np.where(span > 0, span, 1.0))
    got = R.up_rownorm(fmap, H, W)
    assert np.isnan(got[~ok]).all(), "the restatement is 0/0 where the oracle is"
    err = np.abs(got.astype(np.float64) - ref).max(axis=1) / amp
    return float(err[ok].max(initial=0.0)), [r for r in range(Rn) if not ok[r]]


def test_k11_restatement_is_the_oracle_within_the_projects_bar():
    """norm_matrix(resize_maps(...)) over every cell the entry point does not refuse, at 4e-6 * amp; the rows left out as 0/0
    are exactly the maps of one source pixel."""
    left_out, worst = {}, 0.0
    for cell in R.K11_CELLS:
        if R.k11_refuses(cell):
            continue
        ratio, nan_rows = restated_against_oracle(cell)
        print(f"{R.ledger_name(cell)}: err / amp = {ratio:.3e}")
        check(R.ledger_name(cell), ratio, 0, BAR, against="oracle.vit_cx", absolute=True)
        worst = max(worst, ratio)
        if nan_rows:
            left_out[cell] = nan_rows
    print(f"largest restatement-against-oracle err / amp: {worst:.3e}")
    assert left_out == {c: list(range(c[0])) for c in R.K11_CELLS if R.k11_is_constant(c) and not R.k11_refuses(c)}
    assert left_out == {(3, 1, 1, 4, 4): [0, 1, 2]}


def test_the_refused_cell_is_where_antialiasing_matters():
    """(2, 7, 3, 5, 259) shrinks along H: the oracle's antialiased resize and the two-tap formula differ by a sizeable part of
    the row span there (which is why the entry point refuses it), and by rounding only on its up-sampling twin."""
    assert [c for c in R.K11_CELLS if R.k11_refuses(c)] == [(2, 7, 3, 5, 259)]
    assert all(R.k11_refuses(c) for c in R.K11_REFUSED.values())
    assert restated_against_oracle((2, 7, 3, 5, 259))[0] > 1e-2
    assert restated_against_oracle((2, 5, 3, 7, 259))[0] <= BAR


def test_k11_matrix_reaches_what_it_says():
    """The VEC walk's d_row = 256 // W4 and d_col = 256 % W4 in every regime, Q < 256, the re-aligned tap table, the three
    limits alone and together."""
    vec = [c for c in R.K11_CELLS if c[4] % 4 == 0 and not R.k11_refuses(c)]
    w4 = {c[4] // 4 for c in vec}
    assert {3, 7, 56, 256, 257} <= w4
    assert any(256 // k == 0 for k in w4) and any(k == 256 for k in w4) and any(256 % k and k < 256 for k in w4)
    assert any(c[3] * c[4] // 4 < 256 for c in vec)
    assert any(256 % (c[4] // 4) and c[4] // 4 < 256 and c[3] * c[4] // 4 > 256 for c in vec)       # ... and walked: more than one step
    assert any((c[1] * c[4]) % 4 for c in R.K11_CELLS if not R.k11_refuses(c))
    lim = R.K11_LIMITS
    assert (1, 64, 64, 1024, 128) in R.K11_CELLS and (64 * 64, 64 * 128, 1024) == (lim["src"], lim["stretch"], lim["taps"])
    assert any(c[1] * c[4] == lim["stretch"] and c[1] * c[2] < lim["src"] for c in R.K11_CELLS)
    assert any(c[4] > 256 and c[4] % 4 for c in R.K11_CELLS if not R.k11_refuses(c))
    for cell in R.K11_CELLS:                                                   # another map per row
        m = R.k11_maps(cell)
        assert len({m[r].tobytes() for r in range(cell[0])}) == cell[0]


def test_identity_cell_is_rownorm_of_the_input():
    cell = (2, 6, 8, 6, 8)
    fmap = R.k11_maps(cell)
    np.testing.assert_array_equal(R.upsample(fmap, 6, 8).view(np.int32), fmap.view(np.int32))
    np.testing.assert_array_equal(R.up_rownorm(fmap, 6, 8).view(np.int32), R.rownorm(fmap.reshape(2, 48)).view(np.int32))
    np.testing.assert_array_equal(R.rownorm(fmap.reshape(2, 48)), ocx.norm_matrix(fmap.reshape(2, 48)))


def test_dyadic_cells_are_exact_in_any_order():
    """H / h and W / w powers of two, integer data: the taps and every product and sum of the restatement equal the rational
    ones (computed as one sum over four corners, another order), so these cells do not depend on the restatement's order of
    operations; the quotient is then one correctly rounded operation on exact operands, checked against rn32 of the rational
    quotient on the small cells."""
    dyadic = [c for c in R.K11_CELLS if R.k11_is_dyadic(c) and not R.k11_refuses(c)]
    assert set(dyadic) == {(3, 1, 1, 4, 4), (3, 1, 2, 1, 4), (5, 2, 2, 8, 8), (2, 6, 8, 6, 8), (3, 14, 14, 28, 28),
                           (2, 14, 14, 56, 28), (2, 14, 14, 224, 224), (1, 64, 64, 1024, 128)}
    for cell in dyadic:
        Rn, h, w, H, W = cell
        for n_in, n_out in ((h, H), (w, W)):
            i0, i1, l0, l1 = R.taps(n_in, n_out)
            want = R.taps_exact(n_in, n_out)
            assert [(int(a), int(b), Fraction(float(c)), Fraction(float(d))) for a, b, c, d in zip(i0, i1, l0, l1)] == want
        fmap = R.k11_maps(cell, "integer")
        assert np.array_equal(fmap, np.rint(fmap)) and np.abs(fmap).max() <= 8
        v = R.upsample(fmap, H, W)
        exact = R.upsample_exact(fmap, H, W)
        assert (exact == np.vectorize(lambda t: Fraction(float(t)), otypes=[object])(v)).all(), cell
        if H * W <= 28 * 28 and not R.k11_is_constant(cell):
            flat = exact.reshape(Rn, H * W)
            got = R.up_rownorm(fmap, H, W)
            for r in range(Rn):
                lo, hi = min(flat[r]), max(flat[r])
                want_row = np.array([R.rn32((t - lo) / (hi - lo)) for t in flat[r]], np.float32)
                np.testing.assert_array_equal(got[r].view(np.int32), want_row.view(np.int32))


def test_rn32_and_fma32_round_once():
    u = Fraction(1, 2 ** 24)
    assert R.rn32(1 + u) == np.float32(1) and R.rn32(1 + 3 * u) == np.float32(1 + 2.0 ** -22)          # ties to even
    assert R.rn32(1 + u + Fraction(1, 2 ** 80)) == np.float32(1 + 2.0 ** -23)
    assert R.rn32(Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148) and R.rn32(Fraction(1, 2 ** 150)) == 0    # subnormals
    assert R.rn32(Fraction(-5, 3)) == np.float32(-5 / 3)
    # a b = 2^-24 - 2^-70, c = 1 + 2^-23: the fp64 sum is the fp32 tie 1 + 2^-23 + 2^-24 and would round to even, 1 + 2^-22;
    # the exact sum lies below the tie
    a, b, c = np.float32(2.0 ** -24 * (1 + 2.0 ** -23)), np.float32(1 - 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    assert exact == 1 + Fraction(1, 2 ** 23) + Fraction(1, 2 ** 24) - Fraction(1, 2 ** 70)
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1 + 2.0 ** -22)
    assert R.fma32(a, b, c) == R.rn32(exact) == c
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal(2000).astype(np.float32), rng.standard_normal(2000).astype(np.float32)
    C = (-(A * B) + rng.standard_normal(2000).astype(np.float32) * np.float32(1e-6)).astype(np.float32)     # cancelling sums
    want = [R.rn32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(A, B, C)]
    np.testing.assert_array_equal(R.fma32(A, B, C).view(np.int32), np.array(want, np.float32).view(np.int32))


def test_div_by_is_the_ieee_quotient_on_the_adversarial_set():
    """K11 writes RN(q + r y) with y = RN(1 / span), q = RN(num y), r = num - q span.  Held to numpy's fp32 division for
    0 <= num <= span: span significands all ones (less 0 .. 4 ulps) and 1.0 (plus 0 .. 4 ulps: the powers of two), num = span,
    nextafter(span, 0), 0, around span / 2, significands near all ones, random draws; everything again scaled by 2^60 and 2^-60.
    The vectorised model is itself held to the all-rational one on a sample."""
    num, span = R.div_by_cases()
    assert len(num) > 20000
    got = R.div_by_model(num, span)
    want = (num / span).astype(np.float32)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert len(bad) == 0, [(float(num[i]).hex(), float(span[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]]
    for i in np.random.default_rng(1).choice(len(num), 1500, replace=False):
        assert R.div_by_exact(num[i], span[i]).view(np.int32) == got[i].view(np.int32), (float(num[i]).hex(), float(span[i]).hex())
    sig = span.view(np.uint32) & np.uint32(0x7FFFFF)
    assert (sig == 0x7FFFFF).sum() >= 3 * 14 and (sig == 0).sum() >= 3 * 14
    assert (num == span).sum() >= 400 and (num == 0).sum() >= 400 and (num == np.nextafter(span, np.float32(0))).sum() >= 400
    assert span.max() > 2.0 ** 60 and span.min() < 2.0 ** -60


def test_k14_and_k16_cases_can_see_a_contraction():
    """Every K14 case with a non-zero noise scale has elements with fl(fl(x m) + add) != fma(x, m, add); at scale 0 add is +-0
    and no element can (asserted too, so that the claim is not read more widely).  K16: the weighted sums of every case with
    more than one row differ from the chain of FMAs (one row: fl(v w) + 0 is the FMA)."""
    for cell in R.K14_CELLS:
        x, m, noise = R.k14_case(cell)
        assert (m == 0).any() or cell[0] * cell[2] < 5
        assert ((m == 1).any() and (m < 0).any() and (m > 1).any()) or cell[0] * cell[2] < 16
        for s in R.K14_SCALES:
            n = R.k14_contraction_sensitive(x, m, noise, s)
            assert (n > 0) == (s != 0), (cell, s, n)
        np.testing.assert_array_equal(R.causal_stack(x, m, noise, 0.1), ocx.causal_stack(x.reshape(cell[1], 1, -1), m, noise.reshape(cell[0], cell[1], 1, -1)).reshape(2 * cell[0], cell[1], -1))
    for N in R.K16_NS:
        for P in R.K16_PS:
            rows, w = R.k16_case(N, P)
            two, fused = R.masked_sums(rows, w)[0], R.masked_sums(rows, w, fused=True)[0]
            assert (two.view(np.int32) != fused.view(np.int32)).any() == (N > 1), (N, P)


def test_k12_and_k13_inputs_meet_their_own_conditions():
    """At 256 compute units the K12 matrix reaches several slices with R % 8 != 0, a short last slice in both forms and the
    32-slice cap; over a cell's rounds every listed position holds a row's min and a row's max; the K13 clusters are a singleton,
    an empty one and a scattered majority, and the order of addition decides bits there."""
    got = {c: R.k12_slices(*c, 256) for c in R.K12_CELLS}
    assert got == {(1, 1): 1, (1, 2): 1, (9, 1000): 1, (3, 4100): 5, (3, 4099): 5, (8, 1028): 2, (17, 2049): 3, (2, 40000): 32, (600, 2052): 1}
    assert R.k12_seams(4099, 5, False)[1:] == (819, 820) and R.k12_seams(1028, 2, True)[1:] == (512, 516)
    assert R.k12_seams(40000, 32, True)[1:] == (4 * 297, 4 * 313)
    for (Rn, P), slices in got.items():
        seams = sorted(set(R.k12_seams(P, slices, False)[0] + (R.k12_seams(P, slices, True)[0] if P % 4 == 0 else [])))
        at = R.k12_positions(P, seams)
        had_min, had_max = set(), set()
        inf_row, zero_row = R.k12_special_rows(Rn)
        for rnd in range(R.k12_rounds(Rn, P, seams)):
            x = R.k12_rows(Rn, P, seams, rnd)
            for r in range(Rn):
                if r == inf_row:
                    assert np.isinf(x[r]).sum() == 2 and np.isnan(R.rownorm(x)[r]).all()
                elif r == zero_row:
                    assert (x[r] == 0).sum() == 1 and np.signbit(x[r][x[r] == 0]).all() and x[r].min() == 0
                    out = R.rownorm(x)[r]
                    assert out.min() == 0 and not np.signbit(out).any()
                elif P > 2:
                    had_min.add(int(x[r].argmin()))
                    had_max.add(int(x[r].argmax()))
        if P > 2:
            assert had_min == set(at) and had_max == set(at), (Rn, P)
            assert {0, P - 1, P - 3} <= set(at) and all(s in at and s - 1 in at for s in seams)
    assert R.k12_rounds(2, 40000, R.k12_seams(40000, 32, True)[0]) <= 80
    offs, mem = R.K13_OFFS, R.K13_MEMBERS
    sizes = np.diff(offs)
    assert 1 in sizes and 0 in sizes and sizes.max() > R.K13_ROWS // 2
    assert len(set(mem.tolist())) == len(mem) == R.K13_ROWS - 1 and 4 not in mem          # row 4 belongs to no cluster
    big = mem[offs[2]:offs[3]]
    assert (np.diff(big) > 0).all() and (np.diff(big) > 1).any()
    for P in R.K13_PS:
        rows = R.k13_rows(P)
        fwd = R.cluster_sum(rows, mem, offs)
        rev = R.cluster_sum(rows, mem[::-1].copy(), (len(mem) - offs[::-1]).astype(np.int32))[::-1]
        assert (fwd.view(np.int32) != rev.view(np.int32)).any(), "the order of addition would not show"
        assert (fwd[1].view(np.int32) == 0).all()                               # the empty cluster: +0.0
    keep = np.array(sorted(mem.tolist()))
    lab = np.zeros(len(keep), np.int64)
    for k in range(len(offs) - 1):
        lab[np.isin(keep, mem[offs[k]:offs[k + 1]])] = k
    dense = {k: i for i, k in enumerate(sorted(set(lab.tolist())))}                 # the oracle has no empty clusters
    want = ocx.cluster_sums(R.k13_rows(1023)[keep], [dense[k] for k in lab])
    np.testing.assert_array_equal(R.cluster_sum(R.k13_rows(1023), mem, offs)[[0, 2, 3]], want)


def test_masker_edge_ledger_is_complete_and_inside_the_bar():
    """profiles/masker_edges_parity.json is the ledger tests/test_gpu_masker_edges.py wrote on an MI355X
    (XAI_PARITY_REPORT=profiles/masker_edges_parity.json python -m pytest tests/test_gpu_masker_edges.py -m gpu -q): the run
    passed; every kernel comparison in it is bit for bit and leaves no row, so it holds exactly the restatement-against-oracle
    rows, one per K11 cell that is not refused, each inside 4e-6 * amp."""
    led = json.load(open(os.path.join(ROOT, "profiles", "masker_edges_parity.json")))
    assert led["meta"]["exitstatus"] == 0 and led["meta"]["device"] != "cpu"
    rows = led["comparisons"]
    assert sorted(r["name"] for r in rows) == sorted(R.ledger_name(c) for c in R.K11_CELLS if not R.k11_refuses(c))
    for r in rows:
        assert r["tol"] == BAR and r["norm"] == "abs" and r["against"] == "oracle.vit_cx", r
        assert 0.0 <= r["measured"] <= BAR, r
