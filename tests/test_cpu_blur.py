"""tests/blur_restated.py checked on the host before a kernel is held to it: the fp64 restatement against the oracle's dense
blur and the reference-made goldens, the derived error bound against an fp32 emulation of the tap chains over the whole GPU
matrix, the exact-integer cases against their own conditions, and the ledger of tests/test_gpu_blur_edges.py from an MI355X."""
import json
import os

import numpy as np
import pytest

import blur_restated as R
from conftest import ROOT, load_golden, rel_inf
from oracle import perturb as op

TOL = 2e-6            # tests/test_oracle_golden.py's: fp32 results restated, sums may associate differently


def _dense_kernel(k_v, k_h):
    kern = np.zeros((3, 3, len(k_v), len(k_h)))
    kern[0, 0] = kern[1, 1] = kern[2, 2] = np.outer(k_v, k_h)
    return kern


@pytest.mark.parametrize("klen,shape", [(1, (1, 1)), (3, (5, 7)), (5, (2, 9)), (9, (11, 6)), (31, (20, 28))])
def test_blur64_is_the_oracles_dense_blur_on_asymmetric_taps(klen, shape):
    """oracle.perturb.blur_dense (the zero-padded dense cross-correlation conv2d means) with outer(k, k), and with outer(k_v, k_h)
    of two different vectors: which vector runs along which axis and the tap direction are the oracle's.  On the integer data of
    exact_case both are exact, so they agree to the last bit (the oracle accumulates in fp32; float data would show its rounding,
    not fp64's); on N(0, 1) data within the oracle's own fp32 chain of klen^2 products."""
    x, k, want = R.exact_case(klen, (2, 3) + shape, 5)
    k_v = R.exact_case(klen, (1, 1, 1, 1), 6)[1]
    assert klen == 1 or not np.array_equal(k, k_v)
    np.testing.assert_array_equal(R.blur64(x, k, k), want)
    np.testing.assert_array_equal(op.blur_dense(x, _dense_kernel(k, k)).astype(np.float64), R.blur64(x, k, k))
    np.testing.assert_array_equal(op.blur_dense(x, _dense_kernel(k_v, k)).astype(np.float64), R.blur64(x, k, k_v))
    if klen > 1:
        assert not np.array_equal(R.blur64(x, k, k_v), R.blur64(x, k_v, k)), "the case cannot tell the axes apart"
        assert not np.array_equal(R.blur64(x, k, k), R.blur64(x, k[::-1], k)), "the case cannot tell the tap direction"
    xf, kf = R.normal_case(klen, (2, 3) + shape, 7)
    kv = R.taps(klen, 8)
    n = klen * klen + 1                                       # klen^2 products, each rounded, then as many fp32 adds
    slack = n * R.U / (1 - n * R.U) * R.blur64(np.abs(xf), np.abs(kf), np.abs(kv)) + 1e-30
    got = op.blur_dense(xf, _dense_kernel(kv.astype(np.float64), kf.astype(np.float64)))
    assert (np.abs(got - R.blur64(xf, kf, kv)) <= slack).all()


def test_blur64_reproduces_the_reference_made_goldens():
    g = load_golden("kern.npz")
    for klen, sig, xk, wk in ((31, 31, "blur_x", "blur_31_31"), (11, 5, "blur_x", "blur_11_5"), (31, 31, "blur_small_x", "blur_small_31_31")):
        v = op.gkern1d(klen, sig).astype(np.float32)
        assert rel_inf(R.blur64(g[xk], v, v), g[wk]) <= TOL, (klen, sig, xk)


@pytest.mark.parametrize("klen", R.KLENS + R.LONG_KLENS)
def test_an_fp32_tap_chain_stays_inside_the_bound(klen):
    """Every cell of the GPU matrix with the inputs the GPU test uses: the chains in numpy fp32 with a separate multiply and add
    (never better than the kernel's FMA) lie inside bound() at every pixel, and not by orders of magnitude -- the largest ratio
    over a klen's shapes is above 1 / (4 klen), so the bound could not hide an error a few roundings large."""
    worst = 0.0
    for kk, shape in R.cells():
        if kk != klen:
            continue
        x, k = R.normal_case(klen, R.PLANES + shape, 1)
        ratio = np.abs(R.chain32(x, k).astype(np.float64) - R.blur64(x, k, k)) / R.bound(x, k)
        assert ratio.max() <= 1.0, (klen, shape, ratio.max())
        worst = max(worst, float(ratio.max()))
    print(f"klen {klen}: largest |chain32 - blur64| / bound = {worst:.3f}")
    assert worst >= 1.0 / (4 * klen) or klen == 1, worst          # one tap: one exact-or-once-rounded product per pass


def test_the_bound_is_the_stated_formula_on_a_case_worked_by_hand():
    """x = [[1, -2]], k = [3, 5, -7] (r = 1): |k| *h |x| = [5 + 14, 3 + 10] = [19, 13], t = [5 + 14, 3 - 10] = [19, -7];
    one row, so the vertical pass sees the centre tap alone: e2 = 5 (g (|t| + e1) + e1), g = 3u / (1 - 3u)."""
    g = 3 * R.U / (1 - 3 * R.U)
    e1 = g * np.array([19.0, 13.0])
    want = 5 * (g * (np.array([19.0, 7.0]) + e1) + e1) + 6 * 2.0 ** -149
    np.testing.assert_allclose(R.bound(np.array([[1.0, -2.0]]), [3.0, 5.0, -7.0]), want.reshape(1, 2), rtol=1e-15)
    np.testing.assert_array_equal(R.blur64(np.array([[1.0, -2.0]]), [3.0, 5.0, -7.0], [1.0, 2.0, 4.0]), [[38.0, -14.0]])


@pytest.mark.parametrize("klen", R.KLENS + R.LONG_KLENS)
def test_exact_cases_meet_their_own_conditions(klen):
    """Distinct signed non-zero integer taps without symmetry, data in [-2, 2], (sum |k|)^2 max |x| < 2^24 (asserted inside
    exact_case too); the fp32 chain -- any chain -- then returns the int64 correlation element for element."""
    for shape in (R.SHAPES if klen in R.KLENS else R.LONG_SHAPES):
        x, k, want = R.exact_case(klen, R.PLANES + shape, 2)
        assert x.dtype == k.dtype == np.float32 and want.dtype == np.int64 and want.shape == x.shape
        ki = k.astype(np.int64)
        assert len(set(ki.tolist())) == klen and (ki != 0).all() and np.abs(ki).max() <= (klen + 1) // 2
        assert klen == 1 or not np.array_equal(ki, ki[::-1])
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 2
        assert int(np.abs(ki).sum()) ** 2 * 2 < 2 ** 24
        assert np.abs(want).max() < 2 ** 24
        np.testing.assert_array_equal(R.chain32(x, k), want.astype(np.float32))
        np.testing.assert_array_equal(R.blur64(x, k, k), want)
        if klen > 1 and min(shape) > 1:
            assert not np.array_equal(R.blur64(x, k, k[::-1]), want), "a reversed vertical pass would pass"
            assert not np.array_equal(R.blur64(x, k[::-1], k), want), "a reversed horizontal pass would pass"


def test_impulse_responses_are_the_restatements():
    """impulse_response (what the GPU test compares bits with) is blur64 of the impulse wherever fp64 has nothing to round away,
    on a footprint clipped at two borders; and the positions cover corners, seams and an interior pixel without repeats."""
    k = R.taps(31, 3)
    want, foot = R.impulse_response(k, 17, 65, 16, 64)
    x = np.zeros((17, 65))
    x[16, 64] = 1.0
    np.testing.assert_array_equal(want, R.blur64(x, k, k).astype(np.float32))
    assert foot.sum() == 16 * 16 and foot[1:, 49:].all() and np.array_equal(foot, want != 0)
    assert R.impulse_positions(1, 1) == [(0, 0)]
    assert R.impulse_positions(17, 65) == [(0, 0), (0, 64), (16, 0), (16, 64), (15, 63), (5, 43)]
    assert len(R.impulse_positions(33, 129)) == 9


def test_blur_edge_ledger_is_complete_and_inside_the_bound():
    """profiles/blur_edges_parity.json is the ledger tests/test_gpu_blur_edges.py wrote on an MI355X
    (XAI_PARITY_REPORT=profiles/blur_edges_parity.json python -m pytest tests/test_gpu_blur_edges.py -m gpu -q): the run passed, in
    deterministic mode; it holds exactly one row per cell of the matrix and form (K.blur_sep, and the two 1-D passes); every row's
    tolerance is the derived condition 1.0 and every measured |got - blur64| / bound is at most that."""
    led = json.load(open(os.path.join(ROOT, "profiles", "blur_edges_parity.json")))
    assert led["meta"]["exitstatus"] == 0 and led["meta"]["deterministic"] is True
    rows = [r for r in led["comparisons"] if r["name"].startswith("blur_edges/")]
    want = sorted(R.ledger_name(k, s, f) for k, s in R.cells() for f in R.FORMS)
    assert len(want) == 2 * (len(R.KLENS) * len(R.SHAPES) + len(R.LONG_KLENS) * len(R.LONG_SHAPES))
    assert sorted(r["name"] for r in rows) == want
    for r in rows:
        assert r["tol"] == 1.0 and r["norm"] == "abs" and r["against"] == "fp64 restatement", r
        assert 0.0 <= r["measured"] <= 1.0, r
