"""tests/cam_restated.py checked on the host before a kernel is held to it: the fp32 and fp64 restatements of Grad-CAM against
the oracle and the reference-made golden vectors, the bilinear restatement against the oracle bit for bit and against torch's
CPU interpolation inside the derived bound, fp32 inside the derived bound around fp64 on every cell of both matrices, the
host's launch choices on hand-worked cases, the completeness of the matrices, the exact cases' own conditions and what they can
tell apart, and the ledger of tests/test_gpu_cam_edges.py from an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import cam_restated as R
from conftest import BAR, ROOT, load_golden, rel_inf
from oracle import gradcam as ogc

F32 = np.float32
WAVES_DRY = R.WAVES          # a tail above 16 channels: some wave's trip holds a channel at u = 0, 1 and none at a later u


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def inside(got, want, bound):
    """largest |got - want| / bound; where the bound is 0 the two must be equal"""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def test_launch_choices_on_hand_worked_cases():
    assert [R.ppl_for(hw) for hw in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [R.unroll_for(p) for p in (1, 2, 4, 8, 16)] == [8, 8, 4, 2, 2]
    assert R.slices_for(1, 1) == (1, 1) and R.slices_for(1, 127) == (1, 127) and R.slices_for(1, 128) == (2, 64)
    assert R.slices_for(1, 129) == (2, 65) and R.slice_lengths(1, 129) == [65, 64]
    assert R.slices_for(3, 200) == (3, 67) and R.slice_lengths(3, 200) == [67, 67, 66]
    assert R.slices_for(1, 1030) == (16, 65) and R.slice_lengths(1, 1030) == [65] * 15 + [55]
    assert R.slices_for(1, 2048) == (16, 128) and R.slices_for(1, 4096) == (16, 256)
    assert R.slices_for(64, 256) == (1, 256) and R.slices_for(63, 256) == (4, 64) and R.slices_for(1, 256, have_ws=False) == (1, 256)
    assert R.workspace_floats(1, 127, 49) == 0 and R.workspace_floats(3, 200, 49) == 3 * 3 * 49 and R.workspace_floats(64, 256, 49) == 0
    assert R.cam_chain(1, 2048, 49) == 1 + 6 + 1 + 1 + 8 + 16 + 16 and R.cam_chain(1, 17, 1024) == 16 + 6 + 1 + 1 + 2 + 16


def test_cam_restatements_are_the_oracle_and_the_golden_vectors():
    """The existing bar of the Grad-CAM tests: max |d| / max |cam without ReLU| <= 1e-5, for both restatements, against
    oracle.gradcam.cam_reduce and against tests/golden/cam.npz (made by the reference's own CAM code)."""
    g = load_golden("cam.npz")
    for tag in "abc":
        act, grad = g[f"{tag}_act"], g[f"{tag}_grad"]
        scale = np.abs(g[f"{tag}_cam"]).max()
        for relu, key in ((False, "_cam"), (True, "_cam_relu")):
            for mine in (R.cam_fp32(act, grad, relu), R.cam64(act, grad, relu)):
                assert np.abs(mine - g[tag + key]).max() / scale <= BAR
                assert np.abs(mine - ogc.cam_reduce(act, grad, relu=relu)).max() / scale <= BAR
        assert R.cam_fp32(act, grad, False).dtype == F32
    act, grad = R.normal_case(2, 200, 5, 13)
    scale = np.abs(ogc.cam_reduce(act, grad, relu=False)).max()
    for ws in (True, False):
        assert np.abs(R.cam_fp32(act, grad, True, have_ws=ws) - ogc.cam_reduce(act, grad)).max() / scale <= BAR


def test_cam_fp32_on_a_case_small_enough_to_follow_by_hand():
    """C = 3, hw = 3: lanes 0..2 hold one gradient each, the butterfly's first four steps add zeros, offset 2 pairs lane 0 with
    lane 2 and offset 1 brings in lane 1: w = fl(fl(fl(g0 + g2) + g1) / 3).  Waves 0..2 hold one channel each, so
    cam = ((0 + w0 a0) + w1 a1) + w2 a2."""
    act, grad = R.normal_case(1, 3, 1, 3, seed=5)
    g, a = grad[0, :, 0], act[0, :, 0]
    wgt = ((g[:, 0] + g[:, 2]) + g[:, 1]) / F32(3)
    want = (wgt[0] * a[0] + wgt[1] * a[1]) + wgt[2] * a[2]
    np.testing.assert_array_equal(bits(R.cam_fp32(act, grad, False)[0, 0]), bits(want))
    # ... and the butterfly is not a sequential sum: 65 pixels at PPL = 2 put pixel 64 in lane 0 beside pixel 0
    act, grad = R.normal_case(1, 1, 5, 13, seed=5)
    g = grad.reshape(-1)
    s = np.zeros(64, F32)
    s[:] = g[:64]
    s[0] = s[0] + g[64]
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[np.arange(64) ^ off]
    assert len(set(bits(s).tolist())) == 1
    np.testing.assert_array_equal(bits(R.cam_fp32(act, grad, False)), bits((s[0] / F32(65)) * act[:, 0]))


def test_summation_order_is_visible_in_the_bits():
    """What rel 1e-5 cannot see and the bit comparison can: the same case summed in another order (NumPy's pairwise sum of the
    oracle) differs from cam_fp32 in the last bits at some pixel, and the one-slice order differs from the sliced one."""
    act, grad = R.normal_case(1, 1030, 7, 9)
    mine = R.cam_fp32(act, grad, False)
    assert (bits(mine) != bits(ogc.cam_reduce(act, grad, relu=False))).any()
    assert (bits(mine) != bits(R.cam_fp32(act, grad, False, have_ws=False))).any()


@pytest.mark.parametrize("cell", R.cam_cells(), ids=R.cam_name)
def test_cam_fp32_is_inside_the_derived_bound_around_cam64(cell):
    act, grad = R.normal_case(*cell)
    bound = R.cam_bound(act, grad)
    for relu in (False, True):
        got, want = R.cam_fp32(act, grad, relu), R.cam64(act, grad, relu)
        ratio = inside(got, want, bound)
        print(f"{R.cam_name(cell)} relu{int(relu)}: {ratio:.4f} of the bound (n = {R.cam_chain(cell[0], cell[1], cell[2] * cell[3])}), rel_inf {rel_inf(got, want):.2e}")
        assert ratio <= 1.0 and rel_inf(got, want) <= BAR
        if relu:
            assert (got >= 0).all() and not np.signbit(got).any()


def test_bilinear_fp32_is_the_oracle_bit_for_bit():
    for cell in R.bilinear_cells():
        src = R.bilinear_case(cell)
        H, W = cell[3], cell[4]                         # shrinking cells too: the oracle's taps are the kernel's at any size
        np.testing.assert_array_equal(bits(R.bilinear_fp32(src, H, W)), bits(ogc.bilinear_up(src, H, W)), err_msg=str(cell))


def torch_plain(src, H, W):
    return torch.nn.functional.interpolate(torch.from_numpy(src)[:, None], size=(H, W), mode="bilinear", align_corners=False,
                                           antialias=False)[:, 0].numpy()


def torch_antialiased(src, H, W):
    return torch.nn.functional.interpolate(torch.from_numpy(src)[:, None], size=(H, W), mode="bilinear", align_corners=False,
                                           antialias=True)[:, 0].numpy()


@pytest.mark.parametrize("cell", R.bilinear_cells(), ids=R.bilinear_name)
def test_bilinear_restatements_are_inside_the_derived_bound(cell):
    """fp32 around mult * fp64 (|.| of both with take_abs), and torch's CPU interpolation around fp64, both within
    bilinear_bound and within the project's bar."""
    B, h, w, H, W, mult, take_abs = cell
    src = R.bilinear_case(cell)
    want = mult * R.bilinear64(src, H, W)
    want = np.abs(want) if take_abs else want
    got = R.bilinear_fp32(src, H, W, mult, take_abs)
    ratio = inside(got, want, R.bilinear_bound(src, H, W, mult))
    plain = inside(torch_plain(src, H, W), R.bilinear64(src, H, W), R.bilinear_bound(src, H, W))
    print(f"{R.bilinear_name(cell)}: {ratio:.4f} of the bound, torch {plain:.4f}, rel_inf {rel_inf(got, want):.2e}")
    assert ratio <= 1.0 and plain <= 1.0 and rel_inf(got, want) <= BAR
    if take_abs:
        assert (got >= 0).all()


def test_bilinear_edges_by_hand():
    """identity size: src * mult bit for bit; h = 1: every output row the same; w = 1: every column; 1 x 1: a constant; and the
    first and last output pixel of an up-sampling are the first and last source pixel (coordinate clamped / neighbour clamped)."""
    src = R.bilinear_case((3, 8, 8, 8, 8))
    np.testing.assert_array_equal(bits(R.bilinear_fp32(src, 8, 8, -2.0)), bits(src * F32(-2)))
    np.testing.assert_array_equal(bits(R.bilinear_fp32(src, 8, 8, 3.0, True)), bits(np.abs(src * F32(3))))
    for cell, axis in (((3, 1, 9, 5, 65), 1), ((3, 9, 1, 63, 4), 2), ((3, 1, 1, 3, 64), 1), ((3, 1, 1, 3, 64), 2)):
        src = R.bilinear_case(cell)
        R.degenerate_axis_holds(src, R.bilinear_fp32(src, cell[3], cell[4]), axis)
    # "all rows bitwise equal" is NOT a property of this arithmetic: a row with weights (0.8, 0.2) is fl(fl(0.8 t) + fl(0.2 t)),
    # one ulp beside t at some pixels -- in the oracle and in torch's own CPU kernel alike, so a kernel with bitwise equal rows
    # could not have the oracle's bits
    src = R.bilinear_case((3, 1, 9, 5, 65))
    for up in (ogc.bilinear_up(src, 5, 65), torch_plain(src, 5, 65)):
        assert (bits(up) != bits(up[:, :1])).any()
    R.degenerate_axis_holds(src, ogc.bilinear_up(src, 5, 65), 1)
    one = R.bilinear_case((3, 1, 1, 3, 64))
    assert (bits(R.bilinear_fp32(one, 3, 64))[:, :, :32] == bits(one)).all()        # both weights' l1 are 0 there
    src = R.bilinear_case((1, 7, 7, 224, 224))
    up = R.bilinear_fp32(src, 224, 224)
    assert up[0, 0, 0] == src[0, 0, 0] and up[0, -1, -1] == src[0, -1, -1] and up[0, 0, -1] == src[0, 0, -1]


def test_plain_and_antialiased_agree_exactly_when_no_axis_shrinks_and_not_otherwise():
    """The divergence xai_engine.gradcam.gradcam_saliency routes around: the reference resizes with antialias=True, which is
    the plain bilinear of K3 only while no axis shrinks."""
    for h, w, H, W in R.BILINEAR_SHAPES:
        src = R.bilinear_case((1, h, w, H, W))
        gap = float(np.abs(torch_antialiased(src, H, W) - torch_plain(src, H, W)).max())
        if (h, w, H, W) in R.SHRINKS:
            assert gap > 0.1, (h, w, H, W, gap)
        else:
            assert H >= h and W >= w and gap <= float(R.bilinear_bound(src, H, W).max()) * 2, (h, w, H, W, gap)
    assert set(R.SHRINKING) < set(R.SHRINKS) and len(R.SHRINKS) == 12


def test_the_matrices_reach_what_they_say():
    cells = R.cam_cells()
    assert len(set(cells)) == len(cells) and {c[0] for c in cells} == {1, 3, 63, 64}
    assert {c[2] * c[3] for c in cells} == {1, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024}
    assert all(c[1] * c[2] * c[3] <= R.CAM_BUDGET or (c[1] == 1030 and c[2:] in R.CAM_OVER_BUDGET) for c in cells)
    by_ppl = {}
    for B, C, h, w in cells:
        by_ppl.setdefault(R.ppl_for(h * w), []).append((B, C))
    assert sorted(by_ppl) == [1, 2, 4, 8, 16]
    for ppl, bc in by_ppl.items():
        trip = R.WAVES * R.unroll_for(ppl)
        counts = {R.slices_for(B, C)[0] for B, C in bc}
        assert {1, 2, 3, 16} <= counts, (ppl, counts)
        assert {1, 17, 129, 200, 1030} <= {C for _, C in bc}, ppl
        lengths = [R.slice_lengths(B, C) for B, C in bc]
        assert any(len(ln) > 1 and ln[-1] < ln[0] for ln in lengths), ppl                        # a ragged last slice
        assert any(len(ln) == 1 and WAVES_DRY < ln[0] % trip for ln in lengths), ppl             # one slice ends inside a trip ...
        assert any(all(n % trip == 0 for n in ln) for ln in lengths), ppl                        # ... and every slice exactly on one
        assert any(ln[-1] % trip > WAVES_DRY for ln in lengths if len(ln) > 1), ppl              # a sliced tail inside a trip
        assert any(B == 3 and R.slices_for(B, C)[0] == 3 for B, C in bc), ppl
    assert R.slices_for(*R.B64_CELLS[0][:2]) == (1, 256) and R.slices_for(*R.B64_CELLS[1][:2]) == (4, 64)
    assert all(c in cells for c in R.B64_CELLS)
    shapes = {c[1:5] for c in R.bilinear_cells()}
    assert shapes == set(R.BILINEAR_SHAPES) and len(R.BILINEAR_SHAPES) == 20
    assert {(c[5], c[6]) for c in R.bilinear_cells()} == {(1.0, 0), (1.0, 1), (3.0, 1), (-2.0, 0), (-2.0, 1)}
    assert all({1, 3} <= {c[0] for c in R.bilinear_cells() if c[1:5] == s} for s in R.BILINEAR_SHAPES)
    assert {(H, W) for h, w, H, W in R.BILINEAR_SHAPES if (h, w) == (6, 7)} == {(H, W) for H in (3, 4, 5) for W in (63, 64, 65)}
    assert len(set(R.ledger_names())) == len(R.ledger_names())


@pytest.mark.parametrize("cell", R.cam_cells(), ids=R.cam_name)
def test_exact_cases_meet_their_own_conditions(cell):
    """... and cam_fp32 returns them element for element, with and without the slices, as int64."""
    act, grad, weights, cam = R.exact_case(*cell)
    assert R.exact_case_holds(act, grad, weights, cam)
    assert np.abs(weights).max() > 0 or cell[1] == 1
    for ws in (True, False):
        got = R.cam_fp32(act, grad, False, have_ws=ws)
        np.testing.assert_array_equal(got.astype(np.int64), cam)
        assert (got == got.astype(np.int64)).all()
    np.testing.assert_array_equal(R.cam_fp32(act, grad, True).astype(np.int64), np.maximum(cam, 0))


def test_exact_cases_tell_mistakes_apart():
    """Channels of grad paired with the wrong activation, h and w swapped, a channel dropped, a pixel left out of the mean: each
    changes the expected integers."""
    for cell in ((1, 17, 7, 9), (3, 200, 5, 13), (1, 129, 3, 43), (1, 32, 19, 27)):
        B, C, h, w = cell
        act, grad, weights, cam = R.exact_case(*cell)
        perm = np.roll(np.arange(C), 1)
        assert (R.cam_fp32(act, grad[:, perm], False).astype(np.int64) != cam).any()
        swapped = R.cam_fp32(act.transpose(0, 1, 3, 2), grad.transpose(0, 1, 3, 2), False).astype(np.int64)
        assert swapped.shape == (B, w, h) and (swapped.reshape(B, -1) != cam.reshape(B, -1)).any()
        np.testing.assert_array_equal(swapped.transpose(0, 2, 1), cam)
        assert (R.cam_fp32(act[:, :-1], grad[:, :-1], False).astype(np.int64) != cam).any() or (weights[:, -1] == 0).all()
        short = grad.copy()
        short[:, :, -1, -1] = 0
        assert (R.cam_fp32(act, short, False) != cam).any()


def test_cam_edge_ledger_is_complete_and_inside_its_conditions():
    """profiles/cam_edges_parity.json is the ledger tests/test_gpu_cam_edges.py wrote on an MI355X
    (XAI_PARITY_REPORT=profiles/cam_edges_parity.json python -m pytest tests/test_gpu_cam_edges.py -m gpu -q -x): the run passed,
    in deterministic mode; bit-for-bit and int64 comparisons leave no row, so it holds per cell the kernel's distance from the
    fp64 restatement in the project's norm at the 1e-5 bar and, under /bound, as a fraction of the derived bound at 1.0."""
    led = json.load(open(os.path.join(ROOT, "profiles", "cam_edges_parity.json")))
    assert led["meta"]["exitstatus"] == 0 and led["meta"]["deterministic"] is True and led["meta"]["device"] != "cpu"
    rows = [r for r in led["comparisons"] if r["name"].startswith("cam_edges/")]
    assert sorted(r["name"] for r in rows) == R.ledger_names()
    for r in rows:
        if r["name"].endswith("/bound"):
            assert r["tol"] == 1.0 and r["norm"] == "abs", r
        else:
            assert r["tol"] == BAR and r["norm"] == "rel_inf", r
        assert 0.0 <= r["measured"] <= r["tol"], r
