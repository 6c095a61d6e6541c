"""tests/insdel_restated.py checked on the host before a kernel is held to it: the key order against NumPy's stable argsort, the
identity flags of every pattern map, the scratch layout on hand-worked sizes, the fp32 segment sums inside a derived bound that
bites, the argmax rule against torch on the CPU, the fp64 softmax against torch's, the K6 launch plans on hand-worked cases, and
the ledger of tests/test_gpu_insdel_edges.py from an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import insdel_restated as R
from conftest import BAR, ROOT


# ---- K8 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", R.RANK_HW)
def test_order_is_numpys_stable_argsort_on_every_family(hw):
    names, maps = R.rank_case(hw)
    assert len(names) == (26 if hw >= 2 else 10)
    for name, m in zip(names, maps):
        order, rank, _ = R.rank_expect(m)
        np.testing.assert_array_equal(order, np.argsort(m, kind="stable"), err_msg=f"{name} at {hw}")
        np.testing.assert_array_equal(rank[order], np.arange(hw), err_msg=f"{name} at {hw}")
        if name != "specials":
            assert np.isfinite(m).all(), name


@pytest.mark.parametrize("hw", [h for h in R.RANK_HW if h >= len(R.SPECIALS)])
def test_specials_map_places_nans_last_in_index_order(hw):
    names, maps = R.rank_case(hw)
    m = maps[names.index("specials")]
    nan = np.flatnonzero(np.isnan(m))
    u = m.view(np.uint32)
    assert len({int(w) for w in u[nan]}) == R.N_NAN and (u[nan] >> 31).min() == 0 and (u[nan] >> 31).max() == 1
    for w in R.SPECIALS[R.N_NAN:]:
        assert (u == w).any(), hex(int(w))
    order, _, _ = R.rank_expect(m)
    np.testing.assert_array_equal(order[hw - nan.size:], nan)
    zeros = np.flatnonzero(m == 0)                          # -0.0 and +0.0 tie: index order
    pos = np.flatnonzero(np.isin(order, zeros))
    np.testing.assert_array_equal(order[pos], zeros)
    assert pos.max() - pos.min() == zeros.size - 1


def test_sort_key_on_single_values():
    key = lambda w: int(R.sort_key(R.bits([w]))[0])          # noqa: E731
    for w in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0xFF800001):
        assert key(w) == 0xFFFFFFFF
    assert key(0x80000000) == key(0x00000000) == 0x80000000
    assert key(0xFF800000) == 0x007FFFFF and key(0x7F800000) == 0xFF800000
    assert key(0x80000001) == 0x7FFFFFFE and key(0x00000001) == 0x80000001
    assert key(0x3F800000) == 0xBF800000


@pytest.mark.parametrize("hw", [h for h in R.RANK_HW if h >= 2])
def test_every_pattern_map_has_exactly_its_flags(hw):
    """What keeps the GPU test from leaving the identity branch out unnoticed: all 16 patterns at every size, none skipped."""
    names, maps = R.rank_case(hw)
    seen = set()
    for flags in R.PATTERNS:
        m = maps[names.index(R.pattern_name(flags))]
        assert np.isfinite(m).all()
        assert tuple(R.rank_expect(m)[2]) == flags, (hw, flags)
        seen.add(flags)
    assert len(seen) == 16
    if hw > R.TILE:                                          # real bytes are spread: keys move between tiles in every real pass
        for flags in R.PATTERNS[:15]:
            order = R.rank_expect(maps[names.index(R.pattern_name(flags))])[0]
            assert (order // R.TILE != np.arange(hw) // R.TILE).any()


def test_named_families_have_the_flags_the_issue_names():
    for hw in (2, 257, 8193):
        names, maps = R.rank_case(hw)
        flags = {n: tuple(R.rank_expect(m)[2]) for n, m in zip(names, maps)}
        assert flags["zeros"] == (1, 1, 1, 1)
        assert flags["zero_one"][:2] == (1, 1) and flags["small_int"][:2] == (1, 1)
        assert flags["one_two"][3] == 1
        assert flags["quarters"] == (1, 1, 0, 1)
        assert flags["last_smaller"] == (1, 1, 0, 1)         # 1.0 and 0.5: keys 0xBF800000 and 0xBF000000
    assert tuple(R.rank_expect(np.zeros(1, np.float32))[2]) == (1, 1, 1, 1)


def test_workspace_layout_on_hand_computed_sizes():
    assert R.workspace_bytes(1, 1) == (1032 + 260) * 4 == 5168
    assert R.workspace_bytes(3, 1025) == (6168 + 3 * 4612) * 4 == 80016
    assert R.workspace_bytes(16, 16389) == (278656 + 16 * 69908) * 4 == 5588736
    for n_seg, hw in ((1, 1), (3, 1025), (16, 16389), (2, 1024), (64, 16389)):
        nt = R.tiles_of(hw)
        assert R.workspace_bytes(n_seg, hw) == (R.front_words(n_seg, nt) + n_seg * R.seg_words(hw, nt)) * 4
    assert R.tiles_of(1024) == 1 and R.tiles_of(1025) == 2 and R.tiles_of(8192) == 8 and R.tiles_of(16384) == 16
    assert R.front_words(*R.STRIDED_CALL[:1], R.tiles_of(R.STRIDED_CALL[1])) == 1114624
    assert R.zero_fill_strided(*R.STRIDED_CALL) >= 0.73
    assert R.zero_fill_strided(4, 65539) < 0.03              # the largest front of the older tests
    assert len(R.strided_case()) == R.STRIDED_CALL[0]
    assert list(R.flag_words(np.arange(64), 3)) == [24, 25, 26, 27]


def test_flip_of_on_a_hand_computed_case():
    rank = np.array([3, 0, 4, 1, 2], np.int32)
    assert R.flip_of(rank, False, 2).tolist() == [1, 0, 2, 0, 1]
    assert R.flip_of(rank, True, 2).tolist() == [0, 2, 0, 1, 1]
    assert R.flip_of(rank, True, 8).tolist() == [0] * 5


# ---- K10 -------------------------------------------------------------------------------------------------------------------------

def outside(sal, seg, idxs):
    return [t for t, idx in enumerate(idxs) if abs(float(seg[t]) - R.exact_sum(sal, idx)) > R.segment_bound(sal, idx)]


@pytest.mark.parametrize("case", R.K10_CASES, ids=lambda c: "x".join(map(str, c)))
def test_segment_sums_lie_inside_the_derived_bound(case):
    hw, step, n_steps = case
    sal = R.k10_map(hw)
    assert n_steps * step >= hw > (n_steps - 1) * step
    order = R.rank_expect(sal)[0]
    every = np.arange(hw)
    for descending in (0, 1):
        seg, total = R.segment_sums32(sal, order, descending, step, n_steps)
        idxs = R.segment_indices(order, descending, step, n_steps)
        assert sorted(np.concatenate(idxs).tolist()) == every.tolist()
        assert outside(sal, seg, idxs) == []
        assert abs(float(total) - R.exact_sum(sal, every)) <= R.segment_bound(sal, every, total=True)


def test_the_segment_bound_bites():
    """|values| in [0.5, 2]: the bound of the widest segment here is below 1e-3, so a restatement that drops the last element of
    a ragged step, or reads the ascending order for a descending call, falls outside it."""
    hw, step, n_steps = 2500, 63, 40
    sal = R.k10_map(hw)
    order = R.rank_expect(sal)[0]
    idxs = R.segment_indices(order, 1, step, n_steps)
    assert len(idxs[-1]) == 43 and max(R.segment_bound(sal, i) for i in idxs) < 1e-3
    assert R.segment_bound(sal, np.arange(hw), total=True) < 1e-2
    seg, _ = R.segment_sums32(sal, order, 1, step, n_steps)
    short = seg.copy()
    short[-1] = R.butterfly(R.lane_partials(sal[idxs[-1][:-1]], R.WAVE))
    assert outside(sal, short, idxs) == [n_steps - 1]
    wrong, _ = R.segment_sums32(sal, order, 0, step, n_steps)
    assert len(outside(sal, wrong, idxs)) >= n_steps - 1
    # the count of additions of the two bounds on a hand-worked size: 224 elements are 4 per lane, 50176 are 49 per lane
    assert R.segment_bound(np.ones(224, np.float32), np.arange(224)) == R.gamma(10) * 224
    assert R.segment_bound(np.ones(50176, np.float32), np.arange(50176), total=True) == R.gamma(61) * 50176


def test_segment_sums_on_integers_are_exact():
    sal = np.random.default_rng(3).integers(-9, 10, 5000).astype(np.float32)
    order = np.random.default_rng(4).permutation(5000)
    seg, total = R.segment_sums32(sal, order, 1, 65, 77)
    assert seg.tolist() == [float(sal[i].sum()) for i in R.segment_indices(order, 1, 65, 77)] and total == sal.sum()


# ---- K9 --------------------------------------------------------------------------------------------------------------------------

def test_argmax_rule_is_torchs_cpu_order():
    """The claim of xai_common.h's argmax_beats: torch.max on the CPU returns the first NaN if there is one, else the first
    maximum -- on the NaN and tie rows of the GPU test."""
    rows = R.k9_special_rows()
    z = np.stack([r for r, _ in rows.values()])
    got = torch.from_numpy(z).max(1).indices.numpy()
    for k, (name, (row, want)) in enumerate(rows.items()):
        assert R.argmax_rule(row) == want == got[k], (name, R.argmax_rule(row), want, got[k])
    for K in R.K9_K:
        z = R.k9_logits(9, K)
        assert [R.argmax_rule(r) for r in z] == torch.from_numpy(z).max(1).indices.tolist()


def test_softmax_expect_is_torchs_fp64_softmax():
    for K in R.K9_K:
        for B in R.K9_B:
            z = R.k9_logits(B, K)
            assert (z.max(1, keepdims=True) - z).max() <= 78.0
            tgt = np.arange(B) % K
            p, ent, am = R.softmax_expect(z, tgt)
            want = torch.softmax(torch.from_numpy(z).double(), 1)
            np.testing.assert_allclose(p, want[torch.arange(B), torch.from_numpy(tgt)].numpy(), rtol=1e-14, atol=0)
            np.testing.assert_allclose(ent, -(want * torch.log2(want)).sum(1).numpy(), rtol=1e-12, atol=1e-15)
            assert np.isfinite(ent).all() and (p > 0).all()
            np.testing.assert_array_equal(R.softmax_expect(z, -1)[0], R.softmax_expect(z, am)[0])
            assert np.isnan(R.softmax_expect(z, K)[0]).all()
    rows = R.k9_special_rows()
    z = np.stack([r for r, _ in rows.values()])
    p, ent, _ = R.softmax_expect(z, 7)
    want = torch.softmax(torch.from_numpy(z).double(), 1)
    went = -(want * torch.log2(want)).sum(1).numpy()
    np.testing.assert_array_equal(np.isnan(p), np.isnan(want[:, 7].numpy()))
    np.testing.assert_array_equal(np.isnan(ent), np.isnan(went))
    names = list(rows)
    for name in ("all_neg_inf", "two_pos_inf", "nan_70_131"):
        assert np.isnan(p[names.index(name)]) and np.isnan(ent[names.index(name)])
    assert np.isnan(ent[names.index("some_neg_inf")]) and np.isfinite(p[names.index("some_neg_inf")])


# ---- K6 --------------------------------------------------------------------------------------------------------------------------

def test_perturb_plan_on_hand_computed_cases():
    plans = {
        (3, 4, 1): (True, 1, 1, 1), (3, 4, 2049): (True, 2, 1025, 1), (3, 5, 1): (False, 1, 1, 1), (3, 5, 2049): (False, 2, 1025, 1),
        (3, 3000, 1009): (True, 2, 505, 1), (2, 1021, 13): (False, 1, 13, 1), (1, 524289, 3): (False, 3, 1, 1), (1, 524032, 3): (True, 1, 3, 1),
        (4, 4096, 1024): (True, 2, 512, 4), (4, 4096, 1023): (True, 2, 512, 1), (64, 1024, 256): (True, 2, 128, 64),
        (65, 1024, 256): (True, 1, 256, 1), (4, 4096, 1025): (True, 2, 513, 4), (3, 4099, 1365): (False, 2, 683, 3),
    }
    cases = [c[:3] for c in R.K6_SMALL + R.K6_HBM]
    assert sorted(plans) == sorted(cases)
    for case, want in plans.items():
        assert R.perturb_plan(*case) == want, case
    assert R.perturb_plan(1, 524032, 3, aligned=False) == (False, 2, 2, 1)         # 2047 scalar tiles: ceil(2048 / 2047) = 2
    assert R.perturb_plan(4, 4096, 1024, aligned=False) == (False, 2, 512, 4)
    assert R.perturb_plan(3, 4099, 1364) == (False, 12, 114, 1)                    # 67 092 432 bytes, below 64 MiB: 17 tiles, c0 = 121
    assert 4 * 4096 * 1024 * 4 == R.HBM_BYTES == 64 * 1024 * 256 * 4
    assert R.perturb_plan(*R.K6_REFUSED) == (True, 2, 65536, 1)
    assert R.perturb_plan(1, 132, 131070) == (True, 2, 65535, 1)
    assert R.perturb_plan(1, 4, 1 << 20)[2] == 2048 and R.perturb_plan(1, 1, 1) == (False, 1, 1, 1)


def test_images_moves_bits():
    start, finish = R.k6_values(2, 40, 0)
    flip = R.k6_flip(40, 3, 5, 0)
    assert {-1, 0, 3, 7, 8, R.INT32_MAX} <= set(flip.tolist())
    got = R.images(start, finish, flip, 3, 5)
    s, f = start.view(np.int32), finish.view(np.int32)
    assert (s != f).all() and np.isnan(start).sum() >= 6
    for k in range(5):
        for p in range(40):
            assert (got[k, :, p] == (f[:, p] if flip[p] <= 3 + k else s[:, p])).all()


# ---- the ledger ------------------------------------------------------------------------------------------------------------------

def test_insdel_edge_ledger_is_complete_and_its_tolerances_are_measured():
    """profiles/insdel_edges_parity.json is the ledger tests/test_gpu_insdel_edges.py wrote on an MI355X
    (XAI_PARITY_REPORT=profiles/insdel_edges_parity.json python -m pytest tests/test_gpu_insdel_edges.py -m gpu -q): the run
    passed; every K8, flip, K6 and K10 comparison is bit for bit and leaves no row, so it holds the K9 value comparisons, one row
    per K for p and for the entropy.  Their tolerances are the ones asserted today, twice the largest error measured for them
    and never above the bar."""
    led = json.load(open(os.path.join(ROOT, "profiles", "insdel_edges_parity.json")))
    assert led["meta"]["exitstatus"] == 0 and led["meta"]["device"] != "cpu"
    rows = [r for r in led["comparisons"] if r["name"].startswith("insdel_edges/")]
    assert sorted(r["name"] for r in rows) == R.ledger_names()
    for what in ("p", "entropy"):
        mine = [r for r in rows if r["name"].startswith(f"insdel_edges/softmax_{what}/")]
        worst = max(r["measured"] for r in mine)
        assert worst <= R.K9_TOL[what] <= min(BAR, 2 * worst) and R.K9_TOL[what] >= 1.999 * worst      # twice the measurement, no more
        for r in mine:
            assert r["tol"] == R.K9_TOL[what] and r["norm"] == "rel_inf" and r["against"] == "fp64 reference", r
            assert 0.0 <= r["measured"] <= r["tol"], r
