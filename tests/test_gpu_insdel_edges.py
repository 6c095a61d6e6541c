"""K8 (csrc/rank_kernels.hip), the flip-step map, K6, K10 and K9 (csrc/perturb_kernels.hip) on the MI355X against
tests/insdel_restated.py at their edges.

K8, the flip map, K6 and K10 are held bit for bit; K9's argmax and its rules for NaN, +-inf and targets exactly, its values to a
measured tolerance against an fp64 softmax.  Every output lives between guard words that must come back untouched, every input
is read back after the call, and the entry points are called through the raw ABI.  The K8 tests read the four identity flags of
every segment out of the scratch after the call -- the layout restated in insdel_restated.py -- so a case proves that it drove the
branch it claims; which K6 flavour ran is read from a profiler trace."""
import numpy as np
import pytest
import torch

import insdel_restated as R
from conftest import BAR, check, rel_inf
from test_gpu_blur_edges import kernels_of
from test_gpu_masker_edges import POISON, In, Out, call, flavour, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGAINST = "fp64 reference"
SHAPE, UNSUPPORTED = -2, -3
AB = 0xABABABAB


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    return __import__("xai_engine")._lib.load()


def guards_ok(out):
    """Out.get()'s guard check on the device, for outputs too large to haul to the host."""
    torch.cuda.synchronize()
    return bool((out.buf[:out.lo] == POISON).all()) and bool((out.buf[out.lo + out.n:] == POISON).all())


def untouched_on_device(out):
    return guards_ok(out) and bool((out.t == POISON).all())


def same_words(got, want, what):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.int32).ravel(), np.ascontiguousarray(want).view(np.int32).ravel(),
                                  err_msg=str(what))


# ---- K8 --------------------------------------------------------------------------------------------------------------------------

def run_k8(lib, maps):
    """One xai_rank_f32 call over the maps (n_seg, hw) with exactly workspace_bytes of scratch, filled with 0xAB bytes, between
    guards.  -> order, rank (n_seg, hw) int32 and the scratch words (uint32)."""
    n_seg, hw = maps.shape
    nbytes = R.workspace_bytes(n_seg, hw)
    assert lib.xai_rank_workspace_bytes(n_seg, hw) == nbytes
    sal, order, rank = In(maps), Out(n_seg * hw), Out(n_seg * hw)
    ws = Out(nbytes // 4, fill=np.full(nbytes // 4, AB, np.uint32))
    assert lib.xai_rank_f32(sal.ptr, n_seg, hw, order.ptr, rank.ptr, ws.ptr, nbytes, None) == 0
    got = order.get().reshape(n_seg, hw), rank.get().reshape(n_seg, hw), ws.get().view(np.uint32)
    sal.unchanged()
    return got


def hold_k8(maps, got, names, what):
    order, rank, ws = got
    for seg, m in enumerate(maps):
        want_order, want_rank, flags = R.rank_expect(m)
        name = (what, names[seg] if names else seg)
        np.testing.assert_array_equal(R.flag_words(ws, seg), flags, err_msg=f"{name}: identity flags")
        np.testing.assert_array_equal(order[seg], want_order, err_msg=f"{name}: order")
        np.testing.assert_array_equal(rank[seg], want_rank, err_msg=f"{name}: rank")


@pytest.mark.parametrize("hw", R.RANK_HW)
def test_rank_of_every_family_and_identity_pattern(lib, hw):
    """The named families and the 16 identity patterns as the segments of one call: order, rank and the flag words."""
    names, maps = R.rank_case(hw)
    hold_k8(maps, run_k8(lib, maps), names, hw)


def test_rank_with_a_front_the_zero_fill_strides_over(lib):
    n_seg, hw = R.STRIDED_CALL
    assert R.front_words(n_seg, R.tiles_of(hw)) > 1024 * 256
    maps = R.strided_case()
    hold_k8(maps, run_k8(lib, maps), None, "strided")


def test_rank_arguments(lib):
    n_seg, hw = 3, 1025
    _, maps = R.rank_case(hw)
    maps = maps[[0, 9, 20]]
    nbytes = R.workspace_bytes(n_seg, hw)
    sal, order, rank = In(maps), Out(n_seg * hw), Out(n_seg * hw)
    ws = Out(nbytes // 4 + 1, fill=np.full(nbytes // 4 + 1, AB, np.uint32))
    rk = lambda ns, n, p, b: lib.xai_rank_f32(sal.ptr, ns, n, order.ptr, rank.ptr, p, b, None)          # noqa: E731
    assert rk(n_seg, hw, ws.ptr, nbytes - 1) == SHAPE
    assert rk(n_seg, hw, ws.ptr + 2, nbytes) == SHAPE
    assert rk(65536, hw, ws.ptr, nbytes) == UNSUPPORTED
    assert rk(n_seg, 1 << 31, ws.ptr, nbytes) == UNSUPPORTED
    assert rk(0, hw, ws.ptr, nbytes) == SHAPE and rk(n_seg, 0, ws.ptr, nbytes) == SHAPE
    assert order.untouched() and rank.untouched()
    assert (ws.get().view(np.uint32) == AB).all()
    assert rk(n_seg, hw, ws.ptr, nbytes) == 0                              # exactly workspace_bytes: accepted
    got = ws.get().view(np.uint32)
    assert got[-1] == AB                                                   # the word behind it
    hold_k8(maps, (order.get().reshape(n_seg, hw), rank.get().reshape(n_seg, hw), got), None, "exact workspace")


def test_rank_graph_replays_leave_no_flag_behind(lib):
    """One captured sort of two maps, replayed over constant, random, constant, pattern 1101 (the second map a step ahead) with
    the scratch as the replay before left it: every replay has its own flags, order and rank."""
    hw = 2049
    names, pool = R.rank_case(hw)
    seq = [pool[names.index(n)] for n in ("zeros", "ascending", "zeros", "p1101")]
    seq[1] = np.random.default_rng(5).standard_normal(hw).astype(np.float32)
    nbytes = R.workspace_bytes(2, hw)
    sal = torch.zeros(2 * hw, dtype=torch.float32, device=DEV)
    order, rank = Out(2 * hw), Out(2 * hw)
    ws = Out(nbytes // 4, fill=np.full(nbytes // 4, AB, np.uint32))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = lib.xai_rank_f32(sal.data_ptr(), 2, hw, order.ptr, rank.ptr, ws.ptr, nbytes, side.cuda_stream)
    assert rc == 0
    seen = []
    for k in range(5):
        maps = np.stack([seq[k % 4], seq[(k + 1) % 4]])
        sal.copy_(torch.from_numpy(maps.ravel()))
        graph.replay()
        torch.cuda.synchronize()
        got = order.get().reshape(2, hw), rank.get().reshape(2, hw), ws.get().view(np.uint32)
        hold_k8(maps, got, None, f"replay {k}")
        seen.append(tuple(R.flag_words(got[2], 0)))
    assert seen[0] == (1, 1, 1, 1) and seen[1] == (0, 0, 0, 0) and seen[2] == (1, 1, 1, 1) and seen[3] == (1, 1, 0, 1)


# ---- flip ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", R.FLIP_HW)
def test_flip_steps_equal_the_restatement(lib, hw):
    rank = np.random.default_rng([1, hw]).permutation(hw).astype(np.int32)
    for descending in (0, 1):
        for step in sorted({1, 7, hw, hw + 3}):
            rk, flip = In(rank), Out(hw)
            assert lib.xai_flip_steps_i32(rk.ptr, hw, descending, step, flip.ptr, None) == 0
            np.testing.assert_array_equal(flip.get(), R.flip_of(rank, descending, step), err_msg=str((hw, descending, step)))
            rk.unchanged()
    rk, flip = In(rank), Out(hw)
    assert lib.xai_flip_steps_i32(rk.ptr, hw, 0, 0, flip.ptr, None) == SHAPE and flip.untouched()


# ---- K6 --------------------------------------------------------------------------------------------------------------------------

def run_k6(K, case, seed=0, off=(0, 0, 0, 0)):
    """One xai_perturb_batch_f32 call; the words of every image compared on the device with start / finish chosen by
    flip <= first_step + k, three images and the inputs on the host.  -> vec (the flavour that ran), the output words on the
    device."""
    C, hw, n, first = case
    start, finish = R.k6_values(C, hw, seed)
    flip = R.k6_flip(hw, first, n, seed)
    s, f, fl, out = In(start, off[0]), In(finish, off[1]), In(flip, off[2]), Out(n * C * hw, off[3])
    _, names = kernels_of(lambda: call(K, "xai_perturb_batch_f32", s.ptr, f.ptr, fl.ptr, C, hw, first, n, out.ptr))
    vec = flavour(names, "perturb_kernel", true="4", false="1")
    assert guards_ok(out), (case, off, "guards")
    got = out.t.view(n, C, hw)
    step = 256                                                          # images per comparison: the temporaries stay small
    for lo in range(0, n, step):
        t = first + torch.arange(lo, min(lo + step, n), device=DEV, dtype=torch.int64)[:, None, None]
        want = torch.where(fl.t.long()[None, None, :] <= t, f.t.view(1, C, hw), s.t.view(1, C, hw))
        assert torch.equal(got[lo:lo + step], want), (case, off, lo)
    for k in sorted({0, n // 2, n - 1}):
        same_words(got[k].cpu().numpy(), R.images(start, finish, flip, first + k, 1)[0], (case, off, k))
    s.unchanged(), f.unchanged(), fl.unchanged()
    return vec, out.t


@pytest.mark.parametrize("case", R.K6_SMALL + R.K6_HBM, ids=lambda c: "x".join(map(str, c)))
def test_perturb_plans_move_the_bits(K, case):
    """Both sides of every threshold of the launch plan, with NaN payloads, +-0.0, +-inf and denormals in start and finish and
    -1, 0, the steps of the batch, steps beyond it and INT32_MAX in flip; the flavour is the one perturb_plan names."""
    vec, _ = run_k6(K, case)
    assert vec == R.perturb_plan(*case[:3])[0], case


@pytest.mark.parametrize("case", [(3, 1000, 5, 2), (1, 2047 * 256, 3, 1), (4, 4096, 1024, 0)], ids=lambda c: "x".join(map(str, c)))
def test_perturb_with_one_pointer_a_word_off_runs_the_scalar_flavour(K, case):
    """hw % 4 == 0 with start, finish, flip or out one word past a 16-byte boundary, one at a time: perturb_kernel<1> runs and
    gives the words of the aligned call."""
    vec, want = run_k6(K, case)
    assert vec and R.perturb_plan(*case[:3])[0]
    which = range(4) if case[1] == 1000 else (3,)
    for k in which:
        off = tuple(int(j == k) for j in range(4))
        vec, got = run_k6(K, case, off=off)
        assert not vec and not R.perturb_plan(*case[:3], aligned=False)[0], (case, off)
        assert torch.equal(got, want), (case, off)


def test_perturb_refuses_more_than_65535_chunks(lib):
    C, hw, n = R.K6_REFUSED
    assert R.perturb_plan(C, hw, n)[2] > 65535
    start, finish = R.k6_values(C, hw, 0)
    s, f, fl, out = In(start), In(finish), In(R.k6_flip(hw, 0, n, 0)), Out(n * C * hw)
    assert lib.xai_perturb_batch_f32(s.ptr, f.ptr, fl.ptr, C, hw, 0, n, out.ptr, None) == UNSUPPORTED
    assert untouched_on_device(out)
    assert lib.xai_perturb_batch_f32(s.ptr, f.ptr, fl.ptr, C, hw, -1, 1, out.ptr, None) == SHAPE
    assert lib.xai_perturb_batch_f32(s.ptr, f.ptr, fl.ptr, C, hw, 0, n - 1, out.ptr, None) == 0           # 65 535 chunks run
    assert guards_ok(out) and bool((out.t[(n - 1) * hw:] == POISON).all())
    same_words(out.t[(n - 2) * hw:(n - 1) * hw].cpu().numpy(), R.images(start, finish, fl.words, n - 2, 1)[0], "the last image")


# ---- K10 -------------------------------------------------------------------------------------------------------------------------

def run_k10(lib, sal, order, descending, step, n_steps):
    s, o, seg, total = In(sal), In(np.asarray(order, np.int32)), Out(n_steps), Out(1)
    assert lib.xai_segment_sums_f32(s.ptr, o.ptr, sal.size, descending, step, n_steps, seg.ptr, total.ptr, None) == 0
    got = seg.get().view(np.float32), total.get().view(np.float32)
    s.unchanged(), o.unchanged()
    return got


def hold_k10(got, sal, order, descending, step, n_steps, what):
    seg, total = got
    want_seg, want_total = R.segment_sums32(sal, order, descending, step, n_steps)
    same_bits(seg, want_seg, (what, "segments"))
    same_bits(total, [want_total], (what, "total"))


@pytest.mark.parametrize("case", R.K10_CASES, ids=lambda c: "x".join(map(str, c)))
def test_segment_sums_have_the_bits_of_the_restatement(K, lib, case):
    """Both directions with K8's order, and once with an arbitrary permutation: seg and total equal segment_sums32 bit for bit
    and lie inside segment_bound of the exact sum."""
    hw, step, n_steps = case
    sal = R.k10_map(hw)
    order = K.rank(torch.from_numpy(sal[None]).to(DEV))[0][0].cpu().numpy()
    np.testing.assert_array_equal(order, R.rank_expect(sal)[0])
    runs = [(order, 0), (order, 1), (np.random.default_rng([2, hw]).permutation(hw).astype(np.int32), 1)]
    for k, (perm, descending) in enumerate(runs):
        seg, total = run_k10(lib, sal, perm, descending, step, n_steps)
        hold_k10((seg, total), sal, perm, descending, step, n_steps, (case, k))
        for t, idx in enumerate(R.segment_indices(perm, descending, step, n_steps)):
            assert abs(float(seg[t]) - R.exact_sum(sal, idx)) <= R.segment_bound(sal, idx), (case, k, t)
        assert abs(float(total[0]) - R.exact_sum(sal, np.arange(hw))) <= R.segment_bound(sal, np.arange(hw), total=True), (case, k)


@pytest.mark.parametrize("case", [(99, 7, 15), (2500, 63, 40), (5000, 65, 77)], ids=lambda c: "x".join(map(str, c)))
def test_a_nan_or_an_inf_reaches_its_segment_and_the_total_only(lib, case):
    hw, step, n_steps = case
    order = R.rank_expect(R.k10_map(hw))[0]
    for value, where in ((np.nan, hw - 1), (np.inf, hw // 3), (np.nan, 0)):
        sal = R.k10_map(hw)
        sal[where] = value
        for descending in (0, 1):
            seg, total = run_k10(lib, sal, order, descending, step, n_steps)
            hold_k10((seg, total), sal, order, descending, step, n_steps, (case, value, descending))
            pos = int(np.flatnonzero((order[::-1] if descending else order) == where)[0])
            hit = np.isnan(seg) if np.isnan(value) else seg == np.inf
            assert np.flatnonzero(hit).tolist() == [pos // step] and np.isfinite(np.delete(seg, pos // step)).all()
            assert np.isnan(total[0]) if np.isnan(value) else total[0] == np.inf


def test_segment_sums_arguments(lib):
    sal = R.k10_map(100)
    s, o, seg, total = In(sal), In(np.arange(100, dtype=np.int32)), Out(16), Out(1)
    sums = lambda step, n: lib.xai_segment_sums_f32(s.ptr, o.ptr, 100, 0, step, n, seg.ptr, total.ptr, None)         # noqa: E731
    assert sums(7, 14) == SHAPE                                  # 98 < hw
    assert sums(7, 16) == SHAPE                                  # 15 * 7 >= hw
    assert sums(0, 15) == SHAPE and sums(7, 0) == SHAPE
    assert seg.untouched() and total.untouched()
    assert sums(7, 15) == 0
    assert (seg.get()[:15] != POISON).all() and seg.get()[15] == POISON


# ---- K9 --------------------------------------------------------------------------------------------------------------------------

def run_k9(lib, z, t_dev=None, t_host=-1, entropy=True, argmax=True):
    """-> p, entropy, argmax words (int32; None where the output is not asked for)."""
    B, K_ = z.shape
    zin, p, ent, am = In(z), Out(B), Out(B), Out(B)
    td = None if t_dev is None else In(np.array([t_dev], np.int32))
    rc = lib.xai_softmax_stats_f32(zin.ptr, B, K_, None if td is None else td.ptr, t_host, p.ptr, ent.ptr if entropy else None,
                                   am.ptr if argmax else None, None)
    assert rc == 0, rc
    got = p.get(), ent.get(), am.get()
    assert entropy or ent.untouched()
    assert argmax or am.untouched()
    zin.unchanged()
    if td is not None:
        td.unchanged()
    return got[0], got[1] if entropy else None, got[2] if argmax else None


@pytest.mark.parametrize("K_", R.K9_K)
def test_softmax_stats_values_rows_and_targets(lib, K_):
    """For every B: argmax exactly; p with a host target, a device target and the row's own argmax, and the entropy, against the
    fp64 softmax of the fp32 logits (one ledger row per K); every row bit-identical to the same row computed alone at B = 1."""
    got_p, want_p, got_e, want_e = [], [], [], []
    for B in R.K9_B:
        z = R.k9_logits(B, K_)
        host, devt = min(K_ - 1, 3), K_ - 1
        p_h, e_h, a_h = run_k9(lib, z, t_host=host)
        p_d, e_d, a_d = run_k9(lib, z, t_dev=devt)
        p_a, e_a, a_a = run_k9(lib, z, t_host=-1)
        p_n, e_n, a_n = run_k9(lib, z, t_dev=-1)
        same_words(p_n, p_a, (K_, B, "device target < 0"))
        for e, a in ((e_d, a_d), (e_a, a_a), (e_n, a_n)):
            same_words(e, e_h, (K_, B, "entropy"))
            same_words(a, a_h, (K_, B, "argmax"))
        for t, p in ((host, p_h), (devt, p_d), (-1, p_a)):
            wp, we, wa = R.softmax_expect(z, t)
            np.testing.assert_array_equal(a_h, wa, err_msg=str((K_, B)))
            got_p.append(p.view(np.float32)), want_p.append(wp)
        got_e.append(e_h.view(np.float32)), want_e.append(we)
        for r in range(B):
            p1, e1, a1 = run_k9(lib, z[r:r + 1], t_host=host)
            same_words(p1, p_h[r:r + 1], (K_, B, r, "p alone"))
            same_words(e1, e_h[r:r + 1], (K_, B, r, "entropy alone"))
            same_words(a1, a_h[r:r + 1], (K_, B, r, "argmax alone"))
    got_p, want_p, got_e, want_e = (np.concatenate(v) for v in (got_p, want_p, got_e, want_e))
    assert np.isfinite(got_p).all() and np.isfinite(got_e).all()
    print(f"insdel_edges/softmax K={K_}: p {rel_inf(got_p, want_p):.4e}  entropy {rel_inf(got_e, want_e):.4e}")
    check(f"insdel_edges/softmax_p/K{K_}", got_p, want_p, R.K9_TOL["p"], against=AGAINST)
    check(f"insdel_edges/softmax_entropy/K{K_}", got_e, want_e, R.K9_TOL["entropy"], against=AGAINST)


@pytest.mark.parametrize("first", [0, 3], ids=["at_row_0", "at_row_3"])
def test_softmax_stats_discrete_rules(lib, first):
    """The NaN, tie and +-inf rows (behind `first` ordinary rows, so that they change wave and workgroup): argmax is the first NaN,
    else the first maximum; p is exactly 1 on a saturated row, exactly 0 at a -inf entry, NaN on rows with +inf, NaN or nothing
    but -inf; a device target >= K gives NaN, a device target < 0 each row's own argmax."""
    rows = R.k9_special_rows()
    names = list(rows)
    K_ = 200
    z = np.concatenate([R.k9_logits(first, K_), np.stack([r for r, _ in rows.values()])]) if first else np.stack([r for r, _ in rows.values()])
    B = len(z)
    at = {n: first + k for k, n in enumerate(names)}
    want_am = [R.argmax_rule(r) for r in z]
    assert [want_am[at[n]] for n in names] == [a for _, a in rows.values()]
    p_a, e_a, am = run_k9(lib, z, t_host=-1)
    np.testing.assert_array_equal(am, want_am)
    p_a, e_a = p_a.view(np.float32), e_a.view(np.float32)
    p_n = run_k9(lib, z, t_dev=-7)[0]
    same_bits(p_n, p_a, "device target < 0")
    p_0 = run_k9(lib, z, t_dev=0)[0].view(np.float32)                      # index 0 is a -inf entry of some_neg_inf
    assert p_a[at["saturated"]] == 1.0 and np.isnan(e_a[at["saturated"]])   # exp(-300) is 0 in fp32: 0 * log2 0
    assert p_0[at["some_neg_inf"]] == 0.0 and np.signbit(p_0[at["some_neg_inf"]]) == False and np.isnan(e_a[at["some_neg_inf"]])   # noqa: E712
    assert 0 < p_a[at["some_neg_inf"]] < 1
    for n in ("all_neg_inf", "two_pos_inf", "nan_70_131", "nan_beats_max"):
        assert np.isnan(p_a[at[n]]) and np.isnan(p_0[at[n]]) and np.isnan(e_a[at[n]]), n
    for n in ("tie_j_j64", "tie_65_2", "tie_three", "constant"):
        assert np.isfinite(p_a[at[n]]) and np.isfinite(e_a[at[n]]), n
    assert p_a[at["constant"]] == np.float32(1) / np.float32(K_)
    wp, we, _ = R.softmax_expect(z, -1)
    fin = np.isfinite(e_a)                                                 # the saturated row has an entropy in fp64 only
    assert sorted(np.flatnonzero(~fin)) == sorted(at[n] for n in ("saturated", "some_neg_inf", "all_neg_inf", "two_pos_inf", "nan_70_131",
                                                                   "nan_beats_max"))
    np.testing.assert_array_equal(np.isnan(p_a), np.isnan(wp))
    ok = ~np.isnan(wp)
    # values at the project's bar only: the measured tolerances belong to the rows of the ledger
    assert rel_inf(p_a[ok], wp[ok]) <= BAR and rel_inf(e_a[fin], we[fin]) <= BAR
    for t in (K_, K_ + 5, R.INT32_MAX):
        p_k, _, am_k = run_k9(lib, z, t_dev=t)
        assert np.isnan(p_k.view(np.float32)).all()
        np.testing.assert_array_equal(am_k, want_am)
    for r in range(first, B):                                              # the same rows alone
        np.testing.assert_array_equal(run_k9(lib, z[r:r + 1])[2], want_am[r:r + 1])


def test_softmax_stats_optional_outputs_targets_and_slices(K, lib):
    B, K_ = 5, 129
    z = R.k9_logits(B, K_)
    p, e, a = run_k9(lib, z, t_host=4)
    for entropy, argmax in ((False, True), (True, False), (False, False)):
        p2, e2, a2 = run_k9(lib, z, t_host=4, entropy=entropy, argmax=argmax)
        same_words(p2, p, "p without the optional outputs")
        assert (e2 is None or (e2 == e).all()) and (a2 is None or (a2 == a).all())
    zin, po, eo, ao = In(z), Out(B), Out(B), Out(B)
    for t in (K_, K_ + 1):
        assert lib.xai_softmax_stats_f32(zin.ptr, B, K_, None, t, po.ptr, eo.ptr, ao.ptr, None) == SHAPE
    assert lib.xai_softmax_stats_f32(zin.ptr, 0, K_, None, 0, po.ptr, eo.ptr, ao.ptr, None) == SHAPE
    assert po.untouched() and eo.untouched() and ao.untouched()
    # out= / offset: rows [offset, offset + B) of preallocated curves and nothing else
    n, offset = 12, 4
    pc, ec, ac = Out(n), Out(n), Out(n)
    zt = torch.from_numpy(z).to(DEV)
    K.softmax_stats(zt, target=4, out=(pc.t.view(torch.float32), ec.t.view(torch.float32), ac.t), offset=offset)
    for curve, want in ((pc, p), (ec, e), (ac, a)):
        got = curve.get()
        same_words(got[offset:offset + B], want, "the slice")
        assert (got[:offset] == POISON).all() and (got[offset + B:] == POISON).all()
    K.softmax_stats(zt, target=4, want_entropy=False, want_argmax=False, out=(pc.t.view(torch.float32), None, None), offset=n - B)
    same_words(pc.get()[n - B:], p, "the last rows")
    assert (ec.get()[offset + B:] == POISON).all() and (ac.get()[offset + B:] == POISON).all()
