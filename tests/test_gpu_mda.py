"""MDA on the GPU: K36 (compose) bit for bit against the torch select, K37 (select and advance) against a line-by-line
restatement, both searches against the restatement on the device (same pass shapes: equal orders and slots, responses and maps
bit for bit) and against the reference's own run (tests/golden/mda.npz, 1e-5), the harness row, and the proof that no host
read sits inside the search loop."""
import numpy as np
import pytest
import torch

import mda_restated as R
from conftest import BAR, check, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ K36
def _special_labels(n_img, HW, seed):
    """labels with a one-pixel segment (1), a segment at pixel 0 (2), one at the last pixel (3), one across a 4-pixel boundary
    (4: pixels 2 .. 5) and seeded labels 5 .. 9 elsewhere"""
    g = torch.Generator().manual_seed(seed)
    seg = torch.randint(5, 10, (n_img, HW), generator=g, dtype=I32)
    seg[:, 2:6] = 4
    if HW > 7:
        seg[:, 6] = 1
    seg[:, 0] = 2
    seg[:, HW - 1] = 3
    return seg


def _special_values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1)
    n = flat.numel()
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
        flat[(i * 5) % n] = v
        flat[n - 1 - (i * 3) % n] = v
    flat[2 % n] = torch.tensor([0x7FC12345], dtype=I32).view(torch.float32)[0]      # a NaN with a payload
    return x


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("HW", [7, 99, 120, 224 * 224])
@pytest.mark.parametrize("C", [1, 3])
def test_compose_is_the_torch_select_bit_for_bit(C, HW, n_img):
    from xai_engine import kernels as K
    L = 8
    H, W = {7: (7, 1), 99: (11, 9), 120: (12, 10)}.get(HW, (224, 224))
    seg = _special_labels(n_img, HW, 1).view(n_img, H, W).to(DEV)
    start, finish = _special_values((n_img, C, H, W), 2).to(DEV), _special_values((n_img, C, H, W), 3).to(DEV)
    for offset in (0, 1):                                  # 1: every float pointer 4 bytes off a 16-byte boundary -> the scalar path
        def off(t):
            buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
            view = buf[offset:offset + t.numel()].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4 * offset
            return view
        s, f = off(start), off(finish)
        for n_cand in (1, L - 1, L):
            cand = torch.full((n_img, L), -1, dtype=I32)
            labels = [4, 1, 2, 3, 5, 4242, 7, 9]           # 4242: a label no pixel carries
            for b in range(n_img):
                cand[b, :n_cand] = torch.tensor(labels[b:] + labels[:b], dtype=I32)[:n_cand]
            cand = cand.to(DEV)
            out = off(torch.full((n_img * L, C, H, W), 7.0))
            got = K.mda_compose(s, f, seg, cand, out=out)
            assert got.data_ptr() == out.data_ptr()
            want = torch.where((seg[:, None, None] == cand[:, :, None, None, None]), f[:, None], s[:, None]).reshape(n_img * L, C, H, W)
            assert torch.equal(_bits(got), _bits(want)), (offset, n_cand)
            rows = got.view(n_img, L, C, H, W)
            assert torch.equal(_bits(rows[:, n_cand:]), _bits(s[:, None].expand(n_img, L - n_cand, C, H, W)))     # plain copies of start
            if n_cand == L:
                assert torch.equal(_bits(rows[0, 5]), _bits(s[0]))                                                # the absent label


def test_commit_takes_the_last_winners_pixels_and_nothing_else():
    from xai_engine import kernels as K
    for H, W in ((11, 9), (12, 10)):
        seg = _special_labels(3, H * W, 4).view(3, H, W).to(DEV)
        start, finish = _special_values((3, 3, H, W), 5).to(DEV), _special_values((3, 3, H, W), 6).to(DEV)
        state = torch.tensor([[1, 0, 4, 9], [0, 0, -1, 9], [5, 1, 3, 9]], dtype=I32, device=DEV)
        want = torch.where(seg[:, None] == state[:, 2].view(3, 1, 1, 1), finish, start)
        got = K.mda_commit(finish, seg, state, start.clone())
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got[1]), _bits(start[1]))


# ------------------------------------------------------------------------------------------------ K37
def _first(values, maximum):
    """torch.argmax / torch.argmin on the CPU: the first NaN, else the first extreme value"""
    v = np.asarray(values, np.float32)
    nan = np.flatnonzero(np.isnan(v))
    if len(nan):
        return int(nan[0])
    return int(np.flatnonzero(v == (v.max() if maximum else v.min()))[0])


def select_restated(a, mode, stop_test, cutoff):
    """one K37 launch on the host copies in `a` (dict of NumPy arrays), image by image, as the header states it"""
    n_img, L = a["resp"].shape
    S = a["order"].shape[1]
    for b in range(n_img):
        step, done, _, n_plan = a["state"][b]
        if done != 0 or step >= n_plan:
            continue
        slot, n_cand, cutoff_slot = a["plan"][b, step]
        n_next = a["plan"][b, step + 1, 1] if step + 1 < n_plan else 0
        w = _first(a["resp"][b, :n_cand], mode == 1)
        s = a["cand"][b, w]
        a["mr"][b, slot] = a["resp"][b, w]
        a["chosen"][b, slot] = s
        a["taken"][b, s] = 1
        stop = 0
        if mode == 1 and stop_test:
            with np.errstate(all="ignore"):
                q = np.float32(np.float32(a["resp"][b, w] - a["ref"][b, 0]) / a["ref"][b, 1])
            if q >= np.float32(cutoff):
                a["mr"][b, cutoff_slot] = np.float32(cutoff)
                stop = 1
        if stop:
            n_next = 0
        free = [int(x) for x in a["order"][b] if not a["taken"][b, x]]
        a["cand"][b] = -1
        a["cand"][b, :min(n_next, len(free))] = free[:n_next]
        a["state"][b] = (step + 1, stop, s, n_plan)


def _select_case(resp, mode=1, cutoff=0.9, ref=(0.25, 0.5), plan=None, S=17, L=8, n_img=1, preloaded=(), step=0, stop_test=None):
    from xai_engine import mda
    plan = plan if plan is not None else mda.step_plan(S, S, len(preloaded), mode == 1)
    rng = np.random.RandomState(S)
    a = dict(resp=np.zeros((n_img, L), np.float32), order=np.stack([rng.permutation(S) for _ in range(n_img)]).astype(np.int32),
             plan=np.zeros((n_img, max(len(plan), 1), 3), np.int32), ref=np.tile(np.float32(ref), (n_img, 1)),
             mr=np.zeros((n_img, S), np.float32), chosen=np.full((n_img, S), -1, np.int32), taken=np.zeros((n_img, S), np.int32),
             cand=np.full((n_img, L), -1, np.int32), state=np.zeros((n_img, 4), np.int32))
    a["resp"][:, :np.shape(resp)[-1]] = resp
    if plan:
        a["plan"][:, :len(plan)] = plan
    for b in range(n_img):
        for j, s in enumerate(preloaded):
            a["chosen"][b, S - len(preloaded) + j] = s
            a["taken"][b, s] = 1
        # bring the image to `step`: the segments of the first `step` slots are taken
        free = [int(x) for x in a["order"][b] if not a["taken"][b, x]]
        for i in range(step):
            a["chosen"][b, plan[i][0]] = free[i]
            a["taken"][b, free[i]] = 1
        free = free[step:]
        n0 = plan[step][1] if step < len(plan) else 0
        a["cand"][b, :n0] = free[:n0]
        a["state"][b] = (step, 0, -1, len(plan))
    return a, (mode, (mode == 1 and cutoff != 1) if stop_test is None else stop_test, cutoff)


def _launch(a, mode, stop_test, cutoff):
    from xai_engine import kernels as K
    d = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in a.items()}
    K.mda_select(d["resp"], d["order"], d["plan"], d["ref"] if (mode == 1 and stop_test) else None, mode, cutoff, d["mr"], d["chosen"],
                 d["taken"], d["cand"], d["state"], stop_test=stop_test)
    return d


def _same(d, a):
    for k in ("mr", "chosen", "taken", "cand", "state"):
        got, want = d[k].cpu().numpy(), a[k]
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (k, got, want)


TIES = {"first": [0.5, 0.2, 0.5, 0.1, 0.5, 0.3, 0.2, 0.4], "middle": [0.1, 0.2, 0.7, 0.1, 0.7, 0.3, 0.2, 0.4],
        "last": [0.1, 0.2, 0.3, 0.1, 0.4, 0.3, 0.9, 0.9], "low_first": [0.1, 0.2, 0.1, 0.3, 0.5, 0.3, 0.2, 0.4],
        "low_last": [0.6, 0.2, 0.3, 0.4, 0.5, 0.3, 0.05, 0.05],
        "low_middle": [0.6, 0.2, 0.05, 0.4, 0.05, 0.3, 0.2, 0.4], "one_nan": [0.1, 0.9, float("nan"), 0.0, 0.5, 0.3, 0.2, 0.4],
        "two_nans": [0.1, float("nan"), 0.95, float("nan"), 0.0, 0.3, 0.2, 0.4], "nan_first": [float("nan"), 0.2, 0.3, 0.1, 0.4, 0.3, 0.9, 0.0]}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(TIES))
def test_select_takes_the_first_of_equal_values_and_the_first_nan(name, mode):
    a, args = _select_case(TIES[name], mode=mode, cutoff=1)
    cand0 = a["cand"][0].copy()
    d = _launch(a, *args)
    select_restated(a, *args)
    _same(d, a)
    w = _first(TIES[name], mode == 1)
    assert int(d["chosen"][0, 0]) == int(d["state"][0, 2]) == int(cand0[w])
    want = {"first": (0, 3), "low_middle": (0, 2), "middle": (2, 0), "last": (6, 0), "low_first": (4, 0), "low_last": (0, 6), "one_nan": (2, 2), "two_nans": (1, 1),
            "nan_first": (0, 0)}[name][0 if mode == 1 else 1]
    assert w == want


def test_stop_test_is_torchs_fp32_arithmetic_at_equality_one_ulp_below_and_with_cutoff_one():
    c = np.float32(0.9)
    w_eq = np.float32(np.float32(0.25) + np.float32(0.5) * c)
    assert np.float32(np.float32(w_eq - np.float32(0.25)) / np.float32(0.5)) == c        # holds with exact equality
    w_below = np.nextafter(w_eq, np.float32(0))
    # what torch computes for the same values on a 0-d float32 tensor and Python floats (:190)
    assert bool(((torch.tensor(w_eq) - 0.25) / abs(0.75 - 0.25)) >= 0.9) and not bool(((torch.tensor(w_below) - 0.25) / abs(0.75 - 0.25)) >= 0.9)
    for w, cutoff, stops in ((w_eq, 0.9, True), (w_below, 0.9, False), (np.float32(0.99), 1, False), (np.float32(0.99), 0.9, True)):
        a, args = _select_case([0.1, w, 0.2, 0.3, 0.0, 0.1, 0.2, 0.3], cutoff=cutoff)
        d = _launch(a, *args)
        select_restated(a, *args)
        _same(d, a)
        assert int(d["state"][0, 1]) == int(stops)
        assert (float(d["mr"][0, 0]) == float(np.float32(0.9))) == stops                 # phase 1: the slot just filled gets the cutoff
        assert bool((d["cand"][0] == -1).all()) == stops
    # a value that rounds differently when the division is a reciprocal multiply or runs in fp64 is decided as fp32 decides it
    ref = (np.float32(0.1), np.float32(0.7))
    for w in np.float32([0.73, 0.7299999, 0.73000004, 0.72999996]):
        a, args = _select_case([w, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], ref=ref)
        d = _launch(a, *args)
        select_restated(a, *args)
        _same(d, a)
        assert int(d["state"][0, 1]) == int(bool(((torch.tensor(w) - float(ref[0])) / float(ref[1])) >= 0.9))


def test_phase_two_stop_writes_the_cutoff_into_the_phase_local_slot_and_a_second_launch_changes_nothing():
    from xai_engine import kernels as K
    S, L = 17, 8
    step = 12                                              # phase 2 (steps 9 .. 16): slot 12, n_cand 5, cutoff slot 3
    a, args = _select_case([0.2, 0.95, 0.1, 0.3, 0.5], step=step)
    assert tuple(a["plan"][0, step]) == (12, 5, 3)
    a["mr"][0, :step] = np.linspace(0.1, 0.6, step, dtype=np.float32)
    d = _launch(a, *args)
    select_restated(a, *args)
    _same(d, a)
    assert float(d["mr"][0, 3]) == float(np.float32(0.9)) and float(d["mr"][0, 12]) == float(np.float32(0.95)) and int(d["state"][0, 1]) == 1
    before = {k: v.clone() for k, v in d.items()}
    K.mda_select(d["resp"], d["order"], d["plan"], d["ref"], 1, 0.9, d["mr"], d["chosen"], d["taken"], d["cand"], d["state"])
    for k in before:
        assert torch.equal(d[k].view(torch.int32), before[k].view(torch.int32)), k
    # an exhausted plan is left untouched as well
    a, args = _select_case([0.3], mode=0, S=4, L=4, step=4)
    d = _launch(a, *args)
    _same(d, a)


def test_preloaded_tail_segments_never_become_candidates_and_the_whole_deletion_plan_runs():
    from xai_engine import kernels as K
    S, L = 17, 8
    rng = np.random.RandomState(3)
    for input_length in (1, 8, 10, 16):
        pre = [int(s) for s in rng.permutation(S)[:input_length]]
        a, args = _select_case(rng.rand(L).astype(np.float32), mode=0, preloaded=pre)
        assert not set(a["cand"][0][a["cand"][0] >= 0]) & set(pre)
        d = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in a.items()}
        for _ in range(S - input_length + 1):              # one launch more than the plan has rows
            resp = rng.rand(1, L).astype(np.float32)
            a["resp"][:] = resp
            d["resp"].copy_(torch.from_numpy(resp))
            K.mda_select(d["resp"], d["order"], d["plan"], None, 0, 1.0, d["mr"], d["chosen"], d["taken"], d["cand"], d["state"])
            select_restated(a, *args)
            _same(d, a)
            assert not set(a["cand"][0][a["cand"][0] >= 0]) & set(pre)
        assert sorted(a["chosen"][0]) == list(range(S)) and list(a["chosen"][0, S - input_length:]) == pre


def test_three_images_of_which_one_is_done_and_the_cap():
    from xai_engine import XaiHipError, kernels as K
    a, args = _select_case(np.float32([[0.1, 0.95, 0.2, 0.3, 0.0, 0.1, 0.2, 0.3], [0.3, 0.2, 0.1, 0.3, 0.0, 0.1, 0.2, 0.3],
                                       [0.1, 0.2, 0.3, 0.4, 0.5, 0.1, 0.2, 0.3]]), n_img=3)
    a["state"][1, 1] = 1                                   # image 1 is done: untouched; image 0 stops now; image 2 goes on
    d = _launch(a, *args)
    select_restated(a, *args)
    _same(d, a)
    assert d["state"][:, :2].tolist() == [[1, 1], [0, 1], [1, 0]]
    cap = K.mda_max_segments()
    assert cap >= 1024 and K.mda_max_width() >= 28
    for S, ok in ((cap, True), (cap + 1, False)):
        a, args = _select_case([0.5, 0.1, 0.2, 0.3, 0.0, 0.1, 0.2, 0.3], mode=0, S=S, L=8, plan=[(0, 8, -1), (1, 8, -1)])
        if ok:
            d = _launch(a, *args)
            select_restated(a, *args)
            _same(d, a)
        else:
            with pytest.raises(XaiHipError, match="xai_mda_select_f32 failed with code -3"):
                _launch(a, *args)


def test_candidates_are_ranked_across_the_waves_when_the_lanes_hold_a_ragged_share():
    """S = 601 over the select kernel's 256 lanes: three entries of `order` a lane, the last lane with one, 55 lanes with none.  Of the
    first 500 entries all but every 97th are taken, and the minimum of `resp` takes the one at 393: the eight free ones that become
    the next candidates lie in lanes 1, 34, 66, 98, 163, 166 and 167 (two), so the counts of three waves enter the ranks."""
    S = 601
    order = np.random.RandomState(S).permutation(S)                  # the order _select_case gives this S
    pre = [int(order[j]) for j in range(500) if j % 97 != 5]
    a, args = _select_case([0.5, 0.1, 0.2, 0.3, 0.0, 0.1, 0.2, 0.3], mode=0, S=S, L=8, plan=[(0, 8, -1), (1, 8, -1)], preloaded=pre)
    assert a["order"][0].tolist() == order.tolist() and a["cand"][0].tolist() == [int(order[j]) for j in (5, 102, 199, 296, 393, 490, 500, 501)]
    d = _launch(a, *args)
    select_restated(a, *args)
    _same(d, a)
    assert a["cand"][0].tolist() == [int(order[j]) for j in (5, 102, 199, 296, 490, 500, 501, 502)]


# ------------------------------------------------------------------------------------------------ both searches
def _k_resize(x, size):
    from xai_engine import kernels as K
    return K.resize_bilinear(x.to(DEV, torch.float32).contiguous(), size, size).cpu()


def _on_device(c):
    c = dict(c)
    c["model"] = c["model"].to(DEV)
    return c


SMALL = {"small_grid": (32, ("grid", 4), 2, 7, 3.0, 5.0, "blur", False), "small_vor": (32, ("voronoi", 17, 5), 5, 7, 3.0, 5.0, "blur", False),
         "small_never": (32, ("voronoi", 12, 2), 2, 7, 0.5, 2.0, "amplify", True)}


@pytest.fixture(scope="module")
def searched():
    """engine and restatement (the engine's pass shapes, the engine's metric and resize) once per case, on the device"""
    from xai_engine import mda
    out = {}
    for tag, args in list(R.CASES.items()) + list(SMALL.items()):
        c = _on_device(R.build_case(*args))
        S, hw = c["patch_count"], c["img_hw"]
        L = R.subsearch_len(S)
        sms = R.segment_saliency_map(c["saliency_map"], S, hw)
        assert torch.equal(sms, mda.segment_saliency_map(c["saliency_map"], S, hw))
        log = {}
        want = R.MDA(c["trans_img"], c["input_tensor"], c["saliency_map"], S, c["blur"], c["model"], DEV, hw, max_batch_size=5,
                     ordered=c["ordered"], vis=True, segments=c["segments"], pass_rows=L, metric=R.engine_metric(c["model"], hw),
                     resize=_k_resize, log=log)
        ins = mda.find_insertion_patches(c["input_tensor"], sms, c["segments"], c["blur"], S, 1, c["model"], DEV, hw, max_batch_size=5)
        got = mda.MDA(c["trans_img"], c["input_tensor"], c["saliency_map"], S, c["blur"], c["model"], DEV, hw, max_batch_size=5,
                      ordered=c["ordered"], vis=True, segments=c["segments"])
        tk = mda.find_deletion_patches(c["input_tensor"], c["segments"], sms, torch.as_tensor(log["order_a"])[0: log["end_index"] + 1], c["blur"],
                                       S, c["model"], DEV, hw, max_batch_size=5, kappa=(-1 if c["ordered"] else 0.005), test_kappa=True)
        out[tag] = (c, want, log, ins, got, tk)
    return out


@pytest.mark.parametrize("tag", sorted(R.CASES) + sorted(SMALL))
def test_searches_equal_the_restatement_on_the_device_bit_for_bit(searched, tag):
    from xai_engine import mda
    c, want, log, ins, got, tk = searched[tag]
    stopped = "cutoff_slot" in log["insertion"]
    assert (isinstance(ins[0], int) and ins[0] == 0) == stopped
    assert torch.equal(torch.as_tensor(ins[2]), torch.as_tensor(log["order_a"]))                     # the order and every slot
    if stopped:
        assert torch.equal(_bits(torch.as_tensor(ins[3])), _bits(torch.as_tensor(log["MR_ins"])))    # zeros where nothing was written
    else:
        assert np.array_equal(np.asarray(ins[3]), np.asarray(log["MR_ins"]))
    assert mda.end_index_of(ins[3]) == log["end_index"]
    assert torch.equal(tk[2], log["best_segment_list"]) and np.array_equal(tk[3], log["deletion"]["final_curve"])
    assert len(got) == len(want) == 6
    for g, w in zip(got, want):
        assert g.shape == (c["img_hw"], c["img_hw"], 3) and g.dtype == np.float32
        assert np.array_equal(g.view(np.int32), w.view(np.int32))


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_searches_reproduce_the_references_run_within_the_parity_bar(searched, tag):
    g = load_golden("mda.npz")
    c, _, _, ins, got, tk = searched[tag]
    S = c["patch_count"]
    assert np.array_equal(np.asarray(ins[2]), g[f"{tag}_order_a"])
    written = g[f"{tag}_MR_written"]
    check(f"mda_gpu/{tag}/MR_ins", np.where(written, np.asarray(ins[3], np.float64), 0.0), g[f"{tag}_MR_ins"], BAR)
    assert np.array_equal(tk[2].numpy(), g[f"{tag}_best"])
    check(f"mda_gpu/{tag}/del_curve", tk[3], g[f"{tag}_del_curve"], BAR, absolute=True)
    flat = c["segments"].flatten().numpy()
    for name, m in (("g0", got[0]), ("g10", got[4])):
        vals = np.array([m[:, :, 0].reshape(-1)[flat == s][0] for s in range(S)])
        check(f"mda_gpu/{tag}/{name}", vals, g[f"{tag}_{name}"], BAR)


def test_twelve_steps_are_twelve_graph_replays_and_at_most_two_reads_in_between(searched, monkeypatch):
    """the search of the 12-segment never-stopping case: after the first call has captured the step, a call replays it 12 times;
    between the first and the last replay the host reads the done word at most steps / POLL_INTERVAL + 1 times and nothing else"""
    from xai_engine import mda
    c = searched["small_never"][0]
    S, hw = c["patch_count"], c["img_hw"]
    assert S == 12 and len(mda.step_plan(S, S, 0, True)) == 12
    sms = R.segment_saliency_map(c["saliency_map"], S, hw)
    events = []
    real_read, real_replay, real_cpu, real_item = mda.read_back, torch.cuda.CUDAGraph.replay, torch.Tensor.cpu, torch.Tensor.item
    monkeypatch.setattr(mda, "read_back", lambda t: (events.append("read"), real_read(t))[1])
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (events.append("replay"), real_replay(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (events.append("read") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (events.append("read") if self.is_cuda else None, real_item(self))[1])
    before = dict(mda.MDA_COUNTS)
    r = mda.find_insertion_patches(c["input_tensor"], sms, c["segments"], c["blur"], S, 1, c["model"], DEV, hw, max_batch_size=5)
    monkeypatch.undo()
    assert not isinstance(r[0], int)                       # it never stopped
    replays = [i for i, e in enumerate(events) if e == "replay"]
    assert len(replays) == 12 and mda.MDA_COUNTS["steps"] - before["steps"] == 12
    assert mda.MDA_COUNTS["replayed"] - before["replayed"] == 1 and mda.MDA_COUNTS["eager"] == before["eager"]
    inside = events[replays[0]:replays[-1] + 1].count("read")
    assert inside <= 12 // mda.POLL_INTERVAL + 1 and inside == mda.MDA_COUNTS["polls"] - before["polls"] == 1


def test_harness_row_returns_the_map_of_the_direct_call():
    from helpers import vit_mini_from
    from xai_engine import kernels as K
    from xai_engine.blur import blur_until_unconfident
    from xai_engine.mda import MDA
    from xai_engine.sweep import get_VIT_attr
    from xai_engine.vit_attr import Baselines
    g = load_golden("vit_mini.npz")
    model = vit_mini_from(g, DEV)
    x = torch.from_numpy(g["x"])
    t = torch.tensor(int(g["target"]))
    seg = R.grid_labels(32, 4)
    td = {"models": [model, model], "img_hw": 32, "batch_size": 25, "device": DEV, "num_patches": 4, "attr_func": "MDA", "mda_segments": seg}
    got = get_VIT_attr(x.clone(), None, t, td)
    assert got.shape == (32, 32) and got.dtype == np.float32 and (got >= 0).all() and np.isfinite(got).all()
    blur, _, _, _ = blur_until_unconfident(model, x, t, DEV)
    bi, _ = Baselines(model).bidirectional(x.to(DEV), t, device=torch.device(DEV))
    bi = K.resize_bilinear(bi.detach().float().contiguous(), 32, 32)[0].cpu().numpy()[:, :, None] * np.ones((32, 32, 3))
    mda, _, _ = MDA(None, x, bi, 16, blur, model, DEV, 32, max_batch_size=5, segments=seg)
    assert np.array_equal(got, np.abs(np.sum(mda, axis=2)).astype(np.float32))
    with pytest.raises(ValueError, match="trans_img"):
        get_VIT_attr(x.clone(), None, t, dict(td, mda_segments=None))
