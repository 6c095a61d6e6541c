"""MDA (reference util/attribution_methods/MDAFunctions.py, evaluatePerturbation.py:243-263) on the HIP engine: the greedy
patch searches of find_insertion_patches (:39-311) and find_deletion_patches (:313-597) with their loop state on the device.

The reference builds every candidate image on the host (a torch.where over all pixels, a clone and a scatter per candidate),
uploads them five at a time and reads the scores back: at 196 patches about ten thousand host-built images and two thousand
round trips for one attribution.  Here one search step is

    K36 compose (the L candidate images straight into the pass's static input buffer)  ->  the classifier's forward  ->
    softmax and the target column (torch, on the device)  ->  K37 select (argmax / argmin, the writes, the stop test, the
    next candidates)  ->  K38 commit (the winner's pixels into `start`)

captured once and replayed as ONE hipGraph per step through the shared capture path (streams.CapturedCall).  The host never reads
a score inside the loop: it reads the two state words (steps taken, done) every POLL_INTERVAL steps and stops replaying once the
stop test has held; a replay after that changes nothing (K37 leaves a done image untouched), so polling late is safe.

What is restated, not repaired (each is the reference's behaviour): the phase-2 stop writes `cutoff` into the phase-local slot
(:260-261), which decides how many insertion patches MDA() hands to the deletion search (:614-617); the stop test is torch's
fp32 arithmetic on a 0-d float32 tensor and Python floats (K37); argmax / argmin take the first of equal values and the first
NaN.  What differs, and why:
  * `torch.argsort` without stable=True (:107, :110, :356) does not keep tied segment means in index order; the order here is
    the stable sort's.
  * `max_batch_size` only groups the reference's forwards into fives (:141-150); one step here is one pass of L rows (the rows
    above the step's n_cand are copies of `start`), the tail of the deletion search (:497-511, one image per pass there) passes
    of at most L rows written by K6.  The argument is kept and checked as the reference checks it.
  * the reference hard-codes torch.ones((224, 224, 3)) (:96, :346) and so runs at img_hw == 224 only; `img_hw` is used here.
  * the reference works only when n_searches equals the number of segments S (above it indexes past segment_order, below it
    divides by an empty segment's length) and when the labels are 0 .. S-1 without gaps: both are a ValueError here, and so is
    S == 1 (L = 2 > S: the reference indexes out of range).
  * worst_MR_list of the insertion search is torch.empty there (:124); the slots no step wrote are zeros here (no decision
    reads them: a stop writes `cutoff` at or below the last slot filled and :614-617 takes the first index >= 0.9).
  * CLIP_test_info is not None raises NotImplementedError.
After each search everything is the reference's own host arithmetic on S + 1 numbers: the monotone normalisation
(curves.monotone_normalise), normalize_curve = curves.shape_constrained_fit (cvxopt's QP solved exactly; parity with cvxopt's
iterate is unpinned), the two MASMetric.single_run calls on the engine's metric, np.interp, the sparse and dense maps and their
kappa rule, and the antialiased down / up resize of the `_s` outputs (K.resize_bilinear).  The per-segment means that give
segment_order are torch.mean on the host, S numbers once per call.  SLIC is skimage's on the host by default and the same
algorithm on K65-K68 with segments="device" (xai_engine/slic.py).
"""
import numpy as np
import torch

from . import curves
from . import kernels as K
from ._lib import XaiHipError
from .ig import _logits_of, check_input, hip_device
from .perturb import MASMetric
from .streams import LOGIT_RTOL, CapturedCall, ThreadGraphs, read_back

POLL_INTERVAL = 8            # search steps between two reads of the (steps taken, done) words; never one read per step
MDA_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0, "steps": 0, "polls": 0}
_SEARCHES = ThreadGraphs(limit=4)
_NEVER = 1 << 30             # flip step of a pixel the tail pass never flips


def subsearch_len(n_steps):
    """L = min(2 * int(sqrt(S)), 28), the sub-search width (:126, :365)"""
    return min(2 * int(n_steps ** (1 / 2)), 28)


def step_plan(n_steps, n_searches, input_length=0, insertion=True):
    """The (slot, n_cand, cutoff_slot) of every search step, host arithmetic on S, n_searches and input_length only.
    Insertion: n_searches - L steps of width L writing slot = step, then L steps of widths L .. 1 writing slot
    n_searches - L + j, whose stop writes `cutoff` into the phase-local slot j (:260-261).  Deletion: the same with
    input_length taken off (:366, :427-433, :489), no stop test (cutoff_slot -1)."""
    L = subsearch_len(n_steps)
    first = max(n_searches - L - (0 if insertion else input_length), 0)
    width = L if insertion or input_length <= n_searches - L else max(n_searches - input_length, 0)
    base = n_searches - width - (0 if insertion else input_length)
    plan = [(s, L, s if insertion else -1) for s in range(first)]
    plan += [(base + j, width - j, j if insertion else -1) for j in range(width)]
    return plan


def check_segments(segments, n_searches, name):
    """The (H, W) label map on the host -> (int64 tensor, S).  Labels 0 .. S-1 without gaps, S == n_searches, S >= 2."""
    seg = torch.as_tensor(np.asarray(segments.detach().cpu()) if torch.is_tensor(segments) else np.asarray(segments))
    if seg.dim() != 2 or seg.is_floating_point() or seg.dtype == torch.bool:
        raise ValueError(f"{name}: segments must be an (H, W) array of integer labels, got {tuple(seg.shape)} {seg.dtype}")
    seg = seg.to(torch.int64)
    ids = torch.unique(seg)
    S = int(ids.numel())
    if int(ids[0]) != 0 or int(ids[-1]) != S - 1:
        raise ValueError(f"{name}: segment labels must be 0 .. S-1 without gaps, {S} distinct labels span {int(ids[0])} .. "
                         f"{int(ids[-1])}: the reference looks every segment up as `segments == i` for i in range(S)")
    if int(n_searches) != S:
        raise ValueError(f"{name}: n_searches = {int(n_searches)} but the label map has {S} segments: the reference works only "
                         "when the two are equal (above it indexes past segment_order, below it divides by an empty segment's length)")
    if subsearch_len(S) > S:
        raise ValueError(f"{name}: {S} segment(s) give a sub-search width of {subsearch_len(S)}: the reference indexes out of range")
    return seg, S


def _batch_size_ok(n_steps, max_batch_size):
    """:45-49 / :316-320, the reference's own check and message"""
    batch_size = n_steps if n_steps < 50 else 25
    batch_size = max_batch_size if batch_size > max_batch_size else batch_size
    if batch_size > n_steps:
        print("Batch size cannot be greater than number of steps: " + str(n_steps))
        return False
    return True


def _refuse_clip(CLIP_test_info, name):
    if CLIP_test_info is not None:
        raise NotImplementedError(f"{name}: the CLIP path (CLIP_test_info) is not served by the HIP engine")


def segment_order_of(saliency_map_segmented, segments, n_steps, img_hw, descending):
    """:99-110 / :349-356 on the host: |sum over the channels|, torch.mean per segment, the stable argsort."""
    test = torch.abs(torch.sum(torch.as_tensor(saliency_map_segmented).detach().cpu().squeeze(), axis=2))
    flat = segments.flatten()
    segment_saliency = torch.zeros(n_steps)
    for i in range(n_steps):
        segment_saliency[i] = torch.mean(test.reshape(img_hw ** 2)[torch.where(flat == i)[0]])
    order = torch.argsort(segment_saliency, stable=True)
    return torch.flip(order, dims=(0,)) if descending else order


class _Search(CapturedCall):
    """Static buffers of one image's search and its step (module docstring).  One call = the state uploaded from the host
    (`load`), then at most `n_plan` replays of the step with a poll every POLL_INTERVAL steps."""

    warmup = 1

    def __init__(self, model, img_shape, S, L, mode, stop_test, cutoff, dev):
        super().__init__(MDA_COUNTS, (LOGIT_RTOL, 0, 0))
        self.model, self.S, self.L, self.mode, self.stop_test, self.cutoff = model, S, L, int(mode), bool(stop_test), float(cutoff)
        C, H, W = img_shape
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.start, self.finish = torch.zeros((1, C, H, W), **f32), torch.zeros((1, C, H, W), **f32)
        self.start0 = torch.zeros((1, C, H, W), **f32)
        self.seg = torch.zeros((1, H, W), **i32)
        self.rows = torch.zeros((L, C, H, W), **f32)                 # the pass's input, written by K36
        self.resp, self.stop_ref = torch.zeros((1, L), **f32), torch.zeros((1, 2), **f32)
        self.target = torch.zeros(1, dtype=torch.int64, device=dev)
        self.order, self.plan = torch.zeros((1, S), **i32), torch.zeros((1, S, 3), **i32)
        self.mr, self.chosen, self.taken = torch.zeros((1, S), **f32), torch.zeros((1, S), **i32), torch.zeros((1, S), **i32)
        self.cand, self.state = torch.zeros((1, L), **i32), torch.zeros((1, 4), **i32)
        self.init = None                                             # (chosen, taken, cand, state) of step 0, on the device
        self.n_plan = 0

    def load(self, start, finish, seg32, target, order, plan, stop_ref, preloaded):
        """Everything a search starts from.  `preloaded`: {slot: segment} already in worst_segment_list (:363)."""
        S, L, dev = self.S, self.L, self.start.device
        self.start0.copy_(start); self.finish.copy_(finish); self.seg.copy_(seg32); self.target.copy_(target.reshape(1))
        chosen = torch.full((1, S), -1, dtype=torch.int32)
        taken = torch.zeros((1, S), dtype=torch.int32)
        for slot, s in preloaded.items():
            chosen[0, slot] = s
            taken[0, s] = 1
        rows = torch.zeros((1, S, 3), dtype=torch.int32)
        if plan:
            rows[0, :len(plan)] = torch.tensor(plan, dtype=torch.int32)
        free = [int(s) for s in order.tolist() if not taken[0, int(s)]]
        n0 = plan[0][1] if plan else 0
        cand = torch.full((1, L), -1, dtype=torch.int32)
        cand[0, :n0] = torch.tensor(free[:n0], dtype=torch.int32)
        state = torch.tensor([[0, 0, -1, len(plan)]], dtype=torch.int32)
        self.order.copy_(order.to(torch.int32).reshape(1, S)); self.plan.copy_(rows)
        if stop_ref is not None:
            self.stop_ref.copy_(torch.tensor([stop_ref], dtype=torch.float32))
        self.init = tuple(t.to(dev) for t in (chosen, taken, cand, state))
        self.n_plan = len(plan)

    def step(self):
        K.mda_compose(self.start, self.finish, self.seg, self.cand, out=self.rows)
        with torch.no_grad():
            logits = _logits_of(self.model(self.rows)).float()
            self.resp.copy_(torch.softmax(logits, dim=1).index_select(1, self.target).view(1, self.L))
        K.mda_select(self.resp, self.order, self.plan, self.stop_ref if self.stop_test else None, self.mode, self.cutoff, self.mr,
                     self.chosen, self.taken, self.cand, self.state, stop_test=self.stop_test)
        K.mda_commit(self.finish, self.seg, self.state, self.start)
        return self.resp, self.chosen, self.state

    def compose(self, run):
        self.start.copy_(self.start0)
        self.mr.zero_()
        for dst, src in zip((self.chosen, self.taken, self.cand, self.state), self.init):
            dst.copy_(src)
        for i in range(self.n_plan):
            run()
            MDA_COUNTS["steps"] += 1
            if (i + 1) % POLL_INTERVAL == 0 and i + 1 < self.n_plan:
                MDA_COUNTS["polls"] += 1
                if int(read_back(self.state)[0, 1]) != 0:             # the stop test held (or K37 refused the plan): nothing left to do
                    break
        return self.resp, self.chosen, self.state


def _run_search(model, dev, start, finish, seg32, target, order, plan, mode, stop, preloaded, graphs=True):
    """-> (worst_MR_list float32 (S,), worst_segment_list int64 (S,), done, the device `start` after the search)"""
    S = order.numel()
    L = subsearch_len(S)
    if S > K.mda_max_segments() or L > K.mda_max_width():
        raise ValueError(f"MDA: {S} segments are more than K37 takes ({K.mda_max_segments()})")
    stop_test = stop is not None and stop[2] != 1
    cutoff = float(stop[2]) if stop is not None else 1.0
    img_shape = tuple(start.shape[1:])
    key = ("mda", img_shape, S, L, int(mode), stop_test, cutoff)
    search = _SEARCHES.get(model, dev, key, lambda: _Search(model, img_shape, S, L, mode, stop_test, cutoff, dev), cached=bool(graphs))
    stop_ref = None if stop is None else (np.float32(stop[0]), np.float32(abs(stop[1] - stop[0])))
    search.load(start, finish, seg32, target, order, plan, stop_ref, preloaded)
    if plan:
        search.run() if graphs else search.eager()
    host = read_back(torch.cat([search.mr.view(-1), search.chosen.view(-1).float(), search.state.view(-1).float()]))
    if not plan:                                                      # nothing ran: the loaded state is the result
        host[:S] = 0
        host[S:2 * S] = search.init[0].view(-1).float().cpu()
        host[2 * S:] = search.init[3].view(-1).float().cpu()
        search.start.copy_(search.start0)
    done = int(host[2 * S + 1])
    if done == 2:
        raise XaiHipError("MDA: K37 refused a plan row or a candidate outside its range (a bug in the step plan)")
    return host[:S].clone(), host[S:2 * S].to(torch.int64), done, search


def _probe(model, x, target=None):
    """:53-57, :65-67, :74-76: one image's softmax row -> (target (0-d int64 on the device), the probability as a Python float)"""
    with torch.no_grad():
        out = _logits_of(model(x)).detach()
    if target is None:
        _, index = torch.max(out, 1)
        target = index[0]
    return target, torch.nn.functional.softmax(out, dim=1)[0][target].item()


def _prepare(input_tensor, segments, n_searches, device, img_hw, name):
    dev = hip_device(device)
    seg, S = check_segments(segments, n_searches, name)
    x = check_input(torch.as_tensor(input_tensor).to(dev), name)
    if x.shape[0] != 1 or tuple(x.shape[2:]) != (img_hw, img_hw) or tuple(seg.shape) != (img_hw, img_hw):
        raise ValueError(f"{name}: input_tensor must be (1, C, {img_hw}, {img_hw}) and segments ({img_hw}, {img_hw}), got "
                         f"{tuple(x.shape)} and {tuple(seg.shape)}")
    return dev, seg, S, x


def _small(new_map3, n_steps, img_hw, dev):
    """upsize(downsize(.)) of :307-311 / :593-597 for an (H, W, 3) map of three equal channels: Resize(ceil(sqrt(S)),
    antialias=True), then Resize(img_hw, antialias=True), on the device (K.resize_bilinear)."""
    small_side = int(np.ceil(np.sqrt(n_steps)))
    m = new_map3.permute((2, 0, 1)).contiguous().to(dev, torch.float32)
    up = K.resize_bilinear(K.resize_bilinear(m, small_side, small_side).contiguous(), img_hw, img_hw)
    return up.permute((1, 2, 0)).cpu().numpy()


def normalize_curve(normalized_model_response, type=0):
    """:12-37: the curve closest to the response with its end points, 0 <= x <= 1 and non-negative (type 0, convex) or
    non-positive (type 1, concave) second differences -- the QP's unique optimum, computed exactly on the host."""
    return curves.shape_constrained_fit(np.asarray(normalized_model_response, np.float64), "del" if type == 0 else "ins")


def find_insertion_patches(input_tensor, saliency_map_segmented, segments, blur, n_searches, type, model, device, img_hw,
                           max_batch_size=25, cutoff=0.9, CLIP_test_info=None):
    """:39-311.  type 1: insertion from blur(input_tensor), argmax, the stop test; type 0: from zeros, argmin (the reference's
    type 0 names blur_pred in its stop test and so runs with cutoff == 1 only; the same is required here).
    -> (0, 0, worst_segment_list, worst_MR_list) after a stop, else (new_map, its down/up resize, best_segment_list, the
    monotone response), as the reference."""
    _refuse_clip(CLIP_test_info, "find_insertion_patches")
    if cutoff == 0:
        return 0, 0, torch.tensor([]), torch.tensor([0])
    if type not in (0, 1):
        raise ValueError("find_insertion_patches: type is 0 (deletion) or 1 (insertion)")
    if type == 0 and cutoff != 1:
        raise ValueError("find_insertion_patches: type 0 has no blurred prediction for the stop test (the reference raises a "
                         "NameError at :190); pass cutoff=1")
    dev, seg, n_steps, x = _prepare(input_tensor, segments, n_searches, device, img_hw, "find_insertion_patches")
    if not _batch_size_ok(n_steps, max_batch_size):
        return 0
    target, original_pred = _probe(model, x)
    finish = x
    start = torch.zeros_like(x) if type == 0 else blur(torch.as_tensor(input_tensor)).to(dev, torch.float32).contiguous()
    _, base_pred = _probe(model, start, target)                        # black_pred / blur_pred
    order = segment_order_of(saliency_map_segmented, seg, n_steps, img_hw, descending=(type == 1))
    plan = step_plan(n_steps, n_searches, 0, True)
    stop = (base_pred, original_pred, cutoff) if type == 1 else None
    mr, chosen, done, _ = _run_search(model, dev, start, finish, seg.to(torch.int32)[None], target, order, plan, type, stop, {})
    worst_segment_list, worst_MR_list = chosen, mr
    if done:
        return 0, 0, worst_segment_list, worst_MR_list                 # :192 / :262
    if type == 0:                                                      # :264-268
        response = torch.flip(torch.cat((worst_MR_list, torch.tensor([original_pred]))), (0,))
    else:
        response = torch.cat((torch.tensor([base_pred]), worst_MR_list))
    response = response.numpy().copy().astype(np.double)
    original_MR = curves.monotone_normalise(response, base_pred, original_pred, falling=(type == 0))      # :275-285
    fitted = normalize_curve(original_MR, type)
    best_segment_list = torch.flip(worst_segment_list, (0,)) if type == 0 else worst_segment_list
    new_map = torch.zeros((img_hw, img_hw))
    flat = seg.flatten()
    for i in range(1, n_steps + 1):                                    # :297-304
        segment_coords = torch.where(flat == best_segment_list[i - 1])[0]
        target_MR = fitted[i - 1] - fitted[i] if type == 0 else fitted[i] - fitted[i - 1]
        new_map.reshape(img_hw ** 2)[segment_coords] = (torch.ones(len(segment_coords)) / len(segment_coords)) * target_MR
    new_map = new_map.unsqueeze(2) * torch.ones((img_hw, img_hw, 3))
    return new_map.numpy(), _small(new_map, n_steps, img_hw, dev), best_segment_list, original_MR


def find_deletion_patches(input_tensor, segments, saliency_map_segmented, beginning_order, blur, n_searches, model, device, img_hw,
                          max_batch_size=25, kappa=0.005, test_kappa=False, CLIP_test_info=None):
    """:313-597: the worst insertion order from zeros (argmin) over the segments the insertion search did not hand over, the
    cumulative pass over the handed-over tail (K6), the two metric runs and the sparse / dense maps.
    -> (map_0, map_0_s, map_5, map_5_s, map_10, map_10_s, best_segment_list), or the reference's test_kappa tuple."""
    _refuse_clip(CLIP_test_info, "find_deletion_patches")
    dev, seg, n_steps, x = _prepare(input_tensor, segments, n_searches, device, img_hw, "find_deletion_patches")
    if not _batch_size_ok(n_steps, max_batch_size):
        return 0
    beginning_order = torch.as_tensor(beginning_order).to(torch.int64).reshape(-1)
    input_length = len(beginning_order)
    if input_length > n_steps or (input_length and (int(beginning_order.min()) < 0 or int(beginning_order.max()) >= n_steps)) \
            or len(set(beginning_order.tolist())) != input_length:
        raise ValueError(f"find_deletion_patches: beginning_order must hold at most {n_steps} distinct segments of 0 .. {n_steps - 1}")
    target, original_pred = _probe(model, x)
    start, finish = torch.zeros_like(x), x
    _, black_pred = _probe(model, start, target)
    order = segment_order_of(saliency_map_segmented, seg, n_steps, img_hw, descending=False)
    tail = torch.flip(beginning_order, (0,))                           # :363
    preloaded = {n_steps - input_length + j: int(s) for j, s in enumerate(tail.tolist())}
    plan = step_plan(n_steps, n_searches, input_length, False)
    seg32 = seg.to(torch.int32)[None]
    mr, worst_segment_list, _, search = _run_search(model, dev, start, finish, seg32, target, order, plan, 0, None, preloaded)
    worst_MR_list = mr
    if input_length:                                                   # :497-511 as a flip-step perturbation of the searched image
        L = subsearch_len(n_steps)
        table = torch.full((n_steps,), _NEVER, dtype=torch.int32)
        table[tail] = torch.arange(input_length, dtype=torch.int32)
        flip = table.to(dev)[search.seg.view(-1).long()].contiguous()
        parts = []
        with torch.no_grad():
            for lo in range(0, input_length, L):
                n = min(L, input_length - lo)
                images = K.perturb_batch(search.start[0], search.finish[0], flip, lo, n)
                parts.append(torch.softmax(_logits_of(model(images)).float(), dim=1).index_select(1, target.reshape(1)).view(-1))
        worst_MR_list[n_steps - input_length:] = read_back(torch.cat(parts))
    response = torch.cat((worst_MR_list, torch.tensor([original_pred]))).numpy().copy().astype(np.double)[::-1]      # :514-516
    fitted = normalize_curve(curves.monotone_normalise(response, black_pred, original_pred, falling=True), type=0)   # :520-527
    best_segment_list = torch.flip(worst_segment_list, (0,))           # :530
    flat = seg.flatten()
    new_map = torch.zeros((img_hw, img_hw))
    for i in range(1, n_steps + 1):                                    # :534-537
        segment_coords = torch.where(flat == best_segment_list[i - 1])[0]
        target_MR = fitted[i - 1] - fitted[i]
        new_map.reshape(img_hw ** 2)[segment_coords] = (torch.ones(len(segment_coords)) / len(segment_coords)) * target_MR \
            + (target_MR * (n_steps - i) / n_steps)
    new_map = new_map.unsqueeze(2) * torch.ones((img_hw, img_hw, 3))
    new_map_test = np.abs(np.sum(new_map.numpy(), axis=2))             # :543
    MAS_insertion = MASMetric(model, img_hw ** 2, 'ins', img_hw, substrate_fn=blur)
    MAS_deletion = MASMetric(model, img_hw ** 2, 'del', img_hw, substrate_fn=torch.zeros_like)
    _, _, _, _, raw_score_ins = MAS_insertion.single_run(torch.as_tensor(input_tensor), new_map_test, dev, max_batch_size=max_batch_size)
    _, _, _, _, raw_score_del = MAS_deletion.single_run(torch.as_tensor(input_tensor), new_map_test, dev, max_batch_size=max_batch_size)
    x_old = np.linspace(0, 100, len(raw_score_ins))                    # :553-561
    x_new = np.linspace(0, 100, n_steps + 1)
    raw_score_ins = np.interp(x_new, x_old, raw_score_ins)
    raw_score_del = np.interp(x_new, x_old, raw_score_del)
    new_curve = 1 - np.mean([raw_score_ins, 1 - raw_score_del], axis=0)
    fitted = normalize_curve(new_curve, type=0)
    new_map_sparse, new_map_dense = torch.zeros((img_hw, img_hw)), torch.zeros((img_hw, img_hw))
    ones_map = torch.ones((img_hw, img_hw))
    if test_kappa:                                                     # :568-569
        return new_map_dense, seg, best_segment_list, fitted, ones_map, n_steps + 1
    for i in range(1, n_steps + 1):                                    # :571-581
        segment_coords = torch.where(flat == best_segment_list[i - 1])[0]
        target_MR = fitted[i - 1] - fitted[i]
        attr_value = 1 / len(segment_coords) * target_MR + (target_MR * (n_steps - i) / n_steps)
        new_map_sparse.reshape(img_hw ** 2)[segment_coords] = ones_map.reshape(img_hw ** 2)[segment_coords] * attr_value
        if attr_value >= kappa:
            new_map_dense.reshape(img_hw ** 2)[segment_coords] = ones_map.reshape(img_hw ** 2)[segment_coords] * ((n_steps - i) / n_steps)
        else:
            new_map_dense.reshape(img_hw ** 2)[segment_coords] = ones_map.reshape(img_hw ** 2)[segment_coords] * attr_value
    new_map_dense = new_map_dense / new_map_dense.max() * new_map_sparse.max()      # :584
    ones3 = torch.ones((img_hw, img_hw, 3))
    out = []
    for w in (0, 0.5, 1):                                              # :586-597
        m = (((1 - w) * new_map_sparse) + ((w) * new_map_dense)).unsqueeze(2) * ones3
        out += [m.numpy(), _small(m, n_steps, img_hw, dev)]
    return (*out, best_segment_list)


SLIC = ("skimage", "device")


def slic_segments(trans_img, patch_count, which="skimage", device="cuda"):
    """:602-604: SLIC of the un-normalised image.  which "skimage": skimage's, on the host.  "device": the same algorithm (scikit-image
    0.18.3's, in the image's float32) on K65-K68 (xai_engine/slic.py) on `device`; needs no scikit-image."""
    if which not in SLIC:
        raise ValueError(f"MDA: slic must be one of {SLIC}, got {which!r}")
    if which == "device":
        from .slic import slic as device_slic
        segment_img = np.transpose(trans_img.squeeze().detach().cpu().numpy(), (1, 2, 0))
        return torch.tensor(device_slic(segment_img, n_segments=patch_count, compactness=10000, start_label=0, device=device), dtype=int)
    try:
        from skimage.segmentation import slic
        from skimage.util import img_as_float
    except ImportError as e:
        raise ImportError("MDA's own segmentation needs scikit-image (skimage.segmentation.slic), which is not installed; "
                          "without it only callers that pass segments= work") from e
    segment_img = np.transpose(trans_img.squeeze().detach().numpy(), (1, 2, 0))
    segment_img = img_as_float(segment_img)
    return torch.tensor(slic(segment_img, n_segments=patch_count, compactness=10000, start_label=0), dtype=int)


def segment_saliency_map(saliency_map, patch_count, img_hw):
    """:607-609 on the host: the (H, W, 3) attribution down to the patch grid (Resize(int(sqrt(patch_count)), antialias=True)) and
    back up (Resize((img_hw, img_hw), NEAREST_EXACT)); torchvision's resizes are torch's interpolate."""
    x = torch.tensor(np.asarray(saliency_map), dtype=torch.float).permute((2, 0, 1))
    side = int(patch_count ** (1 / 2))
    down = torch.nn.functional.interpolate(x[None], size=(side, side), mode="bilinear", align_corners=False, antialias=True)
    return torch.nn.functional.interpolate(down, size=(img_hw, img_hw), mode="nearest-exact")[0].permute((1, 2, 0))


def end_index_of(MR_ins):
    """:614-617: the first index with MR_ins >= 0.9, else len(MR_ins)"""
    hit = np.where(np.asarray(MR_ins) >= 0.9)[0]
    return int(hit[0]) if len(hit) else len(MR_ins)


def MDA(trans_img, input_tensor, saliency_map, patch_count, blur, model, device, img_hw, max_batch_size=5, ordered=False,
        CLIP_test_info=None, vis=False, segments=None):
    """:600-626.  `segments` (not a reference argument): the (img_hw, img_hw) label map to use instead of SLIC's, or who computes
    SLIC: None or "skimage" on the host, "device" on K65-K68 (`slic_segments`).  The signature is the reference's plus this one
    argument, so the choice of segmenter rides on it.
    -> (MGA_g_0, MGA_g_0_s, MGA_g_10), with vis all six maps, as (H, W, 3) NumPy arrays."""
    _refuse_clip(CLIP_test_info, "MDA")
    if segments is None or isinstance(segments, str):
        segments = slic_segments(trans_img, patch_count, "skimage" if segments is None else segments, device)
    saliency_map_segmented = segment_saliency_map(saliency_map, patch_count, img_hw)
    x = torch.as_tensor(input_tensor).cpu()
    _, _, order_a, MR_ins = find_insertion_patches(x, saliency_map_segmented, segments, blur, patch_count, type=1, model=model,
                                                   device=device, img_hw=img_hw, max_batch_size=max_batch_size)
    end_index = end_index_of(MR_ins)
    res = find_deletion_patches(x, segments, saliency_map_segmented, order_a[0: end_index + 1], blur, patch_count, model, device, img_hw,
                                max_batch_size=max_batch_size, **({"kappa": -1} if ordered else {}))
    MGA_g_0, MGA_g_0_s, MGA_g_5, MGA_g_5_s, MGA_g_10, MGA_g_10_s, _ = res
    if vis is False:
        return MGA_g_0, MGA_g_0_s, MGA_g_10
    return MGA_g_0, MGA_g_0_s, MGA_g_5, MGA_g_5_s, MGA_g_10, MGA_g_10_s
