"""Plain-torch restatement of the reference's MDA flow (util/attribution_methods/MDAFunctions.py: normalize_curve :12-37,
find_insertion_patches :39-311, find_deletion_patches :313-597, MDA :600-626), the yardstick of the MDA tests and the
comparison flow of profiles/bench_mda.py.  It keeps the reference's shape -- every candidate image built on the host with a
clone and a scatter, uploaded, the responses read back, one host decision per step -- and cites it line by line.

What is a parameter here and a constant there:
  * `img_hw`: the reference hard-codes torch.ones((224, 224, 3)) (:96, :346) and so runs at 224 only.
  * `pass_rows`: None groups a step's candidates into the reference's batches (`max_batch_size`, the shrinking `batch_size` of
    :141-150, one image at a time in the tail :497-511; an empty leftover batch is skipped instead of being sent through the
    classifier).  An integer L sends ONE pass of L rows per step -- the rows above the step's n_cand are copies of `start` --
    and the tail in passes of at most L rows: the engine's pass shapes, so that the two can be compared bit for bit.
  * `metric(mode, substrate_fn, input_tensor, saliency, device, max_batch_size)` -> the normalised response curve of
    MASMetric.single_run (its fifth return value, :546-547).  `oracle_metric` is the NumPy oracle (oracle/perturb.py, any
    device), `engine_metric` the engine's own MASMetric (HIP).
  * `resize(x, size)` for the two antialiased resizes of the `_s` outputs (:307-311, :593-597): torchvision's
    Resize(size, antialias=True) of a square (C, H, W) tensor is F.interpolate(bilinear, antialias=True).
  * worst_MR_list of the insertion search is torch.empty in the reference (:124): the slots no step wrote hold whatever the
    allocator left.  They are zeros here.  No decision reads them: a search that stops writes `cutoff` at or below the last
    slot it filled, and MDA() takes the FIRST index with MR_ins >= 0.9 (:614-617).
  * torch.argsort without stable=True (:107, :110, :356) does not keep ties in index order; this sorts stably.
normalize_curve is the project's exact solver (xai_engine.curves.shape_constrained_fit): cvxopt is not importable.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def subsearch_len(n_steps):
    """:126 / :365"""
    return (int(n_steps ** (1 / 2)) * 2) if (int(n_steps ** (1 / 2)) * 2) <= 28 else 28


def reference_step_plan(n_steps, n_searches, input_length, insertion):
    """[(slot, n_cand, cutoff_slot)] per search step, transcribed from the reference's loop bounds: :127 and :195-196, :253, :191,
    :261 for insertion; :366, :427-433, :489 for deletion (cutoff_slot -1: no stop test)."""
    L = subsearch_len(n_steps)
    plan = []
    if insertion:
        for step in range(n_searches - L):                                       # :127
            plan.append((step, L, step))                                         # :183, :191
        subsearch_len_orig = L                                                   # :194
        for step in range(subsearch_len_orig):                                   # :195
            plan.append((step + n_searches - subsearch_len_orig, subsearch_len_orig - step, step))      # :196, :253, :261
        return plan
    for step in range(n_searches - L - input_length):                            # :366
        plan.append((step, L, -1))                                               # :420
    if input_length > n_searches - L:                                            # :427-430
        subsearch_len_orig = n_searches - input_length
    else:
        subsearch_len_orig = L
    for step in range(subsearch_len_orig):                                       # :432
        plan.append((step + n_searches - subsearch_len_orig - input_length, subsearch_len_orig - step, -1))   # :433, :489
    return plan


def resize_antialias(x, size):
    """transforms.Resize(size, antialias=True) of a square (C, H, W) tensor"""
    return F.interpolate(x[None], size=(size, size), mode="bilinear", align_corners=False, antialias=True)[0]


def normalize_curve(normalized_model_response, type=0):
    """:12-37 -- the unique optimum of that QP, computed exactly"""
    from xai_engine import curves
    return curves.shape_constrained_fit(np.asarray(normalized_model_response, np.float64), "del" if type == 0 else "ins")


def oracle_metric(model, img_hw):
    from oracle import perturb as op

    def run(mode, substrate_fn, input_tensor, sal, device, max_batch_size):
        def logits_fn(batch):
            with torch.no_grad():
                return model(torch.from_numpy(np.ascontiguousarray(batch, dtype=np.float32)).to(device)).cpu().numpy()

        def sub(x):
            return substrate_fn(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).cpu().numpy()
        return op.mas(logits_fn, input_tensor.cpu().numpy(), sal, mode, img_hw, sub, None, max_batch_size)[4]
    return run


def engine_metric(model, img_hw):
    from xai_engine.perturb import MASMetric

    def run(mode, substrate_fn, input_tensor, sal, device, max_batch_size):
        return MASMetric(model, img_hw ** 2, mode, img_hw, substrate_fn).single_run(input_tensor, sal, device,
                                                                                     max_batch_size=max_batch_size)[4]
    return run


def _pred(model, x, device, target_class=None):
    """:53-57 / :65-67: the softmax row of one image -> (target, probability)"""
    with torch.no_grad():
        out = model(x.to(device)).detach()
    if target_class is None:
        _, index = torch.max(out, 1)
        target_class = index[0]
    percentage = torch.nn.functional.softmax(out, dim=1)[0]
    return target_class, percentage[target_class].item()


def segment_order_of(saliency_map_segmented, segments, n_steps, img_hw, descending):
    """:99-110 / :349-356"""
    saliency_map_segmented_test = torch.abs(torch.sum(saliency_map_segmented.squeeze(), axis=2))
    segment_saliency = torch.zeros(n_steps)
    for i in range(n_steps):
        segment = torch.where(segments.flatten() == i)[0]
        segment_saliency[i] = torch.mean(saliency_map_segmented_test.reshape(img_hw ** 2)[segment])
    order = torch.argsort(segment_saliency, stable=True)
    return torch.flip(order, dims=(0,)) if descending else order


def _responses(model, device, images, n_cand, target_class, pass_rows, start, batch_size):
    """the candidates' softmax scores, on the host: the reference's batches (:141-175) or one pass of `pass_rows` rows"""
    model_response = torch.zeros(n_cand)
    with torch.no_grad():
        if pass_rows is not None:
            rows = torch.cat([images, start.expand(pass_rows - n_cand, -1, -1, -1)]) if pass_rows > n_cand else images
            output = model(rows.to(device)).detach()
            model_response[:] = nn.functional.softmax(output, dim=1)[:n_cand, target_class].cpu()
            return model_response, batch_size
        batch_size = n_cand if n_cand < batch_size else batch_size                # :141
        num_batches = int(n_cand / batch_size)
        leftover = n_cand % batch_size
        total_steps = 0
        for batch in [batch_size] * num_batches + [leftover]:                     # :149-150
            if batch == 0:
                continue
            output = model(images[total_steps:total_steps + batch].to(device)).detach()
            percentage = nn.functional.softmax(output, dim=1)
            model_response[total_steps:total_steps + batch] = percentage[:, target_class].cpu()
            total_steps += batch
    return model_response, batch_size


def _search(model, device, start, finish, segments, segment_order, worst_segment_list, worst_MR_list, plan, type, target_class,
            pass_rows, batch_size, img_hw, stop=None, log=None):
    """the two loops of a search (:127-192 and :195-262; :366-425 and :432-494) over `plan` -> True if the stop test held"""
    C = start.shape[1]
    flat = segments.flatten()
    for slot, n_cand, cutoff_slot in plan:
        selected_segments = torch.zeros(n_cand)
        search_counter = 0
        index_counter = 0
        while index_counter != n_cand:                                            # :133-139
            if segment_order[search_counter] not in worst_segment_list:
                selected_segments[index_counter] = segment_order[search_counter]
                index_counter += 1
            search_counter += 1
        images = torch.zeros((n_cand, C, img_hw, img_hw))
        for i in range(n_cand):                                                   # :157-162
            start_temp = start.clone()
            segment_coords = torch.where(flat == selected_segments[i])[0]
            start_temp.reshape(C, img_hw ** 2)[:, segment_coords] = finish.reshape(C, img_hw ** 2)[:, segment_coords]
            images[i] = start_temp
        model_response, batch_size = _responses(model, device, images, n_cand, target_class, pass_rows, start, batch_size)
        worst_MR_index = torch.argmin(model_response) if type == 0 else torch.argmax(model_response)      # :177-180
        worst_MR = model_response[worst_MR_index]
        worst_MR_list[slot] = worst_MR                                            # :183 / :253
        worst_segment = selected_segments[worst_MR_index]
        worst_segment_list[slot] = worst_segment
        segment_coords = torch.where(flat == worst_segment)[0]                    # :187-188
        start.reshape(C, img_hw ** 2)[:, segment_coords] = finish.reshape(C, img_hw ** 2)[:, segment_coords]
        if log is not None:
            rest = torch.cat([model_response[:worst_MR_index], model_response[worst_MR_index + 1:]])
            log["winner_margin"].append(float((rest - worst_MR).abs().min()) if len(rest) else float("inf"))
            log["slots"].append(slot)
        if stop is not None:
            blur_pred, original_pred, cutoff = stop
            ratio = (worst_MR - blur_pred) / (abs(original_pred - blur_pred))    # :190 -- torch's fp32 on a 0-d tensor
            if log is not None:
                log["stop_margin"].append(abs(float(ratio) - cutoff))
            if cutoff != 1 and ratio >= cutoff:
                worst_MR_list[cutoff_slot] = cutoff                               # :191 / :261 (the phase-local slot)
                if log is not None:
                    log["cutoff_slot"] = cutoff_slot
                return True
    return False


def _check(segments, n_searches, max_batch_size):
    n_steps = len(np.unique(segments))
    batch_size = n_steps if n_steps < 50 else 25
    batch_size = max_batch_size if batch_size > max_batch_size else batch_size
    if batch_size > n_steps:
        raise ValueError("Batch size cannot be greater than number of steps: " + str(n_steps))
    if n_searches != n_steps:
        raise ValueError(f"n_searches = {n_searches} but the label map has {n_steps} segments")
    return n_steps, batch_size


def find_insertion_patches(input_tensor, saliency_map_segmented, segments, blur, n_searches, type, model, device, img_hw,
                           max_batch_size=25, cutoff=0.9, CLIP_test_info=None, *, pass_rows=None, resize=resize_antialias, log=None):
    """:39-311"""
    if cutoff == 0:
        return 0, 0, torch.tensor([]), torch.tensor([0])
    n_steps, batch_size = _check(segments, n_searches, max_batch_size)
    target_class, original_pred = _pred(model, input_tensor, device)
    finish = input_tensor.clone()
    start = torch.zeros_like(input_tensor) if type == 0 else blur(input_tensor).cpu()
    _, base_pred = _pred(model, start, device, target_class)                      # black_pred / blur_pred
    segment_order = segment_order_of(saliency_map_segmented, segments, n_steps, img_hw, descending=(type == 1))
    worst_segment_list = torch.full((1, n_steps), -1).squeeze()
    worst_MR_list = torch.zeros((1, n_steps)).squeeze()
    plan = reference_step_plan(n_steps, n_searches, 0, True)
    stop = (base_pred, original_pred, cutoff) if type == 1 else None              # :190 names blur_pred: insertion only
    if _search(model, device, start, finish, segments, segment_order, worst_segment_list, worst_MR_list, plan, type, target_class,
               pass_rows, batch_size, img_hw, stop, log):
        return 0, 0, worst_segment_list, worst_MR_list                            # :192 / :262
    if type == 0:                                                                 # :264-268
        normalized_model_response = torch.flip(torch.cat((worst_MR_list, torch.tensor([original_pred]))), (0,))
    else:
        normalized_model_response = torch.cat((torch.tensor([base_pred]), worst_MR_list))
    normalized_model_response = normalized_model_response.detach().cpu().numpy().copy().astype(np.double)
    lo, hi = 1.0, 0.0
    for i in range(n_steps + 1):                                                  # :275-285
        v = np.clip((normalized_model_response[i] - base_pred) / (abs(original_pred - base_pred)), 0.0, 1.0)
        if type == 0:
            lo = min(lo, v)
            normalized_model_response[i] = lo
        else:
            hi = max(hi, v)
            normalized_model_response[i] = hi
    original_MR = normalized_model_response.copy()
    normalized_model_response = normalize_curve(normalized_model_response, type)
    best_segment_list = torch.flip(worst_segment_list, (0,)) if type == 0 else worst_segment_list
    new_map = torch.zeros((img_hw, img_hw))
    for i in range(1, n_steps + 1):                                               # :297-304
        segment_coords = torch.where(segments.flatten() == best_segment_list[i - 1])[0]
        if type == 0:
            target_MR = normalized_model_response[i - 1] - normalized_model_response[i]
        else:
            target_MR = normalized_model_response[i] - normalized_model_response[i - 1]
        new_map.reshape(img_hw ** 2)[segment_coords] = (torch.ones(len(segment_coords)) / len(segment_coords)) * target_MR
    new_map = new_map.unsqueeze(2) * torch.ones((img_hw, img_hw, 3))
    small_side = int(np.ceil(np.sqrt(n_steps)))
    small = resize(resize(new_map.permute((2, 0, 1)), small_side), img_hw).permute((1, 2, 0))
    return new_map.cpu().numpy(), small.cpu().numpy(), best_segment_list, original_MR


def find_deletion_patches(input_tensor, segments, saliency_map_segmented, beginning_order, blur, n_searches, model, device, img_hw,
                          max_batch_size=25, kappa=0.005, test_kappa=False, CLIP_test_info=None, *, pass_rows=None, metric=None,
                          resize=resize_antialias, log=None):
    """:313-597"""
    n_steps, batch_size = _check(segments, n_searches, max_batch_size)
    target_class, original_pred = _pred(model, input_tensor, device)
    start = torch.zeros_like(input_tensor)
    finish = input_tensor.clone()
    _, black_pred = _pred(model, start, device, target_class)
    segment_order = segment_order_of(saliency_map_segmented, segments, n_steps, img_hw, descending=False)
    worst_segment_list = torch.full((1, n_steps), -1).squeeze()
    worst_MR_list = torch.zeros((1, n_steps)).squeeze()
    input_length = len(beginning_order)                                           # :362-363
    worst_segment_list[len(worst_segment_list) - input_length: len(worst_segment_list)] = torch.flip(beginning_order, (0,))
    plan = reference_step_plan(n_steps, n_searches, input_length, False)
    _search(model, device, start, finish, segments, segment_order, worst_segment_list, worst_MR_list, plan, 0, target_class,
            pass_rows, batch_size, img_hw, None, log)
    C = start.shape[1]
    n = len(worst_segment_list)
    tail = []
    for step in range(n - input_length, n):                                       # :497-499
        segment_coords = torch.where(segments.flatten() == worst_segment_list[step])[0]
        start.reshape(C, img_hw ** 2)[:, segment_coords] = finish.reshape(C, img_hw ** 2)[:, segment_coords]
        tail.append(start.clone())
    rows = 1 if pass_rows is None else pass_rows
    with torch.no_grad():
        for lo in range(0, input_length, rows):                                   # :502-506
            output = model(torch.cat(tail[lo:lo + rows]).to(device)).detach()
            got = nn.functional.softmax(output, dim=1)[:, target_class].cpu()
            worst_MR_list[n - input_length + lo: n - input_length + lo + len(got)] = got
    normalized_model_response = torch.cat((worst_MR_list, torch.tensor([original_pred]))).detach().cpu().numpy().copy().astype(np.double)
    normalized_model_response = normalized_model_response[::-1]                   # :514-516
    raw_deletion = normalized_model_response.copy()
    lo_ = 1.0
    for i in range(n_steps + 1):                                                  # :520-524
        v = np.clip((normalized_model_response[i] - black_pred) / (abs(original_pred - black_pred)), 0.0, 1.0)
        lo_ = min(lo_, v)
        normalized_model_response[i] = lo_
    monotone = normalized_model_response.copy()
    normalized_model_response = normalize_curve(normalized_model_response, type=0)
    best_segment_list = torch.flip(worst_segment_list, (0,))                      # :530
    new_map = torch.zeros((img_hw, img_hw))
    for i in range(1, n_steps + 1):                                               # :534-537
        segment_coords = torch.where(segments.flatten() == best_segment_list[i - 1])[0]
        target_MR = normalized_model_response[i - 1] - normalized_model_response[i]
        new_map.reshape(img_hw ** 2)[segment_coords] = (torch.ones(len(segment_coords)) / len(segment_coords)) * target_MR \
            + (target_MR * (n_steps - i) / n_steps)
    new_map = new_map.unsqueeze(2) * torch.ones((img_hw, img_hw, 3))
    new_map_test = np.abs(np.sum(new_map.cpu().numpy(), axis=2))                  # :543
    metric = metric if metric is not None else oracle_metric(model, img_hw)
    raw_score_ins = metric("ins", blur, input_tensor, new_map_test, device, max_batch_size)              # :546
    raw_score_del = metric("del", torch.zeros_like, input_tensor, new_map_test, device, max_batch_size)  # :547
    x_old = np.linspace(0, 100, len(raw_score_ins))                               # :553-561
    x_new = np.linspace(0, 100, n_steps + 1)
    raw_score_ins = np.interp(x_new, x_old, raw_score_ins)
    raw_score_del = np.interp(x_new, x_old, raw_score_del)
    new_curve = np.mean([raw_score_ins, 1 - raw_score_del], axis=0)
    new_curve = 1 - new_curve
    normalized_model_response = normalize_curve(new_curve, type=0)
    if log is not None:
        log.update(raw_deletion=raw_deletion, monotone=monotone, final_curve=normalized_model_response.copy())
    new_map_sparse = torch.zeros((img_hw, img_hw))
    new_map_dense = torch.zeros((img_hw, img_hw))
    ones_map = torch.ones((img_hw, img_hw))
    if test_kappa:                                                                # :568-569
        return new_map_dense, segments, best_segment_list, normalized_model_response, ones_map, n_steps + 1
    for i in range(1, n_steps + 1):                                               # :571-581
        segment_coords = torch.where(segments.flatten() == best_segment_list[i - 1])[0]
        target_MR = normalized_model_response[i - 1] - normalized_model_response[i]
        attr_value = 1 / len(segment_coords) * target_MR + (target_MR * (n_steps - i) / n_steps)
        new_map_sparse.reshape(img_hw ** 2)[segment_coords] = ones_map.reshape(img_hw ** 2)[segment_coords] * attr_value
        if attr_value >= kappa:
            new_map_dense.reshape(img_hw ** 2)[segment_coords] = ones_map.reshape(img_hw ** 2)[segment_coords] * ((n_steps - i) / n_steps)
        else:
            new_map_dense.reshape(img_hw ** 2)[segment_coords] = ones_map.reshape(img_hw ** 2)[segment_coords] * attr_value
    new_map_dense = new_map_dense / new_map_dense.max() * new_map_sparse.max()    # :584
    ones3 = torch.ones((img_hw, img_hw, 3))
    maps = []
    for w in (0, 0.5, 1):                                                         # :586-591
        maps.append((((1 - w) * new_map_sparse) + ((w) * new_map_dense)).unsqueeze(2) * ones3)
    small_side = int(np.ceil(np.sqrt(n_steps)))
    out = []
    for m in maps:                                                                # :597
        out.append(m.cpu().numpy())
        out.append(resize(resize(m.permute((2, 0, 1)), small_side), img_hw).permute((1, 2, 0)).cpu().numpy())
    return (*out, best_segment_list)


def segment_saliency_map(saliency_map, patch_count, img_hw):
    """:607-609: the attribution down to the patch grid (antialiased bilinear) and back up (nearest-exact)"""
    x = torch.tensor(saliency_map, dtype=torch.float).permute((2, 0, 1))
    down = resize_antialias(x, int(patch_count ** (1 / 2)))
    return F.interpolate(down[None], size=(img_hw, img_hw), mode="nearest-exact")[0].permute((1, 2, 0))


def end_index_of(MR_ins):
    """:614-617"""
    try:
        return int(np.where(np.asarray(MR_ins) >= 0.9)[0][0])
    except IndexError:
        return len(MR_ins)


def MDA(trans_img, input_tensor, saliency_map, patch_count, blur, model, device, img_hw, max_batch_size=5, ordered=False,
        CLIP_test_info=None, vis=False, *, segments, pass_rows=None, metric=None, resize=resize_antialias, log=None):
    """:600-626 with the label map given (`slic` stays skimage's)"""
    segments = torch.as_tensor(segments).to(int)
    saliency_map_segmented = segment_saliency_map(saliency_map, patch_count, img_hw)
    ins_log = None if log is None else dict(winner_margin=[], stop_margin=[], slots=[])
    del_log = None if log is None else dict(winner_margin=[], stop_margin=[], slots=[])
    _, _, order_a, MR_ins = find_insertion_patches(input_tensor.cpu(), saliency_map_segmented, segments, blur, patch_count, type=1,
                                                   model=model, device=device, img_hw=img_hw, max_batch_size=max_batch_size,
                                                   pass_rows=pass_rows, resize=resize, log=ins_log)
    end_index = end_index_of(MR_ins)
    res = find_deletion_patches(input_tensor.cpu(), segments, saliency_map_segmented, order_a[0: end_index + 1], blur, patch_count,
                                model, device, img_hw, max_batch_size=max_batch_size, kappa=(-1 if ordered else 0.005),
                                pass_rows=pass_rows, metric=metric, resize=resize, log=del_log)
    if log is not None:
        log.update(order_a=order_a, MR_ins=MR_ins, end_index=end_index, insertion=ins_log, deletion=del_log, best_segment_list=res[6])
    MGA_g_0, MGA_g_0_s, MGA_g_5, MGA_g_5_s, MGA_g_10, MGA_g_10_s, _ = res
    if vis is False:
        return MGA_g_0, MGA_g_0_s, MGA_g_10
    return MGA_g_0, MGA_g_0_s, MGA_g_5, MGA_g_5_s, MGA_g_10, MGA_g_10_s


# ------------------------------------------------------------------------------------------------ seeded inputs
class SmallNet(nn.Module):
    """Conv(3, 6, 5, stride 4) -> ReLU -> AdaptiveAvgPool(7) -> Linear(294, 10), seeded, a few milliseconds per pass of 8 images at
    224 x 224 on a CPU.  Class 0 reads every pooled cell with a weight of one sign and similar size, the other classes almost
    nothing: every patch of the input moves the class-0 margin by a similar amount in the same direction, so the response of a
    search moves patch by patch instead of jumping with the first one."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(int(seed))
        self.conv = nn.Conv2d(3, 6, 5, stride=4)
        self.fc = nn.Linear(6 * 49, 10)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.3)
            self.conv.bias.copy_(torch.randn(6, generator=g) * 0.1)
            self.fc.weight.copy_(torch.randn(self.fc.weight.shape, generator=g) * 0.002)
            self.fc.bias.copy_(torch.randn(10, generator=g) * 0.01)
            self.fc.weight[0] = (1.0 + 0.5 * torch.rand(294, generator=g)) / 294
            self.fc.bias[0] = 0.0
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, x):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(torch.relu(self.conv(x)), 7), 1))


def calibrate(model, x, blurred, d_orig, spread):
    """Rescale the last layer so that the margin of the input's top class over its runner-up differs by `spread` between the
    input and its blur, then shift that class's bias so that the margin at the input is `d_orig` (> 0: it stays the top class).
    A small d_orig with a large spread gives a response that rises late (a stop in the second phase); a seed whose blur scores
    the class higher than the input never stops."""
    def margin(logits, t):
        rest = torch.cat([logits[:t], logits[t + 1:]])
        return float(logits[t] - rest.max())
    with torch.no_grad():
        lo, lb = model(x)[0], model(blurred)[0]
        t = int(torch.argmax(lo))
        g = spread / abs(margin(lo, t) - margin(lb, t))
        model.fc.weight.mul_(g)
        model.fc.bias.mul_(g)
        model.fc.bias[t] += d_orig - margin(model(x)[0], t)
    return model


def grid_labels(img_hw, n):
    """n x n regular grid, labels row-major from 0"""
    cell = -(-img_hw // n)
    r = torch.arange(img_hw) // cell
    return (r[:, None] * n + r[None, :]).to(int)


def voronoi_labels(img_hw, n_cells, seed):
    """Voronoi cells of seeded points, labels 0 .. n_cells-1 without gaps (a point whose cell is empty is drawn again)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:img_hw, 0:img_hw]
    while True:
        pts = rng.uniform(0, img_hw, (n_cells, 2))
        lab = np.argmin((yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2, axis=2)
        if len(np.unique(lab)) == n_cells:
            return torch.from_numpy(lab).to(int)


def amplify(gain):
    """a substrate that is no blur: the input times `gain`.  The classifier scores it HIGHER than the input, so the insertion
    search's stop test never holds (its ratio is negative throughout, -1 at the last step)"""
    return lambda x: x * gain


def box_blur(k):
    """a cheap stand-in for the harness's Gaussian: a k x k mean, zero-padded, channel by channel"""
    def blur(x):
        C = x.shape[1]
        w = torch.full((C, 1, k, k), 1.0 / (k * k), dtype=x.dtype, device=x.device)
        return F.conv2d(x, w, padding=k // 2, groups=C)
    return blur


# tag: (img_hw, segments ("grid", n) or ("voronoi", S, seed), model seed, image seed, d_orig, spread, substrate, ordered); the seeds come
# from tests/golden/make_golden_mda.py's search for well-conditioned cases of each kind
CASES = {
    "grid16_p1": (224, ("grid", 4), 2, 7, 12.0, 12.0, "blur", False),           # S = 16, a regular 4 x 4 grid; stops in phase 1
    "vor17_p2": (224, ("voronoi", 17, 5), 5, 7, 3.0, 5.0, "blur", False),       # S = 17 irregular, L = 8 < S; stops in phase 2: the wrong slot
    "vor17_p1": (224, ("voronoi", 17, 5), 2, 7, 12.0, 12.0, "blur", False),     # stops in phase 1
    "vor17_never": (224, ("voronoi", 17, 5), 2, 7, 0.5, 2.0, "amplify", False),   # the substrate scores higher than the input: never stops
    "grid16_never": (224, ("grid", 4), 2, 7, 0.5, 2.0, "amplify", False),
    "grid16_ordered": (224, ("grid", 4), 5, 8, 3.5, 6.0, "blur", True),         # ordered=True (kappa = -1), a phase-2 stop on the grid
}


def seeded_case(tag):
    """-> dict(img_hw, segments, model, input_tensor, trans_img, saliency_map, blur, patch_count, ordered)"""
    return build_case(*CASES[tag])


def build_case(img_hw, seg, model_seed, image_seed, d_orig, spread, substrate="blur", ordered=False):
    segments = grid_labels(img_hw, seg[1]) if seg[0] == "grid" else voronoi_labels(img_hw, seg[1], seg[2])
    S = int(segments.max()) + 1
    g = torch.Generator().manual_seed(int(image_seed))
    coarse = torch.rand((1, 3, 8, 8), generator=g)
    trans_img = 0.5 * F.interpolate(coarse, size=(img_hw, img_hw), mode="bilinear", align_corners=False) \
        + 0.5 * torch.rand((1, 3, img_hw, img_hw), generator=g)
    input_tensor = (trans_img - 0.5) / 0.25
    # a smooth positive attribution: segment means without ties
    sal = F.interpolate(torch.rand((1, 1, 9, 9), generator=g), size=(img_hw, img_hw), mode="bicubic", align_corners=False)[0, 0]
    saliency_map = (sal.abs()[:, :, None] * torch.ones(3)).numpy().astype(np.float32)
    blur = amplify(1.5) if substrate == "amplify" else box_blur(31 if img_hw >= 64 else 7)
    model = calibrate(SmallNet(model_seed).eval(), input_tensor, blur(input_tensor), d_orig, spread)
    return dict(img_hw=img_hw, segments=segments, model=model, input_tensor=input_tensor, trans_img=trans_img,
                saliency_map=saliency_map, blur=blur, patch_count=S, ordered=ordered)
