"""Torch-tensor front end of the C ABI (include/xai_hip.h and the extension headers beside it): shape/device checks, output
allocation, stream plumbing.  Every function launches asynchronously on torch's current
stream of the tensors' device and returns device tensors; nothing here computes on the CPU.
Every launch goes through `_call(name, dev, *args, lib=<key of _lib.LIBRARIES>)`.
"""
import math

import torch

from . import _lib

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
F16 = torch.float16


def _typed(t, dtype, name):
    """The half of _need that asks no device: a tensor of `dtype` (a tuple: one of them).  On its own in the wrappers that report
    the device last, after every refusal a host can test (shape, limits); _need follows there."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
        raise TypeError(f"{name}: expected {' or '.join(map(str, dtype)) if isinstance(dtype, tuple) else dtype}, got {t.dtype}")
    return t


def _need(t, dtype, name, rows=False):
    """The shared argument check: a tensor, on a HIP device, of `dtype` (a tuple: one of them), contiguous (rows: in its last
    axis, the other strides are passed on)."""
    if isinstance(t, torch.Tensor) and not t.is_cuda:
        raise _lib.XaiHipError(f"{name} lives on '{t.device}': the xai_engine kernels run on a HIP device only "
                               "(pass device='cuda:N'); there is no CPU fallback")
    _typed(t, dtype, name)
    if rows:
        if t.dim() < 1 or (t.shape[-1] > 1 and t.stride(-1) != 1):
            raise ValueError(f"{name} must be contiguous in its last axis")
    elif not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _call(name, dev, *args, lib="hip"):
    """Launch entry `name` of library `lib` (a key of _lib.LIBRARIES) on torch's current stream of `dev`; the
    error texts of every library are the main one's xai_strerror."""
    handle = _lib.load(lib)
    with torch.cuda.device(dev):
        _lib.check(getattr(handle, name)(*args, _stream(dev)), name)


def _base_args(baseline, like, name="baseline"):
    """tensor baseline -> (ptr, 0.0); python scalar -> (None, value)."""
    if isinstance(baseline, torch.Tensor):
        _need(baseline, F32, name)
        if baseline.numel() != like.numel():
            raise ValueError(f"{name} has {baseline.numel()} elements, expected {like.numel()}")
        return baseline, 0.0
    return None, float(baseline)


def _out(t, name, shape, like, wrong=None, dtype=F32, alloc=torch.empty):
    """The caller's buffer `t` once it passed _need and holds as many elements as `shape` (else ValueError(wrong)); for None a new
    tensor from `alloc` on the device of `like` (alloc None: an optional output, None stays None)."""
    if t is None:
        return None if alloc is None else alloc(tuple(shape), dtype=dtype, device=like.device)
    _need(t, dtype, name)
    if t.numel() != math.prod(shape):
        raise ValueError(wrong or f"{name} has the wrong size")
    return t


def _workspace(entry, dev, *extents, lib="hip", required=False, ws=None, wrong=None):
    """-> (uint8 device scratch of `entry`(*extents) bytes, or None for 0 bytes; the byte count).  `entry` is a *_workspace_bytes
    of library `lib`; required: 0 bytes there means the extents are refused, not that no scratch is needed.  `ws`: the caller's
    scratch instead of a new one, uint8 on `dev` and at least that long, else ValueError(wrong)."""
    nbytes = int(getattr(_lib.load(lib), entry)(*extents))
    if ws is not None:
        _need(ws, U8, "ws")
        if ws.device != dev or ws.numel() < nbytes:
            raise ValueError(wrong)
        return ws, nbytes
    if required and nbytes <= 0:
        raise ValueError(f"{entry}{extents}: no such workspace (an extent is not positive, or too large)")
    return (torch.empty(nbytes, dtype=U8, device=dev) if nbytes else None), nbytes


def _shaped_like(t, like, name, like_name, dtype=F32):
    """An operand (None: absent) that must have the shape of `like`."""
    if t is not None:
        _need(t, dtype, name)
        if t.shape != like.shape:
            raise ValueError(f"{name} must have the shape of {like_name}")


def _int(v, name, least=None):
    """A Python int (no bool, no float), at least `least`"""
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name}: expected an int, got {type(v).__name__}")
    if least is not None and v < least:
        raise ValueError(f"{name} must be >= {least}, got {v}")
    return v


def _suffix(t):
    """The ending of the entry of t's dtype, in the libraries that have one entry per dtype"""
    return {F16: "f16", F32: "f32", F64: "f64"}[t.dtype]


def _bhwc(t, dtype, name):
    """t (B, H, W, C) of `dtype` with at least one element -> (B, H, W, C) as ints.  The front half of a segmenter's image check:
    its own limits come next, then _need for the device and the contiguity."""
    _typed(t, dtype, name)
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError(f"{name} must be (B, H, W, C) with at least one element, got {tuple(t.shape)}")
    return tuple(int(v) for v in t.shape)


def _status(lib, status, n=None, dev=None, count=None):
    """The int32 status words of library `lib`.  None: `n` new ones on `dev`, cleared by the library's xai_<lib>_clear_i32.  A
    caller's: with `n`, exactly n of them on `dev`, returned as they are; without, at least one, cleared."""
    if status is None:
        status = torch.empty(n, dtype=I32, device=dev)
    else:
        _need(status, I32, "status")
        if n is not None:
            if status.numel() != n or status.device != dev:
                raise ValueError(f"status must hold {count or n} int32 on the device of its images")
            return status
        if status.numel() < 1:
            raise ValueError("status must hold at least one int32")
    _call(f"xai_{lib}_clear_i32", status.device, _ptr(status), status.numel(), lib=lib)
    return status


# ------------------------------------------------------------------------------ IG
def ig_interp(x, baseline, alphas, out=None):
    """x: (n_img, *img) ; alphas: (n_alpha,) shared or (n_img, n_alpha) -> (n_img, n_alpha, *img)."""
    _need(x, F32, "x"); _need(alphas, F32, "alphas")
    n_img = x.shape[0]
    n_elem = x[0].numel()
    if alphas.dim() == 1:
        n_alpha, stride = alphas.shape[0], 0
    else:
        if alphas.shape[0] != n_img:
            raise ValueError("alphas must be (n_alpha,) or (n_img, n_alpha)")
        n_alpha, stride = alphas.shape[1], alphas.shape[1]
    b, bs = _base_args(baseline, x)
    out = _out(out, "out", (n_img, n_alpha) + tuple(x.shape[1:]), x)
    _call("xai_ig_interp_f32", x.device, _ptr(x), _ptr(b), bs, _ptr(alphas), stride, n_img, n_alpha, n_elem, _ptr(out))
    return out


def ig_cutoff(logits, alpha_star):
    """logits (n_img, n_steps) -> int32 (n_img,) number of leading steps Left-IG averages."""
    _need(logits, F32, "logits")
    n_img, n_steps = logits.shape
    n_use = torch.empty(n_img, dtype=I32, device=logits.device)
    _call("xai_ig_cutoff_f32", logits.device, _ptr(logits), n_img, n_steps, float(alpha_star), _ptr(n_use))
    return n_use


def ig_accum(grads, x, baseline, n_use=None, w1=None, w2=None, want_abs=False, timing_events=None):
    """grads (n_img, n_steps, C, H, W); x (n_img, C, H, W) -> out (n_img, C, H, W)[, abs (n_img, H, W)].
    n_use: None (all steps), int, or int32 device tensor (n_img,).
    timing_events: optional (start, stop) pair of torch.cuda.Event(enable_timing=True): the kernel's own start / stop
    timestamps are recorded into them by the dispatch (xai_ig_accum_timed_f32), start.elapsed_time(stop) is the kernel time."""
    _need(grads, F32, "grads"); _need(x, F32, "x")
    n_img, n_steps, Cc = grads.shape[0], grads.shape[1], grads.shape[2]
    hw = grads[0, 0, 0].numel()
    if x.numel() != n_img * Cc * hw:
        raise ValueError("x does not match grads")
    b, bs = _base_args(baseline, x)
    n_dev, n_host = None, n_steps
    if isinstance(n_use, torch.Tensor):
        n_dev = _need(n_use, I32, "n_use")
        if n_dev.numel() != n_img:
            raise ValueError("n_use tensor must have one entry per image")
    elif n_use is not None:
        n_host = int(n_use)
    for w, nm in ((w1, "w1"), (w2, "w2")):
        if w is not None:
            _need(w, F32, nm)
            if w.numel() != n_img * n_steps:
                raise ValueError(f"{nm} must be (n_img, n_steps)")
    out = torch.empty((n_img,) + tuple(grads.shape[2:]), dtype=F32, device=x.device)
    out_abs = torch.empty((n_img,) + tuple(grads.shape[3:]), dtype=F32, device=x.device) if want_abs else None
    if timing_events is None:
        _call("xai_ig_accum_f32", x.device, _ptr(grads), n_img, n_steps, _ptr(n_dev), n_host, _ptr(w1), _ptr(w2), _ptr(x), _ptr(b), bs,
              Cc, hw, _ptr(out), _ptr(out_abs))
    else:
        e0, e1 = timing_events
        stream = torch.cuda.current_stream(x.device)
        for e in (e0, e1):                         # torch creates the hipEvent_t on the first record; the dispatch re-records it
            e.record(stream)
        _call("xai_ig_accum_timed_f32", x.device, _ptr(grads), n_img, n_steps, _ptr(n_dev), n_host, _ptr(w1), _ptr(w2), _ptr(x), _ptr(b),
              bs, Cc, hw, _ptr(out), _ptr(out_abs), e0.cuda_event, e1.cuda_event)
    return (out, out_abs) if want_abs else out


def store_grads(src, dst):
    """dst <- src (same element count, both contiguous) with streaming non-temporal stores."""
    _need(src, F32, "src"); _need(dst, F32, "dst")
    if src.numel() != dst.numel():
        raise ValueError("src and dst differ in size")
    _call("xai_ig_store_grads_f32", dst.device, _ptr(src), _ptr(dst), src.numel())
    return dst


def ig_accum_add(grads, acc):
    """acc (N elems) += sum over rows of grads (n_batch, N elems)."""
    _need(grads, F32, "grads"); _need(acc, F32, "acc")
    n_batch = grads.shape[0]
    if grads[0].numel() != acc.numel():
        raise ValueError("acc does not match one row of grads")
    _call("xai_ig_accum_add_f32", acc.device, _ptr(grads), n_batch, _ptr(acc), acc.numel())
    return acc


def ig_finish(acc, n_steps, x, baseline, want_abs=False):
    """acc, x: (n_img, C, H, W) -> acc / n_steps * (x - baseline)."""
    _need(acc, F32, "acc"); _need(x, F32, "x")
    n_img, Cc = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()
    b, bs = _base_args(baseline, x)
    out = torch.empty_like(x)
    out_abs = torch.empty((n_img,) + tuple(x.shape[2:]), dtype=F32, device=x.device) if want_abs else None
    _call("xai_ig_finish_f32", x.device, _ptr(acc), n_img, int(n_steps), _ptr(x), _ptr(b), bs, Cc, hw, _ptr(out), _ptr(out_abs))
    return (out, out_abs) if want_abs else out


def sumsq(rows):
    """(n_rows, ...) -> (n_rows,) sum of squares per row."""
    _need(rows, F32, "rows")
    out = torch.empty(rows.shape[0], dtype=F32, device=rows.device)
    _call("xai_sumsq_f32", rows.device, _ptr(rows), rows.shape[0], rows[0].numel(), _ptr(out))
    return out


def idgi_accum(grads, logits, sq):
    """grads (n_steps, *img), logits (n_steps,), sq (n_steps,) -> (*img)."""
    _need(grads, F32, "grads"); _need(logits, F32, "logits"); _need(sq, F32, "sumsq")
    out = torch.empty(tuple(grads.shape[1:]), dtype=F32, device=grads.device)
    _call("xai_idgi_accum_f32", grads.device, _ptr(grads), grads.shape[0], _ptr(logits), _ptr(sq), grads[0].numel(), _ptr(out))
    return out


# ------------------------------------------------------------------------------ Grad-CAM
def gradcam(act, grad, relu=True):
    """(B,C,h,w) x2 -> (B,h,w)."""
    _need(act, F32, "act"); _need(grad, F32, "grad")
    if act.shape != grad.shape or act.dim() != 4:
        raise ValueError("act and grad must both be (B,C,h,w)")
    B, Cc, h, w = act.shape
    cam = torch.empty((B, h, w), dtype=F32, device=act.device)
    ws, nbytes = _workspace("xai_gradcam_workspace_bytes", act.device, B, Cc, h, w)
    _call("xai_gradcam_f32", act.device, _ptr(act), _ptr(grad), B, Cc, h, w, int(bool(relu)), _ptr(cam), _ptr(ws), nbytes)
    return cam


def bilinear_up(src, H, W, scale=1.0, take_abs=False):
    """(B,h,w) -> (B,H,W), align_corners=False.  Plain two-tap bilinear on both axes: equal to the reference's antialiased
    resize (torchvision Resize(antialias=True)) only when no axis shrinks -- `resize_bilinear` is the call that follows the
    reference either way."""
    _need(src, F32, "src")
    B, h, w = src.shape
    dst = torch.empty((B, H, W), dtype=F32, device=src.device)
    _call("xai_bilinear_up_f32", src.device, _ptr(src), B, h, w, int(H), int(W), float(scale), int(bool(take_abs)), _ptr(dst))
    return dst


def resize_bilinear(src, H, W, scale=1.0, take_abs=False):
    """The reference's `Resize((H, W), antialias=True)` of (B,h,w) maps, times `scale`, optionally |.|: K3's `bilinear_up` while no
    axis shrinks (there the antialias filter is the two bilinear taps); with a shrinking axis the filter widens, and the map is
    torch's antialiased interpolation on the device.  A torch build without that op on the device is an error, never the plain
    bilinear."""
    _need(src, F32, "src")
    B, h, w = src.shape
    H, W = int(H), int(W)
    if H >= h and W >= w:
        return bilinear_up(src, H, W, scale=scale, take_abs=take_abs)
    try:
        out = torch.nn.functional.interpolate(src[:, None], size=(H, W), mode="bilinear", align_corners=False, antialias=True)[:, 0]
    except (RuntimeError, NotImplementedError) as e:
        raise _lib.XaiHipError(f"resize_bilinear: ({h}, {w}) -> ({H}, {W}) shrinks an axis, which needs the antialiased bilinear "
                               f"interpolation, and this torch build has none for {src.device}: {e}") from e
    out = out * float(scale)
    return out.abs() if take_abs else out


# ------------------------------------------------------------------------------ RISE
def rise_apply(grid, shift, cell, image, want_masked=True, want_masks=False, out=None):
    """grid (n,s,s) uint8, shift (n,2) int32, image (C,H,W) -> masked (n,C,H,W) and/or masks (n,H,W)."""
    _need(grid, torch.uint8, "grid"); _need(shift, I32, "shift"); _need(image, F32, "image")
    n, s = grid.shape[0], grid.shape[1]
    Cc, H, W = image.shape
    masked = _out(out, "out", (n, Cc, H, W), image) if want_masked else None
    masks = torch.empty((n, H, W), dtype=F32, device=image.device) if want_masks else None
    _call("xai_rise_apply_f32", image.device, _ptr(grid), _ptr(shift), n, s, int(cell[0]), int(cell[1]), _ptr(image), Cc, H, W,
          _ptr(masked), _ptr(masks))
    if want_masked and want_masks:
        return masked, masks
    return masked if want_masked else masks


def rise_accum(grid, shift, scores, cell, H, W, scale, acc=None):
    """acc (H,W) float64 += scale * sum_n scores[n] * mask_n."""
    _need(grid, torch.uint8, "grid"); _need(shift, I32, "shift"); _need(scores, F32, "scores")
    n, s = grid.shape[0], grid.shape[1]
    if scores.numel() != n:
        raise ValueError("one score per mask")
    acc = _out(acc, "acc", (H, W), grid, dtype=F64, alloc=torch.zeros)
    _call("xai_rise_accum_f64", grid.device, _ptr(grid), _ptr(shift), _ptr(scores), n, s, int(cell[0]), int(cell[1]), int(H), int(W),
          float(scale), _ptr(acc))
    return acc


# ------------------------------------------------------------------------------ ins/del
def rank(sal):
    """sal (n_seg, hw) -> (order, rank) int32: stable ascending argsort and its inverse."""
    _need(sal, F32, "sal")
    n_seg, hw = sal.shape
    ws, nbytes = _workspace("xai_rank_workspace_bytes", sal.device, n_seg, hw)
    order = torch.empty((n_seg, hw), dtype=I32, device=sal.device)
    rk = torch.empty((n_seg, hw), dtype=I32, device=sal.device)
    _call("xai_rank_f32", sal.device, _ptr(sal), n_seg, hw, _ptr(order), _ptr(rk), _ptr(ws), nbytes)
    return order, rk


def flip_steps(rk, descending, step_size):
    """rank (hw,) int32 -> flip step per pixel (hw,) int32."""
    _need(rk, I32, "rank")
    out = torch.empty_like(rk)
    _call("xai_flip_steps_i32", rk.device, _ptr(rk), rk.numel(), int(bool(descending)), int(step_size), _ptr(out))
    return out


def perturb_batch(start, finish, flip, first_step, n_batch, out=None):
    """start, finish (C,H,W); flip (H*W,) int32 -> (n_batch, C, H, W)."""
    _need(start, F32, "start"); _need(finish, F32, "finish"); _need(flip, I32, "flip_step")
    Cc = start.shape[0]
    hw = start[0].numel()
    if finish.shape != start.shape or flip.numel() != hw:
        raise ValueError("start/finish/flip_step shapes disagree")
    out = _out(out, "out", (n_batch,) + tuple(start.shape), start)
    _call("xai_perturb_batch_f32", start.device, _ptr(start), _ptr(finish), _ptr(flip), Cc, hw, int(first_step), int(n_batch), _ptr(out))
    return out


def segment_sums(sal, order, descending, step_size, n_steps):
    """-> (seg (n_steps,), total (1,)) float32."""
    _need(sal, F32, "sal"); _need(order, I32, "order")
    seg = torch.empty(n_steps, dtype=F32, device=sal.device)
    total = torch.empty(1, dtype=F32, device=sal.device)
    _call("xai_segment_sums_f32", sal.device, _ptr(sal), _ptr(order), sal.numel(), int(bool(descending)), int(step_size), int(n_steps),
          _ptr(seg), _ptr(total))
    return seg, total


def blur_sep(x, k1d):
    """x (B,C,H,W), k1d (klen,) on device -> zero-padded separable blur.  Up to 63 taps both passes run in
    one launch (tile + halo in LDS); longer kernels take two 1-D passes through a scratch tensor."""
    _need(x, F32, "x"); _need(k1d, F32, "k1d")
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    klen = k1d.numel()
    if klen <= 63:
        _call("xai_blur_sep_f32", x.device, _ptr(x), _ptr(k1d), klen, B, Cc, H, W, _ptr(out))
    else:
        tmp = torch.empty_like(x)
        _call("xai_blur_1d_f32", x.device, _ptr(x), _ptr(k1d), klen, 1, B, Cc, H, W, _ptr(tmp))
        _call("xai_blur_1d_f32", x.device, _ptr(tmp), _ptr(k1d), klen, 0, B, Cc, H, W, _ptr(out))
    return out


def softmax_stats(logits, target=None, want_entropy=True, want_argmax=True, out=None, offset=0):
    """logits (B,K); target: None (row argmax), int, or int32 device tensor (1,).
    -> (p_target (B,), entropy_bits (B,) or None, argmax (B,) int32 or None).
    `out=(p, entropy, argmax)` (1-D fp32/fp32/int32 device tensors) writes rows [offset, offset+B) of
    preallocated curves instead of allocating (the ins/del loop fills its curves in place)."""
    _need(logits, F32, "logits")
    B, K = logits.shape
    t_dev, t_host = None, -1
    if isinstance(target, torch.Tensor):
        t_dev = _need(target, I32, "target")
    elif target is not None:
        t_host = int(target)
    if out is None:
        p = torch.empty(B, dtype=F32, device=logits.device)
        ent = torch.empty(B, dtype=F32, device=logits.device) if want_entropy else None
        am = torch.empty(B, dtype=I32, device=logits.device) if want_argmax else None
    else:
        p, ent, am = out
        _need(p, F32, "out p")
        if ent is not None:
            _need(ent, F32, "out entropy")
        if am is not None:
            _need(am, I32, "out argmax")
        for t in (p, ent, am):
            if t is not None and (t.dim() != 1 or offset < 0 or offset + B > t.numel()):
                raise ValueError("out tensors must be 1-D with room for rows [offset, offset+B)")
        p, ent, am = p[offset:offset + B], (None if ent is None else ent[offset:offset + B]), (None if am is None else am[offset:offset + B])
    _call("xai_softmax_stats_f32", logits.device, _ptr(logits), B, K, _ptr(t_dev), t_host, _ptr(p), _ptr(ent), _ptr(am))
    return p, ent, am


# ------------------------------------------------------------------------------ feature-map maskers (ViT-CX)
def up_rownorm(src, H, W):
    """src (R,h,w) -> (R, H*W): bilinear up-sample (align_corners=False) and per-row min-max normalisation.
    H >= h and W >= w: the reference's Resize(antialias=True) is plain bilinear only when up-sampling, so a smaller target
    in either axis raises (XAI_E_UNSUPPORTED) instead of returning the un-filtered samples."""
    _need(src, F32, "src")
    R, h, w = src.shape
    out = torch.empty((R, int(H) * int(W)), dtype=F32, device=src.device)
    _call("xai_up_rownorm_f32", src.device, _ptr(src), R, h, w, int(H), int(W), _ptr(out))
    return out


def rownorm(x, out=None):
    """x (R,P) -> (x - rowmin) / (rowmax - rowmin); out may alias x."""
    _need(x, F32, "x")
    R, P = x.shape
    if out is None:
        out = torch.empty_like(x)
    else:
        _need(out, F32, "out")
        if out.shape != x.shape:
            raise ValueError("out must have the shape of x")
    _call("xai_rownorm_f32", x.device, _ptr(x), R, P, _ptr(out))
    return out


def cluster_sum(rows, members, offs):
    """rows (R,P); members (R,) int32 row ids grouped by cluster; offs (K+1,) int32 -> (K,P) ordered sums."""
    _need(rows, F32, "rows"); _need(members, I32, "members"); _need(offs, I32, "offs")
    R, P = rows.shape
    K_ = offs.numel() - 1
    if K_ < 1 or members.numel() > R * max(K_, 1) or members.dim() != 1 or offs.dim() != 1:
        raise ValueError("members must be 1-D and offs (K+1,) with K >= 1")
    out = torch.empty((K_, P), dtype=F32, device=rows.device)
    _call("xai_cluster_sum_f32", rows.device, _ptr(rows), _ptr(members), _ptr(offs), K_, P, _ptr(out))
    return out


def masked_sums(rows, weights):
    """rows (N,P), weights (N,) -> (sum_n w_n rows_n / N, sum_n rows_n / N), each (P,): one read of the stack."""
    _need(rows, F32, "rows"); _need(weights, F32, "weights")
    N, P = rows.shape
    if weights.numel() != N:
        raise ValueError("one weight per row")
    weighted = torch.empty(P, dtype=F32, device=rows.device)
    plain = torch.empty(P, dtype=F32, device=rows.device)
    _call("xai_masked_sums_f32", rows.device, _ptr(rows), _ptr(weights), N, P, _ptr(weighted), _ptr(plain))
    return weighted, plain


def causal_apply(x, masks, noise, noise_scale=0.1):
    """x (C,H,W); masks (N,H*W); noise (N,C,H,W) standard normal -> (2N,C,H,W): masked+noise rows then image+noise rows."""
    _need(x, F32, "x"); _need(masks, F32, "masks"); _need(noise, F32, "noise")
    Cc, H, W = x.shape
    N = masks.shape[0]
    if masks.shape != (N, H * W) or noise.shape != (N, Cc, H, W):
        raise ValueError(f"masks must be ({N},{H * W}) and noise ({N},{Cc},{H},{W})")
    stack = torch.empty((2 * N, Cc, H, W), dtype=F32, device=x.device)
    _call("xai_causal_apply_f32", x.device, _ptr(x), _ptr(masks), _ptr(noise), N, Cc, H * W, float(noise_scale), _ptr(stack))
    return stack


# ------------------------------------------------------------------------------ opt-in classifier-side fusion
def _need_bn(weight, bias, mean, var, suffix=""):
    for name, t in (("weight", weight), ("bias", bias), ("mean", mean), ("var", var)):
        _need(t, F32, name + suffix)


def _bn2_fwd(bn2):
    """bn2 = (weight, bias, mean, var, eps) of the identity operand's own BatchNorm, or None -> the five ABI arguments"""
    if bn2 is None:
        return None, None, None, None, 0.0
    w2, b2, m2, v2, eps2 = bn2
    _need_bn(w2, b2, m2, v2, "2")
    return w2, b2, m2, v2, eps2


def _bn2_bwd(bn2, want_identity):
    """bn2 = (weight2, var2, eps2) or None -> (the three ABI arguments, want_identity): with bn2 g_identity is always wanted"""
    if bn2 is None:
        return None, None, 0.0, want_identity
    w2, v2, eps2 = bn2
    _need(w2, F32, "weight2"); _need(v2, F32, "var2")
    return w2, v2, eps2, True


def _pooled(H, W, kernel, stride, pad):
    return (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1


def bn_act_fwd(x, identity, weight, bias, mean, var, eps, variant, relu=True, bn2=None):
    """y = act(bn(x) [+ identity]) for eval-mode BatchNorm2d statistics; x (N,C,H,W) contiguous.
    bn2 = (weight, bias, mean, var, eps): the identity operand gets its own BatchNorm first (down-sample branch)."""
    _need(x, F32, "x")
    _need_bn(weight, bias, mean, var)
    _shaped_like(identity, x, "identity", "x")
    w2, b2, m2, v2, eps2 = _bn2_fwd(bn2)
    N, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    y = torch.empty_like(x)
    _call("xai_bn_act_fwd_f32", x.device, _ptr(x), _ptr(identity), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(var), float(eps),
          _ptr(w2), _ptr(b2), _ptr(m2), _ptr(v2), float(eps2), int(variant), int(bool(relu)), N, Cc, HW, _ptr(y))
    return y


def bn_relu_bwd(gy, y, weight, var, eps, variant, want_identity=False, gy2=None, bn2=None):
    """-> (gx, g_identity or None) for y = relu(bn(x) [+ identity]); the incoming gradient is gy (+ gy2).
    bn2 = (weight2, var2, eps2): g_identity is the gradient of the identity operand BEFORE its own BatchNorm."""
    _need(gy, F32, "gy"); _need(y, F32, "y"); _need(weight, F32, "weight"); _need(var, F32, "var")
    _shaped_like(gy2, gy, "gy2", "gy")
    w2, v2, eps2, want_identity = _bn2_bwd(bn2, want_identity)
    N, Cc = y.shape[0], y.shape[1]
    HW = y[0, 0].numel()
    gx = torch.empty_like(y)
    gid = torch.empty_like(y) if want_identity else None
    _call("xai_bn_relu_bwd_f32", y.device, _ptr(gy), _ptr(gy2), _ptr(y), _ptr(weight), _ptr(var), float(eps), _ptr(w2), _ptr(v2), float(eps2),
          int(variant), N, Cc, HW, _ptr(gx), _ptr(gid))
    return gx, gid


def maxpool_bwd(gy, indices, H, W, kernel, stride, pad):
    """gy, indices (N,C,PH,PW) (indices int64 from F.max_pool2d(..., return_indices=True)) -> gx (N,C,H,W)."""
    _need(gy, F32, "gy"); _need(indices, torch.int64, "indices")
    N, Cc, PH, PW = gy.shape
    gx = torch.empty((N, Cc, int(H), int(W)), dtype=F32, device=gy.device)
    _call("xai_maxpool_bwd_f32", gy.device, _ptr(gy), _ptr(indices), N * Cc, int(H), int(W), PH, PW, int(kernel), int(stride), int(pad), _ptr(gx))
    return gx


def bn_relu_maxpool_fwd(x, weight, bias, mean, var, eps, variant, kernel, stride, pad):
    """max_pool2d(relu(bn(x)), kernel, stride, pad) for inference; x (N,C,H,W) -> (N,C,PH,PW)."""
    _need(x, F32, "x")
    _need_bn(weight, bias, mean, var)
    N, Cc, H, W = x.shape
    PH, PW = _pooled(H, W, kernel, stride, pad)
    y = torch.empty((N, Cc, PH, PW), dtype=F32, device=x.device)
    _call("xai_bn_relu_maxpool_fwd_f32", x.device, _ptr(x), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(var), float(eps), int(variant),
          N, Cc, H, W, PH, PW, int(kernel), int(stride), int(pad), _ptr(y))
    return y


def bn_gate_mask_bytes(n):
    """Bytes of the 1-bit ReLU gate mask of an n-element activation (xai_bn_gate_mask_bytes)."""
    return int(_lib.load().xai_bn_gate_mask_bytes(int(n)))


def bn_relu_fwd_mask(x, identity, weight, bias, mean, var, eps, variant, bn2=None, mask=None):
    """-> (y, mask): y = relu(bn(x) [+ identity]) exactly as bn_act_fwd, plus the gate `y > 0` of every element as one bit in
    `mask` (uint8 storage of bn_gate_mask_bytes(x.numel()) bytes, allocated here unless given; every word is written) for
    bn_relu_bwd_mask.  The bit layout is private to the two kernels."""
    _need(x, F32, "x")
    _need_bn(weight, bias, mean, var)
    _shaped_like(identity, x, "identity", "x")
    w2, b2, m2, v2, eps2 = _bn2_fwd(bn2)
    N, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    need = bn_gate_mask_bytes(x.numel())
    if mask is None:
        mask = torch.empty(need, dtype=torch.uint8, device=x.device)
    else:
        _need(mask, torch.uint8, "mask")
        if mask.numel() < need:
            raise ValueError(f"mask has {mask.numel()} bytes, needs {need}")
    y = torch.empty_like(x)
    _call("xai_bn_relu_fwd_mask_f32", x.device, _ptr(x), _ptr(identity), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(var), float(eps),
          _ptr(w2), _ptr(b2), _ptr(m2), _ptr(v2), float(eps2), int(variant), N, Cc, HW, _ptr(y), _ptr(mask))
    return y, mask


def bn_relu_bwd_mask(gy, mask, weight, var, eps, variant, want_identity=False, gy2=None, bn2=None, guided=False):
    """bn_relu_bwd with the gate mask of bn_relu_fwd_mask in place of y; gy (N,C,H,W) gives the shape.
    guided: Guided Backprop's rule -- the summed gradient gy (+ gy2) goes through g <= 0 ? +0 : g before the gate."""
    _need(gy, F32, "gy"); _need(mask, torch.uint8, "mask"); _need(weight, F32, "weight"); _need(var, F32, "var")
    if gy.dim() < 3:
        raise ValueError("gy must be (N, C, ...)")
    if mask.numel() < bn_gate_mask_bytes(gy.numel()):
        raise ValueError(f"mask has {mask.numel()} bytes, needs {bn_gate_mask_bytes(gy.numel())}")
    _shaped_like(gy2, gy, "gy2", "gy")
    w2, v2, eps2, want_identity = _bn2_bwd(bn2, want_identity)
    N, Cc = gy.shape[0], gy.shape[1]
    HW = gy[0, 0].numel()
    gx = torch.empty_like(gy)
    gid = torch.empty_like(gy) if want_identity else None
    _call("xai_bn_relu_bwd_mask_guided_f32" if guided else "xai_bn_relu_bwd_mask_f32", gy.device, _ptr(gy), _ptr(gy2), _ptr(mask), _ptr(weight), _ptr(var), float(eps), _ptr(w2), _ptr(v2),
          float(eps2), int(variant), N, Cc, HW, _ptr(gx), _ptr(gid))
    return gx, gid


# ---- the same kernels on compact / channel-major operands (K62-K64, include/xai_hip_compact.h)
def _strided(n, stride):
    return (n - 1) // stride + 1


def stride_gather_cnhw(side, stride):
    """side (N,C,H,W) -> (C,N,Ho,Wo) = side[:, :, ::stride, ::stride].permute(1, 0, 2, 3), contiguous: the input of a kernel-1,
    pad-0 convolution at `stride`, compact and channel-major (K62)."""
    _need(side, F32, "side")
    if side.dim() != 4 or int(stride) < 1:
        raise ValueError("side must be (N, C, H, W) and stride >= 1")
    N, Cc, H, W = side.shape
    out = torch.empty((Cc, N, _strided(H, stride), _strided(W, stride)), dtype=F32, device=side.device)
    _call("xai_stride_gather_cnhw_f32", side.device, _ptr(side), N, Cc, H, W, int(stride), _ptr(out), lib="compact")
    return out


def _cnhw_twin(t, like, name, like_name):
    """`t` must hold `like`'s elements channel-major: (N,C,...) -> C*N*prod(...) elements, contiguous (any view of them)."""
    _need(t, F32, name)
    if t.numel() != like.numel():
        raise ValueError(f"{name} must have the element count of {like_name}")


def bn_relu_fwd_cnhw(x, identity_cnhw, weight, bias, mean, var, eps, variant, bn2=None, gated=True):
    """-> (y, mask): bn_relu_fwd_mask with the identity operand in CNHW order, [C][N][HW] (K63); gated=False writes no mask
    (-> (y, None), bn_act_fwd's result)."""
    _need(x, F32, "x")
    _need_bn(weight, bias, mean, var)
    _cnhw_twin(identity_cnhw, x, "identity_cnhw", "x")
    w2, b2, m2, v2, eps2 = _bn2_fwd(bn2)
    N, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    mask = torch.empty(bn_gate_mask_bytes(x.numel()), dtype=torch.uint8, device=x.device) if gated else None
    y = torch.empty_like(x)
    _call("xai_bn_relu_fwd_cnhw_f32", x.device, _ptr(x), _ptr(identity_cnhw), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(var), float(eps),
          _ptr(w2), _ptr(b2), _ptr(m2), _ptr(v2), float(eps2), int(variant), N, Cc, HW, _ptr(y), _ptr(mask), lib="compact")
    return y, mask


def _bwd_mask_common(numel, mask, weight, var, bn2, want_identity):
    _need(mask, torch.uint8, "mask"); _need(weight, F32, "weight"); _need(var, F32, "var")
    if mask.numel() < bn_gate_mask_bytes(numel):
        raise ValueError(f"mask has {mask.numel()} bytes, needs {bn_gate_mask_bytes(numel)}")
    return _bn2_bwd(bn2, want_identity)


def bn_relu_bwd_compact(gy, mask, weight, var, eps, variant, want_identity=False, gy2=None, gy2_compact=None, stride=2, bn2=None,
                        guided=False, identity_cnhw=False):
    """bn_relu_bwd_mask (K64) with either of: `gy2_compact` (C,N,Ho,Wo) in place of the dense gy2 -- the input gradient of a
    kernel-1 convolution at `stride`, added where stride divides (h, w), +0 added elsewhere; `identity_cnhw`: g_identity comes back
    channel-major, shaped (1, C, N*H, W).  gy must be (N,C,H,W)."""
    _need(gy, F32, "gy")
    if gy.dim() != 4:
        raise ValueError("gy must be (N, C, H, W)")
    _shaped_like(gy2, gy, "gy2", "gy")
    w2, v2, eps2, want_identity = _bwd_mask_common(gy.numel(), mask, weight, var, bn2, want_identity or identity_cnhw)
    N, Cc, H, W = gy.shape
    if gy2_compact is not None:
        _need(gy2_compact, F32, "gy2_compact")
        if gy2 is not None or gy2_compact.numel() != Cc * N * _strided(H, stride) * _strided(W, stride):
            raise ValueError("gy2_compact must hold (C, N, Ho, Wo) elements of this stride, and excludes gy2")
    gx = torch.empty_like(gy)
    gid = None
    if want_identity:
        gid = torch.empty((1, Cc, N * H, W), dtype=F32, device=gy.device) if identity_cnhw else torch.empty_like(gy)
    _call("xai_bn_relu_bwd_compact_f32", gy.device, _ptr(gy), _ptr(gy2), _ptr(gy2_compact), W, int(stride), _ptr(mask), _ptr(weight),
          _ptr(var), float(eps), _ptr(w2), _ptr(v2), float(eps2), int(variant), int(bool(guided)), N, Cc, H * W, _ptr(gx), _ptr(gid),
          int(bool(identity_cnhw)), lib="compact")
    return gx, gid


def bn_relu_bwd_bcast(grad_out, fc_weight, targets, shape, mask, weight, var, eps, variant, want_identity=False, gy2=None, bn2=None,
                      guided=False, scale=None, divisor=0.0):
    """bn_relu_bwd_mask (K64) of an activation of `shape` (N,C,H,W) whose gradient is the head's broadcast
    gy[n][c][:] = (grad_out[n] * fc_weight[targets[n]][c]) * scale (default 1/HW rounded to fp32, PyTorch's mean backward), or
    `/ divisor` where divisor != 0."""
    _need(grad_out, F32, "grad_out"); _need(fc_weight, F32, "fc_weight"); _need(targets, torch.int64, "targets")
    N, Cc = int(shape[0]), int(shape[1])
    HW = 1
    for v in shape[2:]:
        HW *= int(v)
    if grad_out.numel() != N or targets.numel() != N or fc_weight.dim() != 2 or fc_weight.shape[1] != Cc:
        raise ValueError("grad_out and targets must hold N elements and fc_weight be (classes, C)")
    if gy2 is not None:
        _need(gy2, F32, "gy2")
        if tuple(gy2.shape) != tuple(shape):
            raise ValueError("gy2 must have the shape of the activation")
    w2, v2, eps2, want_identity = _bwd_mask_common(N * Cc * HW, mask, weight, var, bn2, want_identity)
    if scale is None:
        scale = float(torch.tensor(1.0, dtype=F32) / torch.tensor(float(HW), dtype=F32))
    gx = torch.empty(tuple(shape), dtype=F32, device=grad_out.device)
    gid = torch.empty_like(gx) if want_identity else None
    _call("xai_bn_relu_bwd_bcast_f32", grad_out.device, _ptr(grad_out), _ptr(fc_weight), _ptr(targets), int(fc_weight.shape[0]),
          float(scale), float(divisor), _ptr(gy2), _ptr(mask), _ptr(weight), _ptr(var), float(eps), _ptr(w2), _ptr(v2), float(eps2),
          int(variant), int(bool(guided)), N, Cc, HW, _ptr(gx), _ptr(gid), lib="compact")
    return gx, gid


# ---- the 1x1 convolution backward-data GEMM with its order of summation as an argument (K78-K79, include/xai_conv.h)
# a walk = (splits, membership, grouping, order, from_zero) in the words of csrc/xai_conv_walk.h
WALK_CONTIGUOUS, WALK_ROUND_ROBIN = 0, 1
WALK_K_CONSECUTIVE, WALK_K_STRIDE4 = 0, 1
WALK_ASCENDING, WALK_DESCENDING = 0, 1


def conv1x1_bwd_data(gy, weight, walk, tile_rows=0, simple=False, out=None):
    """gx (N,C,H,W) = the input gradient of a kernel-1, stride-1, pad-0 convolution with `weight` (K,C,1,1) or (K,C) for the output
    gradient gy (N,K,H,W), summed over k as `walk` says (K78).  simple: by the one-wave-per-tile kernel K79, which takes no
    tile_rows."""
    _need(gy, F32, "gy"); _need(weight, F32, "weight")
    if gy.dim() != 4 or weight.dim() not in (2, 4) or weight.numel() != weight.shape[0] * weight.shape[1] or weight.shape[0] != gy.shape[1]:
        raise ValueError("gy must be (N, K, H, W) and weight (K, C) or (K, C, 1, 1)")
    splits, membership, grouping, order, from_zero = (int(v) for v in walk)
    N, K, H, W = gy.shape
    Cc = int(weight.shape[1])
    gx = _out(out, "out", (N, Cc, H, W), gy)
    if simple:
        _call("xai_conv1x1_bwd_data_simple_f32", gy.device, _ptr(gy), _ptr(weight), N, K, Cc, H * W, splits, membership, grouping, order,
              from_zero, _ptr(gx), lib="conv")
    else:
        _call("xai_conv1x1_bwd_data_f32", gy.device, _ptr(gy), _ptr(weight), N, K, Cc, H * W, splits, membership, grouping, order,
              from_zero, int(tile_rows), _ptr(gx), lib="conv")
    return gx.view(N, Cc, H, W)


def conv1x1_bwd_data_wide(gy, weight, walk, simple=False, out=None):
    """gx (N,C,H,W) as conv1x1_bwd_data gives it, for large planes (K80: every element of gy read from global memory once), summed
    over k in one partial sum as `walk` = (grouping, from_zero, depth, tile, axis, stagger, stride) says: the K loop of `depth` k per
    iteration starts, for the outputs of tile number w of `tile` along hw (axis 0) or c (axis 1), at the iteration csrc/xai_conv_walk.h's
    xai_stagger_plan gives for a GEMM kernel named SU<stagger>_SUS<stride>; stagger 0: at k = 0.  simple: by the one-wave-per-tile
    kernel K81, which takes both axes."""
    _need(gy, F32, "gy"); _need(weight, F32, "weight")
    if gy.dim() != 4 or weight.dim() not in (2, 4) or weight.numel() != weight.shape[0] * weight.shape[1] or weight.shape[0] != gy.shape[1]:
        raise ValueError("gy must be (N, K, H, W) and weight (K, C) or (K, C, 1, 1)")
    grouping, from_zero, depth, tile, axis, stagger, stride = (int(v) for v in walk)
    N, K, H, W = gy.shape
    Cc = int(weight.shape[1])
    gx = _out(out, "out", (N, Cc, H, W), gy)
    _call("xai_convw_bwd_data_simple_f32" if simple else "xai_convw_bwd_data_f32", gy.device, _ptr(gy), _ptr(weight), N, K, Cc, H * W,
          grouping, from_zero, depth, tile, axis, stagger, stride, _ptr(gx), lib="convw")
    return gx.view(N, Cc, H, W)


def bn_relu_maxpool_fwd_code(x, weight, bias, mean, var, eps, variant, kernel, stride, pad):
    """-> (y, code): max_pool2d(relu(bn(x)), kernel, stride, pad) and one uint8 per pooled output for bn_relu_maxpool_bwd (the
    window-local arg-max, or 255 for a closed ReLU gate); x (N,C,H,W) -> (N,C,PH,PW) twice."""
    _need(x, F32, "x")
    _need_bn(weight, bias, mean, var)
    N, Cc, H, W = x.shape
    PH, PW = _pooled(H, W, kernel, stride, pad)
    y = torch.empty((N, Cc, PH, PW), dtype=F32, device=x.device)
    code = torch.empty((N, Cc, PH, PW), dtype=torch.uint8, device=x.device)
    _call("xai_bn_relu_maxpool_fwd_code_f32", x.device, _ptr(x), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(var), float(eps), int(variant),
          N, Cc, H, W, PH, PW, int(kernel), int(stride), int(pad), _ptr(y), _ptr(code))
    return y, code


def bn_relu_maxpool_bwd(gy, code, weight, var, eps, variant, H, W, kernel, stride, pad, gy2=None, guided=False):
    """Input gradient (N,C,H,W) of the fused stem from the gradient(s) gy (+ gy2) of its pooled output and the forward's codes.
    guided: Guided Backprop's rule -- each position's sum over the windows that selected it goes through g <= 0 ? +0 : g."""
    _need(gy, F32, "gy"); _shaped_like(code, gy, "code", "gy", U8); _need(weight, F32, "weight"); _need(var, F32, "var")
    _shaped_like(gy2, gy, "gy2", "gy")
    N, Cc, PH, PW = gy.shape
    gx = torch.empty((N, Cc, int(H), int(W)), dtype=F32, device=gy.device)
    _call("xai_bn_relu_maxpool_bwd_guided_f32" if guided else "xai_bn_relu_maxpool_bwd_f32", gy.device, _ptr(gy), _ptr(gy2), _ptr(code), _ptr(weight), _ptr(var), float(eps), int(variant),
          N, Cc, int(H), int(W), PH, PW, int(kernel), int(stride), int(pad), _ptr(gx))
    return gx


# ------------------------------------------------------------------------------ Guided Backprop / Guided Grad-CAM (K28)
def guided_map(grad, cam=None, want_attr=True, want_map=False, attr=None, map=None):
    """K28: grad (B,C,H,W) [x cam (B,h,w), nearest-upsampled to (H,W)] -> attr (B,C,H,W) and/or the harness map (B,H,W) =
    |sum over channels, left to right|.  -> attr, map, or (attr, map).  `attr` / `map`: preallocated outputs."""
    _need(grad, F32, "grad")
    if grad.dim() != 4:
        raise ValueError("grad must be (B,C,H,W)")
    B, Cc, H, W = grad.shape
    h = w = 0
    if cam is not None:
        _need(cam, F32, "cam")
        if cam.dim() != 3 or cam.shape[0] != B:
            raise ValueError(f"cam must be ({B},h,w), got {tuple(cam.shape)}")
        h, w = cam.shape[1], cam.shape[2]
    if not (want_attr or want_map):
        raise ValueError("nothing to compute: neither the attribution nor the map")
    if want_attr:
        attr = _out(attr, "attr", grad.shape, grad)
    if want_map:
        map = _out(map, "map", (B, H, W), grad)
    _call("xai_guided_map_f32", grad.device, _ptr(grad), _ptr(cam), B, Cc, H, W, int(h), int(w), _ptr(attr if want_attr else None),
          _ptr(map if want_map else None))
    if want_attr and want_map:
        return attr, map
    return attr if want_attr else map


# ------------------------------------------------------------------------------ ViT explainers (K17-K21)
def _image0(t, name, dim):
    """(B, *rest) or (*rest) float32 device tensor -> image 0 as a contiguous (*rest) tensor (a copy only if it is strided)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dim() == dim + 1:
        t = t[0]
    if t.dim() != dim:
        raise ValueError(f"{name} must have {dim} dimensions (or {dim + 1} with a leading image axis), got {tuple(t.shape)}")
    return _need(t.contiguous(), F32, name)


def _table(tensors, dev):
    """device array of the tensors' data pointers (the pointer-table argument of K17, K18, K20); the caller keeps it referenced
    until the launch is issued.  Staged through pinned memory and copied asynchronously on the current stream: no host sync."""
    host = torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).pin_memory()
    return host.to(dev, non_blocking=True)


def _per_block(ts, name, dim):
    ts = [_image0(t, f"{name}[{l}]", dim) for l, t in enumerate(ts)]
    if not ts:
        raise ValueError(f"{name}: no blocks")
    if any(t.shape != ts[0].shape or t.device != ts[0].device for t in ts):
        raise ValueError(f"{name}: every block must have the same shape and device")
    return ts


def attn_head_importance(attns, grads):
    """K17: per-block attention maps and their gradients, L tensors (H,S,S) each (or (B,H,S,S): image 0) -> Ih (L,H), the mean of
    |A_h^T G_h| over its S x S entries, normalised to sum 1 over the heads of each block."""
    attns, grads = _per_block(attns, "attns", 3), _per_block(grads, "grads", 3)
    if len(attns) != len(grads) or attns[0].shape != grads[0].shape:
        raise ValueError("attns and grads must be the same number of equally shaped blocks")
    dev = attns[0].device
    L, (H, S, _) = len(attns), attns[0].shape
    Ih = torch.empty((L, H), dtype=F32, device=dev)
    ws, nbytes = _workspace("xai_attn_head_importance_workspace_bytes", dev, L, H, S)
    atab, gtab = _table(attns, dev), _table(grads, dev)        # held until the launch: a freed table's block is reused at once
    _call("xai_attn_head_importance_f32", dev, _ptr(atab), _ptr(gtab), L, H, S, _ptr(Ih), _ptr(ws), nbytes)
    return Ih


def rave_matrices(attns, Ih, b1, b2, bgrads=None, ablate=0):
    """K18: the row-normalised InFlow matrices (L,S,S) of compute_RAVE from the blocks' attention maps (L tensors (H,S,S)), their head
    importance Ih (L,H), the residual shares b1, b2 (L,2,S) and, for withgrad, the blocks' bottom-up attention gradients."""
    if ablate not in (0, 1):
        raise ValueError("ablate must be 0 or 1")
    attns = _per_block(attns, "attns", 3)
    dev = attns[0].device
    L, (H, S, _) = len(attns), attns[0].shape
    _need(Ih, F32, "Ih"); _need(b1, F32, "b1"); _need(b2, F32, "b2")
    if tuple(Ih.shape) != (L, H) or tuple(b1.shape) != (L, 2, S) or tuple(b2.shape) != (L, 2, S):
        raise ValueError(f"Ih must be ({L},{H}) and b1, b2 ({L},2,{S})")
    gtab = None
    if bgrads is not None:
        bgrads = _per_block(bgrads, "bgrads", 3)
        if len(bgrads) != L or bgrads[0].shape != attns[0].shape:
            raise ValueError("bgrads must match attns")
        gtab = _table(bgrads, dev)
    aug = torch.empty((L, S, S), dtype=F32, device=dev)
    atab = _table(attns, dev)
    _call("xai_rave_matrices_f32", dev, _ptr(atab), _ptr(gtab), _ptr(Ih), _ptr(b1), _ptr(b2), L, H, S, int(ablate), _ptr(aug))
    return aug


def rollout_row(aug, target_token):
    """K19: row `target_token` of aug[L-1] @ ... @ aug[0]; aug (L,S,S) -> (S,), or (n,L,S,S) -> (n,S)."""
    _need(aug, F32, "aug")
    one = aug.dim() == 3
    a = aug[None] if one else aug
    if a.dim() != 4 or a.shape[-1] != a.shape[-2]:
        raise ValueError("aug must be (L,S,S) or (n,L,S,S)")
    n, L, S, _ = a.shape
    t = int(target_token)
    if not -S <= t < S:
        raise IndexError(f"target_token {target_token} out of range for {S} tokens")
    out = torch.empty((n, S), dtype=F32, device=aug.device)
    _call("xai_rollout_row_f32", aug.device, _ptr(a), n, L, S, t % S, _ptr(out))
    return out[0] if one else out


def residual_shares(inputs, attn_outs, resid1s, mlps):
    """K20: per block the token 2-norm shares ((input, attention output), (input + attention, MLP output)), each L tensors (S,D)
    (or (B,S,D): image 0) -> b1, b2 (L,2,S), p=1-normalised over the pair."""
    groups = [_per_block(ts, name, 2) for ts, name in ((inputs, "inputs"), (attn_outs, "attn_outs"), (resid1s, "resid1s"), (mlps, "mlps"))]
    L, (S, D) = len(groups[0]), groups[0][0].shape
    if any(len(g) != L or g[0].shape != (S, D) for g in groups):
        raise ValueError("inputs, attn_outs, resid1s and mlps must be the same number of equally shaped blocks")
    dev = groups[0][0].device
    b1 = torch.empty((L, 2, S), dtype=F32, device=dev)
    b2 = torch.empty((L, 2, S), dtype=F32, device=dev)
    tab = _table([g[l] for l in range(L) for g in groups], dev)
    _call("xai_residual_shares_f32", dev, _ptr(tab), L, S, D, _ptr(b1), _ptr(b2))
    return b1, b2


def attn_cam(attn, grad):
    """K21: cam_attn of one block, attn and grad (B,H,S,S) -> (B,S-1): min-max normalised clamp(mean_h(A*G), 0) of the CLS row's
    token columns (NaN where the map is constant, as in the reference)."""
    _need(attn, F32, "attn"); _need(grad, F32, "grad")
    if attn.shape != grad.shape or attn.dim() != 4 or attn.shape[-1] != attn.shape[-2]:
        raise ValueError("attn and grad must both be (B,H,S,S)")
    B, H, S, _ = attn.shape
    out = torch.empty((B, S - 1), dtype=F32, device=attn.device)
    _call("xai_attn_cam_f32", attn.device, _ptr(attn), _ptr(grad), B, H, S, _ptr(out))
    return out


# ------------------------------------------------------------------------------ Guided IG (K22)
GIG_STATUS = {1: "a selection key is NaN (NaN gradient): the reference would loop forever",
              2: "the step's L1 target was not reached within the selection cap",
              3: "gamma <= 0 or NaN (the reference's assert gamma > 0)",
              4: "more step launches than steps"}


def gig_init(x_input, x_baseline, x, attr, l1_total, state):
    """x = baseline, attr = 0, l1_total = sum |x_input - baseline| per image, state = 0.  All (B, ...) device tensors."""
    for t, n in ((x_input, "x_input"), (x_baseline, "x_baseline"), (x, "x"), (attr, "attr"), (l1_total, "l1_total")):
        _need(t, F32, n)
    _need(state, I32, "state")
    B = x_input.shape[0]
    n = x_input[0].numel()
    if not (x_baseline.numel() == x.numel() == attr.numel() == B * n and l1_total.numel() == B and state.numel() == 4 * B):
        raise ValueError("gig_init: inconsistent sizes")
    _call("xai_gig_init_f32", x_input.device, _ptr(x_input), _ptr(x_baseline), B, n, _ptr(x), _ptr(attr), _ptr(l1_total), _ptr(state))


def gig_step(x_input, x_baseline, grad, steps, fraction, max_dist, x, attr, l1_total, state):
    """One Guided IG step (K22) of every image: reads the step index from `state`, updates x and attr in place."""
    for t, n in ((x_input, "x_input"), (x_baseline, "x_baseline"), (grad, "grad"), (x, "x"), (attr, "attr"), (l1_total, "l1_total")):
        _need(t, F32, n)
    _need(state, I32, "state")
    B = x_input.shape[0]
    n = x_input[0].numel()
    if not (x_baseline.numel() == grad.numel() == x.numel() == attr.numel() == B * n and l1_total.numel() == B
            and state.numel() == 4 * B):
        raise ValueError("gig_step: inconsistent sizes")
    _call("xai_gig_step_f32", x_input.device, _ptr(x_input), _ptr(x_baseline), _ptr(grad), B, n, int(steps), float(fraction),
          float(max_dist), _ptr(x), _ptr(attr), _ptr(l1_total), _ptr(state))


# ------------------------------------------------------------------------------ AGI (K23-K25)
AGI_REASON = {0: "running", 1: "reached the class", 2: "skipped: the class is init_pred", 3: "max_iter updates"}


def _agi_pairs(data, classes, x_cur, c_delta, state, name):
    _need(data, F32, "data"); _need(classes, I32, "classes"); _need(x_cur, F32, "x_cur"); _need(c_delta, F32, "c_delta")
    _need(state, I32, "state")
    B, K = data.shape[0], classes.numel()
    n = data[0].numel() if B else 0
    if B < 1 or K < 1 or n < 1:
        raise ValueError(f"{name}: empty data or classes")
    if not (x_cur.numel() == c_delta.numel() == B * K * n and state.numel() == 4 * B * K):
        raise ValueError(f"{name}: x_cur, c_delta must hold {B * K} x {n} and state {B * K} x 4 elements")
    return B, K, n


def agi_init(logits, data, classes, init_pred, x_cur, c_delta, state):
    """K23: init_pred (int64 (B,)) = argmax of logits (B, n_out); x_cur = data per pair, c_delta = 0, state per pair.
    Pair p = image * K + k attacks classes[k] (int32 (K,), each in [0, n_out))."""
    B, K, n = _agi_pairs(data, classes, x_cur, c_delta, state, "agi_init")
    _need(logits, F32, "logits"); _need(init_pred, I64, "init_pred")
    if logits.dim() != 2 or logits.shape[0] != B or init_pred.numel() != B:
        raise ValueError("agi_init: logits must be (B, n_out) and init_pred (B,)")
    _call("xai_agi_init_f32", data.device, _ptr(logits), _ptr(data), _ptr(classes), B, K, logits.shape[1], n, _ptr(init_pred),
          _ptr(x_cur), _ptr(c_delta), _ptr(state))


def agi_step(logits, g_adv, g_lab, data, classes, epsilon, max_iter, x_cur, c_delta, state):
    """K24: one pgd_step iteration of every pair; logits (B*K, n_out) of the forward of x_cur, g_adv / g_lab the gradients of
    the class's and init_pred's softmax probabilities with respect to x_cur.  Updates x_cur, c_delta and state in place."""
    B, K, n = _agi_pairs(data, classes, x_cur, c_delta, state, "agi_step")
    _need(logits, F32, "logits"); _need(g_adv, F32, "g_adv"); _need(g_lab, F32, "g_lab")
    if logits.dim() != 2 or logits.shape[0] != B * K:
        raise ValueError(f"agi_step: logits must be ({B * K}, n_out)")
    if not g_adv.numel() == g_lab.numel() == B * K * n:
        raise ValueError("agi_step: g_adv and g_lab must have the shape of x_cur")
    if int(max_iter) < 1:
        raise ValueError("agi_step: max_iter must be >= 1")
    _call("xai_agi_step_f32", data.device, _ptr(logits), _ptr(g_adv), _ptr(g_lab), _ptr(data), _ptr(classes), B, K, logits.shape[1],
          n, float(epsilon), int(max_iter), _ptr(x_cur), _ptr(c_delta), _ptr(state))


def agi_heatmap(c_delta, n_img, q_lo=80, q_hi=99, out=None, step_grad=None, qu=None):
    """K25: c_delta (n_img * K, C, H, W) -> the normalised heat map (n_img, H, W) of evaluatePerturbation.py:132-138; optionally
    writes step_grad (n_img, C, H, W) and qu (n_img, 2) = the two percentiles."""
    _need(c_delta, F32, "c_delta")
    if c_delta.dim() != 4 or n_img < 1 or c_delta.shape[0] % n_img:
        raise ValueError("agi_heatmap: c_delta must be (n_img * K, C, H, W)")
    if not (0.0 <= float(q_lo) <= 100.0 and 0.0 <= float(q_hi) <= 100.0):
        raise ValueError("agi_heatmap: percentiles must be in [0, 100]")
    K, C, H, W = c_delta.shape[0] // n_img, c_delta.shape[1], c_delta.shape[2], c_delta.shape[3]
    hold = "agi_heatmap: {} must hold {} elements".format
    out = _out(out, "out", (n_img, H, W), c_delta, hold("out", n_img * H * W))
    _out(step_grad, "step_grad", (n_img, C, H, W), c_delta, hold("step_grad", n_img * C * H * W), alloc=None)
    _out(qu, "qu", (n_img, 2), c_delta, hold("qu", 2 * n_img), alloc=None)
    _call("xai_agi_heatmap_f32", c_delta.device, _ptr(c_delta), n_img, K, C, H * W, float(q_lo), float(q_hi), _ptr(out), _ptr(step_grad),
          _ptr(qu))
    return out


# ------------------------------------------------------------------------------ Feature Ablation / Occlusion (K26, K27)
def window_counts(H, W, window, strides):
    """(count_h, count_w) of captum's Occlusion over (H, W): ceil((dim - window) / stride) + 1 shifts per axis."""
    (wh, ww), (sh, sw) = window, strides
    if not (1 <= wh <= H and 1 <= ww <= W):
        raise ValueError(f"occlusion: window {tuple(window)} must fit the image ({H}, {W})")
    if not (sh >= 1 and sw >= 1 and (sh <= wh or wh == H) and (sw <= ww or ww == W)):
        raise ValueError(f"occlusion: strides {tuple(strides)} must be >= 1 and, where the window can move, at most the window {tuple(window)}")
    return -((wh - H) // sh) + 1, -((ww - W) // sw) + 1


def _ablation_ids(ids, Cc, H, W):
    """ids int32 (H, W) or (C, H, W) -> ids_C"""
    _need(ids, I32, "ids")
    if tuple(ids.shape) == (H, W):
        return 1
    if tuple(ids.shape) == (Cc, H, W):
        return Cc
    raise ValueError(f"ids must be ({H}, {W}) or ({Cc}, {H}, {W}), got {tuple(ids.shape)}")


def _ablation_base(baseline, x):
    if isinstance(baseline, torch.Tensor):
        _need(baseline, F32, "baseline")
        if tuple(baseline.shape) != tuple(x.shape[1:]):
            raise ValueError(f"baseline must be a scalar or {tuple(x.shape[1:])}, got {tuple(baseline.shape)}")
        return baseline, 0.0
    return None, float(baseline)


def _ablation_rows(x, n_total, first, n, out):
    B, Cc, H, W = x.shape
    if not (n >= 1 and 0 <= first and first + n <= B * n_total):
        raise ValueError(f"rows [{first}, {first + n}) are not inside the {B} x {n_total} altered images")
    return _out(out, "out", (n, Cc, H, W), x)


def ablate_features(x, ids, id_min, n_total, baseline, first, n, out=None):
    """K26: rows [first, first + n) of the flat list of altered images (image * n_total + id - id_min) of x (B, C, H, W):
    x * (1 - m) + baseline * m with m = (ids == id) -> (n, C, H, W).  ids: int32 (H, W) or (C, H, W); baseline: scalar or (C, H, W)."""
    _need(x, F32, "x")
    if x.dim() != 4:
        raise ValueError("x must be (B, C, H, W)")
    B, Cc, H, W = x.shape
    ids_C = _ablation_ids(ids, Cc, H, W)
    b, bs = _ablation_base(baseline, x)
    out = _ablation_rows(x, int(n_total), int(first), int(n), out)
    _call("xai_ablate_features_f32", x.device, _ptr(x), _ptr(ids), ids_C, int(id_min), int(n_total), _ptr(b), bs, B, Cc, H, W, int(first),
          int(n), _ptr(out))
    return out


def ablate_windows(x, window, strides, baseline, first, n, out=None):
    """K26, occlusion mode: rows [first, first + n) of the flat list (image * n_windows + k), window k of captum's enumeration
    (row shift fastest), all channels; window, strides: (h, w) pairs."""
    _need(x, F32, "x")
    if x.dim() != 4:
        raise ValueError("x must be (B, C, H, W)")
    B, Cc, H, W = x.shape
    ch, cw = window_counts(H, W, window, strides)
    b, bs = _ablation_base(baseline, x)
    out = _ablation_rows(x, ch * cw, int(first), int(n), out)
    _call("xai_ablate_windows_f32", x.device, _ptr(x), int(window[0]), int(window[1]), int(strides[0]), int(strides[1]), _ptr(b), bs, B, Cc,
          H, W, int(first), int(n), _ptr(out))
    return out


def _finish_outputs(s0, scores, B, n_total, shape, g, want_attr):
    _need(s0, F32, "s0"); _need(scores, F32, "scores")
    if s0.numel() != B or scores.numel() != B * n_total:
        raise ValueError(f"s0 must hold {B} and scores {B} x {n_total} values")
    if not want_attr and g is None:
        raise ValueError("nothing to compute: neither the attribution nor samples")
    if g is not None and int(g) < 1:
        raise ValueError("g must be >= 1")
    attr = torch.empty(shape, dtype=F32, device=s0.device) if want_attr else None
    samples = torch.empty((shape[0], shape[1], int(g), int(g)), dtype=F32, device=s0.device) if g is not None else None
    return attr, samples


def ablation_finish_features(s0, scores, ids, id_min, shape, g=None, want_attr=True):
    """K27: s0 (B,), scores (B, n_total), ids int32 (H, W) or (C, H, W) -> (attr (B, C, H, W) or None, samples (B, C, g, g) or None):
    captum's FeatureAblation attribution and its nearest-exact g x g samples."""
    B, Cc, H, W = (int(v) for v in shape)
    n_total = scores.shape[-1]
    attr, samples = _finish_outputs(s0, scores, B, n_total, (B, Cc, H, W), g, want_attr)
    ids_C = _ablation_ids(ids, Cc, H, W)
    _call("xai_ablation_finish_features_f32", s0.device, _ptr(s0), _ptr(scores), _ptr(ids), ids_C, int(id_min), int(n_total), B, Cc, H, W,
          int(g or 0), _ptr(attr), _ptr(samples))
    return attr, samples


def ablation_finish_windows(s0, scores, window, strides, shape, g=None, want_attr=True):
    """K27, occlusion mode: the sum of s0 - scores[k] over the windows covering an element, ascending k, over their count."""
    B, Cc, H, W = (int(v) for v in shape)
    ch, cw = window_counts(H, W, window, strides)
    attr, samples = _finish_outputs(s0, scores, B, ch * cw, (B, Cc, H, W), g, want_attr)
    _call("xai_ablation_finish_windows_f32", s0.device, _ptr(s0), _ptr(scores), int(window[0]), int(window[1]), int(strides[0]),
          int(strides[1]), B, Cc, H, W, int(g or 0), _ptr(attr), _ptr(samples))
    return attr, samples


# ------------------------------------------------------------------------------ XRAI (K29, K30)
XRAI_STATUS = {1: "masks remain but none has a gain above -inf (NaN or -inf in the attribution): the reference crashes at this "
                  "point with KeyError on remaining_masks[None] (XRAIBuilder.py:682)",
               2: "a full-mask gain is NaN: the order of the reference's sort (XRAIBuilder.py:754-755) is undefined"}


def xrai_words(H, W):
    return (H * W + 63) // 64


def xrai_pack(H, W, radius, M, labels=None, label_min=None, label_max=None, masks=None):
    """K29: label maps (S, H, W) int32 with per-map label_min / label_max (S,) int32, or masks (M, H, W) uint8 -> the dilated
    bit planes (M, n_words) int64 and span (M, 2) int32 (first, last non-empty word).  `M` in label mode: the sum of
    label_max - label_min + 1 (the caller knows the ranges; nothing is read back here)."""
    if (labels is None) == (masks is None):
        raise ValueError("xrai_pack: pass label maps or masks, not both")
    if labels is not None:
        _need(labels, I32, "labels"); _need(label_min, I32, "label_min"); _need(label_max, I32, "label_max")
        S, src = labels.shape[0], labels
        if labels.dim() != 3 or tuple(labels.shape[1:]) != (H, W) or label_min.numel() != S or label_max.numel() != S:
            raise ValueError("xrai_pack: labels must be (S, H, W) and label_min, label_max (S,)")
    else:
        _need(masks, U8, "masks")
        S, src = 0, masks
        if masks.dim() != 3 or tuple(masks.shape) != (M, H, W):
            raise ValueError("xrai_pack: masks must be (M, H, W)")
    bits = torch.empty((M, xrai_words(H, W)), dtype=I64, device=src.device)
    span = torch.empty((M, 2), dtype=I32, device=src.device)
    if M:
        _call("xai_xrai_pack_u64", src.device, _ptr(labels), _ptr(label_min), _ptr(label_max), S, _ptr(masks), M, H, W, int(radius),
              _ptr(bits), _ptr(span))
    return bits, span


def xrai_rank(attr, bits, span, mask_first, min_pixel_diff, area_threshold, fast=False):
    """K30: attr (B, H, W), the planes of all images and mask_first (B + 1,) int32 -> out (B, H, W) fp32, pixel_iter (B, H, W)
    int32, sel_key (M,) int32, sel_gain (M,) fp32, state (B, 4) int32 = selections, uncomputed pixels, status, covered pixels."""
    _need(attr, F32, "attr"); _need(bits, I64, "bits"); _need(span, I32, "span"); _need(mask_first, I32, "mask_first")
    if attr.dim() != 3:
        raise ValueError("xrai_rank: attr must be (B, H, W)")
    B, H, W = attr.shape
    M = bits.shape[0]
    if bits.dim() != 2 or bits.shape[1] != xrai_words(H, W) or span.numel() != 2 * M or mask_first.numel() != B + 1:
        raise ValueError("xrai_rank: bits must be (M, ceil(H*W/64)), span (M, 2) and mask_first (B + 1,)")
    dev = attr.device
    out = torch.empty((B, H, W), dtype=F32, device=dev)
    pixel_iter = torch.empty((B, H, W), dtype=I32, device=dev)
    sel_key = torch.empty(M, dtype=I32, device=dev)
    sel_gain = torch.empty(M, dtype=F32, device=dev)
    state = torch.empty((B, 4), dtype=I32, device=dev)
    ws, nbytes = _workspace("xai_xrai_workspace_bytes", dev, B, H, W, M)
    _call("xai_xrai_rank_f32", dev, _ptr(attr), _ptr(bits) if M else None, _ptr(span) if M else None, _ptr(mask_first), B, M, H, W,
          int(min_pixel_diff), float(area_threshold), int(bool(fast)), _ptr(out), _ptr(pixel_iter), _ptr(sel_key) if M else None,
          _ptr(sel_gain) if M else None, _ptr(state), _ptr(ws), nbytes)
    return out, pixel_iter, sel_key, sel_gain, state


# ------------------------------------------------------------------------------ LIME (K31, K32, K33)
def lime_max_features():
    """The largest number of superpixels of one image K32 fits."""
    return int(_lib.load().xai_lime_max_features())


def lime_words(d_max):
    return (int(d_max) + 63) // 64


def _lime_rows(rows, D, B, name):
    """rows int64 (B * N, words) bit rows, D int32 (B,) -> (N, words)"""
    _need(rows, I64, "rows"); _need(D, I32, "D")
    if rows.dim() != 2 or D.numel() != B or rows.shape[0] % B or rows.shape[0] == 0 or rows.shape[1] == 0:
        raise ValueError(f"{name}: rows must be (B * n_samples, words) and D ({B},)")
    return rows.shape[0] // B, rows.shape[1]


def lime_compose(x, seg, rows, D, hide, first, n, fudged=None, out=None):
    """K31: rows [first, first + n) of the flat list of perturbed images (image * n_samples + sample) of x (B, C, H, W):
    x where the row keeps the pixel's superpixel, else `fudged` (B, C, H, W) or `hide` (C,) -> (n, C, H, W).  seg: int32 (B, H, W);
    rows: int64 (B * n_samples, words) bit rows; D: int32 (B,) superpixels per image."""
    _need(x, F32, "x"); _need(seg, I32, "seg")
    if x.dim() != 4:
        raise ValueError("x must be (B, C, H, W)")
    B, Cc, H, W = x.shape
    if tuple(seg.shape) != (B, H, W):
        raise ValueError(f"seg must be ({B}, {H}, {W}), got {tuple(seg.shape)}")
    N, words = _lime_rows(rows, D, B, "lime_compose")
    if fudged is not None:
        _need(fudged, F32, "fudged")
        if tuple(fudged.shape) != tuple(x.shape):
            raise ValueError(f"fudged must be {tuple(x.shape)}, got {tuple(fudged.shape)}")
    if hide is not None:
        _need(hide, F32, "hide")
        if hide.numel() != Cc:
            raise ValueError(f"hide must hold {Cc} values")
    if hide is None and fudged is None:
        raise ValueError("lime_compose: pass hide or fudged")
    out = _ablation_rows(x, N, int(first), int(n), out)
    _call("xai_lime_compose_f32", x.device, _ptr(x), _ptr(seg), _ptr(rows), _ptr(D), words, _ptr(hide), _ptr(fudged), B, Cc, H, W, N,
          int(first), int(n), _ptr(out))
    return out


def lime_fit(rows, D, Y, kernel_width=0.25, alpha_select=0.01, alpha=1.0, d_stride=None):
    """K32: rows int64 (B * N, words), D int32 (B,), Y float32 (B, N, L) -> dict of fp64 device tensors coef (B, L, d_stride),
    intercept, score, local_pred (B, L), dist, weight (B, N) and int32 order (B, L, d_stride).  An image whose D is above
    `lime_max_features()` is skipped: its entries stay zero (order -1)."""
    _need(Y, F32, "Y")
    if Y.dim() != 3:
        raise ValueError("lime_fit: Y must be (B, N, L)")
    B, N, L = Y.shape
    n_rows, words = _lime_rows(rows, D, B, "lime_fit")
    if n_rows != N or L == 0:
        raise ValueError(f"lime_fit: rows hold {n_rows} samples per image, Y {N} with {L} labels")
    d_stride = words * 64 if d_stride is None else int(d_stride)
    dev = Y.device
    res = dict(coef=torch.zeros((B, L, d_stride), dtype=F64, device=dev), order=torch.full((B, L, d_stride), -1, dtype=I32, device=dev),
               intercept=torch.zeros((B, L), dtype=F64, device=dev), score=torch.zeros((B, L), dtype=F64, device=dev),
               local_pred=torch.zeros((B, L), dtype=F64, device=dev), dist=torch.zeros((B, N), dtype=F64, device=dev),
               weight=torch.zeros((B, N), dtype=F64, device=dev))
    _call("xai_lime_fit_f64", dev, _ptr(rows), words, _ptr(D), _ptr(Y), B, N, L, d_stride, float(kernel_width), float(alpha_select),
          float(alpha), _ptr(res["coef"]), _ptr(res["intercept"]), _ptr(res["score"]), _ptr(res["local_pred"]), _ptr(res["order"]),
          _ptr(res["dist"]), _ptr(res["weight"]))
    return res


def lime_paint(table, seg):
    """K33: table float32 (B, d_stride), seg int32 (B, H, W) -> (B, H, W) float32, table[b][seg[b]] (0 for an id outside the table)."""
    _need(table, F32, "table"); _need(seg, I32, "seg")
    if table.dim() != 2 or seg.dim() != 3 or seg.shape[0] != table.shape[0] or table.shape[1] == 0:
        raise ValueError("lime_paint: table must be (B, d_stride) and seg (B, H, W)")
    B, H, W = seg.shape
    out = torch.empty((B, H, W), dtype=F32, device=seg.device)
    _call("xai_lime_paint_f32", seg.device, _ptr(table), _ptr(seg), B, table.shape[1], H, W, _ptr(out))
    return out


# ------------------------------------------------------------------------------ GradientShap (K34, K35; libxai_ext.so)
def _gshap_rows(x, baselines, idx, n_rows, n_samples, name):
    """x (B, ...) per image or (B * n_samples, ...) per row, baselines (N_b, ...) of the same item shape, idx int64 (n_rows,)
    -> (x_per_row, N_b, elements per item)"""
    _need(x, F32, "x"); _need(baselines, F32, "baselines"); _need(idx, I64, "idx")
    n_samples = int(n_samples)
    if n_samples < 1 or n_rows % n_samples:
        raise ValueError(f"{name}: {n_rows} rows are no multiple of n_samples = {n_samples}")
    if x.dim() < 2 or baselines.dim() != x.dim() or baselines.shape[1:] != x.shape[1:] or baselines.shape[0] == 0 or x[0].numel() == 0:
        raise ValueError(f"{name}: baselines must be (N_b,) + {tuple(x.shape[1:])}, got {tuple(baselines.shape)}")
    if x.shape[0] not in (n_rows, n_rows // n_samples):
        raise ValueError(f"{name}: x must hold {n_rows // n_samples} images or {n_rows} rows, got {x.shape[0]}")
    if idx.numel() != n_rows:
        raise ValueError(f"{name}: idx must hold {n_rows} values, got {idx.numel()}")
    # n_samples == 1: one row per image either way, the two layouts coincide
    return int(x.shape[0] == n_rows and n_samples > 1), baselines.shape[0], x[0].numel()


def gshap_scale(x, baselines, alpha, idx, n_samples, out=None):
    """K34: out[r] = alpha[r] * xr[r] + (1 - alpha[r]) * baselines[idx[r]] for the R = alpha.numel() rows of GradientShap, two
    products and a sum in fp32.  x (R / n_samples, ...) one input per image (row r reads image r // n_samples) or (R, ...) one per
    row; baselines (N_b, ...); alpha float32 (R,), idx int64 (R,) in [0, N_b) on the device -> (R, ...)."""
    _need(alpha, F32, "alpha")
    R = alpha.numel()
    per_row, n_base, E = _gshap_rows(x, baselines, idx, R, n_samples, "gshap_scale")
    out = _out(out, "out", (R,) + tuple(x.shape[1:]), x)
    _call("xai_gshap_scale_f32", x.device, _ptr(x), _ptr(baselines), _ptr(alpha), _ptr(idx), R, int(n_samples), E, n_base, per_row,
          _ptr(out), lib="ext")
    return out


def gshap_finish(grads, x, baselines, idx, n_samples, want_attr=True, want_map=False, attr=None, map=None):
    """K35: grads (B * n_samples, C, H, W) -> attr (B, C, H, W) = the mean over an image's samples of (xr - baselines[idx]) * grads
    (summed ascending from +0, divided by n_samples) and/or the harness map (B, H, W) = |sum over channels, left to right|.
    x per image or per row as for K34.  -> attr, map, or (attr, map).  `attr` / `map`: preallocated outputs."""
    _need(grads, F32, "grads")
    if grads.dim() != 4:
        raise ValueError("grads must be (B * n_samples, C, H, W)")
    R, Cc, H, W = grads.shape
    per_row, n_base, _ = _gshap_rows(x, baselines, idx, R, n_samples, "gshap_finish")
    if x.shape[1:] != grads.shape[1:]:
        raise ValueError(f"gshap_finish: x must be (.., {Cc}, {H}, {W}), got {tuple(x.shape)}")
    if not (want_attr or want_map):
        raise ValueError("nothing to compute: neither the attribution nor the map")
    B = R // int(n_samples)
    if want_attr:
        attr = _out(attr, "attr", (B, Cc, H, W), grads)
    if want_map:
        map = _out(map, "map", (B, H, W), grads)
    _call("xai_gshap_finish_f32", grads.device, _ptr(grads), _ptr(x), _ptr(baselines), _ptr(idx), B, int(n_samples), Cc, H * W, n_base,
          per_row, _ptr(attr if want_attr else None), _ptr(map if want_map else None), lib="ext")
    if want_attr and want_map:
        return attr, map
    return attr if want_attr else map


# ------------------------------------------------------------------------------ MDA (K36, K37, K38; libxai_ext2.so)
def mda_max_segments():
    """The largest number of segments of one image K37 takes."""
    return int(_lib.load("ext2").xai_mda_max_segments())


def mda_max_width():
    """The largest sub-search width (candidates per step) K37 takes."""
    return int(_lib.load("ext2").xai_mda_max_width())


def _mda_images(start, finish, seg, name):
    """start, finish (n_img, C, H, W) float32, seg (n_img, H, W) int32 -> (n_img, C, H * W)"""
    _need(start, F32, "start"); _need(finish, F32, "finish"); _need(seg, I32, "seg")
    if start.dim() != 4 or finish.shape != start.shape or start.numel() == 0:
        raise ValueError(f"{name}: start and finish must be (n_img, C, H, W) of one shape")
    n_img, Cc, H, W = start.shape
    if tuple(seg.shape) != (n_img, H, W):
        raise ValueError(f"{name}: seg must be ({n_img}, {H}, {W}), got {tuple(seg.shape)}")
    return n_img, Cc, H * W


def mda_compose(start, finish, seg, cand, out=None):
    """K36: out[img][r] = start[img] with the pixels of segment cand[img][r] taken from finish[img] (a select; a label no pixel
    carries, such as K37's -1, gives a copy of start).  start, finish (n_img, C, H, W); seg int32 (n_img, H, W); cand int32
    (n_img, L) -> (n_img * L, C, H, W)."""
    n_img, Cc, hw = _mda_images(start, finish, seg, "mda_compose")
    _need(cand, I32, "cand")
    if cand.dim() != 2 or cand.shape[0] != n_img or cand.shape[1] == 0:
        raise ValueError(f"mda_compose: cand must be ({n_img}, L), got {tuple(cand.shape)}")
    L = cand.shape[1]
    out = _out(out, "out", (n_img * L,) + tuple(start.shape[1:]), start)
    _call("xai_mda_compose_f32", start.device, _ptr(start), _ptr(finish), _ptr(seg), _ptr(cand), n_img, L, Cc, hw, _ptr(out), lib="ext2")
    return out


def mda_select(resp, order, plan, stop_ref, mode, cutoff, mr, chosen, taken, cand, state, stop_test=None):
    """K37: one search step's decision for every image, in place on the caller's arrays: resp float32 (n_img, L); order int32
    (n_img, S); plan int32 (n_img, plan_stride, 3) rows of (slot, n_cand, cutoff_slot); stop_ref float32 (n_img, 2) = (blur_pred,
    |original_pred - blur_pred|) or None; mr float32, chosen, taken int32 (n_img, S); cand int32 (n_img, L); state int32 (n_img, 4)
    = (steps taken, done, last winner, plan rows).  mode 1: argmax and the stop test against `cutoff` (stop_test: default
    cutoff != 1, the reference's guard); mode 0: argmin."""
    _need(resp, F32, "resp"); _need(order, I32, "order"); _need(plan, I32, "plan"); _need(mr, F32, "mr")
    _need(chosen, I32, "chosen"); _need(taken, I32, "taken"); _need(cand, I32, "cand"); _need(state, I32, "state")
    if resp.dim() != 2 or order.dim() != 2 or plan.dim() != 3 or plan.shape[2] != 3 or plan.shape[1] == 0:
        raise ValueError("mda_select: resp must be (n_img, L), order (n_img, S) and plan (n_img, plan_stride, 3)")
    n_img, L = resp.shape
    S = order.shape[1]
    if order.shape[0] != n_img or plan.shape[0] != n_img or L == 0 or S == 0:
        raise ValueError("mda_select: resp, order and plan disagree about the number of images")
    for t, shape, name in ((mr, (n_img, S), "mr"), (chosen, (n_img, S), "chosen"), (taken, (n_img, S), "taken"),
                           (cand, (n_img, L), "cand"), (state, (n_img, 4), "state")):
        if tuple(t.shape) != shape:
            raise ValueError(f"mda_select: {name} must be {shape}, got {tuple(t.shape)}")
    if mode not in (0, 1):
        raise ValueError("mda_select: mode is 0 (argmin) or 1 (argmax and the stop test)")
    stop_test = (mode == 1 and cutoff != 1) if stop_test is None else bool(stop_test)
    if mode == 1 and stop_test:
        if stop_ref is None:
            raise ValueError("mda_select: the stop test needs stop_ref")
        _need(stop_ref, F32, "stop_ref")
        if tuple(stop_ref.shape) != (n_img, 2):
            raise ValueError(f"mda_select: stop_ref must be ({n_img}, 2), got {tuple(stop_ref.shape)}")
    _call("xai_mda_select_f32", resp.device, _ptr(resp), _ptr(order), _ptr(plan), _ptr(stop_ref), n_img, S, L, plan.shape[1],
          int(mode), int(stop_test), float(cutoff), _ptr(mr), _ptr(chosen), _ptr(taken), _ptr(cand), _ptr(state), lib="ext2")


def mda_commit(finish, seg, state, start):
    """K38: start[img] takes the pixels of segment state[img][2] (the last winner; < 0: none) from finish[img], in place."""
    n_img, Cc, hw = _mda_images(start, finish, seg, "mda_commit")
    _need(state, I32, "state")
    if tuple(state.shape) != (n_img, 4):
        raise ValueError(f"mda_commit: state must be ({n_img}, 4), got {tuple(state.shape)}")
    _call("xai_mda_commit_f32", start.device, _ptr(finish), _ptr(seg), _ptr(state), n_img, Cc, hw, _ptr(start), lib="ext2")
    return start


# ------------------------------------------------------------------------------ sanity test (K39-K43; libxai_ext2.so)
def _maps(t, name):
    """(n, H, W) float32 maps with at least one element"""
    _need(t, F32, name)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name} must be (n, H, W) with n, H, W >= 1, got {tuple(t.shape)}")
    return t.shape


def sanity_normalize(x, guard=True, out=None):
    """K39: x (n, ...) float32 -> every map normalize_image'd (evaluateSanity.py:68-79; guard=False: sanityForMethods.py:60-72)."""
    _need(x, F32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"sanity_normalize: x must be (n, ...) with at least one element per map, got {tuple(x.shape)}")
    out = _out(out, "out", x.shape, x)
    _call("xai_sanity_normalize_f32", x.device, _ptr(x), x.shape[0], x[0].numel(), int(bool(guard)), _ptr(out), lib="ext2")
    return out.view(x.shape)


def ssim_tile():
    """The extent of K40's square output tile."""
    return int(_lib.load("ext2").xai_ssim_tile())


def ssim_weights(sigma=1.5, truncate=3.5):
    """The distinct weights of scipy.ndimage's Gaussian, outermost first and the centre last, computed as _gaussian_kernel1d does
    (NumPy's exp and its sum, so the bits are scipy's): six fp64 numbers for sigma 1.5 and truncate 3.5."""
    import numpy as np
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return [float(v) for v in (phi / phi.sum())[:radius + 1]]


def ssim(x, y, data_range=2.0, want_map=False):
    """K40: x, y (n, H, W) float32 -> mean SSIM (n,) float64 [, the full S map (n, H, W) float32]: skimage's
    structural_similarity(gaussian_weights=True, data_range=data_range) per pair."""
    n, H, W = _maps(x, "x")
    _shaped_like(y, x, "y", "x")
    if H < 11 or W < 11:
        raise ValueError(f"ssim: the Gaussian window is 11 x 11, the maps are {H} x {W}")
    c1, c2 = (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2
    ws, nbytes = _workspace("xai_ssim_workspace_bytes", x.device, n, H, W, lib="ext2", required=True)
    mean = torch.empty(n, dtype=F64, device=x.device)
    S = torch.empty((n, H, W), dtype=F32, device=x.device) if want_map else None
    _call("xai_ssim_f32", x.device, _ptr(x), _ptr(y), n, H, W, *ssim_weights(), c1, c2, _ptr(mean), _ptr(S), _ptr(ws),
          nbytes, lib="ext2")
    return (mean, S) if want_map else mean


def tie_ranks_chunk():
    """The number of sorted positions one workgroup of K41 handles."""
    return int(_lib.load("ext2").xai_tie_ranks_chunk())


def tie_ranks(vals, order):
    """K41: vals (n_rows, n) float32 and their stable ascending argsort (K8's `order`) -> int32 (n_rows, n): twice each element's
    rankdata(method='average') rank."""
    _need(vals, F32, "vals"); _need(order, I32, "order")
    if vals.dim() != 2 or vals.numel() == 0 or order.shape != vals.shape:
        raise ValueError(f"tie_ranks: vals and order must be (n_rows, n) of one shape, got {tuple(vals.shape)} and {tuple(order.shape)}")
    out = torch.empty_like(order)
    _call("xai_tie_ranks_i32", vals.device, _ptr(vals), _ptr(order), vals.shape[0], vals.shape[1], _ptr(out), lib="ext2")
    return out


def rank_corr_max_n():
    """The largest row length K42 takes."""
    return int(_lib.load("ext2").xai_rank_corr_max_n())


def rank_corr(ra, rb, a=None, b=None):
    """K42: doubled ranks ra, rb int32 (n_pairs, n) [, the ranked values a, b float32 for the NaN test] -> float64 (n_pairs,):
    scipy.stats.spearmanr's statistic of each pair."""
    _need(ra, I32, "ra"); _need(rb, I32, "rb")
    if ra.dim() != 2 or ra.numel() == 0 or rb.shape != ra.shape:
        raise ValueError(f"rank_corr: ra and rb must be (n_pairs, n) of one shape, got {tuple(ra.shape)} and {tuple(rb.shape)}")
    _shaped_like(a, ra, "a", "ra"); _shaped_like(b, ra, "b", "ra")
    out = torch.empty(ra.shape[0], dtype=F64, device=ra.device)
    _call("xai_rank_corr_f64", ra.device, _ptr(ra), _ptr(rb), _ptr(a), _ptr(b), ra.shape[0], ra.shape[1], _ptr(out), lib="ext2")
    return out


def hog(img, cell=(16, 16)):
    """K43: img (n, H, W) float32 -> float32 (n, (H // ch - 2) * (W // cw - 2) * 81): skimage.feature.hog(orientations=9,
    pixels_per_cell=cell, cells_per_block=(3, 3), block_norm='L2-Hys') of every map, flattened as skimage flattens it."""
    n, H, W = _maps(img, "img")
    ch, cw = int(cell[0]), int(cell[1])
    if ch < 1 or cw < 1 or H // ch < 3 or W // cw < 3:
        raise ValueError(f"hog: {H} x {W} pixels in cells of {ch} x {cw} give fewer than 3 cells on an axis")
    ws, nbytes = _workspace("xai_hog_workspace_bytes", img.device, n, H, W, ch, cw, lib="ext2", required=True)
    out = torch.empty((n, (H // ch - 2) * (W // cw - 2) * 81), dtype=F32, device=img.device)
    _call("xai_hog_f32", img.device, _ptr(img), n, H, W, ch, cw, _ptr(out), _ptr(ws), nbytes, lib="ext2")
    return out


# ------------------------------------------------------------------------------ segmentation evaluation (K44-K45; libxai_ext3.so)
def seg_normalize(x, out=None):
    """K44: x (n, ...) float32 -> (out, thr, stats): every map min-max normalised in fp32 (evaluateImageNetSeg.py:215-217; Inf is not
    replaced, a constant map becomes NaN), thr (n,) float32 the mean of each normalised map in the header's stated fp64 tree, stats
    (n, 2) float32 the (min, max) used.  out may be x."""
    _need(x, F32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"seg_normalize: x must be (n, ...) with at least one element per map, got {tuple(x.shape)}")
    out = _out(out, "out", x.shape, x)
    n = x.shape[0]
    thr = torch.empty(n, dtype=F32, device=x.device)
    stats = torch.empty((n, 2), dtype=F32, device=x.device)
    _call("xai_seg_normalize_f32", x.device, _ptr(x), n, x[0].numel(), _ptr(out), _ptr(thr), _ptr(stats), lib="ext3")
    return out.view(x.shape), thr, stats


def seg_counts(res, labels, thr):
    """K45: res (n, H, W) float32, labels (n, H, W) int32, thr (n, T) float32 with 1 <= T <= 16 -> (counts, other): counts int32
    (n, T, H, 2, 3) = pixels of a row by label (0 / 1) and state (<= thr, > thr, neither), other int32 (n,) = pixels whose label is
    neither 0 nor 1."""
    n, H, W = _maps(res, "res")
    _shaped_like(labels, res, "labels", "res", dtype=I32)
    _need(thr, F32, "thr")
    if thr.dim() != 2 or thr.shape[0] != n or thr.shape[1] == 0:
        raise ValueError(f"seg_counts: thr must be ({n}, T) with T >= 1, got {tuple(thr.shape)}")
    T = thr.shape[1]
    counts = torch.empty((n, T, H, 2, 3), dtype=I32, device=res.device)
    other = torch.empty(n, dtype=I32, device=res.device)
    _call("xai_seg_counts_i32", res.device, _ptr(res), _ptr(labels), _ptr(thr), n, H, W, T, _ptr(counts), _ptr(other), lib="ext3")
    return counts, other


# ------------------------------------------------------------------------------ Transformer Attribution (K46-K52; libxai_ext4.so)
def _images(t, name):
    """(B, elements per image) of an operand whose leading axis counts images"""
    _need(t, F32, name)
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError(f"{name} must be (B, ...) with at least one element per image, got {tuple(t.shape)}")
    return t.shape[0], t[0].numel()


def lrp_split(x, pos=None, neg=None):
    """K46: x (B, ...) -> (clamp(x, min=0), clamp(x, max=0))"""
    B, n = _images(x, "x")
    pos, neg = _out(pos, "pos", x.shape, x), _out(neg, "neg", x.shape, x)
    _call("xai_lrp_split_f32", x.device, _ptr(x), B, n, _ptr(pos), _ptr(neg), lib="ext4")
    return pos, neg


def lrp_ratio(r, z1, z2=None, out=None):
    """K47: safe_divide(r, z1 + z2) (layers_ours.py:10-13), or safe_divide(r, z1) without z2; out may be one of the operands"""
    B, n = _images(r, "r")
    _shaped_like(z1, r, "z1", "r"); _shaped_like(z2, r, "z2", "r")
    if z1 is None:
        raise TypeError("z1: expected a torch.Tensor, got NoneType")
    out = _out(out, "out", r.shape, r)
    _call("xai_lrp_ratio_f32", r.device, _ptr(r), _ptr(z1), _ptr(z2), B, n, _ptr(out), lib="ext4")
    return out


def lrp_gather(x, g1, g2, out=None):
    """K48: clamp(x, min=0) * g1 + clamp(x, max=0) * g2; out may be g1 or g2"""
    B, n = _images(x, "x")
    for t, name in ((g1, "g1"), (g2, "g2")):
        _need(t, F32, name)
        _shaped_like(t, x, name, "x")
    out = _out(out, "out", x.shape, x)
    _call("xai_lrp_gather_f32", x.device, _ptr(x), _ptr(g1), _ptr(g2), B, n, _ptr(out), lib="ext4")
    return out


def lrp_half_product(x, c, out=None, slot=None):
    """K49: x * c / 2.  Plain (slot None): any shape (B, ...), out like x.  slot 0 / 1 / 2: x, c (B, h, N, d) and `out` the
    (B, N, 3 * h * d) cam_qkv buffer, of which only the slot's third is written."""
    _need(x, F32, "x"); _need(c, F32, "c")
    _shaped_like(c, x, "c", "x")
    if slot is None:
        B, n = _images(x, "x")
        if n > 2 ** 31 - 1:
            raise ValueError(f"lrp_half_product: {n} elements per image are more than K49 takes")
        out = _out(out, "out", x.shape, x)
        _call("xai_lrp_half_product_f32", x.device, _ptr(x), _ptr(c), B, 1, n, 1, 1, 0, _ptr(out), lib="ext4")
        return out
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"lrp_half_product: a slot needs x of (B, h, N, d), got {tuple(x.shape)}")
    if slot not in (0, 1, 2):
        raise ValueError("slot must be 0, 1 or 2")
    B, h, N, d = x.shape
    if out is None:
        raise TypeError("lrp_half_product: a slot needs the cam_qkv buffer as out")
    _out(out, "out", (B, N, 3 * h * d), x, wrong=f"out must be the ({B}, {N}, {3 * h * d}) cam_qkv buffer")
    _call("xai_lrp_half_product_f32", x.device, _ptr(x), _ptr(c), B, h, N, d, 3, int(slot), _ptr(out), lib="ext4")
    return out


def lrp_add_chunk():
    """the elements of an image one workgroup of K50 sums"""
    return _lib.load("ext4").xai_lrp_add_chunk()


def lrp_add(x0, x1, r, a=None, b=None, ws=None):
    """K50: Add.relprop (layers_ours.py:106-125) per image, x0, x1, r (B, ...) -> (a, b); the sums are fp64 in the header's tree.
    ws: a uint8 scratch of at least xai_lrp_add_workspace_bytes(B, n) bytes (allocated when None)."""
    B, n = _images(r, "r")
    for t, name in ((x0, "x0"), (x1, "x1")):
        _need(t, F32, name)
        _shaped_like(t, r, name, "r")
    a, b = _out(a, "a", r.shape, r), _out(b, "b", r.shape, r)
    nbytes = _lib.load("ext4").xai_lrp_add_workspace_bytes(B, n)
    if nbytes == 0:
        raise ValueError(f"lrp_add: {B} images of {n} elements are more than K50 takes")
    if ws is None:
        ws = torch.empty(nbytes, dtype=U8, device=r.device)
    _need(ws, U8, "ws")
    _call("xai_lrp_add_parts_f32", r.device, _ptr(x0), _ptr(x1), _ptr(r), B, n, _ptr(a), _ptr(b), _ptr(ws), ws.numel(), lib="ext4")
    _call("xai_lrp_add_scale_f32", r.device, _ptr(a), _ptr(b), B, n, _ptr(ws), ws.numel(), lib="ext4")
    return a, b


def lrp_clone(x, r1, r2, out=None):
    """K51: x * (safe_divide(r1, x) + safe_divide(r2, x)); out may be r1 or r2"""
    B, n = _images(x, "x")
    for t, name in ((r1, "r1"), (r2, "r2")):
        _need(t, F32, name)
        _shaped_like(t, x, name, "x")
    out = _out(out, "out", x.shape, x)
    _call("xai_lrp_clone_f32", x.device, _ptr(x), _ptr(r1), _ptr(r2), B, n, _ptr(out), lib="ext4")
    return out


LRP_MATRICES, LRP_ROLLOUT, LRP_CLS_ROW = 0, 1, 2


def lrp_attn_matrices(cam, grad=None, mode=LRP_ROLLOUT):
    """K52: cam (and grad, or None) (L, B, h, S, S) -> the head mean of clamp(grad * cam, min=0) of every block, heads added in
    ascending order: LRP_MATRICES (B, L, S, S); LRP_ROLLOUT the same plus the identity, every row divided by its sum (what K19,
    `rollout_row`, chains); LRP_CLS_ROW (B, L, S), row 0 only."""
    _need(cam, F32, "cam")
    if cam.dim() != 5 or cam.shape[-1] != cam.shape[-2] or cam.numel() == 0:
        raise ValueError(f"cam must be (L, B, h, S, S), got {tuple(cam.shape)}")
    _shaped_like(grad, cam, "grad", "cam")
    if mode not in (LRP_MATRICES, LRP_ROLLOUT, LRP_CLS_ROW):
        raise ValueError("mode must be LRP_MATRICES, LRP_ROLLOUT or LRP_CLS_ROW")
    L, B, h, S, _ = cam.shape
    out = torch.empty((B, L, S) if mode == LRP_CLS_ROW else (B, L, S, S), dtype=F32, device=cam.device)
    _call("xai_lrp_attn_matrices_f32", cam.device, _ptr(cam), _ptr(grad), L, B, h, S, int(mode), _ptr(out), lib="ext4")
    return out


# ------------------------------------------------------------------------------ quickshift superpixels (K53-K55; libxai_ext5.so)
def quickshift_lds_bytes(C, kernel_size):
    """The LDS bytes a workgroup of K53 / K54 stages; the entries refuse more than 65536 (include/xai_hip_ext5.h, THE CAP)"""
    return _lib.load("ext5").xai_quickshift_lds_bytes(int(C), float(kernel_size))


def quickshift_density(features, noise, kernel_size, out=None):
    """K53: features (B, H, W, C) fp64, noise (B, H, W) fp64 -> the densities (B, H, W) fp64, the tie noise added"""
    B, H, W, C = _bhwc(features, F64, "features")
    _need(features, F64, "features")
    _need(noise, F64, "noise")
    if tuple(noise.shape) != (B, H, W):
        raise ValueError(f"noise must be {(B, H, W)}, got {tuple(noise.shape)}")
    out = _out(out, "out", (B, H, W), features, dtype=F64)
    _call("xai_quickshift_density_f64", features.device, _ptr(features), _ptr(noise), B, H, W, C, float(kernel_size), _ptr(out), lib="ext5")
    return out


def quickshift_parent(features, dens, kernel_size, max_dist, want_tree=False):
    """K54: -> (parent (B, H, W) int32 with the max_dist cut, closest (B, H, W) fp64, dist = sqrt(closest), tree): tree is the
    parent before the cut (skimage's return_tree) with `want_tree`, else None"""
    B, H, W, C = _bhwc(features, F64, "features")
    _need(features, F64, "features")
    _need(dens, F64, "dens")
    if tuple(dens.shape) != (B, H, W):
        raise ValueError(f"dens must be {(B, H, W)}, got {tuple(dens.shape)}")
    parent = torch.empty((B, H, W), dtype=I32, device=features.device)
    tree = torch.empty_like(parent) if want_tree else None
    closest = torch.empty((B, H, W), dtype=F64, device=features.device)
    dist = torch.empty_like(closest)
    _call("xai_quickshift_parent_f64", features.device, _ptr(features), _ptr(dens), B, H, W, C, float(kernel_size), float(max_dist),
          _ptr(parent), _ptr(tree), _ptr(closest), _ptr(dist), lib="ext5")
    return parent, closest, dist, tree


def quickshift_labels(parent, labels=None):
    """K55: parent (B, H, W) int32 -> (labels (B, H, W) int32 = np.unique(roots, return_inverse=True)[1] per image, D (B,) int32)"""
    _need(parent, I32, "parent")
    if parent.dim() != 3 or parent.numel() == 0:
        raise ValueError(f"parent must be (B, H, W) with at least one element, got {tuple(parent.shape)}")
    B, H, W = parent.shape
    labels = _out(labels, "labels", (B, H, W), parent, dtype=I32)
    D = torch.empty((B,), dtype=I32, device=parent.device)
    ws, _ = _workspace("xai_quickshift_workspace_bytes", parent.device, B, H, W, lib="ext5")
    if ws is None:                                         # 0 bytes: a shape the entry refuses; it says how, given an address
        ws = torch.empty(4, dtype=U8, device=parent.device)
    _call("xai_quickshift_labels_i32", parent.device, _ptr(parent), B, H, W, _ptr(labels), _ptr(D), _ptr(ws), ws.numel(), lib="ext5")
    return labels, D


# ------------------------------------------------------------------------------ complete linkage (K56-K57; libxai_ext6.so)
LINKAGE_OK, LINKAGE_NONFINITE, LINKAGE_BOUND = 0, 1, 2       # info[0] of K56 / K57 (XAI_LINKAGE_*)


def linkage_max_n():
    """The largest n K56 / K57 take (include/xai_hip_ext6.h, THE CAP)"""
    return _lib.load("ext6").xai_linkage_max_n()


def _linkage_n(distance):
    _typed(distance, F32, "distance")
    if distance.dim() != 2 or distance.shape[0] != distance.shape[1]:
        raise ValueError(f"distance must be (n, n), got {tuple(distance.shape)}")
    n = int(distance.shape[0])
    if n < 2:
        raise ValueError(f"distance must be (n, n) with n >= 2, got n = {n}")
    if n > linkage_max_n():
        raise ValueError(f"distance must be (n, n) with n <= {linkage_max_n()} (include/xai_hip_ext6.h, THE CAP), got n = {n}")
    _need(distance, F32, "distance")
    return n


def linkage_workspace(distance):
    """The scratch K56 fills and K57 reads: uint8, xai_linkage_workspace_bytes(n) bytes"""
    n = _linkage_n(distance)
    return _workspace("xai_linkage_workspace_bytes", distance.device, n, lib="ext6")[0]


def linkage_complete(distance, ws, info, lanes=0):
    """K56: distance (n, n) fp32, only i < j read -> the merges in the chain's order inside `ws`, info (4,) int32 = [status, row
    scans, pushes, merges].  `lanes`: 64, 256 or 1024 lanes in the chain's one workgroup, 0 = the library's default."""
    n = _linkage_n(distance)
    _need(ws, U8, "ws")
    _need(info, I32, "info")
    if info.numel() != 4:
        raise ValueError("info must hold 4 int32")
    if int(lanes) not in (0, 64, 256, 1024):
        raise ValueError(f"lanes must be 0, 64, 256 or 1024, got {lanes!r}")
    _call("xai_linkage_complete_f32", distance.device, _ptr(distance), n, _ptr(ws), ws.numel(), _ptr(info), int(lanes), lib="ext6")
    return info


def linkage_sort_relabel(n, ws, children, heights, info):
    """K57: the merges in `ws` -> children (n - 1, 2) int32 and heights (n - 1,) fp32, sklearn's children_ and distances_"""
    n = int(n)
    _need(ws, U8, "ws")
    _need(children, I32, "children")
    _need(heights, F32, "heights")
    _need(info, I32, "info")
    if children.numel() != 2 * (n - 1) or heights.numel() != n - 1 or info.numel() != 4:
        raise ValueError(f"children, heights and info must hold {2 * (n - 1)}, {n - 1} and 4 elements")
    _call("xai_linkage_sort_relabel_i32", ws.device, n, _ptr(ws), ws.numel(), _ptr(children), _ptr(heights), _ptr(info), lib="ext6")
    return children, heights


# ------------------------------------------------------------------------------ k-means (K58-K61; libxai_ext7.so)
KMEANS_STATE_WORDS = 6                                       # state: iterations, done, status, 0, err (a double in words 4 and 5)
KMEANS_OK, KMEANS_BAD_INDEX = 0, 1                           # state[2] (XAI_KMEANS_*)


def kmeans_limits():
    """(the most points, features, clusters) K58-K61 take (include/xai_hip_ext7.h, THE LIMITS)"""
    lib = _lib.load("ext7")
    return lib.xai_kmeans_max_points(), lib.xai_kmeans_max_features(), lib.xai_kmeans_max_clusters()


def _kmeans_extents(points, k):
    """points (n, d) fp32 contiguous on a HIP device and 1 <= k <= n inside THE LIMITS -> (n, d, k); the one check of every wrapper"""
    _typed(points, F32, "points")
    if points.dim() != 2 or points.shape[0] < 1 or points.shape[1] < 1:
        raise ValueError(f"points must be (n, d) with n, d >= 1, got {tuple(points.shape)}")
    n, d = int(points.shape[0]), int(points.shape[1])
    if not 1 <= _int(k, "n_clusters") <= n:
        raise ValueError(f"n_clusters must be in [1, n = {n}], got {k}")
    cap = kmeans_limits()
    if n > cap[0] or d > cap[1] or k > cap[2]:
        raise ValueError(f"(n, d, k) = ({n}, {d}, {k}) is over THE LIMITS {cap} (include/xai_hip_ext7.h)")
    if not points.is_contiguous():                         # said here, ahead of _need: the device is reported last
        raise ValueError("points must be contiguous")
    _need(points, F32, "points")
    return n, d, k


def _kmeans_buffers(points, n, d, k, C, ws, state, assign=None, counts=None):
    for t, dtype, name, numel in ((C, F32, "C", k * d), (state, I32, "state", KMEANS_STATE_WORDS), (assign, I32, "assign", n),
                                  (counts, I32, "counts", k)):
        if t is not None:
            _need(t, dtype, name)
            if t.numel() != numel or t.device != points.device:
                raise ValueError(f"{name} must hold {numel} elements on the device of points")
    _workspace("xai_kmeans_workspace_bytes", points.device, n, d, k, lib="ext7", ws=_typed(ws, U8, "ws"),
               wrong="ws must be kmeans_workspace(points, k) on the device of points")


def kmeans_workspace(points, k):
    """The scratch of K58-K61 (e_j, xx_i, cc_j): uint8, xai_kmeans_workspace_bytes(n, d, k) bytes"""
    n, d, k = _kmeans_extents(points, k)
    return _workspace("xai_kmeans_workspace_bytes", points.device, n, d, k, lib="ext7")[0]


def kmeans_init(points, first, C, ws, state):
    """K58: xx_i into `ws`, C (k, d) = points[first], cc_j, state zeroed.  first (k,) int64 on the device of points."""
    _need(first, I64, "first")
    n, d, k = _kmeans_extents(points, int(first.numel()))
    _kmeans_buffers(points, n, d, k, C, ws, state)
    if first.device != points.device:
        raise ValueError("first must be on the device of points")
    _call("xai_kmeans_init_f32", points.device, _ptr(points), _ptr(first), n, d, k, _ptr(C), _ptr(ws), ws.numel(), _ptr(state), lib="ext7")
    return C


def kmeans_assign(points, C, assign, ws, state):
    """K59: assign (n,) int32 = the first index of the maximal score against the centroids C (k, d); nothing when state[1] is set"""
    n, d, k = _kmeans_extents(points, int(C.shape[0]) if isinstance(C, torch.Tensor) and C.dim() == 2 else 0)
    _kmeans_buffers(points, n, d, k, C, ws, state, assign)
    _call("xai_kmeans_assign_f32", points.device, _ptr(points), n, d, k, _ptr(C), _ptr(assign), _ptr(ws), ws.numel(), _ptr(state), lib="ext7")
    return assign


def _kmeans_stop(max_iter, tol):
    return _int(max_iter, "max_iter", 1), float(tol)


def kmeans_update(points, C, assign, counts, ws, state, max_iter, tol):
    """K60, K61: counts (k,) int32, C replaced by the new centroids, err, the iteration counter and `done` in state"""
    n, d, k = _kmeans_extents(points, int(C.shape[0]) if isinstance(C, torch.Tensor) and C.dim() == 2 else 0)
    _kmeans_buffers(points, n, d, k, C, ws, state, assign, counts)
    max_iter, tol = _kmeans_stop(max_iter, tol)
    _call("xai_kmeans_update_f32", points.device, _ptr(points), n, d, k, _ptr(C), _ptr(assign), _ptr(counts), _ptr(ws), ws.numel(),
          _ptr(state), max_iter, tol, lib="ext7")
    return C


def kmeans_iterate(points, C, assign, counts, ws, state, max_iter, tol, iterations):
    """`iterations` Lloyd iterations (K59, K60, K61 each) on the current stream, no read-back; those after the stop change nothing"""
    n, d, k = _kmeans_extents(points, int(C.shape[0]) if isinstance(C, torch.Tensor) and C.dim() == 2 else 0)
    _kmeans_buffers(points, n, d, k, C, ws, state, assign, counts)
    max_iter, tol = _kmeans_stop(max_iter, tol)
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 1 <= iterations <= max_iter:
        raise ValueError(f"iterations must be an int in [1, max_iter = {max_iter}], got {iterations!r}")
    _call("xai_kmeans_iterate_f32", points.device, _ptr(points), n, d, k, _ptr(C), _ptr(assign), _ptr(counts), _ptr(ws), ws.numel(),
          _ptr(state), max_iter, tol, iterations, lib="ext7")
    return C


# ------------------------------------------------------------------------------ SLIC superpixels (K65-K68; libxai_slic.so)
SLIC_UNCOVERED, SLIC_EMPTY, SLIC_IRREGULAR = 1, 2, 4         # the bits of status[b] (XAI_SLIC_*)


def slic_limits():
    """(the most clusters, channels, pixels of an image) K65-K68 take (include/xai_hip_slic.h, THE LIMITS)"""
    lib = _lib.load("slic")
    return lib.xai_slic_max_clusters(), lib.xai_slic_max_channels(), lib.xai_slic_max_pixels()


def _slic_shape(features, name="features"):
    """features (B, H, W, C) float32 or float64, contiguous, on a HIP device, inside THE LIMITS -> (B, H, W, C)"""
    B, H, W, C = _bhwc(features, (F32, F64), name)
    cap = slic_limits()
    if C > cap[1] or H * W > cap[2] or B > 65535 or H > 16 * 65535:
        raise ValueError(f"(B, H * W, C) = ({B}, {H * W}, {C}) is over THE LIMITS (65535, {cap[2]}, {cap[1]}), or H = {H} is over "
                         f"{16 * 65535} (include/xai_hip_slic.h)")
    _need(features, features.dtype, name)
    return B, H, W, C


def _slic_centres(centres, features, B, C):
    """centres (B, S, 2 + C) of the features' dtype on their device, 1 <= S <= the limit -> S"""
    _typed(centres, features.dtype, "centres")
    if centres.dim() != 3 or centres.shape[0] != B or centres.shape[1] < 1 or centres.shape[2] != 2 + C:
        raise ValueError(f"centres must be (B, S, 2 + C) = ({B}, S >= 1, {2 + C}), got {tuple(centres.shape)}")
    S = int(centres.shape[1])
    if S > slic_limits()[0]:
        raise ValueError(f"S = {S} clusters are over THE LIMITS ({slic_limits()[0]}) (include/xai_hip_slic.h)")
    _need(centres, features.dtype, "centres")
    if centres.device != features.device:
        raise ValueError("centres must be on the device of features")
    return S


def _slic_image_ints(t, name, like=None):
    """an int32 (B, H, W) device tensor (of the shape and device of `like`)"""
    _need(t, I32, name)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name} must be (B, H, W) with at least one element, got {tuple(t.shape)}")
    if like is not None and (tuple(t.shape) != tuple(like.shape[:3]) or t.device != like.device):
        raise ValueError(f"{name} must be {tuple(like.shape[:3])} on the device of features")
    return tuple(int(v) for v in t.shape)


def _slic_apart(a, b, name_a, name_b):
    """K67 and K68 read other pixels of their input while they write their output: the two may share no byte"""
    lo_a, lo_b = a.data_ptr(), b.data_ptr()
    if lo_a < lo_b + b.numel() * b.element_size() and lo_b < lo_a + a.numel() * a.element_size():
        raise ValueError(f"{name_a} must not overlap {name_b}")


def slic_clear(status):
    """status (B,) int32 = 0, by a kernel"""
    return _status("slic", _typed(status, I32, "status"))


def slic_assign(features, centres, step, labels=None, status=None):
    """K65: labels (B, H, W) int32 = the lowest k of the least distance among the clusters whose window holds the pixel, -1 and the
    UNCOVERED bit of status[b] where none does.  `status` None: a new, cleared word per image."""
    B, H, W, C = _slic_shape(features)
    S = _slic_centres(centres, features, B, C)
    step = _int(step, "step", 1)
    if labels is None:
        labels = torch.empty((B, H, W), dtype=I32, device=features.device)
    _slic_image_ints(labels, "labels", features)
    status = _status("slic", status, B, features.device)
    _call(f"xai_slic_assign_{_suffix(features)}", features.device, _ptr(features), _ptr(centres), B, H, W, C, S, step, _ptr(labels),
          _ptr(status), lib="slic")
    return labels, status


def slic_update(features, labels, centres, step, status=None):
    """K66: centres (B, S, 2 + C) replaced by the means of (y, x, features) over each cluster's pixels, summed sequentially in raster
    order; the EMPTY bit of status[b] for a cluster without a pixel (its centre becomes NaN)"""
    B, H, W, C = _slic_shape(features)
    S = _slic_centres(centres, features, B, C)
    step = _int(step, "step", 1)
    _slic_image_ints(labels, "labels", features)
    status = _status("slic", status, B, features.device)
    _call(f"xai_slic_update_{_suffix(features)}", features.device, _ptr(features), _ptr(labels), B, H, W, C, S, step, _ptr(centres),
          _ptr(status), lib="slic")
    return centres, status


def slic_iterate(features, centres, step, iterations, labels=None, status=None):
    """status cleared, then `iterations` times K65 and K66 on the current stream, no read-back -> (labels of the last assignment,
    status); centres is updated in place"""
    B, H, W, C = _slic_shape(features)
    S = _slic_centres(centres, features, B, C)
    step = _int(step, "step", 1)
    iterations = _int(iterations, "max_iter", 1)
    if labels is None:
        labels = torch.empty((B, H, W), dtype=I32, device=features.device)
    _slic_image_ints(labels, "labels", features)
    status = torch.empty(B, dtype=I32, device=features.device) if status is None else _status("slic", status, B, features.device)
    _call(f"xai_slic_iterate_{_suffix(features)}", features.device, _ptr(features), B, H, W, C, S, step, iterations, _ptr(centres),
          _ptr(labels), _ptr(status), lib="slic")
    return labels, status


def slic_workspace(labels):
    """The scratch of K67 and K68: uint8, xai_slic_workspace_bytes(B, H, W) bytes"""
    B, H, W = _slic_image_ints(labels, "labels")
    return _workspace("xai_slic_workspace_bytes", labels.device, B, H, W, lib="slic", required=True)[0]


_SLIC_WS = "ws must be slic_workspace(labels) on the device of labels"


def slic_components(labels, min_size, max_size, status=None, ws=None, comp=None):
    """K67: comp (B, H, W) int32 = the least flat index of each pixel's 4-connected component of equal label; the IRREGULAR bit of
    status[b] when a component's size is outside [min_size, max_size) or the sweeps ran out.  A given `comp` may not overlap labels."""
    B, H, W = _slic_image_ints(labels, "labels")
    min_size = _int(min_size, "min_size", 0)
    max_size = _int(max_size, "max_size", min_size)
    ws, _ = _workspace("xai_slic_workspace_bytes", labels.device, B, H, W, lib="slic", required=True, ws=ws, wrong=_SLIC_WS)
    comp = torch.empty_like(labels) if comp is None else comp
    _slic_image_ints(comp, "comp", labels)
    _slic_apart(comp, labels, "comp", "labels")
    status = _status("slic", status, B, labels.device)
    _call("xai_slic_components_i32", labels.device, _ptr(labels), B, H, W, min_size, max_size, _ptr(comp), _ptr(status), _ptr(ws),
          ws.numel(), lib="slic")
    return comp


def slic_number(comp, start_label=0, ws=None, out=None):
    """K68: (out (B, H, W) int32 = start_label + the rank of a component's first pixel among all first pixels, counts (B,) int32).
    A given `out` may not overlap comp."""
    B, H, W = _slic_image_ints(comp, "comp")
    if start_label not in (0, 1):
        raise ValueError("start_label should be 0 or 1.")
    ws, _ = _workspace("xai_slic_workspace_bytes", comp.device, B, H, W, lib="slic", required=True, ws=ws, wrong=_SLIC_WS)
    out = torch.empty_like(comp) if out is None else out
    _slic_image_ints(out, "out", comp)
    _slic_apart(out, comp, "out", "comp")
    counts = torch.empty(B, dtype=I32, device=comp.device)
    _call("xai_slic_number_i32", comp.device, _ptr(comp), B, H, W, int(start_label), _ptr(out), _ptr(counts), _ptr(ws), ws.numel(),
          lib="slic")
    return out, counts


# ------------------------------------------------------------------------------ Felzenszwalb segmentation (K69-K74; libxai_felz.so)
FELZ_NONFINITE, FELZ_INVARIANT = 1, 2                        # the bits of the status word (XAI_FELZ_*)


def felz_limits():
    """(the most pixels of an image, channels, scales per call, radius) K69-K74 take (include/xai_hip_felz.h, THE LIMITS)"""
    lib = _lib.load("felz")
    return lib.xai_felz_max_pixels(), lib.xai_felz_max_channels(), lib.xai_felz_max_scales(), lib.xai_felz_max_radius()


def felz_edges(H, W):
    """E of an H x W image: right, down, down-right and up-right edges"""
    return H * (W - 1) + (H - 1) * W + 2 * (H - 1) * (W - 1)


def _felz_image(image, name="image"):
    """image (B, H, W, C) float64, contiguous, on a HIP device, inside THE LIMITS -> (B, H, W, C)"""
    B, H, W, C = _bhwc(image, F64, name)
    cap = felz_limits()
    if H * W > cap[0] or C > cap[1] or B > 65535:
        raise ValueError(f"(B, H * W, C) = ({B}, {H * W}, {C}) is over THE LIMITS (65535, {cap[0]}, {cap[1]}) (include/xai_hip_felz.h)")
    _need(image, F64, name)
    return B, H, W, C


def felz_clear(status):
    """status (n,) int32 = 0, by a kernel"""
    return _status("felz", _typed(status, I32, "status"))


def felz_smooth(image, weights, axis):
    """K69: one axis (0 = rows, 1 = columns) of the symmetric correlate1d with reflected indices; weights (2 r + 1,) float64 on the
    device of image -> a new (B, H, W, C) float64 tensor"""
    B, H, W, C = _felz_image(image)
    _need(weights, F64, "weights")
    if weights.dim() != 1 or weights.numel() % 2 != 1 or weights.device != image.device:
        raise ValueError("weights must be (2 r + 1,) on the device of image")
    radius = weights.numel() // 2
    if radius > felz_limits()[3]:
        raise ValueError(f"the radius {radius} of the weights is over THE LIMITS ({felz_limits()[3]}) (include/xai_hip_felz.h)")
    if axis not in (0, 1):
        raise ValueError(f"axis must be 0 or 1, got {axis!r}")
    out = torch.empty_like(image)
    _call("xai_felz_smooth_f64", image.device, _ptr(image), _ptr(weights), radius, int(axis), B, H, W, C, _ptr(out), lib="felz")
    return out


def felz_costs(image, status=None):
    """K70: (keys (B, E) int64 = the bits of the costs, index (B, E) int32 = the edges' numbers, status (1,) int32).  The 1 x 1 image
    has no edge: its arrays hold one column that nothing reads or writes, so that they have an address."""
    B, H, W, C = _felz_image(image)
    E = felz_edges(H, W)
    status = _status("felz", status, 1, image.device, "one")
    keys = torch.empty((B, max(E, 1)), dtype=I64, device=image.device)
    index = torch.empty((B, max(E, 1)), dtype=I32, device=image.device)
    _call("xai_felz_costs_u64", image.device, _ptr(image), B, H, W, C, _ptr(keys), _ptr(index), _ptr(status), lib="felz")
    return keys, index, status


def felz_workspace(dev, B, H, W, S):
    """The scratch of K71-K73: uint8, xai_felz_workspace_bytes(B, H, W, S) bytes"""
    return _workspace("xai_felz_workspace_bytes", dev, B, H, W, S, lib="felz", required=True)[0]


_FELZ_WS = "ws must be felz_workspace(device, B, H, W, S) on the device of the keys"


def _felz_pairs(keys, index, H, W):
    _need(keys, I64, "keys")
    _need(index, I32, "index")
    if keys.dim() != 2 or keys.shape != index.shape or keys.shape[1] != max(felz_edges(H, W), 1) or keys.device != index.device:
        raise ValueError(f"keys and index must be (B, E = {felz_edges(H, W)}) on one device, got {tuple(keys.shape)} and "
                         f"{tuple(index.shape)}")
    return int(keys.shape[0])


def felz_sort(keys, index, H, W, S=1, ws=None):
    """K71 / K72: (keys, index) of every image sorted in place by key, equal keys by index (stable) -> (keys, index)"""
    B = _felz_pairs(keys, index, H, W)
    ws, _ = _workspace("xai_felz_workspace_bytes", keys.device, B, H, W, S, lib="felz", required=True, ws=ws, wrong=_FELZ_WS)
    _call("xai_felz_sort_u64", keys.device, _ptr(keys), _ptr(index), B, H, W, S, _ptr(ws), ws.numel(), lib="felz")
    return keys, index


def felz_merge(keys, order, scales, H, W, min_size, status=None, ws=None):
    """K73: the sorted (keys, order) of B images, scales (S,) float64 on their device (scale / 255) -> (roots (B, S, H, W) int32,
    stats (B, S, 2) int32 = edges tested and merged by the first walk, status)"""
    B = _felz_pairs(keys, order, H, W)
    _need(scales, F64, "scales")
    S = int(scales.numel())
    if scales.dim() != 1 or S < 1 or S > felz_limits()[2] or scales.device != keys.device:
        raise ValueError(f"scales must be (S,), 1 <= S <= {felz_limits()[2]}, on the device of the keys")
    min_size = _int(min_size, "min_size", 0)
    ws, _ = _workspace("xai_felz_workspace_bytes", keys.device, B, H, W, S, lib="felz", required=True, ws=ws, wrong=_FELZ_WS)
    status = _status("felz", status, 1, keys.device, "one")
    roots = torch.empty((B, S, H, W), dtype=I32, device=keys.device)
    stats = torch.empty((B, S, 2), dtype=I32, device=keys.device)
    _call("xai_felz_merge_f64", keys.device, _ptr(keys), _ptr(order), _ptr(scales), B, S, H, W, min_size, _ptr(roots),
          _ptr(stats), _ptr(status), _ptr(ws), ws.numel(), lib="felz")
    return roots, stats, status


def felz_labels(roots, status=None):
    """K74: roots (..., H, W) int32 -> (labels of the same shape = the rank of a pixel's root among the roots in pixel order,
    counts (...) int32 = the roots of every map, status)"""
    _need(roots, I32, "roots")
    if roots.dim() < 3 or roots.numel() == 0:
        raise ValueError(f"roots must be (..., H, W) with at least one element, got {tuple(roots.shape)}")
    n = int(roots.shape[-1] * roots.shape[-2])
    M = roots.numel() // n
    if n > felz_limits()[0]:
        raise ValueError(f"H * W = {n} is over THE LIMITS ({felz_limits()[0]}) (include/xai_hip_felz.h)")
    status = _status("felz", status, 1, roots.device, "one")
    labels = torch.empty_like(roots)
    counts = torch.empty(tuple(roots.shape[:-2]), dtype=I32, device=roots.device)
    _call("xai_felz_labels_i32", roots.device, _ptr(roots), M, n, _ptr(labels), _ptr(counts), _ptr(status), lib="felz")
    return labels, counts, status


# ------------------------------------------------------------------------------ CLIP: the class-token row (K75-K77, include/xai_clip.h)
CLIP_DTYPES = (F32, F16)


def clip_limits():
    """(XAI_CLIP_MAX_TOKENS, XAI_CLIP_MAX_WIDTH, XAI_CLIP_MAX_TEXTS) of the built library"""
    lib = _lib.load("clip")
    return lib.xai_clip_max_tokens(), lib.xai_clip_max_width(), lib.xai_clip_max_texts()


def _clip_tokens(t, name, like=None):
    """An (L, B, D) operand as the model produces it (the K or V third of the in-projection: any strides over L and B, the last
    axis contiguous) -> (L, B, D, stride of L, stride of B); `like`: an operand whose dtype, device and shape it must have."""
    _need(t, CLIP_DTYPES if like is None else like.dtype, name, rows=True)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name} must be (L, B, D), got {tuple(t.shape)}")
    L, B, D = t.shape
    if L < 2:
        raise ValueError(f"{name}: L = {L}; the class token and at least one patch are needed (L >= 2)")
    max_l, max_d, _ = clip_limits()
    if D > max_d or L > max_l:
        raise ValueError(f"{name}: D = {D}, L = {L} are over the limits of K75-K77 (D <= {max_d}, L <= {max_l}: a row of each in LDS)")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name} must have the shape and device of {tuple(like.shape)} on {like.device}")
    return L, B, D, t.stride(0), t.stride(1)


def _clip_rows(t, shape, like, name):
    """A dense operand of `shape` in the dtype and on the device of `like`"""
    _need(t, like.dtype, name)
    if tuple(t.shape) != tuple(shape) or t.device != like.device:
        raise ValueError(f"{name} must be {tuple(shape)} on {like.device}, got {tuple(t.shape)} on {t.device}")
    return t


def _clip_per_text(t, B, D, like, name):
    """A dense (B, T, D) operand in the dtype and on the device of `like` -> T"""
    _need(t, like.dtype, name)
    if t.dim() != 3 or t.shape[0] != B or t.shape[2] != D or t.device != like.device:
        raise ValueError(f"{name} must be ({B}, T, {D}) on {like.device}, got {tuple(t.shape)} on {t.device}")
    return int(t.shape[1])


def _clip_txt(txt, B, E, like):
    """txt (T, E), shared by the images, or (B, T, E), in the dtype and on the device of `like`: what a host can test of it, the
    caller's _need follows or went before -> (T, the stride from image to image: T * E, or 0 for shared texts)"""
    _typed(txt, like.dtype, "txt")
    if txt.dim() not in (2, 3) or txt.numel() == 0 or txt.shape[-1] != E or (txt.dim() == 3 and txt.shape[0] != B) \
            or txt.device != like.device:
        raise ValueError(f"txt must be (T, {E}) or ({B}, T, {E}) on {like.device}, got {tuple(txt.shape)} on {txt.device}")
    T = int(txt.shape[-2])
    return T, T * E if txt.dim() == 3 else 0


def _texts_within(T, limit, kernels):
    if not 1 <= T <= limit:
        raise ValueError(f"T = {T} texts: {kernels} take 1 .. {limit}")
    return T


def clip_cls_attention(q0, k, v, want_scores=False):
    """K75: q0 (B, D) the class row of q, k and v (L, B, D) -> (attn (B, L), att_out (B, D)) in the operands' dtype: row 0 of the
    one-head attention of generate_emap.py:288-307.  want_scores: a third result, the (B, L) scores in front of the softmax."""
    L, B, D, kl, kb = _clip_tokens(k, "k")
    _, _, _, vl, vb = _clip_tokens(v, "v", like=k)
    _clip_rows(q0, (B, D), k, "q0")
    attn = torch.empty((B, L), dtype=k.dtype, device=k.device)
    att_out = torch.empty((B, D), dtype=k.dtype, device=k.device)
    scores = torch.empty((B, L), dtype=k.dtype, device=k.device) if want_scores else None
    _call(f"xai_clip_cls_attention_{_suffix(k)}", k.device, _ptr(q0), _ptr(k), kl, kb, _ptr(v), vl, vb, B, L, D,
          float(D) ** -0.5, _ptr(scores), _ptr(attn), _ptr(att_out), lib="clip")
    return (attn, att_out, scores) if want_scores else (attn, att_out)


def clip_eclip_map(q_out0, k_out, v, grad_cls=None, texts=None, withksim=True, withgrad=True):
    """K76: q_out0 (B, D), k_out and v (L, B, D), grad_cls (B, T, D) (None without withgrad: then `texts` = T) -> (B, L - 1) fp32,
    grad_eclip of generate_emap.py:453-485 summed over the T texts."""
    L, B, D, vl, vb = _clip_tokens(v, "v")
    kl = kb = 0
    if withksim:
        _, _, _, kl, kb = _clip_tokens(k_out, "k_out", like=v)
        _clip_rows(q_out0, (B, D), v, "q_out0")
    if withgrad:
        texts = _clip_per_text(grad_cls, B, D, v, "grad_cls")
    elif texts is None:
        raise TypeError("clip_eclip_map: without withgrad there is no grad_cls to count the texts; pass texts=T")
    T = _texts_within(int(texts), clip_limits()[2], "K76 and K77")
    out = torch.empty((B, L - 1), dtype=F32, device=v.device)
    _call(f"xai_clip_eclip_map_{_suffix(v)}", v.device, _ptr(q_out0) if withksim else None, _ptr(k_out) if withksim else None, kl, kb,
          _ptr(v), vl, vb, _ptr(grad_cls) if withgrad else None, B, L, D, T, int(bool(withksim)), int(bool(withgrad)), _ptr(out),
          lib="clip")
    return out


def clip_maskclip_map(v_final, txt, k_out):
    """K77: v_final (B, L - 1, E), txt (T, E) shared or (B, T, E), k_out (L, B, D) -> (B, L - 1) fp32, mask_clip of
    generate_emap.py:500-529 summed over the T texts."""
    L, B, D, kl, kb = _clip_tokens(k_out, "k_out")
    _need(v_final, k_out.dtype, "v_final")
    if v_final.dim() != 3 or tuple(v_final.shape[:2]) != (B, L - 1) or v_final.shape[2] < 1 or v_final.device != k_out.device:
        raise ValueError(f"v_final must be ({B}, {L - 1}, E) on {k_out.device}, got {tuple(v_final.shape)} on {v_final.device}")
    E = v_final.shape[2]
    if E > clip_limits()[1]:
        raise ValueError(f"v_final: E = {E} is over the limit of K77 (E <= {clip_limits()[1]})")
    T, txt_ld = _clip_txt(_need(txt, k_out.dtype, "txt"), B, E, k_out)
    _texts_within(T, clip_limits()[2], "K76 and K77")
    out = torch.empty((B, L - 1), dtype=F32, device=k_out.device)
    _call(f"xai_clip_maskclip_map_{_suffix(k_out)}", k_out.device, _ptr(v_final), _ptr(txt), txt_ld,
          _ptr(k_out), kl, kb, B, L, D, E, T, _ptr(out), lib="clip")
    return out


# ------------------------------------------------------------------------------ CLIP: the attention rows (K82-K85, include/xai_cattn.h)
def cattn_limits():
    """(XAI_CATTN_MAX_TOKENS, XAI_CATTN_MAX_WIDTH, XAI_CATTN_MAX_TEXTS) of the built library"""
    lib = _lib.load("cattn")
    return lib.xai_cattn_max_tokens(), lib.xai_cattn_max_width(), lib.xai_cattn_max_texts()


def _cattn_rows(t, name, like=None):
    """The class-token rows a0 (B, H, L) of every head's attention, dense -> (B, H, L); `like`: an operand whose dtype and device it has"""
    _typed(t, CLIP_DTYPES if like is None else like.dtype, name)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name} must be (B, H, L), got {tuple(t.shape)}")
    B, H, L = t.shape
    max_l, max_d, _ = cattn_limits()
    if L < 2 or L > max_l or H > max_d:
        raise ValueError(f"{name}: L = {L}, H = {H}; K82 and K83 take 2 <= L <= {max_l} and H <= {max_d}")
    _need(t, t.dtype, name)
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} must be on {like.device}, got {t.device}")
    return B, H, L


def clip_game_map(g, v, a0):
    """K82: g (B, T, D) the gradients of the T logits with respect to row 0 of the last block's attention output, v (L, B, D), a0
    (B, H, L) the class-token row of every head -> (B, L - 1) fp32, mm_interpret of generate_emap.py:133-174 summed over the texts."""
    L, B, D, vl, vb = _clip_tokens(v, "v")
    _, H, _ = _cattn_rows(a0, "a0", like=v)
    if tuple(a0.shape) != (B, H, L) or D % H:
        raise ValueError(f"a0 must be ({B}, H, {L}) with H dividing D = {D}, got {tuple(a0.shape)}")
    T = _texts_within(_clip_per_text(g, B, D, v, "g"), cattn_limits()[2], "K82 and K83")
    out = torch.empty((B, L - 1), dtype=F32, device=v.device)
    _call(f"xai_cattn_game_map_{_suffix(v)}", v.device, _ptr(g), _ptr(v), vl, vb, _ptr(a0), B, L, D, H, T, _ptr(out), lib="cattn")
    return out


def clip_rollout_row(a0, texts=1):
    """K83: a0 (B, H, L) -> (B, L - 1) fp32, the rollout row of compute_rollout_attention (generate_emap.py:269-285) on the one matrix
    mm_interpret(rollout=True) hands it; `texts`: how often the reference repeats the image in its batch."""
    _int(texts, "texts")
    B, H, L = _cattn_rows(a0, "a0")
    T = _texts_within(texts, cattn_limits()[2], "K82 and K83")
    out = torch.empty((B, L - 1), dtype=F32, device=a0.device)
    _call(f"xai_cattn_rollout_row_{_suffix(a0)}", a0.device, _ptr(a0), B, H, L, T, _ptr(out), lib="cattn")
    return out


def clip_lrp_matrices(attn, grad, out=None):
    """K84: attn and grad (n, B, H, L, L) -> c (B, n, L, L) in their dtype, mean over the heads of clamp(grad * attn, min=0)
    (generate_emap.py:231-237).  `out`: the caller's buffer for c."""
    _typed(attn, CLIP_DTYPES, "attn")
    if attn.dim() != 5 or attn.numel() == 0 or attn.shape[3] != attn.shape[4]:
        raise ValueError(f"attn must be (n, B, H, L, L), got {tuple(attn.shape)}")
    n, B, H, L, _ = attn.shape
    max_l, max_d, _ = cattn_limits()
    if L < 2 or L > max_l or H > max_d or n * B > 65535:
        raise ValueError(f"attn: L = {L}, H = {H}, n * B = {n * B}; K84 takes 2 <= L <= {max_l}, H <= {max_d} and n * B <= 65535")
    _need(attn, attn.dtype, "attn")
    _need(grad, attn.dtype, "grad")
    if grad.shape != attn.shape or grad.device != attn.device:
        raise ValueError(f"grad must have the shape and device of attn, {tuple(attn.shape)} on {attn.device}")
    c = _out(out, "out", (B, n, L, L), attn, dtype=attn.dtype)
    if c.device != attn.device:
        raise ValueError(f"out must be on {attn.device}")
    _call(f"xai_cattn_lrp_matrices_{_suffix(attn)}", attn.device, _ptr(attn), _ptr(grad), n, B, H, L, _ptr(c), lib="cattn")
    return c.view(B, n, L, L)


def clip_lrp_row(c):
    """K85: c (B, n, L, L) as K84 writes it -> (B, L - 1) fp32, row 0 of the relevance R of clip_lrp (generate_emap.py:226-239) without
    its first column, by n vector-matrix products from the last block down."""
    _typed(c, CLIP_DTYPES, "c")
    if c.dim() != 4 or c.numel() == 0 or c.shape[2] != c.shape[3]:
        raise ValueError(f"c must be (B, n, L, L), got {tuple(c.shape)}")
    B, n, L, _ = c.shape
    if L < 2 or L > cattn_limits()[0] or n * B > 65535:
        raise ValueError(f"c: L = {L}, n * B = {n * B}; K85 takes 2 <= L <= {cattn_limits()[0]} and n * B <= 65535")
    _need(c, c.dtype, "c")
    out = torch.empty((B, L - 1), dtype=F32, device=c.device)
    _call(f"xai_cattn_lrp_row_{_suffix(c)}", c.device, _ptr(c), n, B, L, _ptr(out), lib="cattn")
    return out


# ------------------------------------------------------------------------------ CLIP Surgery (K86-K87, include/xai_csurg.h)
def csurg_limits():
    """(XAI_CSURG_MAX_TOKENS, XAI_CSURG_MAX_WIDTH, XAI_CSURG_MAX_TEXTS, XAI_CSURG_LDS_FLOATS, XAI_CSURG_VV_WAVES) of the built library"""
    lib = _lib.load("csurg")
    return (lib.xai_csurg_max_tokens(), lib.xai_csurg_max_width(), lib.xai_csurg_max_texts(), lib.xai_csurg_lds_floats(),
            lib.xai_csurg_vv_waves())


def clip_vv_attention(v, heads, want_scores=False):
    """K86: v (n, L, B, D) fp32, the V third of n blocks' in-projections where it lies (any strides over n, L and B, the last axis
    contiguous), `heads` = H -> out (n, B, L, D) fp32, per block, image and head softmax((v @ v.T) * d ** -0.5) @ v with d = D / H,
    laid out as the reference's (attn @ v).transpose(1, 2).reshape(B, N, C) (clip_surgery_model.py:82-99).  want_scores: a second
    result, the (n, B, H, L, L) scores in front of the softmax."""
    _typed(v, F32, "v")
    H = _int(heads, "heads", least=1)
    if v.dim() != 4 or v.numel() == 0:
        raise ValueError(f"v must be (n, L, B, D), got {tuple(v.shape)}")
    n, L, B, D = v.shape
    if L < 2 or D % H:
        raise ValueError(f"v: L = {L}, D = {D}, heads = {H}; K86 takes L >= 2 and heads dividing D")
    max_l, max_d, _, lds, waves = csurg_limits()
    d = D // H
    if L > max_l or D > max_d or L * (d + 1 + waves) > lds or n * B > 65535 or B > 65535 or H > 65535:
        raise ValueError(f"v: L = {L}, D = {D}, d = {d}, n * B = {n * B} are over the limits of K86 (L <= {max_l}, D <= {max_d}, "
                         f"L * (d + {1 + waves}) <= {lds}: one head's V and a row per wave in LDS, n * B <= 65535)")
    _need(v, F32, "v", rows=True)
    out = torch.empty((n, B, L, D), dtype=F32, device=v.device)
    scores = torch.empty((n, B, H, L, L), dtype=F32, device=v.device) if want_scores else None
    _call("xai_csurg_vv_attention_f32", v.device, _ptr(v), v.stride(0), v.stride(1), v.stride(2), n, B, L, D, H, float(d) ** -0.5,
          _ptr(scores), _ptr(out), lib="csurg")
    return (out, scores) if want_scores else out


def clip_surgery_similarity(features, txt, texts_out=1, want_weights=False):
    """K87: features (B, L, E) fp32 as ln_post and the projection leave them (not normalised), txt (T, E) shared or (B, T, E) ->
    (B, texts_out, L - 1) fp32: the reference's division by the norm over the tokens (generate_emap.py:121), clip_feature_surgery
    (clip.py:287-308) in closed form and the min-max of get_similarity_map (clip.py:274), for the first texts_out texts.
    want_weights: a second result, the (B, T) weights w of clip_feature_surgery."""
    _typed(features, F32, "features")
    if features.dim() != 3 or features.numel() == 0:
        raise ValueError(f"features must be (B, L, E), got {tuple(features.shape)}")
    B, L, E = features.shape
    if L < 2:
        raise ValueError(f"features: L = {L}; the class token and at least one patch are needed (L >= 2)")
    T, txt_ld = _clip_txt(txt, B, E, features)
    T_out = _int(texts_out, "texts_out", least=1)
    if T_out > T:
        raise ValueError(f"texts_out = {T_out} of T = {T} texts")
    max_l, max_e, max_t, lds, _ = csurg_limits()
    if L > max_l or E > max_e or T > max_t or 2 * E + T > lds or B > 65535:
        raise ValueError(f"features, txt: L = {L}, E = {E}, T = {T} are over the limits of K87 (L <= {max_l}, E <= {max_e}, T <= {max_t}, "
                         f"2 * E + T <= {lds})")
    _need(features, F32, "features")
    _need(txt, F32, "txt")
    out = torch.empty((B, T_out, L - 1), dtype=F32, device=features.device)
    w = torch.empty((B, T), dtype=F32, device=features.device) if want_weights else None
    _call("xai_csurg_similarity_map_f32", features.device, _ptr(features), _ptr(txt), txt_ld, B, L, E, T, T_out,
          _ptr(w), _ptr(out), lib="csurg")
    return (out, w) if want_weights else out


# ------------------------------------------------------------------------------ CLIP M2IB (K88-K90, include/xai_hip_cm2ib.h)
def cm2ib_limits():
    """(XAI_CM2IB_MAX_TOKENS, XAI_CM2IB_MAX_WIDTH, XAI_CM2IB_MAX_COPIES) of the built library"""
    lib = _lib.load("cm2ib")
    return lib.xai_cm2ib_max_tokens(), lib.xai_cm2ib_max_width(), lib.xai_cm2ib_max_copies()


def _m2ib_operands(alpha, x9, eps, least_tokens=1, more=()):
    """The checks K88-K90 share, the device last: alpha (B, L, D) fp32, x9 of its shape in fp32 or fp16, eps (None: absent)
    (B, R, L, D) fp32, and `more`: (tensor, name, dtype, the tensor whose shape it must have, the words for that) -> (B, R, L, D),
    R = 1 without eps"""
    _typed(alpha, F32, "alpha")
    if alpha.dim() != 3 or alpha.numel() == 0:
        raise ValueError(f"alpha must be (B, L, D), got {tuple(alpha.shape)}")
    B, L, D = alpha.shape
    if L < least_tokens:
        raise ValueError(f"alpha: L = {L}; the class token and at least one patch are needed (L >= {least_tokens})")
    _typed(x9, (F32, F16), "x9")
    if x9.shape != alpha.shape:
        raise ValueError(f"x9 must be ({B}, {L}, {D}) like alpha, got {tuple(x9.shape)}")
    R = 1
    if eps is not None:
        _typed(eps, F32, "eps")
        if eps.dim() != 4 or eps.numel() == 0 or (eps.shape[0], *eps.shape[2:]) != (B, L, D):
            raise ValueError(f"eps must be ({B}, R, {L}, {D}), got {tuple(eps.shape)}")
        R = int(eps.shape[1])
    for t, name, dtype, like, wrong in more:
        _typed(t, dtype, name)
        if t.shape != like.shape:
            raise ValueError(f"{name} must {wrong}, got {tuple(t.shape)}")
    max_l, max_d, max_r = cm2ib_limits()
    if L > max_l or D > max_d or R > max_r or B > 65535:
        raise ValueError(f"B = {B}, R = {R}, L = {L}, D = {D} are over the limits of K88-K90 (B <= 65535, R <= {max_r}, L <= {max_l}, "
                         f"D <= {max_d})")
    for t, name in ((alpha, "alpha"), (x9, "x9"), (eps, "eps")) + tuple(m[:2] for m in more):
        if t is not None:
            _need(t, t.dtype, name)
            if t.device != alpha.device:
                raise ValueError(f"{name} must be on {alpha.device}, got {t.device}")
    return B, R, L, D


def m2ib_sample(alpha, x9, eps):
    """K88: alpha (B, L, D) fp32, x9 (B, L, D) in the model's dtype T (fp32 or fp16), eps (B, R, L, D) fp32 -> t (B, R, L, D) of T:
    the sample of M2IB's information bottleneck, sigmoid(alpha) * x9 + (1 - sigmoid(alpha)) * eps in the reference's sequence
    (iba.py:104-108, :122-127), rounded to T once."""
    if eps is None:
        raise TypeError("eps: expected a torch.Tensor, got NoneType")
    B, R, L, D = _m2ib_operands(alpha, x9, eps)
    t = torch.empty((B, R, L, D), dtype=x9.dtype, device=alpha.device)
    _call(f"xai_cm2ib_sample_{_suffix(x9)}", alpha.device, _ptr(alpha), _ptr(x9), _ptr(eps), B, R, L, D, _ptr(t), lib="cm2ib")
    return t


def m2ib_adam_step(gt, eps, x9, alpha, m, v, beta, w1, b2, w2, bc2s, step_size, adam_eps):
    """K89, in place: gt (B, R, L, D) of x9's dtype, dL/dt of the R copies; eps (B, R, L, D) fp32, the noise K88 was given; x9, alpha as
    for K88; m, v (B, L, D) fp32, Adam's moments.  Forms the gradient autograd gives the reference's alpha (the fitting part from gt,
    the compression part beta / (L * D) * d capacity / d alpha) and takes one step of torch's single-tensor Adam with the host-made
    scalars of the step (m2ib.adam_scalars) -> alpha"""
    if eps is None:
        raise TypeError("eps: expected a torch.Tensor, got NoneType")
    _typed(x9, (F32, F16), "x9")
    B, R, L, D = _m2ib_operands(alpha, x9, eps, more=((gt, "gt", x9.dtype, eps, "have the shape of eps"),
                                                      (m, "m", F32, alpha, "have the shape of alpha"),
                                                      (v, "v", F32, alpha, "have the shape of alpha")))
    _call(f"xai_cm2ib_adam_step_{_suffix(x9)}", alpha.device, _ptr(gt), _ptr(eps), _ptr(x9), B, R, L, D, float(beta), float(w1), float(b2),
          float(w2), float(bc2s), float(step_size), float(adam_eps), _ptr(alpha), _ptr(m), _ptr(v), lib="cm2ib")
    return alpha


def m2ib_saliency(alpha, x9, want_capacity=False):
    """K90: alpha, x9 (B, L, D) fp32 -> (B, L - 1) fp32, per patch token the nansum over D of the bottleneck's capacity
    -0.5 * (1 + log(var) - mu ** 2 - var) (iba.py:111-114, :154).  want_capacity: a second result, the (B, L, D) capacities."""
    _typed(x9, F32, "x9")
    B, _, L, D = _m2ib_operands(alpha, x9, None, least_tokens=2)
    out = torch.empty((B, L - 1), dtype=F32, device=alpha.device)
    cap = torch.empty((B, L, D), dtype=F32, device=alpha.device) if want_capacity else None
    _call("xai_cm2ib_saliency_f32", alpha.device, _ptr(alpha), _ptr(x9), B, L, D, _ptr(cap), _ptr(out), lib="cm2ib")
    return (out, cap) if want_capacity else out
