"""Transformer Attribution (`t_attr`; Chefer et al.'s LRP-based ViT explainer) on the HIP engine: the reference's
`LRP(model).generate_LRP` (util/attribution_methods/VIT_LRP/ViT_explanation_generator.py:107-133) with its relevance pass in closed form.

The reference keeps a second, timm-derived "LRP model" whose layers carry a `relprop` (ViT_LRP_timm.py, util/layers_ours.py) and pays
for each of them with a torch.autograd.grad call and a dozen small torch kernels.  `generate_LRP` hard-codes alpha = 1, which leaves:

  Linear   Z = clamp(X,min=0) @ clamp(W,min=0)^T + clamp(X,max=0) @ clamp(W,max=0)^T;  S = safe_divide(R, Z);
           C = clamp(X,min=0) * (S @ clamp(W,min=0)) + clamp(X,max=0) * (S @ clamp(W,max=0))            (layers_ours.py:213-236)
  einsum   S = safe_divide(R, A @ V);  cam_A = A * (S @ V^T) / 2;  cam_V = V * (A^T @ S) / 2; the same for Q K^T (ViT_LRP_timm.py:355-378)
  Add      a = X0 * S, b = X1 * S, S = safe_divide(R, X0 + X1), rescaled with a.sum(), b.sum(), R.sum()     (layers_ours.py:100-125)
  Clone    X * (safe_divide(r1, X) + safe_divide(r2, X))                                                    (layers_ours.py:157-175)
  LayerNorm, GELU, softmax, dropout: the relevance passes unchanged                                         (layers_ours.py:45-46)

so there is no second model and no autograd inside the pass: it runs on the engine's hooked ViT (`zoo.VisionTransformer`, or any
model of that layout), forward hooks record the tensors the rules read, the GEMMs are torch.matmul (rocBLAS) and what lies between
two GEMMs is one launch of K46-K52 (include/xai_hip_ext4.h).  The clamped weight pairs are made once per model and cached
(`clear_cache()` frees them; they double the weight memory).  The pass stops where nothing below is read: `last_layer` ends inside the
last block, `start_layer = s` inside block s.

Deliberate divergences from the reference:
  (a) the inhibitor term of Linear.relprop, which the reference computes and multiplies by beta = 0, is not computed; the results
      differ only where that term would be non-finite (0 * Inf = NaN in the reference);
  (b) the three global sums of Add.relprop are fp64 sums in a fixed order (xai_hip_ext4.h), not torch's fp32 sums;
  (c) the head mean of the attention matrices is an ascending sum divided by the number of heads (K52), not torch's mean();
  (d) method "full" raises NotImplementedError: in the reference it raises AttributeError (the model has no `self.add`);
  (e) a negative start_layer raises IndexError; the reference starts its rollout at block depth + start_layer and then multiplies
      by every block from 0 again;
  (f) the caller's `input.requires_grad` is not mutated and `model.zero_grad()` is not called (nothing here accumulates into .grad).
"""
import numpy as np
import torch

from . import kernels as K
from .ig import check_input, class_targets, hip_device
from .streams import GRAD_RTOL, CapturedCall, ThreadGraphs, backward_turn

LRP_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0}
_PASSES = ThreadGraphs(limit=4)

METHODS = ("transformer_attribution", "grad", "rollout", "last_layer", "second_layer", "last_layer_attn")
_REFUSED = {"full": 'method "full" is not implemented: the reference raises AttributeError here (its model has no `self.add`)',
            "InFlow": 'method "InFlow" is not implemented on the relevance pass; Baselines.generate_RAVE serves the InFlow row'}

_BLOCK_LAYOUT = ("norm1", "attn.qkv", "attn.proj", "attn.get_attention_map", "attn.get_attn_gradients", "norm2", "mlp.fc1", "mlp.act",
                 "mlp.fc2")


def check_layout(model):
    """The layout the pass reads -- patch_embed, blocks[i].{norm1, attn.{qkv, proj}, norm2, mlp.{fc1, act, fc2}}, norm, head and the
    attention-map / attention-gradient accessors -- or a TypeError naming what is missing."""
    def need(obj, path, where):
        for name in path.split("."):
            if not hasattr(obj, name):
                raise TypeError(f"LRP needs a ViT of the engine's layout: {type(model).__name__} has no `{where}{path}`")
            obj = getattr(obj, name)
    for path in ("patch_embed", "blocks", "norm", "head"):
        need(model, path, "")
    if len(model.blocks) == 0:
        raise TypeError(f"LRP needs a ViT of the engine's layout: {type(model).__name__} has no `blocks[0]`")
    for i, blk in enumerate(model.blocks):
        for path in _BLOCK_LAYOUT:
            need(blk, path, f"blocks[{i}].")


def check_method(method):
    if method in _REFUSED:
        raise NotImplementedError(_REFUSED[method])
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {', '.join(METHODS)}")


def blocks_needed(method, depth, start_layer):
    """The blocks whose attn_cam the method reads, ascending (the pass stops inside the lowest); IndexError where the reference's
    indexing raises one."""
    if method in ("transformer_attribution", "grad", "rollout"):
        if not 0 <= start_layer < depth:
            raise IndexError(f"index {start_layer} is out of bounds for dimension 0 with size {depth}")
        return list(range(start_layer, depth))
    if method == "last_layer":
        return [depth - 1]
    if method == "second_layer":
        if depth < 2:
            raise IndexError("index 1 is out of range")
        return [1]
    return []


def needs_gradients(method, withgrad, is_ablation):
    return (method in ("transformer_attribution", "grad") and withgrad) or (method in ("last_layer", "second_layer") and is_ablation)


# ------------------------------------------------------------------------------------------------ the forward tensors
class Tape:
    """Forward hooks on the submodules record, detached, what relprop reads: per block `x_in` (the block's input: Clone 1, Add 1),
    `n1` (qkv's X), `qkv` (its output: q, k, v), `pv` (proj's X), `attn_out` (Add 1), `x_mid` (norm2's input: Clone 2, Add 2), `n2`
    (fc1's X), `g` (fc2's X), `mlp_out` (Add 2); `norm_out` (IndexSelect's X) and `head_in`."""

    def __init__(self, model):
        self.model, self.blocks, self.top, self._handles = model, [dict() for _ in model.blocks], {}, []

    def _pre(self, module, store, key):
        self._handles.append(module.register_forward_pre_hook(lambda m, args: store.__setitem__(key, args[0].detach())))

    def _post(self, module, store, key):
        self._handles.append(module.register_forward_hook(lambda m, args, out: store.__setitem__(key, out.detach())))

    def __enter__(self):
        for blk, rec in zip(self.model.blocks, self.blocks):
            self._pre(blk, rec, "x_in")
            self._pre(blk.attn.qkv, rec, "n1")
            self._post(blk.attn.qkv, rec, "qkv")
            self._pre(blk.attn.proj, rec, "pv")
            self._post(blk.attn, rec, "attn_out")
            self._pre(blk.norm2, rec, "x_mid")
            self._pre(blk.mlp.fc1, rec, "n2")
            self._pre(blk.mlp.fc2, rec, "g")
            self._post(blk.mlp, rec, "mlp_out")
        self._post(self.model.norm, self.top, "norm_out")
        self._pre(self.model.head, self.top, "head_in")
        return self

    def __exit__(self, *exc):
        for h in self._handles:
            h.remove()
        self._handles = []


def record(model, x, targets, gradients):
    """One forward of the hooked ViT under a Tape and, for `gradients`, one backward of the target logits (the sum over the batch:
    every image's attention gradient is its own) -> (tape, targets (B,) int64, attention maps, attention gradients or None).
    targets None: the argmax, on the device."""
    x0 = x.detach().requires_grad_(True) if gradients else x.detach()
    with Tape(model) as tape, torch.set_grad_enabled(gradients):
        out = model(x0, register_hook=True) if gradients else model(x0)
    tgt = out.detach().argmax(dim=1) if targets is None else targets
    grads = None
    if gradients:
        score = out.gather(1, tgt.view(-1, 1)).sum()
        if score.is_cuda:
            with backward_turn(score.device):
                score.backward()
        else:
            score.backward()
        grads = [blk.attn.get_attn_gradients() for blk in model.blocks]
    attns = [blk.attn.get_attention_map().detach() for blk in model.blocks]
    tape.logits = out.detach()
    return tape, tgt, attns, grads


def record_per_image(model, x, targets, gradients):
    """`record` image by image, the recorded tensors concatenated along the image axis.  The classifier folds a batch into the rows of
    its GEMMs, rocBLAS picks its kernel by the row count, and another kernel is another order of summation: an image's forward tensors
    would depend on how many images share its batch.  The relevance pass divides by sums that cancel and amplifies such last-bit
    differences a thousandfold and more (the reference's own fp32 result lies up to 1.6e-2 from its fp64 result), so the classifier
    runs on each image alone, as in the image's own one-image call."""
    B = x.shape[0]
    if B == 1:
        return record(model, x, targets, gradients)
    parts = [record(model, x[j:j + 1], None if targets is None else targets[j:j + 1], gradients) for j in range(B)]
    tape = parts[0][0]
    for i, rec in enumerate(tape.blocks):
        for key in rec:
            rec[key] = torch.cat([p[0].blocks[i][key] for p in parts])
    for key in tape.top:
        tape.top[key] = torch.cat([p[0].top[key] for p in parts])
    tape.logits = torch.cat([p[0].logits for p in parts])
    depth = len(tape.blocks)
    attns = [torch.cat([p[2][i] for p in parts]) for i in range(depth)]
    grads = [torch.cat([p[3][i] for p in parts]) for i in range(depth)] if gradients else None
    return tape, torch.cat([p[1] for p in parts]), attns, grads


def split_heads(qkv, heads):
    """qkv's output (B, N, 3 * h * d) -> q, k, v, each (B, h, N, d) and contiguous ('b n (qkv h d) -> qkv b h n d')"""
    B, N, D3 = qkv.shape
    t = qkv.reshape(B, N, 3, heads, D3 // (3 * heads)).permute(2, 0, 3, 1, 4)
    return t[0].contiguous(), t[1].contiguous(), t[2].contiguous()


def safe_divide(a, b):
    """layers_ours.py:10-13, for the (B, D) vectors of the head and the pooling that stay torch ops"""
    den = b.clamp(min=1e-9) + b.clamp(max=1e-9)
    den = den + den.eq(0).to(den.dtype) * 1e-9
    return a / den * b.ne(0).to(b.dtype)


# ------------------------------------------------------------------------------------------------ the clamped weights
_WEIGHTS = {}        # (data_ptr, _version, shape, device) -> (the weight, which keeps its storage from being reused, (pos, neg))


def clamped_weights(w):
    """(clamp(W, min=0), clamp(W, max=0)) of a Linear weight, made once with K46 and kept until the parameter is written again
    (its `_version` changes) or moves (its `data_ptr` changes)."""
    key = (w.data_ptr(), w._version, tuple(w.shape), str(w.device))
    hit = _WEIGHTS.get(key)
    if hit is None:
        wd = w.detach()
        wc = wd if wd.is_contiguous() and wd.dtype == torch.float32 else wd.float().contiguous()
        hit = _WEIGHTS[key] = (wd, K.lrp_split(wc))
    return hit[1]


def linear_weights(model):
    """the Linear weights the pass reads, top down"""
    ws = [model.head.weight]
    for blk in model.blocks:
        ws += [blk.mlp.fc2.weight, blk.mlp.fc1.weight, blk.attn.proj.weight, blk.attn.qkv.weight]
    return ws


def clear_cache():
    """Drop the cached clamped weights (about as many bytes as the models' Linear weights, twice) and this thread's captured passes."""
    _WEIGHTS.clear()
    _PASSES.entries().clear()


# ------------------------------------------------------------------------------------------------ the relevance pass
def _mm(a, b):
    """torch.matmul(a, b), image by image when a holds more than one: every image gets the GEMM call of its own one-image pass.  Folded
    into one larger or batched GEMM, rocBLAS may pick another kernel and with it another order of summation than for the image
    alone (measured: it does, for some shapes and batch sizes), and this method amplifies such last-bit differences.  b: a weight
    (2-D, shared) or an operand with the same image axis."""
    B = a.shape[0]
    if B == 1:
        return torch.matmul(a, b)
    return torch.cat([torch.matmul(a[j:j + 1], b if b.dim() == 2 else b[j:j + 1]) for j in range(B)])


def _linear(R, X, weight):
    """Linear.relprop with alpha = 1: K46, two GEMMs, K47, two GEMMs, K48"""
    wp, wn = clamped_weights(weight)
    px, nx = K.lrp_split(X)
    z1 = _mm(px, wp.t())
    z2 = _mm(nx, wn.t())
    s = K.lrp_ratio(R, z1, z2, out=z1)
    g1 = _mm(s, wp)
    g2 = _mm(s, wn)
    return K.lrp_gather(X, g1, g2, out=g1)


def relevance_pass(model, tape, tgt, attns, need):
    """The relevance of the target logits from the head down to the attention of block need[0] -> cams (len(need), B, h, S, S):
    the attn_cam (ViT_LRP_timm.py:361-366) of the blocks in `need`.  The blocks between need[0] and the top are all walked."""
    blocks = list(model.blocks)
    heads = attns[0].shape[1]
    B, S = attns[0].shape[0], attns[0].shape[-1]
    dev = attns[0].device
    cams = torch.empty((len(need), B, heads, S, S), dtype=torch.float32, device=dev)
    logits = tape.logits
    one_hot = torch.zeros_like(logits).scatter_(1, tgt.view(-1, 1), 1.0)
    cam = _linear(one_hot, tape.top["head_in"].contiguous(), model.head.weight)                 # (B, D)
    x0 = tape.top["norm_out"][:, 0]
    R = torch.zeros_like(tape.top["norm_out"])
    R[:, 0] = x0 * safe_divide(cam, x0)                                                          # IndexSelect.relprop; norm passes
    R = R.contiguous()
    ws = None
    for i in range(len(blocks) - 1, need[0] - 1, -1):
        blk, rec = blocks[i], tape.blocks[i]
        if ws is None:
            ws = torch.empty(K._lib.load("ext4").xai_lrp_add_workspace_bytes(B, rec["x_in"][0].numel()), dtype=torch.uint8, device=dev)
        cam1, cam2 = K.lrp_add(rec["x_mid"].contiguous(), rec["mlp_out"].contiguous(), R, ws=ws)  # add2
        cam2 = _linear(cam2, rec["g"].contiguous(), blk.mlp.fc2.weight)                           # fc2; act passes
        cam2 = _linear(cam2, rec["n2"].contiguous(), blk.mlp.fc1.weight)                          # fc1; norm2 passes
        R = K.lrp_clone(rec["x_mid"].contiguous(), cam1, cam2, out=cam2)                          # clone2
        cam1, cam2 = K.lrp_add(rec["x_in"].contiguous(), rec["attn_out"].contiguous(), R, ws=ws)  # add1
        c = _linear(cam2, rec["pv"].contiguous(), blk.attn.proj.weight)                           # proj
        N, D = c.shape[1], c.shape[2]
        c = c.reshape(B, N, heads, D // heads).permute(0, 2, 1, 3).contiguous()                   # 'b n (h d) -> b h n d'
        q, k, v = split_heads(rec["qkv"], heads)
        A = attns[i].contiguous()
        z = _mm(A, v)                                                                    # matmul2: attn = A V
        s = K.lrp_ratio(c, z, out=z)
        c0 = _mm(s, v.transpose(-1, -2))
        slot = need.index(i) if i in need else None
        camA = K.lrp_half_product(A, c0, out=cams[slot] if slot is not None else c0)              # attn_cam; softmax passes
        if i == need[0]:
            break
        cam_qkv = torch.empty((B, N, 3 * D), dtype=torch.float32, device=dev)
        K.lrp_half_product(v, _mm(A.transpose(-1, -2), s), out=cam_qkv, slot=2)
        z = _mm(q, k.transpose(-1, -2))                                                  # matmul1: Q K^T, unscaled
        s = K.lrp_ratio(camA, z, out=z)
        K.lrp_half_product(q, _mm(s, k), out=cam_qkv, slot=0)
        K.lrp_half_product(k, _mm(s.transpose(-1, -2), q), out=cam_qkv, slot=1)
        cam2 = _linear(cam_qkv, rec["n1"].contiguous(), blk.attn.qkv.weight)                      # qkv; norm1 passes
        R = K.lrp_clone(rec["x_in"].contiguous(), cam1, cam2, out=cam2)                           # clone1
    return cams


def _attribute(model, x, targets, method, is_ablation, start_layer, withgrad):
    """One call on (B, C, H, W) inputs on the device -> ((B, p, p) map, cams): forward, backward where the method reads the
    attention gradients, the relevance pass and the method's read-out.  No host synchronisation: capturable."""
    depth = len(model.blocks)
    need = blocks_needed(method, depth, start_layer)
    gradients = needs_gradients(method, withgrad, is_ablation)
    tape, tgt, attns, grads = record_per_image(model, x, targets, gradients)
    B, h, S, _ = attns[0].shape
    if method == "last_layer_attn":
        # ViT_LRP_timm.py:748-758 with end_layer = depth; only the CLS row is read, and the row's arithmetic is element-wise
        cam = 0
        for i in range(start_layer, depth):
            cam = cam + attns[i][:, :, 0, :]
        if not torch.is_tensor(cam):
            raise TypeError("'int' object is not subscriptable")                   # the reference's `cam[0]` on cam = 0
        row, cams = cam.clamp(min=0).mean(dim=1), None
    else:
        cams = relevance_pass(model, tape, tgt, attns, need)
        g = None
        if gradients:
            g = torch.empty_like(cams)
            for slot, i in enumerate(need):
                g[slot].copy_(grads[i])
        if method in ("last_layer", "second_layer"):
            row = K.lrp_attn_matrices(cams, g, K.LRP_CLS_ROW)[:, 0]
        else:
            row = K.rollout_row(K.lrp_attn_matrices(cams, g, K.LRP_ROLLOUT), 0)
    side = int(np.sqrt(S - 1))
    return row[:, 1:].reshape(B, side, side).contiguous(), cams


class _LrpPass(CapturedCall):
    """One call of `_attribute` on static input / target buffers, replayed from a hipGraph of exactly that -- forward, backward,
    relevance pass, read-out -- once the graph has proven itself on the caller's first real input (streams.CapturedCall)."""

    def __init__(self, model, example, argmax, method, is_ablation, start_layer, withgrad):
        super().__init__(LRP_COUNTS, (GRAD_RTOL,))
        self.model, self.argmax = model, argmax
        # the graph reads the clamped weights' pointers: they must outlive a clear_cache() for as long as the graph can be replayed
        self.weights = [clamped_weights(w) for w in linear_weights(model)]
        self.args = (method, is_ablation, start_layer, withgrad)
        self.x = torch.zeros(tuple(example.shape), dtype=torch.float32, device=example.device)
        self.tgt = torch.zeros((self.x.shape[0],), dtype=torch.int64, device=self.x.device)

    def step(self):
        return (_attribute(self.model, self.x, None if self.argmax else self.tgt, *self.args)[0],)

    def _replay(self):
        # the graph holds backward kernels: the replay alone takes the device's turn (gradcam.CapturedGradCam._replay has the why)
        with backward_turn(self.x.device):
            return super()._replay()

    def __call__(self, x, targets):
        self.x.copy_(x, non_blocking=True)
        if not self.argmax:
            self.tgt.copy_(targets, non_blocking=True)
        (out,) = self.run()
        return out.clone()                                # a replay overwrites the graph's own output


def transformer_attribution_batch(x, model, targets, method="transformer_attribution", withgrad=True, start_layer=0, is_ablation=False,
                                  graphs=True, return_cams=False):
    """`LRP(model).generate_LRP` for a batch: x (B, C, H, W) on a HIP device, targets one class index or one per image (None: each
    image's argmax) -> (B, p, p) on the device, each image what its own one-image call gives: every sum of the pass is per image, the classifier runs image by
    image (`record_per_image`) and so do the GEMMs of the pass (`_mm`); the kernels between them take the whole batch.  graphs=True: the whole call replays as one hipGraph per (model, shape, method) and host thread, proven on the first real
    input, eager if the capture is refused (LRP_COUNTS).  return_cams=True (eager only): also the attn_cam of the blocks the method
    reads, (blocks, B, h, S, S)."""
    check_method(method)
    check_layout(model)
    x = check_input(x, "transformer_attribution_batch")
    B = x.shape[0]
    blocks_needed(method, len(model.blocks), start_layer)                     # the reference's IndexError, before any launch
    tgt = None if targets is None else class_targets(targets, B, x.device, "transformer_attribution_batch")
    if graphs and not return_cams:
        # a weight that was written again or moved gets new clamped copies, which a graph captured before does not read
        versions = tuple((w.data_ptr(), w._version) for w in linear_weights(model))
        key = (tuple(x.shape), targets is None, method, bool(is_ablation), int(start_layer), bool(withgrad), versions)
        cap = _PASSES.get(model, x.device, key, lambda: _LrpPass(model, x, targets is None, method, bool(is_ablation), int(start_layer),
                                                                  bool(withgrad)))
        return cap(x, tgt)
    LRP_COUNTS["eager"] += 1
    out, cams = _attribute(model, x, tgt, method, bool(is_ablation), int(start_layer), bool(withgrad))
    return (out, cams) if return_cams else out


class LRP:
    """The reference's `LRP` (ViT_explanation_generator.py:107-133) on the engine's hooked ViT: there is no second "LRP model".
    `graphs=True` replays each call from a hipGraph (see `transformer_attribution_batch`); the default runs eagerly."""

    def __init__(self, model, graphs=False):
        check_layout(model)
        self.model = model
        self.model.eval()
        self.graphs = graphs

    def generate_LRP(self, input, target_class, method="transformer_attribution", is_ablation=False, start_layer=0, withgrad=True,
                     device="cuda:0"):
        """-> (1, p, p) on the device.  target_class None: the argmax."""
        check_method(method)
        dev = hip_device(device)
        x = input.to(dev, torch.float32)
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError(f"generate_LRP attributes one (1, C, H, W) image, got {tuple(x.shape)}; transformer_attribution_batch takes more")
        if target_class is not None and not torch.is_tensor(target_class):
            target_class = int(np.asarray(target_class).reshape(-1)[0])
        return transformer_attribution_batch(x, self.model, target_class, method=method, withgrad=withgrad, start_layer=start_layer,
                                             is_ablation=is_ablation, graphs=self.graphs)
