"""GradientShap (captum 0.7.0 `GradientShap` as the reference's harness calls it, evaluatePerturbation.py:164-167) on K34 and K35.

For every image `n_samples` rows: a baseline chosen at random among the given ones and a point on the straight line between it and
the input at a random coefficient; one classifier forward and one backward over all rows (the gradient of the raw target logit);
then attr = mean over an image's rows of (input - baseline) * gradient.  Row r = b * n_samples + s belongs to image b (captum's
repeat_interleave).  In full:

  1. stdevs != 0 only: xr = x.repeat_interleave(n, 0) + torch.normal(0, stdev_expanded), in torch on the device (the device
     generator's stream is torch's).  At stdevs == 0 NO device noise is drawn and xr[r] is x[b] itself, never materialised.
  2. host draws from NumPy's global state, in captum's order: idx = np.random.choice(N_b, n * B), then
     alpha = float32(np.random.uniform(0.0, 1.0, n * B)) -- both also when N_b == 1, once on the calling thread for the whole
     batch before it is cut into passes (`draw`).  captum brings the coefficients back through the host on every call; here the
     two arrays are uploaded once and nothing is read back.
  3. K34: scaled[r] = alpha[r] * xr[r] + (1 - alpha[r]) * baselines[idx[r]]: two products and a sum, each rounded.
  4. g = d(sum_r logits(scaled)[r, t[b(r)]]) / d scaled: raw logits.
  5. K35: attr[b] = (+0 + sum over s ascending of (xr[r] - baselines[idx[r]]) * g[r]) / n, a true fp32 division, and
  6. the harness's map |(attr[b][0] + attr[b][1]) + attr[b][2]| from the same read of the gradients.

captum itself reduces step 5 with `.mean` over a reshaped tensor: the order of that sum over the samples is torch's and UNPINNED;
the order above is this engine's and the one tests/gshap_restated.py restates.  Parity with captum itself is unpinned as for
guided.py: captum is not part of the reference tree (unpinned third-party boundaries).

One pass -- K34, forward, the logit gather, backward, K35 -- runs on static buffers and is replayed from a hipGraph once the graph
has proven itself on the caller's first real batch (streams.CapturedCall, per host thread, model and shape); alpha, idx, the
targets and x are copied into the static buffers before each replay.
"""
import numpy as np
import torch

from . import kernels as K
from ._lib import XaiHipError
from .ig import _logits_of, check_input, class_targets
from .streams import GRAD_RTOL, CapturedCall, ThreadGraphs, backward_turn, cat_parts, run_passes

GSHAP_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0}
_PASSES = ThreadGraphs(limit=4)


def draw(n_base, n_rows):
    """Step 2: captum's two host draws from NumPy's global state, in its order -> (idx int64 (n_rows,), alpha float32 (n_rows,)).
    Both calls are made whatever n_base is, so the state moves as under captum."""
    idx = np.random.choice(int(n_base), int(n_rows))
    alpha = np.random.uniform(0.0, 1.0, int(n_rows)).astype(np.float32)
    return idx, alpha


def _upload_draws(draws, n_base, n_rows, dev):
    """(idx, alpha) as NumPy arrays, lists or tensors -> int64 / float32 device tensors of n_rows values.  Host values are checked
    against [0, n_base); a device tensor is not read back (K34 / K35 clamp what they read)."""
    idx, alpha = draws
    if not torch.is_tensor(idx):
        idx = np.asarray(idx)
        if idx.shape != (n_rows,) or idx.dtype.kind not in "iu" or (idx.size and (idx.min() < 0 or idx.max() >= n_base)):
            raise ValueError(f"gradient_shap_batch: draws[0] must hold {n_rows} baseline indices in [0, {n_base})")
        idx = torch.from_numpy(idx.astype(np.int64))
    if not torch.is_tensor(alpha):
        alpha = torch.from_numpy(np.asarray(alpha, dtype=np.float32))
    if idx.numel() != n_rows or alpha.numel() != n_rows or idx.is_floating_point():
        raise ValueError(f"gradient_shap_batch: draws must be ({n_rows} indices, {n_rows} coefficients)")
    return (idx.to(dev, torch.int64, non_blocking=True).reshape(-1).contiguous(),
            alpha.to(dev, torch.float32, non_blocking=True).reshape(-1).contiguous())


class _GshapPass(CapturedCall):
    """Static buffers of k images (k * n rows); a call is K34 + forward + logit gather + backward + K35, replayed from a hipGraph of
    exactly that once it has proven itself on the caller's first real batch (streams.CapturedCall)."""

    def __init__(self, model, k, img_shape, dev, n, n_base, per_row, want_attr, want_map):
        super().__init__(GSHAP_COUNTS, (GRAD_RTOL,) * (int(want_attr) + int(want_map)))
        self.model, self.n, self.want_attr, self.want_map = model, n, want_attr, want_map
        rows = k * n
        self.x = torch.zeros((rows if per_row else k,) + img_shape, dtype=torch.float32, device=dev)
        self.base = torch.zeros((n_base,) + img_shape, dtype=torch.float32, device=dev)
        self.alpha = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.idx = torch.zeros(rows, dtype=torch.int64, device=dev)
        self.tgt = torch.zeros((rows, 1), dtype=torch.int64, device=dev)
        self.scaled = torch.zeros((rows,) + img_shape, dtype=torch.float32, device=dev)          # the pass's static input

    def step(self):
        K.gshap_scale(self.x, self.base, self.alpha, self.idx, self.n, out=self.scaled)
        with torch.enable_grad():
            xs = self.scaled.detach().requires_grad_(True)
            score = _logits_of(self.model(xs)).gather(1, self.tgt).sum()
            with backward_turn(xs.device):
                (g,) = torch.autograd.grad(score, xs)
        out = K.gshap_finish(g.detach().float().contiguous(), self.x, self.base, self.idx, self.n, want_attr=self.want_attr,
                             want_map=self.want_map)
        return out if isinstance(out, tuple) else (out,)

    def __call__(self, x, base, alpha, idx, tgt, graphs):
        self.x.copy_(x)
        self.base.copy_(base)
        self.alpha.copy_(alpha)
        self.idx.copy_(idx)
        self.tgt.copy_(tgt.view(-1, 1).expand(-1, self.n).reshape(-1, 1))           # row r = b * n + s carries image b's class
        out = self.run() if graphs else self.eager()
        return tuple(t.clone() for t in out)             # a replay overwrites the graph's own outputs


def gradient_shap_batch(x, model, targets, baselines, n_samples=5, stdevs=0.0, want_attr=True, want_map=False, pass_images=None,
                        streams=1, graphs=True, draws=None):
    """GradientShap of B images: x (B, C, H, W) and `baselines` (N_b, C, H, W) on a HIP device, `targets` one class index or one
    per image (a device tensor is not read back).  `n_samples` rows per image, `stdevs` (a number) the standard deviation of the
    Gaussian noise added to every row's input (0.0: none is drawn).
    -> the attribution (B, C, H, W) (`want_attr`), the harness's map |sum over channels| (B, H, W) (`want_map`), or (attr, map).
    `draws` = (idx, alpha), B * n_samples values each: the baseline of every row and its coefficient, instead of the two NumPy draws
    (`draw`).  `pass_images` (default: all B): images per classifier pass; `streams` > 1: the passes run on that many stream workers
    (streams.py).  `graphs`: replay a pass from a hipGraph, kept per thread, model and shape."""
    x = check_input(x, "gradient_shap_batch")
    if not (want_attr or want_map):
        raise ValueError("gradient_shap_batch: nothing to return (neither want_attr nor want_map)")
    n = int(n_samples)
    if n < 1:
        raise ValueError(f"gradient_shap_batch: n_samples must be >= 1, got {n_samples}")
    if not torch.is_tensor(baselines) or not baselines.is_cuda:
        raise XaiHipError("gradient_shap_batch needs its baselines on a HIP device ('cuda:N'); there is no CPU fallback")
    if baselines.dim() != 4 or baselines.shape[0] < 1 or baselines.shape[1:] != x.shape[1:]:
        raise ValueError(f"gradient_shap_batch: baselines must be (N_b, {', '.join(map(str, x.shape[1:]))}), got {tuple(baselines.shape)}")
    if isinstance(stdevs, (tuple, list)) or torch.is_tensor(stdevs):
        raise NotImplementedError("gradient_shap_batch: stdevs must be one number")
    stdevs = float(stdevs)
    B, dev, img_shape = x.shape[0], x.device, tuple(x.shape[1:])
    tgt = class_targets(targets, B, dev, "gradient_shap_batch")
    base = baselines.detach().to(dev, torch.float32).contiguous()
    n_base = base.shape[0]
    per_row = stdevs != 0.0
    if per_row:                                           # step 1, for the whole batch: the device generator's stream does not depend on the cut
        xr = x.repeat_interleave(n, 0)
        xr = xr + torch.normal(0, torch.full_like(xr, stdevs))
    idx, alpha = _upload_draws(draws if draws is not None else draw(n_base, n * B), n_base, n * B, dev)

    def one_pass(lo, hi):
        k = hi - lo
        key = (k, img_shape, n, n_base, per_row, bool(want_attr), bool(want_map))
        p = _PASSES.get(model, dev, key, lambda: _GshapPass(model, k, img_shape, dev, n, n_base, per_row, bool(want_attr), bool(want_map)),
                        cached=bool(graphs))
        return p(xr[lo * n:hi * n] if per_row else x[lo:hi], base, alpha[lo * n:hi * n], idx[lo * n:hi * n], tgt[lo:hi], bool(graphs))

    kind = ("gradient_shap_batch", id(model), pass_images, img_shape, n, n_base, per_row, bool(want_attr), bool(want_map), bool(graphs))
    out = cat_parts(run_passes(dev, B, pass_images, one_pass, streams, kind))
    return out if len(out) > 1 else out[0]


class GradientShap:
    """captum.attr.GradientShap's call shape on the HIP path, for what the harness uses (evaluatePerturbation.py:164-167)."""

    def __init__(self, model):
        self.model = model

    def attribute(self, inputs, baselines, n_samples=5, stdevs=0.0, target=None):
        """-> (B, C, H, W) device tensor"""
        return gradient_shap_batch(inputs, self.model, target, baselines, n_samples=n_samples, stdevs=stdevs)


def patch_captum():
    """Opt-in, like guided.patch_captum: make `from captum.attr import GradientShap` -- evaluatePerturbation.py:43 -- resolve to the
    class above.  Only this one name of an installed captum's `captum.attr` is rebound.  -> the GradientShap that was replaced, or
    None when captum is not importable."""
    try:
        import captum.attr as cattr
    except ImportError:
        return None
    old = getattr(cattr, "GradientShap", None)
    cattr.GradientShap = GradientShap
    return old
