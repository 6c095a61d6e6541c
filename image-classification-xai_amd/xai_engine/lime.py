"""LIME for images (reference util/attribution_methods/lime: limeAttr.py, lime_image.py, lime_base.py) on the HIP kernels K31 - K33.

The reference explains one image with 1000 perturbed copies: each is built on the host with a `copy.deepcopy` and one full-image
compare per switched-off superpixel (lime_image.py:255-262), the classifier sees them ten at a time with a read-back after every
call (:263-269), and six sklearn Ridge fits on the 1000 x D matrix follow, on the host (lime_base.py:78-80, :189-193 for five
labels).  Here the perturbed images of ALL inputs of a call form one flat list (row = image * num_samples + sample); the 0/1 matrix
is drawn on the host with the reference's own calls, packed to 64-bit words and uploaded once; the list is cut into classifier
passes of `pass_size` rows, K31 writes a pass's rows straight into the pass's static input buffer, the forward runs under
`no_grad`, and the softmax probabilities of the image's label columns are gathered on the device.  One K32 launch then computes
the distances, the kernel weights and both ridge fits of every label of every image in fp64, and K33 paints the chosen
superpixels.  Nothing is read back between the passes, K32 and K33.  Every distinct pass size is one hipGraph
(streams.CapturedCall, per host thread).

`lime_batch` is the multi-image entry; `LimeImageExplainer` / `ImageExplanation` keep the reference's call shape
(util/attribution_methods/lime/lime_image.py serves them), `get_lime_attr` / `batch_predict` / `make_tensor` are limeAttr.py's.
The segmentation (quickshift, skimage, on the host) stays the reference's dependency: `quickshift_segments` calls it when
skimage is installed, callers that pass `segments=` / `segmentation_fn=` need none.  `device_quickshift_segments` is the opt-in
segmenter that needs no skimage: the same quickshift on the kernels K53 - K55 (xai_engine/quickshift.py), accepted by identity by
`lime_batch(segments=...)` and `explain_instance(segmentation_fn=...)`.

Parity: sklearn's weighted Ridge and cosine distance are pinned through tests/golden/lime.npz (the reference's own run);
skimage's quickshift is UNPINNED (unpinned third-party boundaries).
"""
import collections
import threading

import numpy as np
import torch

from . import kernels as K
from .ig import _logits_of, check_input, hip_device
from .streams import LOGIT_RTOL, CapturedCall, ThreadGraphs, read_back, run_passes

PASS_SIZE = 100                    # rows per classifier pass: the harness's 1000 samples are ten passes of one size, one hipGraph
REFERENCE_BATCH = 10               # lime_image.py:132, the batch size this engine replaces
ALPHA_SELECT, ALPHA = 0.01, 1.0    # lime_base.py:78 and :189
LIME_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0, "rows": 0, "host_fits": 0}
_PASSES = ThreadGraphs(limit=4)

LimeDetails = collections.namedtuple("LimeDetails", "data labels distances weights coef intercept score local_pred order top_labels")
LimeDetails.__doc__ = """What `lime_batch(..., want="details")` adds.  data: the host 0/1 matrices, one (N, D_b) array per image; the
rest are device tensors: labels (B, N, L) float32 (the gathered probabilities), distances, weights (B, N) fp64, coef (B, L, d_stride)
fp64 indexed by superpixel, intercept, score, local_pred (B, L) fp64, order (B, L, d_stride) int32 (the superpixels by descending
|coef|, -1 behind the image's D_b), top_labels (B, L) int64 (the label columns, the most probable first)."""


class _ProbPass(CapturedCall):
    """The forward of `b` rows on a static input buffer `x` (K31 writes the rows into it), softmax over the classes
    (limeAttr.py:18-19) and the gather of each row's label columns from the static `cols`, replayed as one hipGraph by the thread
    that captured it once the replay has proven itself on the caller's first real rows (streams.CapturedCall)."""

    def __init__(self, model, b, img_shape, n_labels, dev):
        super().__init__(LIME_COUNTS, (LOGIT_RTOL,))
        self.model = model
        self.x = torch.zeros((b,) + tuple(img_shape), dtype=torch.float32, device=dev)
        self.cols = torch.zeros((b, n_labels), dtype=torch.int64, device=dev)

    def step(self):
        with torch.no_grad():
            return (torch.softmax(_logits_of(self.model(self.x)).float(), dim=1).gather(1, self.cols),)


def _refuse(unsupported, name):
    if unsupported:
        raise NotImplementedError(f"{name}: {', '.join(sorted(unsupported))} not supported on the HIP path")


def _random_state(seed):
    """sklearn.utils.check_random_state, restated: None -> numpy's global RandomState, an int -> a new one, a RandomState -> itself."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def draw_seed(random_state):
    """lime_image.py:174-175: the segmentation seed the reference draws whenever `random_seed is None`, used or not."""
    return random_state.randint(0, high=1000)


def draw_data(random_state, num_samples, n_features):
    """lime_image.py:249-252: the (num_samples, n_features) 0/1 matrix, row 0 all ones."""
    data = random_state.randint(0, 2, num_samples * n_features).reshape((num_samples, n_features))
    data[0, :] = 1
    return data


def pack_rows(data, words=None):
    """A 0/1 matrix (N, D) -> (N, words) uint64: column z is bit z % 64 of word z // 64; the bits behind D are zero."""
    data = np.asarray(data)
    if data.ndim != 2 or data.shape[1] < 1:
        raise ValueError(f"data must be (num_samples, n_features), got {data.shape}")
    N, D = data.shape
    words = K.lime_words(D) if words is None else int(words)
    if words * 64 < D:
        raise ValueError(f"{words} words hold {words * 64} features, the data has {D}")
    bits = np.zeros((N, words * 64), np.uint8)
    bits[:, :D] = data != 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(N, words)


def check_segments(segments, name="lime"):
    """One image's (H, W) integer superpixel ids on the host -> (int32 array, D).  The ids must be 0 .. D - 1 without gaps."""
    seg = segments.detach().cpu().numpy() if torch.is_tensor(segments) else np.asarray(segments)
    if seg.ndim != 2 or seg.dtype.kind not in "iu":
        raise ValueError(f"{name}: segments of one image must be an (H, W) array of integer ids, got {seg.shape} {seg.dtype}")
    ids = np.unique(seg)
    D = int(ids.shape[0])
    if int(ids[0]) < 0:
        raise ValueError(f"{name}: negative superpixel id {int(ids[0])}: the reference counts np.unique(segments) features and switches "
                         "off `segments == z` for z in 0 .. D - 1 only (lime_image.py:248-260), so this superpixel would never be perturbed")
    if int(ids[-1]) != D - 1:
        gap = int(np.flatnonzero(ids != np.arange(D))[0])
        raise ValueError(f"{name}: superpixel ids must be 0 .. D - 1 without gaps, {D} distinct ids reach {int(ids[-1])} and {gap} is missing: "
                         f"the reference would perturb nothing for column {gap} and never perturb id {int(ids[-1])} (lime_image.py:248-260)")
    return np.ascontiguousarray(seg, dtype=np.int32), D


def segment_mean_image(image, segments):
    """lime_image.py:186-192: every superpixel filled with its mean colour, per channel, in the image's dtype.  image: (H, W, C)."""
    image = np.asarray(image)
    fudged = image.copy()
    for s in np.unique(segments):
        sel = segments == s
        fudged[sel] = tuple(np.mean(image[sel][:, c]) for c in range(image.shape[2]))
    return fudged


def ridge_fit(X, y, w, alpha):
    """sklearn's Ridge(alpha, fit_intercept=True).fit(X, y, sample_weight=w) as a closed form in fp64 -> (coef, intercept)."""
    X, y, w = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(w, np.float64)
    sums = (np.column_stack([np.ones(len(w)), X]) * w[:, None]).sum(0)       # one order for every column: a column of ones has the mean 1
    xbar, ybar = sums[1:] / sums[0], (w * y).sum() / sums[0]
    Xc, yc = X - xbar, y - ybar
    A = (Xc * w[:, None]).T @ Xc + alpha * np.eye(X.shape[1])
    coef = np.linalg.solve(A, (Xc * w[:, None]).T @ yc)
    return coef, ybar - xbar @ coef


def host_fit(data, Y, kernel_width=0.25, alpha_select=ALPHA_SELECT, alpha=ALPHA):
    """What K32 computes for one image, on the host in fp64, for images with more superpixels than `K.lime_max_features()`.
    data (N, D) 0/1, Y (N, L) -> dict of coef (L, D), order (L, D), intercept, score, local_pred (L,), dist, weight (N,)."""
    X = (np.asarray(data) != 0).astype(np.float64)
    Y = np.asarray(Y, np.float64)
    N, D = X.shape
    dist = 1.0 - np.sqrt(X.sum(1) / D)
    w = np.sqrt(np.exp(-(dist ** 2) / kernel_width ** 2))
    out = dict(coef=np.zeros((Y.shape[1], D)), order=np.zeros((Y.shape[1], D), np.int32), intercept=np.zeros(Y.shape[1]),
               score=np.zeros(Y.shape[1]), local_pred=np.zeros(Y.shape[1]), dist=dist, weight=w)
    for l in range(Y.shape[1]):
        y = Y[:, l]
        c1, _ = ridge_fit(X, y, w, alpha_select)
        used = sorted(range(D), key=lambda j: np.abs(c1[j] * X[0, j]), reverse=True)
        c2, icpt = ridge_fit(X[:, used], y, w, alpha)
        final = sorted(range(D), key=lambda i: np.abs(c2[i]), reverse=True)
        out["coef"][l, used] = c2
        out["order"][l] = [used[i] for i in final]
        out["intercept"][l] = icpt
        out["local_pred"][l] = icpt + X[0, used] @ c2
        ybar = (w * y).sum() / w.sum()
        num, den = (w * (y - (X[:, used] @ c2 + icpt)) ** 2).sum(), (w * (y - ybar) ** 2).sum()
        out["score"][l] = np.nan if N < 2 else ((1.0 if num == 0 else 0.0) if den == 0 else 1.0 - num / den)
    return out


def _hide_args(hide_color, x, segs):
    """hide_color -> (hide (C,) device tensor or None, fudged (B, C, H, W) device tensor or None)"""
    B, C = x.shape[:2]
    if hide_color is None:                       # the per-superpixel mean colour, the reference's expression on the host
        host = x.cpu().numpy()
        fudged = np.stack([segment_mean_image(host[b].transpose(1, 2, 0), segs[b]).transpose(2, 0, 1) for b in range(B)])
        return None, torch.from_numpy(np.ascontiguousarray(fudged)).to(x.device)
    if torch.is_tensor(hide_color) and hide_color.dim() == 4:
        if tuple(hide_color.shape) != tuple(x.shape):
            raise ValueError(f"lime_batch: a replacement image must be {tuple(x.shape)}, got {tuple(hide_color.shape)}")
        return None, hide_color.to(x.device, torch.float32).contiguous()
    h = np.asarray(hide_color.cpu() if torch.is_tensor(hide_color) else hide_color, dtype=np.float32).reshape(-1)
    if h.size not in (1, C):
        raise ValueError(f"lime_batch: hide_color must be a number, one value per channel or None, got {h.size} values")
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(h, (C,)))).to(x.device), None


def lime_batch(x01, model, segments, num_samples=1000, top_labels=5, labels=None, hide_color=0, kernel_width=.25, data=None,
               random_state=None, num_features=5, pass_size=PASS_SIZE, streams=1, graphs=True, want="mask"):
    """LIME explanations of B independent images.

    x01: (B, C, H, W) on a HIP device, the un-normalised image the reference perturbs (limeAttr.py feeds it to the classifier
    as it is).  segments: (B, H, W) or (H, W) integer superpixel ids 0 .. D_b - 1, array or tensor, or a callable
    `(image_hwc, random_seed) -> (H, W)` run on the host per image, or `device_quickshift_segments` itself (taken by identity, as
    `explain_instance` takes `batch_predict`): quickshift on K53 - K55 with the drawn seed; the labels never leave the device, only
    D_b is read back (the data matrix is drawn from it), and a host copy is made only for `hide_color=None`.
    data: one (num_samples, D_b) 0/1 matrix per image (a single array for B = 1); None: drawn from `random_state` (None, an int or a RandomState) with the reference's calls in the
    reference's order, per image the seed draw of lime_image.py:174-175 and then the matrix of :249-252.
    top_labels: explain the L most probable classes of every image (the unperturbed image's softmax, topk on the device); 0 / None:
    the classes `labels`, shared by the images.  hide_color: a number, one per channel, a (B, C, H, W) replacement image, or None
    for the per-superpixel mean colour (:186-192).
    -> want="mask": (B, H, W) float32 device map, 3 on the first `num_features` superpixels with a positive weight in the
    explanation of the first label, 0 elsewhere: the harness's |sum over 3 channels| of get_image_and_mask's mask
    (limeAttr.py:34-36, evaluatePerturbation.py:181).  want="weights": the first label's coefficient of every pixel's superpixel.
    want="details": (the mask map, `LimeDetails`).
    An image with more superpixels than `K.lime_max_features()` is fitted on the host in fp64 (LIME_COUNTS["host_fits"])."""
    if want not in ("mask", "weights", "details"):
        raise ValueError(f"lime_batch: want must be 'mask', 'weights' or 'details', got {want!r}")
    x = check_input(x01, "lime_batch")
    B, C, H, W = x.shape
    dev = x.device
    N = int(num_samples)
    if N < 1:
        raise ValueError("lime_batch: num_samples must be >= 1")
    rs = _random_state(random_state) if data is None else None
    if data is not None and not isinstance(data, (list, tuple)):
        data = [data] if np.ndim(data) == 2 else list(data)
    if data is not None and len(data) != B:
        raise ValueError(f"lime_batch: {len(data)} data matrices for {B} images")

    device_seg = segments is device_quickshift_segments
    seg_dims = 0 if callable(segments) else (segments.dim() if torch.is_tensor(segments) else np.ndim(segments))
    if seg_dims == 3 and len(segments) != B:
        raise ValueError(f"lime_batch: segments of {len(segments)} images for {B} images")
    host_x = None
    segs, Ds, mats = [], [], []
    for b in range(B):
        seed = draw_seed(rs) if rs is not None else None
        if callable(segments) and host_x is None:
            host_x = x.cpu().numpy()
        if device_seg:
            s, D = _device_segments(host_x[b].transpose(1, 2, 0), seed, dev)      # ids 0 .. D - 1 by construction (K55)
        else:
            s = segments(host_x[b].transpose(1, 2, 0), seed) if callable(segments) else segments if seg_dims == 2 else segments[b]
            s, D = check_segments(s, "lime_batch")
        if tuple(s.shape) != (H, W):
            raise ValueError(f"lime_batch: segments of image {b} are {tuple(s.shape)}, the image is {(H, W)}")
        m = draw_data(rs, N, D) if rs is not None else np.asarray(data[b])
        if m.shape != (N, D):
            raise ValueError(f"lime_batch: data of image {b} must be {(N, D)}, got {m.shape}")
        segs.append(s); Ds.append(D); mats.append(m)
    words = K.lime_words(max(Ds))
    d_stride = words * 64
    rows = torch.from_numpy(np.concatenate([pack_rows(m, words) for m in mats]).view(np.int64)).to(dev)
    if device_seg:
        seg_t = torch.stack(segs)
        segs = [t.cpu().numpy() for t in segs] if hide_color is None else None     # the mean colours are the host's (:186-192)
    else:
        seg_t = torch.from_numpy(np.stack(segs)).to(dev)
    D_t = torch.tensor(Ds, dtype=torch.int32).to(dev)
    hide, fudged = _hide_args(hide_color, x, segs)

    if top_labels:
        L = int(top_labels)
        with torch.no_grad():
            cols = torch.softmax(_logits_of(model(x)).float(), dim=1).topk(L, dim=1).indices        # lime_image.py:210-212
    else:
        lab = [int(v) for v in labels]
        if not lab:
            raise ValueError("lime_batch: no labels to explain (top_labels is 0 / None and labels is empty)")
        L = len(lab)
        cols = torch.tensor(lab, dtype=torch.int64).to(dev).expand(B, L).contiguous()
    rows_cols = cols.repeat_interleave(N, dim=0)
    Y = torch.empty((B * N, L), dtype=torch.float32, device=dev)
    img_shape = (C, H, W)
    eager = {}

    def pass_of(b):
        make = lambda: _ProbPass(model, b, img_shape, L, dev)  # noqa: E731
        if graphs:
            return _PASSES.get(model, dev, (b, img_shape, L), make)
        key = (threading.get_ident(), b)
        if key not in eager:
            eager[key] = make()
        return eager[key]

    def one_pass(lo, hi):
        p = pass_of(hi - lo)
        K.lime_compose(x, seg_t, rows, D_t, hide, lo, hi - lo, fudged=fudged, out=p.x)
        p.cols.copy_(rows_cols[lo:hi])
        Y[lo:hi].copy_((p.run() if graphs else p.eager())[0])

    run_passes(dev, B * N, pass_size, one_pass, streams, kind=("lime", id(model), int(pass_size), img_shape, L, bool(graphs)))
    LIME_COUNTS["rows"] += B * N
    Y = Y.view(B, N, L)

    cap = K.lime_max_features()
    res = K.lime_fit(rows, D_t, Y, kernel_width, ALPHA_SELECT, ALPHA, d_stride=d_stride)
    for b in [b for b in range(B) if Ds[b] > cap]:
        h = host_fit(mats[b], read_back(Y[b]).numpy(), kernel_width)
        LIME_COUNTS["host_fits"] += 1
        for k in ("coef", "order"):
            res[k][b, :, :Ds[b]] = torch.from_numpy(h[k]).to(dev)
        for k in ("intercept", "score", "local_pred", "dist", "weight"):
            res[k][b] = torch.from_numpy(h[k]).to(dev)

    if want == "weights":
        return K.lime_paint(res["coef"][:, 0].float().contiguous(), seg_t)
    # lime_image.py:68-69 with min_weight 0: the first num_features entries of the sorted explanation with a weight above 0
    order = res["order"][:, 0].long()
    at = order.clamp(min=0)
    positive = (order >= 0) & (res["coef"][:, 0].gather(1, at) > 0)
    chosen = positive & (positive.cumsum(1) <= int(num_features))
    table = torch.zeros((B, d_stride), dtype=torch.float32, device=dev).scatter_add_(1, at, chosen.float() * 3.0)
    out = K.lime_paint(table, seg_t)
    if want == "mask":
        return out
    return out, LimeDetails(mats, Y, res["dist"], res["weight"], res["coef"], res["intercept"], res["score"], res["local_pred"],
                            res["order"], cols)


def quickshift_segments(image, random_seed):
    """The reference's default segmentation (lime_image.py:177-180): skimage's quickshift with kernel_size 4, max_dist 200,
    ratio 0.2 and the drawn seed, on the host.  image: (H, W, 3)."""
    try:
        from skimage.segmentation import quickshift
    except ImportError as e:
        raise ImportError("LIME's own segmentation needs scikit-image (skimage.segmentation.quickshift), which is not installed; "
                          "without it only callers that pass segments= / segmentation_fn= work") from e
    return quickshift(np.asarray(image), kernel_size=4, max_dist=200, ratio=0.2, random_seed=random_seed)


QUICKSHIFT_ARGS = dict(kernel_size=4, max_dist=200, ratio=0.2)      # lime_image.py:177-180


def _device_segments(image, random_seed, dev):
    """LIME's quickshift of one (H, W, 3) host image on the kernels K53 - K55 -> ((H, W) int32 labels on `dev`, D).  The Lab
    features and the tie noise are made on the host in fp64 (xai_engine/quickshift.py) and uploaded; only D is read back."""
    from . import quickshift as Q
    f = Q.quickshift_features(image, QUICKSHIFT_ARGS["ratio"])
    noise = Q.tie_noise(random_seed, f.shape[0], f.shape[1])
    labels, D = Q.quickshift_batch(torch.from_numpy(f)[None].to(dev), torch.from_numpy(noise)[None].to(dev),
                                   QUICKSHIFT_ARGS["kernel_size"], QUICKSHIFT_ARGS["max_dist"])
    return labels[0], int(read_back(D)[0])


def device_quickshift_segments(image, random_seed):
    """`quickshift_segments` without skimage: the same algorithm (scikit-image 0.18.3's, fp64) with the same arguments on the current
    HIP device (K53 - K55).  image: (H, W, 3) -> (H, W) int64 ids on the host.  `lime_batch` and `explain_instance` take this
    function by identity; `lime_batch` then keeps the labels on the device."""
    return _device_segments(image, random_seed, hip_device("cuda"))[0].cpu().numpy().astype(np.int64)


def make_tensor(img):
    """limeAttr.py:8-9"""
    return torch.tensor(np.transpose(img, (2, 0, 1)))


def batch_predict(images, model, device):
    """limeAttr.py:11-20: softmax probabilities of a list of (H, W, C) images, as a host array.  `explain_instance` takes this
    function as the token for "the classifier behind `model`" and never calls it: its passes run the same forward and softmax on
    the device."""
    model.eval()
    batch = torch.stack(tuple(make_tensor(i) for i in images), dim=0).to(hip_device(device))
    with torch.no_grad():
        return torch.softmax(_logits_of(model(batch)), dim=1).cpu().numpy()


class ImageExplanation(object):
    """lime_image.py:19-86."""

    def __init__(self, image, segments):
        self.image = image
        self.segments = segments
        self.intercept = {}
        self.local_exp = {}
        self.local_pred = None

    def get_image_and_mask(self, label, positive_only=True, negative_only=False, hide_rest=False, num_features=5, min_weight=0.):
        """-> (image, mask): the image with the explanation's superpixels shown (the rest zero with `hide_rest`) and the integer mask
        of the first `num_features` superpixels of `label`'s explanation: 1 for the ones kept by `positive_only` (weight above 0
        and `min_weight`) or `negative_only`; with neither, 1 / -1 by sign, the superpixel's channel 1 / 0 set to the image's maximum."""
        if label not in self.local_exp:
            raise KeyError('Label not in explanation')
        if positive_only & negative_only:
            raise ValueError("Positive_only and negative_only cannot be true at the same time.")
        segments, image, exp = self.segments, self.image, self.local_exp[label]
        mask = np.zeros(segments.shape, segments.dtype)
        temp = np.zeros(image.shape) if hide_rest else image.copy()
        if positive_only or negative_only:
            if positive_only:
                fs = [f for f, w in exp if w > 0 and w > min_weight][:num_features]
            if negative_only:
                fs = [f for f, w in exp if w < 0 and abs(w) > min_weight][:num_features]
            for f in fs:
                temp[segments == f] = image[segments == f].copy()
                mask[segments == f] = 1
            return temp, mask
        for f, w in exp[:num_features]:
            if np.abs(w) < min_weight:
                continue
            c = 0 if w < 0 else 1
            mask[segments == f] = -1 if w < 0 else 1
            temp[segments == f] = image[segments == f].copy()
            temp[segments == f, c] = np.max(image)
        return temp, mask


class LimeImageExplainer(object):
    """lime_image.py:89-220 on the HIP path, for what the harness uses: the exponential kernel on cosine distances, the
    'highest_weights' selection the reference's num_features=100000 leads to, the default Ridge."""

    def __init__(self, kernel_width=.25, kernel=None, verbose=False, feature_selection='auto', random_state=None):
        if kernel is not None:
            _refuse(["kernel"], "LimeImageExplainer")
        if feature_selection not in ("auto", "highest_weights"):
            _refuse([f"feature_selection={feature_selection!r}"], "LimeImageExplainer")
        self.kernel_width = float(kernel_width)
        self.verbose = verbose
        self.feature_selection = feature_selection
        self.random_state = _random_state(random_state)

    def explain_instance(self, image, classifier_fn, model, device, labels=(1,), hide_color=None, top_labels=5, num_features=100000,
                         num_samples=1000, batch_size=10, segmentation_fn=None, distance_metric='cosine', model_regressor=None,
                         random_seed=None):
        """-> ImageExplanation.  image: (H, W, 3) array (a 2-d one is repeated to three channels); classifier_fn: this module's
        `batch_predict`; segmentation_fn: a host callable image -> (H, W) ids (None: quickshift, needs skimage;
        `device_quickshift_segments`, taken by identity: quickshift on the device with the drawn seed); batch_size: rows per
        classifier pass, the reference's default of 10 being what this engine replaces (-> PASS_SIZE)."""
        name = "LimeImageExplainer.explain_instance"
        if classifier_fn is not batch_predict:
            raise NotImplementedError(f"{name}: classifier_fn must be xai_engine.lime.batch_predict (limeAttr.batch_predict of the "
                                      "mirror): the passes run `softmax(model(batch))` on the device, another function cannot be served")
        unsupported = []
        if model_regressor is not None:
            unsupported.append("model_regressor")
        if distance_metric != "cosine":
            unsupported.append(f"distance_metric={distance_metric!r}")
        _refuse(unsupported, name)
        image = np.asarray(image)
        if len(image.shape) == 2:
            image = np.stack([image] * 3, axis=-1)           # skimage.color.gray2rgb
        if random_seed is None:
            random_seed = draw_seed(self.random_state)
        if segmentation_fn is None:
            segments = quickshift_segments(image, random_seed)
        elif segmentation_fn is device_quickshift_segments:
            segments = _device_segments(image, random_seed, hip_device(device))[0].cpu().numpy().astype(np.int64)
        else:
            segments = segmentation_fn(image)
        seg32, D = check_segments(segments, name)
        if int(num_features) < D or (self.feature_selection == "auto" and int(num_features) <= 6):
            raise NotImplementedError(f"{name}: num_features={num_features} with {D} superpixels selects features by forward selection "
                                      "or truncates them; only the reference's own call (every feature, 'highest_weights') is served")
        n = int(batch_size)
        if n < 1:
            raise ValueError(f"{name}: batch_size must be >= 1")
        dev = hip_device(device)
        data = draw_data(self.random_state, int(num_samples), D)
        x = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1), dtype=np.float32))[None].to(dev)
        hide = hide_color
        if hide_color is None:
            fudged = segment_mean_image(image, segments)
            hide = torch.from_numpy(np.ascontiguousarray(fudged.transpose(2, 0, 1), dtype=np.float32))[None].to(dev)
        model.eval()
        _, det = lime_batch(x, model, seg32, num_samples=num_samples, top_labels=top_labels, labels=labels, hide_color=hide,
                            kernel_width=self.kernel_width, data=[data], pass_size=PASS_SIZE if n == REFERENCE_BATCH else n,
                            want="details")
        ret_exp = ImageExplanation(image, np.asarray(segments))
        top = [int(v) for v in read_back(det.top_labels[0]).tolist()]
        if top_labels:
            ret_exp.top_labels = list(top)
        coef, order = read_back(det.coef[0]).numpy(), read_back(det.order[0]).numpy()
        icpt, score, pred = (read_back(t[0]).numpy() for t in (det.intercept, det.score, det.local_pred))
        for i, label in enumerate(top):
            ret_exp.intercept[label] = float(icpt[i])
            ret_exp.local_exp[label] = [(int(f), float(coef[i, f])) for f in order[i, :D]]
        # the reference's loop leaves the score and local_pred of the label it fits last (:213-219): with top_labels that is the
        # most probable one (it walks `top` in ascending probability, :210-213), else the last of `labels`
        last = 0 if top_labels else len(top) - 1
        ret_exp.score, ret_exp.local_pred = float(score[last]), np.array([pred[last]])
        ret_exp.details = det
        return ret_exp


def get_lime_attr(img, model, device):
    """limeAttr.py:23-36: the mask of the five most positive superpixels of the top class, times ones(3, H, W)."""
    explainer = LimeImageExplainer()
    explanation = explainer.explain_instance(img, batch_predict, model, device, top_labels=5, hide_color=0, num_samples=1000)
    _, mask = explanation.get_image_and_mask(explanation.top_labels[0], positive_only=True, hide_rest=False)
    return torch.tensor(mask.reshape(1, mask.shape[0], mask.shape[1])) * torch.ones((3, mask.shape[0], mask.shape[1]))
