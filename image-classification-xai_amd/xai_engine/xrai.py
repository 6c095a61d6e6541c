"""XRAI (reference util/attribution_methods/XRAIBuilder.py) on the HIP kernels K29 / K30.

XRAI ranks image segments by the density of a base attribution: it starts from an empty mask and repeatedly adds the segment
whose not-yet-covered pixels have the largest mean attribution (XRAI._xrai, :619-711).  The reference walks every remaining
boolean mask over all H*W pixels in every iteration, on the host; here the masks are packed once into 64-bit planes
(`pack_segments`: K29, which also unpacks label maps, :287-292, and dilates, :256-258) and the whole greedy loop of every image
of a batch runs in one launch (`xrai_batch`: K30, one workgroup per image).  The base attribution comes from this engine too
(`ig.IG`, evaluatePerturbation.py:144).

`XRAI`, `XRAIParameters`, `XRAIOutput` keep the reference's signatures (:295-616; the mirror module
util/attribution_methods/XRAIBuilder.py serves them).  The segmentation itself (Felzenszwalb) is skimage's on the host by default,
the reference's dependency: `felzenszwalb_label_maps` calls it when skimage is installed.  `device_felzenszwalb_label_maps` computes
the same six maps on the kernels K69-K74 (xai_engine/felzenszwalb.py) and needs no skimage: `segments="device"`.  Callers that pass
their own `segments=` need neither.
"""
import collections

import numpy as np
import torch

from . import kernels as K
from .ig import check_input, hip_device
from .streams import read_back

# :37-41 (the resize to 224 x 224 is off in the reference's call, :583 -> :200-203)
FELZENSZWALB_SCALE_VALUES = [50, 100, 150, 250, 500, 1200]
FELZENSZWALB_SIGMA_VALUES = [0.8]
FELZENSZWALB_IM_VALUE_RANGE = [-1.0, 1.0]
FELZENSZWALB_MIN_SEGMENT_SIZE = 150

PackedSegments = collections.namedtuple("PackedSegments", "bits span mask_first counts H W")
PackedSegments.__doc__ = """Device-resident segments of a batch: bits (M, ceil(H*W/64)) int64 planes, span (M, 2) int32, mask_first
(B + 1,) int32 on the device, counts = the masks of every image (host list)."""
XraiRanking = collections.namedtuple("XraiRanking", "pixel_iter sel_key sel_gain n_sel n_uncomputed")
XraiRanking.__doc__ = """What `xrai_batch(..., want_segments=True)` adds: pixel_iter (B, H, W) int32 on the device (the selection that
covered a pixel, -1 = uncomputed), per image the selected keys and gains in selection order (device tensors), and the
selection / uncomputed-pixel counts (host lists)."""


def _is_mask_dtype(dt):
    return dt in (torch.bool, torch.uint8, np.dtype(bool), np.dtype(np.uint8))


def _one_image(entry):
    """-> ("labels" | "masks", (n, H, W) torch tensor) or None for an image without segments."""
    if isinstance(entry, (list, tuple)):
        if len(entry) == 0:
            return None
        entry = torch.stack([torch.as_tensor(np.asarray(e) if not torch.is_tensor(e) else e) for e in entry])
    t = entry if torch.is_tensor(entry) else torch.as_tensor(np.ascontiguousarray(entry))
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3:
        raise ValueError(f"segments of one image must be (n, H, W) label maps or masks, got {tuple(t.shape)}")
    if _is_mask_dtype(t.dtype):
        return "masks", t
    if t.is_floating_point():
        raise TypeError("label maps must have an integer dtype, boolean masks bool or uint8")
    return "labels", t


def _pack_group(kind, tensors, H, W, radius, dev):
    """One K29 call for the images of a batch (all label maps or all masks) -> bits, span, masks per image."""
    if kind == "masks":
        counts = [int(t.shape[0]) for t in tensors]
        masks = torch.cat([t.to(dev).to(torch.uint8) for t in tensors]).contiguous()
        bits, span = K.xrai_pack(H, W, radius, sum(counts), masks=masks)
        return bits, span, counts
    lo = [[int(v) for v in t.reshape(t.shape[0], -1).amin(1).tolist()] for t in tensors]
    hi = [[int(v) for v in t.reshape(t.shape[0], -1).amax(1).tolist()] for t in tensors]
    counts = [sum(b - a + 1 for a, b in zip(l, h)) for l, h in zip(lo, hi)]
    labels = torch.cat([t.to(dev).to(torch.int32) for t in tensors]).contiguous()
    label_min = torch.tensor([v for l in lo for v in l], dtype=torch.int32).to(dev)
    label_max = torch.tensor([v for h in hi for v in h], dtype=torch.int32).to(dev)
    bits, span = K.xrai_pack(H, W, radius, sum(counts), labels=labels, label_min=label_min, label_max=label_max)
    return bits, span, counts


def pack_segments(segs_or_label_maps, dilation_rad=5, device=None, shape=None):
    """Segments -> `PackedSegments` on the HIP device (K29).

    One image: integer label maps (S, H, W) -- one mask per label in [min, max] of every map, in order, absent labels as empty
    masks that keep their index (_unpack_segs_to_masks, :287-292) -- or boolean / uint8 masks (M, H, W), or a list of (H, W)
    masks.  A batch: a list with one such entry per image (an empty list for an image without segments), or a 4-d array.
    Every mask is dilated with skimage's disk(dilation_rad) (:256-258); 0 or None only packs.
    `device`: where to pack (default: the device of a device tensor among the segments, else the current HIP device);
    `shape`: (H, W), needed only when no image has a segment."""
    entries = segs_or_label_maps
    if torch.is_tensor(entries) or isinstance(entries, np.ndarray):
        entries = list(entries) if entries.ndim == 4 else [entries]
    elif isinstance(entries, (list, tuple)):
        first = entries[0] if len(entries) else None
        if first is None or (not isinstance(first, (list, tuple)) and np.ndim(first) == 2):
            entries = [entries]                                      # one image given as a list of (H, W) masks
    else:
        raise TypeError("segments must be arrays, tensors or lists of them")
    images = [_one_image(e) for e in entries]
    tensors = [im[1] for im in images if im is not None]
    if device is None:
        device = next((t.device for t in tensors if t.is_cuda), "cuda")
    dev = hip_device(device)
    if tensors:
        H, W = (int(v) for v in tensors[0].shape[1:])
        if any(tuple(t.shape[1:]) != (H, W) for t in tensors):
            raise ValueError("all segments of a batch must have one (H, W)")
    elif shape is not None:
        H, W = (int(v) for v in shape)
    else:
        raise ValueError("pack_segments: no segments at all; pass shape=(H, W)")
    radius = int(dilation_rad or 0)
    if radius < 0:
        raise ValueError("dilation_rad must be >= 0")
    kinds = {im[0] for im in images if im is not None}
    if len(kinds) > 1:
        raise ValueError("pack_segments: label maps and masks cannot be mixed in one batch")
    counts = [0] * len(images)
    if tensors:                                                      # one launch for the whole batch
        bits, span, cnt = _pack_group(kinds.pop(), tensors, H, W, radius, dev)
        for i, c in zip([i for i, im in enumerate(images) if im is not None], cnt):
            counts[i] = c
    else:
        bits = torch.empty((0, K.xrai_words(H, W)), dtype=torch.int64, device=dev)
        span = torch.empty((0, 2), dtype=torch.int32, device=dev)
    mask_first = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    return PackedSegments(bits, span, mask_first, counts, H, W)


def xrai_batch(attr, segments, area_threshold=1.0, min_pixel_diff=50, algorithm="full", want_segments=False):
    """XRAI maps of B independent images in one launch of K30.

    attr: (B, C, H, W) base attribution on a HIP device, reduced by max over C first (_attr_aggregation_max, :262), or (B, H, W).
    segments: a `PackedSegments` of the same B images, or whatever `pack_segments` takes (packed as given, without dilation).
    -> out (B, H, W) float32 on the device: every pixel holds the gain of the selection that covered it, the uncomputed ones
    the mean attribution over them (:699-701) [and, with want_segments, an `XraiRanking`].
    algorithm: "full" (XRAI._xrai) or "fast" (_xrai_fast, which ignores area_threshold)."""
    if algorithm not in ("full", "fast"):
        raise ValueError(f"Unknown algorithm type: {algorithm}")
    if int(min_pixel_diff) < 1:
        raise NotImplementedError("xrai: min_pixel_diff < 1 is not supported: the reference then never drops a mask that adds "
                                  "nothing, loops over empty masks and crashes (XRAIBuilder.py:667-682)")
    if torch.is_tensor(attr) and attr.dim() == 3:
        attr = attr.unsqueeze(1)
    a = check_input(attr, "xrai_batch")
    a = (torch.amax(a, dim=1) if a.shape[1] > 1 else a[:, 0]).contiguous()
    B, H, W = a.shape
    if not isinstance(segments, PackedSegments):
        segments = pack_segments(segments, dilation_rad=0, device=a.device, shape=(H, W))
    if (segments.H, segments.W) != (H, W) or len(segments.counts) != B:
        raise ValueError(f"xrai: the segments are of {len(segments.counts)} images of {segments.H} x {segments.W}, "
                         f"the attribution of {B} images of {H} x {W}")
    out, pixel_iter, sel_key, sel_gain, state = K.xrai_rank(a, segments.bits, segments.span, segments.mask_first,
                                                            int(min_pixel_diff), float(area_threshold), algorithm == "fast")
    st = read_back(state).tolist()
    for i, (n_sel, n_unc, status, _) in enumerate(st):
        if status != 0:
            raise ValueError(f"xrai: image {i}, after {n_sel} selections: {K.XRAI_STATUS.get(status, 'unknown status')}")
    if not want_segments:
        return out
    first = np.concatenate([[0], np.cumsum(segments.counts)])
    keys = [sel_key[int(first[i]):int(first[i]) + st[i][0]] for i in range(B)]
    gains = [sel_gain[int(first[i]):int(first[i]) + st[i][0]] for i in range(B)]
    return out, XraiRanking(pixel_iter, keys, gains, [s[0] for s in st], [s[1] for s in st])


def ranked_segments(pixel_iter, sel_gain, flatten=True):
    """The second return value of XRAI._xrai (:702-711) from K30's outputs (host arrays of one image): the selections in a stable
    order of descending gain, the uncomputed pixels last; as the (H, W) rank image (1 = most important) or the mask list."""
    pixel_iter = np.asarray(pixel_iter)
    order = np.argsort(-np.asarray(sel_gain, dtype=np.float32), kind="stable")
    uncomputed = pixel_iter < 0
    if flatten:
        rank_of = np.empty(len(order) + 1, dtype=int)
        rank_of[order] = np.arange(1, len(order) + 1)
        rank_of[-1] = len(order) + 1                                 # pixel_iter -1
        return rank_of[pixel_iter]
    masks = [pixel_iter == s for s in order]
    if uncomputed.any():
        masks.append(uncomputed)
    return masks


def _normalize_image(x_hwc):
    """_normalize_image (:186-189) to FELZENSZWALB_IM_VALUE_RANGE, on the host in the image's dtype -> a host tensor"""
    im = x_hwc.detach().cpu() if torch.is_tensor(x_hwc) else torch.as_tensor(np.asarray(x_hwc))
    lo, hi = FELZENSZWALB_IM_VALUE_RANGE
    im_max, im_min = torch.max(im), torch.min(im)
    im = (im - im_min) / (im_max - im_min)
    return im * (hi - lo) + lo


def device_felzenszwalb_label_maps(x_hwc, device=None):
    """`felzenszwalb_label_maps` on the kernels K69-K74, without skimage: x_hwc one (H, W, C) image or a (B, H, W, C) batch (every
    image rescaled by its own extremes, on the host as above) -> (6, H, W) or (B, 6, H, W) int32 label maps on the HIP device, for
    `pack_segments(..., dilation_rad=5)`.  The six scales share one smoothing, one set of costs and one sort."""
    from . import felzenszwalb as F
    x = x_hwc if torch.is_tensor(x_hwc) else torch.as_tensor(np.asarray(x_hwc))
    if x.dim() not in (3, 4):
        raise ValueError(f"device_felzenszwalb_label_maps: expected (H, W, C) or (B, H, W, C), got {tuple(x.shape)}")
    if device is None:
        device = x.device if x.is_cuda else "cuda"
    images = torch.stack([_normalize_image(im) for im in (x if x.dim() == 4 else x[None])])
    assert FELZENSZWALB_SIGMA_VALUES == [0.8]
    labels, _ = F.felzenszwalb_batch(images.to(torch.float64).numpy(), FELZENSZWALB_SCALE_VALUES, FELZENSZWALB_SIGMA_VALUES[0],
                                     FELZENSZWALB_MIN_SEGMENT_SIZE, device=device)
    return labels if x.dim() == 4 else labels[0]


def felzenszwalb_label_maps(x_hwc):
    """The six Felzenszwalb label maps XRAI segments an (H, W, C) image with (_get_segments_felzenszwalb, :230-254, without the
    resize): the image rescaled to [-1, 1] as _normalize_image does (:186-189), scales 50 ... 1200, sigma 0.8, min_size 150
    (:37-41, :241-246) -> (6, H, W) integer array for `pack_segments(..., dilation_rad=5)`.  Runs on the host, in skimage."""
    try:
        from skimage import segmentation
    except ImportError as e:
        raise ImportError("XRAI's own segmentation needs scikit-image (skimage.segmentation.felzenszwalb), which is not installed; "
                          "without it pass segments=, or opt in to the device segmenter: XRAI.GetMask(..., segments=\"device\"), "
                          "testing_dict[\"xrai_felzenszwalb\"] = \"device\", --xrai_felzenszwalb device") from e
    im = _normalize_image(x_hwc).numpy()
    segs = []
    for scale in FELZENSZWALB_SCALE_VALUES:
        for sigma in FELZENSZWALB_SIGMA_VALUES:
            segs.append(np.asarray(segmentation.felzenszwalb(im, scale=scale, sigma=sigma, min_size=FELZENSZWALB_MIN_SEGMENT_SIZE)))
    return np.stack(segs)


def call_model_function(images, model, device, call_model_args=None, expected_keys=None):
    """The gradient of the target class's softmax probability (XRAIBuilder.py:376-390), on the HIP device; the same function as
    Guided IG's."""
    from .guided_ig import call_model_function as gig_call
    return gig_call(images, model, device, call_model_args=call_model_args, expected_keys=expected_keys)


class XRAIParameters(object):
    """Parameters of XRAI.GetMask / GetMaskWithDetails (XRAIBuilder.py:295-344)."""

    def __init__(self, steps=100, area_threshold=1.0, return_baseline_predictions=False, return_ig_attributions=False,
                 return_xrai_segments=False, flatten_xrai_segments=True, algorithm='full'):
        self.steps = steps
        self.area_threshold = area_threshold
        self.return_ig_attributions = return_ig_attributions
        self.return_xrai_segments = return_xrai_segments
        self.flatten_xrai_segments = flatten_xrai_segments
        self.algorithm = algorithm
        self.experimental_params = {'min_pixel_diff': 50}


class XRAIOutput(object):
    """Output of XRAI.GetMaskWithDetails (XRAIBuilder.py:347-374)."""

    def __init__(self, attribution_mask):
        self.attribution_mask = attribution_mask
        self.baselines = None
        self.ig_attribution = None
        self.segments = None


class XRAI(object):
    """XRAI with the reference's interface (XRAIBuilder.py:392-616) on the current HIP device.  As in the reference, the base
    attribution has to be passed (its GetMaskWithDetails has no model to compute one with and fails on `attr` when it is None)."""

    def GetMask(self, x_value, baselines=None, segments=None, base_attribution=None, batch_size=1, extra_parameters=None):
        return self.GetMaskWithDetails(x_value, baselines=baselines, segments=segments, base_attribution=base_attribution,
                                       batch_size=batch_size, extra_parameters=extra_parameters).attribution_mask

    def GetMaskWithDetails(self, x_value, baselines=None, segments=None, base_attribution=None, batch_size=1,
                           extra_parameters=None):
        """-> XRAIOutput: attribution_mask is the (H, W) float64 array of the float32 gains, as the reference's; segments (with
        return_xrai_segments) the rank image or the mask list of :702-711.  x_value: (H, W, C); base_attribution: the same shape
        (or (H, W)), array or tensor -- a device tensor stays on its device; segments: a list of (H, W) boolean masks, taken as
        they are, None for skimage's Felzenszwalb segmentation of x_value dilated by 5, or "device" for the same segmentation on
        the kernels K69-K74 (no skimage needed)."""
        if extra_parameters is None:
            extra_parameters = XRAIParameters()
        if extra_parameters.algorithm not in ("full", "fast"):
            raise ValueError('Unknown algorithm type: {}'.format(extra_parameters.algorithm))
        if isinstance(segments, str) and segments != "device":
            raise ValueError(f"XRAI: segments must be masks, None or 'device', got {segments!r}")
        if base_attribution is None:
            raise ValueError("XRAI.GetMask needs base_attribution (the reference's GetMaskWithDetails fails without it: `attr` is "
                             "never assigned, XRAIBuilder.py:562-577); compute it with saliencyMethods.IG as the harness does")
        if not torch.is_tensor(base_attribution) and not isinstance(base_attribution, np.ndarray):
            base_attribution = np.array(base_attribution)
        if tuple(base_attribution.shape) != tuple(x_value.shape):
            raise ValueError('The base attribution shape should be the same as the shape of `x_value`. Expected {}, got {}'.format(
                tuple(x_value.shape), tuple(base_attribution.shape)))
        attrs = base_attribution
        a = torch.as_tensor(base_attribution)
        if a.dim() not in (2, 3):
            raise ValueError(f"XRAI: the attribution must be (H, W) or (H, W, C), got {tuple(a.shape)}")
        dev = a.device if a.is_cuda else hip_device("cuda" if torch.cuda.is_available() else "cpu")
        a = a.to(dev, torch.float32)
        a = a.permute(2, 0, 1)[None] if a.dim() == 3 else a[None, None]
        H, W = a.shape[2:]
        if isinstance(segments, str):
            packed = pack_segments(device_felzenszwalb_label_maps(x_value, device=dev), dilation_rad=5, device=dev)
        elif segments is not None:
            packed = pack_segments([list(segments)], dilation_rad=0, device=dev, shape=(H, W))
        else:
            packed = pack_segments(felzenszwalb_label_maps(x_value), dilation_rad=5, device=dev)
        out, rk = xrai_batch(a, packed, area_threshold=extra_parameters.area_threshold,
                             min_pixel_diff=extra_parameters.experimental_params['min_pixel_diff'],
                             algorithm=extra_parameters.algorithm, want_segments=True)
        results = XRAIOutput(out[0].cpu().numpy().astype(np.float64))
        if extra_parameters.return_xrai_segments:
            results.segments = ranked_segments(rk.pixel_iter[0].cpu().numpy(), rk.sel_gain[0].cpu().numpy(),
                                               extra_parameters.flatten_xrai_segments)
        if extra_parameters.return_ig_attributions:
            results.ig_attribution = attrs
        return results
