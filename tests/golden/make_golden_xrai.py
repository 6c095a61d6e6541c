"""Regenerate tests/golden/xrai.npz and tests/golden/xrai_api.json from the reference project.

    XAI_REFERENCE_ROOT=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_xrai.py

The reference's own _unpack_segs_to_masks, XRAI._xrai, XRAI._xrai_fast and XRAI().GetMaskWithDetails(segments=...,
base_attribution=...) (util/attribution_methods/XRAIBuilder.py:287-292, :415-789) run unmodified, on the CPU.  Its four skimage
imports (:30-33) are satisfied by empty stub modules in sys.modules: no skimage function runs when segments are passed.  The
dilation of :256-258 is scipy's binary_dilation with the disk footprint (checked here to equal grey_dilation with the reflecting
border, which is what skimage's dilation calls).

Inputs (tests/xrai_restated.seeded_case): seeded Voronoi label maps at several granularities, stored as int16, and a smoothed
seeded (H, W, 3) attribution, at 40 x 36 and 65 x 63 only.  Per case <tag>: <tag>_keys, <tag>_gains (a wrapper around
_gain_density logs every candidate gain; the selections are recovered from the log), <tag>_out (float32: the reference's float64
array holds float32 values), <tag>_ranks, <tag>_cond = [margin, gain_err] (the smallest margin between a winner and the best
candidate with a different pixel set, by the fp64 restatement; the largest |float32 gain - fp64 gain| over all logged candidates)
and <tag>_params = [input index, radius, min_pixel_diff, area_threshold, fast].  Every case is held to
margin >= 100 * gain_err and to equal selections of the reference and the fp64 restatement; a seed that fails is not used.

xrai_api.json: parameter names and defaults (inspect.signature) of the public methods.
"""
import inspect
import json
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XAI_REFERENCE_ROOT")
if not REF or not os.path.isdir(REF):
    sys.exit("make_golden_xrai.py: set XAI_REFERENCE_ROOT to the root of a checkout of the reference project")
sys.dont_write_bytecode = True
for name in ("skimage", "skimage.segmentation", "skimage.morphology", "skimage.transform"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["skimage"].segmentation = sys.modules["skimage.segmentation"]
sys.modules["skimage.morphology"].dilation = sys.modules["skimage.morphology"].disk = sys.modules["skimage.transform"].resize = None
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from util.attribution_methods import XRAIBuilder as X  # noqa: E402
import xrai_restated as R                               # noqa: E402

# (H, W, cells per label map, seed)
INPUTS = [(40, 36, (12, 5, 2), 1), (40, 36, (12, 5, 2), 2), (65, 63, (30, 12, 4), 1), (65, 63, (30, 12, 4), 2)]
# tag: (input, radius, min_pixel_diff, area_threshold, fast)
CASES = {"a": (0, 2, 50, 1.0, 0), "b": (1, 5, 1, 1.0, 0), "c": (2, 5, 50, 1.0, 0), "d": (3, 5, 50, 0.3, 0),
         "e": (0, 2, 50, 1.0, 1), "f": (3, 5, 1, 1.0, 1)}
API_CASE = "c"


def masks_of(maps, radius):
    masks = X._unpack_segs_to_masks([m.astype(int) for m in maps])
    if radius:
        fp = R.disk(radius)
        zero = [ndimage.binary_dilation(m, structure=fp) for m in masks]
        assert all(np.array_equal(z, ndimage.grey_dilation(m, footprint=fp)) for z, m in zip(zero, masks)), "reflect != zero border"
        masks = zero
    return masks


def run(attr, masks, mpd, th, fast):
    log = []

    def logged(mask1, a, mask2=None):
        g = X._gain_density(mask1, a, mask2)
        sel = mask1 if mask2 is None else X._get_diff_mask(mask1, mask2)
        if np.any(sel):
            log.append(abs(float(g) - float(a.astype(np.float64)[sel].sum() / np.count_nonzero(sel))))
        return g
    if fast:
        out, ranks = X.XRAI._xrai_fast(attr, masks, gain_fun=logged, min_pixel_diff=mpd)
        mine32, mine64 = R.xrai_fast(attr, masks, mpd, np.float32), R.xrai_fast(attr, masks, mpd, np.float64)
    else:
        out, ranks = X.XRAI._xrai(attr, masks, gain_fun=logged, area_perc_th=th, min_pixel_diff=mpd)
        mine32, mine64 = R.xrai(attr, masks, th, mpd, np.float32), R.xrai(attr, masks, th, mpd, np.float64)
    # the reference returns no keys: they are the float32 restatement's, whose out and ranks equal the reference's to the bit
    assert np.array_equal(out, mine32["out"]) and np.array_equal(ranks, mine32["ranks"]), "the float32 restatement left the reference"
    assert np.array_equal(mine32["keys"], mine64["keys"]) and np.array_equal(mine32["pixel_iter"], mine64["pixel_iter"]), "fp64 selects otherwise"
    margin, gain_err = mine64["margin"], max(log)
    assert margin >= 100 * gain_err, ("ill conditioned", margin, gain_err)
    assert np.array_equal(out, out.astype(np.float32))
    return out, ranks, mine32["keys"], mine32["gains"], margin, gain_err


def sig(fn, drop_self):
    params = list(inspect.signature(fn).parameters.values())[1 if drop_self else 0:]
    return [{"name": p.name, "has_default": p.default is not inspect.Parameter.empty,
             "default": None if p.default is inspect.Parameter.empty else p.default} for p in params]


def main():
    store = {}
    inputs = [R.seeded_case(H, W, counts, seed) for H, W, counts, seed in INPUTS]
    for i, (maps, attr3) in enumerate(inputs):
        store[f"in{i}_maps"], store[f"in{i}_attr"] = maps, attr3
    for tag, (i, radius, mpd, th, fast) in CASES.items():
        maps, attr3 = inputs[i]
        masks = masks_of(maps, radius)
        out, ranks, keys, gains, margin, gain_err = run(X._attr_aggregation_max(attr3), masks, mpd, th, fast)
        store.update({f"{tag}_out": out.astype(np.float32), f"{tag}_ranks": ranks.astype(np.int16), f"{tag}_keys": keys.astype(np.int16),
                      f"{tag}_gains": gains, f"{tag}_cond": np.array([margin, gain_err]),
                      f"{tag}_params": np.array([i, radius, mpd, th, fast], np.float64)})
        print(f"{tag}: {out.shape} masks {len(masks)} selections {len(keys)} uncomputed {int((ranks == len(keys) + 1).sum())} "
              f"margin {margin:.3e} gain_err {gain_err:.3e} relative margin {margin / np.abs(gains).max():.3e}")
    # the public entry: segments and base attribution passed, default parameters + the rank image, then the mask list
    i, radius = CASES[API_CASE][:2]
    maps, attr3 = inputs[i]
    masks = masks_of(maps, radius)
    p = X.XRAIParameters(return_xrai_segments=True)
    res = X.XRAI().GetMaskWithDetails(np.zeros_like(attr3), segments=masks, base_attribution=attr3, extra_parameters=p)
    assert res.attribution_mask.dtype == np.float64
    store["api_mask"], store["api_segments"] = res.attribution_mask.astype(np.float32), res.segments.astype(np.int16)
    p.flatten_xrai_segments = False
    res = X.XRAI().GetMaskWithDetails(np.zeros_like(attr3), segments=masks, base_attribution=attr3, extra_parameters=p)
    store["api_mask_list"] = np.packbits(np.stack(res.segments), axis=None)
    store["api_mask_count"] = np.int64(len(res.segments))
    np.savez_compressed(os.path.join(HERE, "xrai.npz"), **store)

    api = {"XRAI.GetMask": sig(X.XRAI.GetMask, True), "XRAI.GetMaskWithDetails": sig(X.XRAI.GetMaskWithDetails, True),
           "XRAIParameters.__init__": sig(X.XRAIParameters.__init__, True), "XRAIOutput.__init__": sig(X.XRAIOutput.__init__, True),
           "call_model_function": sig(X.call_model_function, False)}
    with open(os.path.join(HERE, "xrai_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
    for n in ("xrai.npz", "xrai_api.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
