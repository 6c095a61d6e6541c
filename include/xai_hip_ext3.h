/*
 * xai_hip_ext3.h -- C ABI of libxai_ext3.so, the third extension library beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11, include/xai_hip_ext.h at 1.0 and include/xai_hip_ext2.h at 1.1 (MDA and the sanity
 * test); entry points added after that live here, in a library of their own with a version pair of its own.  The grammar is
 * xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int and take the
 * caller's stream last), so xai_engine/_lib.py binds all four headers with the same strict reader, and so are the conventions:
 * device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state.
 * Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so) has the
 * text.  Every argument check comes before the first HIP call, so a refused call needs no device.
 */
#ifndef XAI_HIP_EXT3_H
#define XAI_HIP_EXT3_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext3_version() = XAI_EXT3_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext3_version_minor() = XAI_EXT3_MINOR: bumped whenever entry points are added:
 *   0 = xai_seg_max_hw, xai_seg_max_thresholds, xai_seg_normalize_f32, xai_seg_counts_i32 */
#define XAI_EXT3_VERSION 1
#define XAI_EXT3_MINOR 0

int xai_ext3_version(void);
int xai_ext3_version_minor(void);

/* ---- ImageNet-segmentation evaluation (xai_engine/segeval.py): the per-image scoring of evaluateImageNetSeg.py ---- */

/* the largest map size hw K44 takes (2^30 elements), and the largest number of thresholds T of K45 (16) */
int xai_seg_max_hw(void);
int xai_seg_max_thresholds(void);

/* K44 per map m < n, in fp32:
 *       mn, mx = min, max of x[m] with torch's rule: one NaN makes both NaN (a zero extreme may come back as either +0 or -0)
 *       out[m] = (x[m] - mn) / (mx - mn): one subtraction and one true division, each rounded once.  +-Inf is NOT replaced (K39 of
 *           xai_hip_ext2.h does that; it is another function): a map with an Inf gets 0 at its finite pixels and NaN at the Inf.
 *           A constant map becomes all NaN (0 / 0).
 *       stats[m] = {mn, mx}
 *       thr[m] = fp32(S / hw), a division in fp64, where S is the fp64 sum of the fp32 values out[m][i] in this fixed tree:
 *           lane t of 1024 owns the elements i with (i / 4) % 1024 == t and adds them in ascending i, starting from +0.0;
 *           the 64 lanes of a wave are combined by an xor butterfly with offsets 32, 16, 8, 4, 2, 1 (a + b at both partners);
 *           the 16 wave sums are added in ascending wave order, starting from +0.0.
 *           The tree does not depend on which access width was used.  A NaN anywhere in out[m] gives thr[m] = NaN.
 * replaces  evaluateImageNetSeg.py:215-217 (get_CNN_attr), :332-334 (get_VIT_attr) and :463-465 (get_CLIP_attr):
 *           Res = (Res - Res.min()) / (Res.max() - Res.min());  ret = Res.mean()   -- torch's own mean() order is not pinned
 *   x, out : [n][hw] (out may be x);  thr : [n];  stats : [n][2]
 *   16-byte accesses when hw % 4 == 0 and x, out are 16-byte aligned, scalar ones otherwise
 *   NULL -> XAI_E_NULL;  n <= 0 or hw <= 0 -> XAI_E_SHAPE;  hw > xai_seg_max_hw() -> XAI_E_UNSUPPORTED */
int xai_seg_normalize_f32(const float* x, int n, int64_t hw, float* out, float* thr, float* stats, xai_stream_t stream);

/* K45 the count table every score of the evaluation is a function of.  For map m < n, threshold t < T, image row r < H:
 *       counts[m][t][r][l][s] = the number of pixels of row r with labels == l (0 or 1) in prediction state s:
 *           s = 0: res <= thr[m][t];  s = 1: res > thr[m][t];  s = 2: neither (a NaN pixel or a NaN threshold)
 *       other[m] = the number of pixels of map m whose label is neither 0 nor 1; such a pixel enters no cell
 *     so the six cells of a row add up to W minus that row's other-label pixels.  Every cell has one owner (one wave per row and
 *     threshold set; one workgroup per other[m]): no atomics, nothing to zero beforehand, the same bytes on every run.  A pixel
 *     is read once for all T thresholds.
 * replaces  evaluateImageNetSeg.py:471-472 and :348-349 (Res.gt(ret), Res.le(ret)) and the pixel passes of metrices.py:136-158
 *           (batch_pix_accuracy), :161-184 (batch_intersection_union), :82-100 (get_ap_scores) and :26-39 (get_f1_scores, whose
 *           "batch" is the image row)
 *   res : [n][H][W];  labels : [n][H][W] int32;  thr : [n][T];  counts : [n][T][H][2][3] int32;  other : [n] int32
 *   NULL -> XAI_E_NULL;  n, H, W or T <= 0 -> XAI_E_SHAPE;  T > xai_seg_max_thresholds(), n > 65535 or H * W > xai_seg_max_hw()
 *   -> XAI_E_UNSUPPORTED */
int xai_seg_counts_i32(const float* res, const int32_t* labels, const float* thr, int n, int H, int W, int T, int32_t* counts,
                       int32_t* other, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT3_H */
