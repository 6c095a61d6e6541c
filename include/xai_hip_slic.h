/*
 * xai_hip_slic.h -- C ABI of libxai_slic.so: SLIC superpixels (Achanta et al., TPAMI 2012) as scikit-image 0.18.3 computes them, for
 * MDA's segmentation (xai_engine/slic.py, xai_engine/mda.py).
 *
 * The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int and
 * take the caller's stream last), so xai_engine/_lib.py binds this header with the same strict reader, and so are the conventions:
 * device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state, no
 * memset enqueued, the same bytes on every run.  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the
 * launch; xai_strerror (libxai_hip.so) has the text.  Every argument check comes before the first HIP call, so a refused call needs no
 * device.  The only atomics are integer ones (an OR into the status word, an add into a component's size): their result does not
 * depend on their order.
 *
 * The definition is the binary of scikit-image 0.18.3: skimage/segmentation/slic_superpixels.py:298-328 calls _slic_cython and
 * _enforce_label_connectivity_cython of _slic.pyx; the steps are cited below by those lines.  T is float (_f32) or double (_f64), one
 * template; every operation is rounded once, in the order written (the library is compiled with -ffp-contract=off).  Every entry takes
 * a leading image count B: per-image features, centres and outputs, shared H, W, C, S and step.
 *
 * THE K-MEANS CONTRACT (slic_superpixels.py:316-318, `labels = _slic_cython(image, mask, segments, step, max_iter, spacing, ...)` with
 * a depth of 1, spacing 1, no mask, slic_zero off)
 *   features [B][H][W][C] T: skimage's `image * (1 / compactness)`;  centres [B][S][2 + C] T: (y, x, c_0 .. c_{C-1}), skimage's
 *   `segments` without its z column, which is 0 and stays 0;  step: `max(steps)`, an integer in value
 *   an iteration = an assignment, then an update; exactly max_iter of them run (skimage's early stop never fires: its distances are
 *   reset every iteration); the labels are those of the last assignment
 *   the window of cluster k:  rows [trunc(max(cy - 2 step, 0)), trunc(min(cy + 2 step + 1, H))), columns the same with cx and W, the
 *     bounds computed in T.  Both ends are then clamped to [0, H] ([0, W]), which changes no window that holds a pixel; a centre
 *     coordinate that is NaN has the empty window
 *   assignment: dist starts at DBL_MAX converted to T (+inf in float); the clusters are visited in ascending k; inside the window
 *     d = ((cy - y)^2 + (cx - x)^2) * (1 / (step * step)) + (((0 + c_0^2) + c_1^2) + ...),  c_i = feature_i - centre_i
 *     a pixel takes k when dist > d, strictly: the lowest k wins a tie, a NaN d takes nothing
 *   update: per cluster a count and the sums of y, x and the channels over its pixels, in T, from +0, sequentially in raster order;
 *     then sum / T(count)
 * Two states skimage leaves undefined are reported in `status`, never guessed: a pixel that took no cluster (label -1 here) and a
 * cluster without a pixel (its centre becomes 0 / 0).
 *
 * THE CONNECTIVITY CONTRACT (slic_superpixels.py:320-328, `_enforce_label_connectivity_cython(labels, min_size, max_size, start_label)`)
 *   skimage's pass is sequential: a raster scan with a breadth-first fill per unlabelled pixel, cut at max_size, a component below
 *   min_size handed to the last labelled neighbour.  When every 4-connected component of equal raw label has min_size <= size <
 *   max_size (the regular case) that pass is a renumbering of the components by their first pixel in raster order, which K67 and K68
 *   compute.  Any other case sets XAI_SLIC_IRREGULAR and is finished by the caller on the host; the device never guesses it.
 *
 * THE LIMITS: 1 <= S <= XAI_SLIC_MAX_CLUSTERS, 1 <= C <= XAI_SLIC_MAX_CHANNELS, H * W <= XAI_SLIC_MAX_PIXELS, B <= 65535 (a grid
 * extent); for K65, K66 and the whole k-means also H <= 16 * 65535 = 1048560 (K65's rows of 16 x 16 tiles are a grid extent in y; its
 * columns of tiles, at the most 65536, are one in x, which takes them).  K67 gives one image to one workgroup of 1024 lanes, a lane visiting H * W / 1024 pixels per sweep: at the limit of 2^20
 * pixels that is 1024 pixels per lane and sweep, XAI_SLIC_MAX_SWEEPS sweeps at the most, and every flat index fits an int32.
 */
#ifndef XAI_HIP_SLIC_H
#define XAI_HIP_SLIC_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_slic_version() = XAI_SLIC_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_slic_version_minor() = XAI_SLIC_MINOR: bumped whenever entry points are added:
 *   0 = xai_slic_max_clusters, xai_slic_max_channels, xai_slic_max_pixels, xai_slic_workspace_bytes, xai_slic_clear_i32,
 *       xai_slic_assign_f32, xai_slic_assign_f64, xai_slic_update_f32, xai_slic_update_f64, xai_slic_iterate_f32, xai_slic_iterate_f64,
 *       xai_slic_components_i32, xai_slic_number_i32 */
#define XAI_SLIC_VERSION 1
#define XAI_SLIC_MINOR 0

int xai_slic_version(void);
int xai_slic_version_minor(void);

#define XAI_SLIC_MAX_CLUSTERS 4096
#define XAI_SLIC_MAX_CHANNELS 8
#define XAI_SLIC_MAX_PIXELS 1048576
#define XAI_SLIC_MAX_SWEEPS 64
/* the bits of status[b] */
#define XAI_SLIC_UNCOVERED 1 /* K65: a pixel of image b took no cluster; its label is -1 */
#define XAI_SLIC_EMPTY 2     /* K66: a cluster of image b has no pixel; its centre is 0 / 0 */
#define XAI_SLIC_IRREGULAR 4 /* K67: a component outside [min_size, max_size), or the sweeps ran out: finish on the host */

/* = XAI_SLIC_MAX_CLUSTERS, XAI_SLIC_MAX_CHANNELS, XAI_SLIC_MAX_PIXELS */
int xai_slic_max_clusters(void);
int xai_slic_max_channels(void);
int xai_slic_max_pixels(void);

/* The bytes of the `ws` of K67 and K68, 0 for extents outside THE LIMITS: three int32 per pixel (the two sides of K67's sweeps, which
 * K68 reuses for the ranks, and the component sizes). */
size_t xai_slic_workspace_bytes(int B, int H, int W);

/* status[b] = 0 for b < B, by a kernel.
 *   NULL -> XAI_E_NULL;  B < 1 -> XAI_E_SHAPE */
int xai_slic_clear_i32(int32_t* status, int B, xai_stream_t stream);

/* K65 the assignment of THE K-MEANS CONTRACT.  One lane per pixel, a workgroup per 16 x 16 tile: it lists, 256 clusters at a time
 * in ascending k, the clusters whose window meets the tile (centre and integer bounds in LDS); each lane walks the list with its own
 * containment test and the strict compare.  ORs XAI_SLIC_UNCOVERED into status[b].
 * replaces  _slic.pyx, the assignment loop of _slic_cython (`for k in range(n_segments)` ... `if distance[z, y, x] > dist_center`)
 *   features : [B][H][W][C];  centres : [B][S][2 + C];  labels : [B][H][W] int32, written;  status : [B] int32
 *   NULL -> XAI_E_NULL;  an extent < 1, step < 1 -> XAI_E_SHAPE;  an extent over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_slic_assign_f32(const float* features, const float* centres, int B, int H, int W, int C, int S, int step, int32_t* labels,
                        int32_t* status, xai_stream_t stream);
int xai_slic_assign_f64(const double* features, const double* centres, int B, int H, int W, int C, int S, int step, int32_t* labels,
                        int32_t* status, xai_stream_t stream);

/* K66 the update.  One wave per cluster walks the cluster's window (of the centre the assignment used) in raster order: a ballot of
 * the members per 64 pixels, the members added in ascending lane order into one accumulator per feature; then the division.  The new
 * centre replaces the old one (no other wave reads row k).  ORs XAI_SLIC_EMPTY into status[b].
 * replaces  _slic.pyx, the update of _slic_cython (`segments[k, j] += ...` over z, y, x, then `segments[k, j] /= n_segment_elems[k]`)
 *   centres : read and written;  refusals as xai_slic_assign_f32 */
int xai_slic_update_f32(const float* features, const int32_t* labels, int B, int H, int W, int C, int S, int step, float* centres,
                        int32_t* status, xai_stream_t stream);
int xai_slic_update_f64(const double* features, const int32_t* labels, int B, int H, int W, int C, int S, int step, double* centres,
                        int32_t* status, xai_stream_t stream);

/* The whole k-means: status cleared, then `iterations` times K65 and K66, on one stream with no read-back.
 * replaces  slic_superpixels.py:316-318
 *   refusals as xai_slic_assign_f32;  iterations < 1 -> XAI_E_SHAPE */
int xai_slic_iterate_f32(const float* features, int B, int H, int W, int C, int S, int step, int iterations, float* centres,
                         int32_t* labels, int32_t* status, xai_stream_t stream);
int xai_slic_iterate_f64(const double* features, int B, int H, int W, int C, int S, int step, int iterations, double* centres,
                         int32_t* labels, int32_t* status, xai_stream_t stream);

/* K67 the 4-connected components of equal label: comp[p] = the least flat index of p's component.  One workgroup per image; a
 * sweep gives every pixel the least root among itself and its equal neighbours, following each root once (both sides of a sweep
 * are separate arrays, so a sweep's result does not depend on the lanes' order), until a sweep changes nothing or
 * XAI_SLIC_MAX_SWEEPS have run.  Then the sizes and the regular test of THE CONNECTIVITY CONTRACT.  ORs XAI_SLIC_IRREGULAR into
 * status[b] (comp is then unspecified if the sweeps ran out).
 * replaces  slic_superpixels.py:320-328 in the regular case, together with K68
 *   labels, comp : [B][H][W] int32;  ws : >= xai_slic_workspace_bytes(B, H, W) bytes, 4-byte aligned
 *   NULL -> XAI_E_NULL;  an extent < 1, min_size < 0, max_size < min_size, ws_bytes too small -> XAI_E_SHAPE;  over THE LIMITS ->
 *   XAI_E_UNSUPPORTED */
int xai_slic_components_i32(const int32_t* labels, int B, int H, int W, int min_size, int max_size, int32_t* comp, int32_t* status,
                            void* ws, size_t ws_bytes, xai_stream_t stream);

/* K68 the numbering: out[p] = start_label + the rank of comp[p] among the first pixels (comp[q] == q) in raster order, by an integer
 * prefix scan in pixel order; nlabels[b] = the number of first pixels.  An entry of comp outside [0, H * W) is never followed.
 * replaces  the renumbering `_enforce_label_connectivity_cython` amounts to in the regular case
 *   refusals as xai_slic_components_i32 (no sizes) */
int xai_slic_number_i32(const int32_t* comp, int B, int H, int W, int start_label, int32_t* out, int32_t* nlabels, void* ws,
                        size_t ws_bytes, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_SLIC_H */
