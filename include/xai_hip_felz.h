/*
 * xai_hip_felz.h -- C ABI of libxai_felz.so: Felzenszwalb-Huttenlocher graph segmentation (IJCV 2004) as scikit-image 0.18.3 computes
 * it, for XRAI's six label maps per image (xai_engine/felzenszwalb.py, xai_engine/xrai.py).
 *
 * The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int and
 * take the caller's stream last), so xai_engine/_lib.py binds this header with the same strict reader, and so are the conventions:
 * device pointers owned by the caller, asynchronous launches, nothing allocated or retained, no memset enqueued, the same bytes on
 * every run.  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so)
 * has the text.  Every argument check comes before the first HIP call, so a refused call needs no device.  The only atomics are
 * integer ones (an OR into the status word, an AND that clears K73's bits in LDS): their result does not depend on their order.
 *
 * The definition is the binary of scikit-image 0.18.3, skimage/segmentation/_felzenszwalb_cy.pyx (_felzenszwalb_cython), with
 * scipy.ndimage.gaussian_filter for its smoothing.  Every step is fp64 and every operation is rounded once, in the order written
 * (the library is compiled with -ffp-contract=off).  Every entry takes B images at once.
 *
 * THE CONTRACT
 *   smooth  per axis (0 = rows, then 1 = columns) of a [B][H][W][C] image, with host-computed symmetric weights w[0 .. 2r]:
 *             t = x[l] * w[r];  for ll = -r .. -1:  t += (x[l + ll] + x[l - ll]) * w[ll + r]
 *           an index outside [0, n) reflects with period 2n:  m = idx mod 2n,  m >= n -> 2n - 1 - m  (also for r >= n)
 *   costs   four families of edges, concatenated: right (y, x)-(y, x+1), down (y, x)-(y+1, x), down-right (y, x)-(y+1, x+1),
 *           up-right (y, x+1)-(y+1, x), each raveled in raster order over its (H or H-1) x (W or W-1) grid, so an edge's two pixels
 *           follow from its index e in [0, E), E = H (W-1) + (H-1) W + 2 (H-1) (W-1).
 *           cost = sqrt(d_0 d_0 + d_1 d_1 + ...), d = a - b, summed sequentially over the channels; the sqrt is correctly rounded.
 *           The key of an edge is the bit pattern of its cost, monotone because a cost is >= +0.
 *   order   ascending key, equal keys by ascending edge index (a stable sort).  skimage's np.argsort leaves the order among equal
 *           costs unpinned; this rule is the engine's.
 *   merge   a union-find in which the lower pixel index is always the root; every root has size 1 and cint 0.0.  For each edge in
 *           order: the two roots a, b; equal -> skip;  cost < min(cint[a] + scale / size[a], cint[b] + scale / size[b]) -> join, the
 *           new root gets size[a] + size[b] and cint = cost.  `scale` is the caller's (skimage's scale / 255.0).
 *   minimum size   a second walk over the same order: roots differ and (size[a] < min_size or size[b] < min_size) -> join.
 *   labels  a pixel's label is the rank of its root among the roots in ascending pixel index.
 *
 * THE LIMITS: 1 <= C <= XAI_FELZ_MAX_CHANNELS (a lane's channel loop), 1 <= S <= XAI_FELZ_MAX_SCALES scales per call, 0 <= r <=
 * XAI_FELZ_MAX_RADIUS (the weights, 2r + 1 doubles), H * W <= XAI_FELZ_MAX_PIXELS = 65536: K73's forest holds a pixel's parent as a
 * 16-bit word in LDS, 2 H W bytes <= 128 KiB of a CU's 160 KiB, and a 16-bit word names 65536 pixels; a bit per pixel beside it (the
 * roots the current 64 edges joined) takes H W / 8 bytes <= 8 KiB, the staging of 64 edges under 2 KiB; 224 x 224 = 50176 takes 104 KiB.
 * (The other placement, int32 parents in L2-resident global memory, was measured beside it and removed: 198 ms against 145 ms for
 * XRAI's six chains at 224 x 224, profiles/r20_felzenszwalb.txt.)
 * Then E <= 4 H W = 262144 fits an int32, K71 / K72 give an image at the most 256 chunks of 1024 edges, and B * S <= 2^20 chains and
 * B <= 65535 are grid extents.
 */
#ifndef XAI_HIP_FELZ_H
#define XAI_HIP_FELZ_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_felz_version() = XAI_FELZ_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_felz_version_minor() = XAI_FELZ_MINOR: bumped whenever entry points are added:
 *   0 = xai_felz_max_pixels, xai_felz_max_channels, xai_felz_max_scales, xai_felz_max_radius, xai_felz_edges,
 *       xai_felz_workspace_bytes, xai_felz_clear_i32, xai_felz_smooth_f64, xai_felz_costs_u64, xai_felz_sort_u64, xai_felz_merge_f64,
 *       xai_felz_labels_i32 */
#define XAI_FELZ_VERSION 1
#define XAI_FELZ_MINOR 0

int xai_felz_version(void);
int xai_felz_version_minor(void);

#define XAI_FELZ_MAX_PIXELS 65536
#define XAI_FELZ_MAX_CHANNELS 8
#define XAI_FELZ_MAX_SCALES 16
#define XAI_FELZ_MAX_RADIUS 64
/* the bits of the status word */
#define XAI_FELZ_NONFINITE 1 /* K70: a cost is not finite (a NaN or infinite pixel) */
#define XAI_FELZ_INVARIANT 2 /* K72-K74: an edge index outside [0, E), a parent above its child, a root walk over H * W hops */

/* = XAI_FELZ_MAX_PIXELS, XAI_FELZ_MAX_CHANNELS, XAI_FELZ_MAX_SCALES, XAI_FELZ_MAX_RADIUS */
int xai_felz_max_pixels(void);
int xai_felz_max_channels(void);
int xai_felz_max_scales(void);
int xai_felz_max_radius(void);

/* E of THE CONTRACT for an H x W image, 0 for extents outside THE LIMITS (and for the 1 x 1 image, which has no edge). */
int xai_felz_edges(int H, int W);

/* The bytes of the `ws` of K71-K73, 0 for extents outside THE LIMITS: the larger of the sort's (the second side of the keys and
 * indices, 12 bytes per edge, and 256 counters per chunk of 1024 edges) and the merge's (per chain and pixel a double cint and an
 * int32 size; the parents are in LDS). */
size_t xai_felz_workspace_bytes(int B, int H, int W, int S);

/* status[i] = 0 for i < n, by a kernel.
 *   NULL -> XAI_E_NULL;  n < 1 -> XAI_E_SHAPE */
int xai_felz_clear_i32(int32_t* status, int n, xai_stream_t stream);

/* K69 one axis of the smoothing of THE CONTRACT, one lane per sample.  A skipped axis (sigma <= 1e-15) is the caller's not to launch.
 * replaces  scipy.ndimage.gaussian_filter(image, [sigma, sigma, 0]) of _felzenszwalb_cython, one correlate1d (symmetric branch,
 *           mode reflect) per call
 *   src, dst : [B][H][W][C] double, dst may not be src;  weights : [2 * radius + 1] double on the device;  axis : 0 or 1
 *   NULL -> XAI_E_NULL;  an extent < 1, radius < 0, axis not 0 or 1, dst == src -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_felz_smooth_f64(const double* src, const double* weights, int radius, int axis, int B, int H, int W, int C, double* dst,
                        xai_stream_t stream);

/* K70 the costs: keys[b][e] = the bits of cost e, index[b][e] = e, one lane per edge; ORs XAI_FELZ_NONFINITE into status[0].
 * replaces  the four np.sqrt(np.sum(d * d, axis=-1)) and the np.hstack of _felzenszwalb_cython
 *   image : [B][H][W][C] double;  keys : [B][E] uint64;  index : [B][E] int32;  status : [1] int32.  E = 0 launches nothing.
 *   NULL -> XAI_E_NULL;  an extent < 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_felz_costs_u64(const double* image, int B, int H, int W, int C, uint64_t* keys, int32_t* index, int32_t* status,
                       xai_stream_t stream);

/* K71 / K72 the order: a stable least-significant-digit radix sort of (key, index) per image, eight passes of eight bits.  A pass:
 * K71 counts the digits of every chunk of 1024 consecutive edges (one wave per chunk, the lanes of equal digit found by ballots, no
 * atomic), an exclusive scan of the counters in (digit, chunk) order (one workgroup per image), K72 places every edge at its
 * digit's offset plus its rank among the equal digits before it.  The sorted pairs end where they began.
 * replaces  np.argsort(costs) of _felzenszwalb_cython, with the stable rule of THE CONTRACT
 *   keys : [B][E] uint64, index : [B][E] int32, read and written;  ws : >= xai_felz_workspace_bytes bytes, 8-byte aligned
 *   NULL -> XAI_E_NULL;  an extent < 1, ws_bytes too small, ws misaligned -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_felz_sort_u64(uint64_t* keys, int32_t* index, int B, int H, int W, int S, void* ws, size_t ws_bytes, xai_stream_t stream);

/* K73 merge and minimum size: one workgroup of one wave per (image, scale).  The wave takes 64 consecutive edges of the order: every
 * lane finds the roots of its edge's two pixels in the LDS forest (and points the pixels it passed at them: roots do not change meanwhile), a ballot
 * keeps the lanes whose roots differ (equal roots stay equal), each with the rule evaluated on its two roots as they are, and lane 0
 * commits the kept edges in ascending order: it takes the lane's answer where no earlier commit of these 64 edges joined either root
 * (a bit per root says so), and looks again where one did.  Then the same walk with the minimum-size rule, then roots[b][s][p] = the root of pixel p.  A parent is never above its
 * child, so every root walk descends; a walk is still capped at H * W hops.  A violated invariant ORs XAI_FELZ_INVARIANT into
 * status[0] and ends the chain.  stats[b][s] = (edges that reached the test of the two thresholds, edges that merged) of the first
 * walk.
 * replaces  the two `for e in range(costs.size)` loops of _felzenszwalb_cython
 *   keys, order : [B][E] as xai_felz_sort_u64 left them;  scales : [S] double on the device (scale / 255.0);  roots : [B][S][H][W]
 *   int32;  stats : [B][S][2] int32;  ws as xai_felz_sort_u64
 *   NULL -> XAI_E_NULL;  an extent < 1, min_size < 0, ws_bytes too small -> XAI_E_SHAPE;  over THE LIMITS ->
 *   XAI_E_UNSUPPORTED */
int xai_felz_merge_f64(const uint64_t* keys, const int32_t* order, const double* scales, int B, int S, int H, int W, int min_size,
                       int32_t* roots, int32_t* stats, int32_t* status, void* ws, size_t ws_bytes, xai_stream_t stream);

/* K74 the labels: per map, a flag per root (roots[p] == p), an integer prefix scan in pixel order, labels[p] = the rank of roots[p],
 * counts[m] = the number of roots.  One workgroup per map.  An entry of roots that is no root ORs XAI_FELZ_INVARIANT and labels -1.
 * replaces  the np.unique(..., return_inverse=True) of _felzenszwalb_cython
 *   roots, labels : [M][n] int32, labels may not be roots;  counts : [M] int32
 *   NULL -> XAI_E_NULL;  M < 1, n < 1, labels == roots -> XAI_E_SHAPE;  n > XAI_FELZ_MAX_PIXELS, M > 2^20 -> XAI_E_UNSUPPORTED */
int xai_felz_labels_i32(const int32_t* roots, int M, int n, int32_t* labels, int32_t* counts, int32_t* status, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_FELZ_H */
