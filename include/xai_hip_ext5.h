/*
 * xai_hip_ext5.h -- C ABI of libxai_ext5.so, the fifth extension library beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11, include/xai_hip_ext.h at 1.0, include/xai_hip_ext2.h at 1.1, include/xai_hip_ext3.h at 1.0
 * and include/xai_hip_ext4.h is pinned at 1.0 by its tests; entry points added after that live here, in a library of their own with a
 * version pair of its own.  The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 /
 * _i32 / _u64, return int and take the caller's stream last), so xai_engine/_lib.py binds all six headers with the same strict
 * reader, and so are the conventions: device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated
 * or retained, no global state, no atomics (the same bytes on every run).  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*,
 * >0 = hipError_t of the launch; xai_strerror (libxai_hip.so) has the text.  Every argument check comes before the first HIP call, so a
 * refused call needs no device.
 *
 * These are the three steps of quickshift superpixels (Vedaldi and Soatto, ECCV 2008) as scikit-image 0.18.3 computes them
 * (skimage/segmentation/_quickshift.py:71-73 calls _quickshift_cython of _quickshift_cy.pyx; its steps are cited below by the
 * comment that heads each of them in that file), for LIME's segmentation
 * (xai_engine/quickshift.py, xai_engine/lime.py).  Everything is fp64 and every difference, product and sum is rounded once, in
 * the order written (the library is compiled with -ffp-contract=off).  Every entry takes a leading image count B: per-image
 * features, noise and outputs, shared H, W, C, kernel_size and max_dist; an image is what skimage's one-image call sees.
 *
 * Common to K53 and K54:
 *   kw = (int)ceil(3 * kernel_size) (`kernel_width`), inv = -0.5 / (kernel_size * kernel_size) (`inv_kernel_size_sqr`)
 *   the window of pixel (r, c) is r_ in [max(r - kw, 0), min(r + kw + 1, H)), c_ in [max(c - kw, 0), min(c + kw + 1, W)), scanned with
 *   r_ ascending and inside a row c_ ascending (`r_min`, `r_max`, `c_min`, `c_max`); the pixel itself is part of it
 *   d(r, c, r_, c_) = the sum, starting from +0, over the channels ch = 0 .. C-1 ascending of (f[r][c][ch] - f[r_][c_][ch])^2, then
 *   + (double)(r - r_)^2, then + (double)(c - c_)^2 (`dist`)
 * One lane owns one pixel and walks its window in scan order, so no result depends on how the image is cut into tiles.  A workgroup
 * is a 16 x 16 block of pixels and stages the features of its block plus a halo of kw pixels in LDS:
 *   xai_quickshift_lds_bytes(C, kernel_size) = (16 + 2 * kw)^2 * C * 8
 * THE CAP: a call whose xai_quickshift_lds_bytes exceeds 65536 returns XAI_E_UNSUPPORTED.  With C = 3 that admits kw <= 18, i.e.
 * kernel_size <= 6 (LIME's kernel_size 4: kw = 12, 38400 bytes; skimage's default 5: kw = 15, 50784 bytes); with C = 1 kw <= 37.
 */
#ifndef XAI_HIP_EXT5_H
#define XAI_HIP_EXT5_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext5_version() = XAI_EXT5_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext5_version_minor() = XAI_EXT5_MINOR: bumped whenever entry points are added:
 *   0 = xai_quickshift_lds_bytes, xai_quickshift_density_f64, xai_quickshift_parent_f64, xai_quickshift_workspace_bytes,
 *       xai_quickshift_labels_i32 */
#define XAI_EXT5_VERSION 1
#define XAI_EXT5_MINOR 0

int xai_ext5_version(void);
int xai_ext5_version_minor(void);

/* The LDS bytes a workgroup of K53 / K54 stages (the formula above); 0 for arguments those entries answer with XAI_E_SHAPE
 * (C <= 0, kernel_size < 1 or NaN) and SIZE_MAX for a kernel_size above 10000. */
size_t xai_quickshift_lds_bytes(int C, double kernel_size);

/* K53 dens[r][c] = (the sum, starting from +0, over the window in scan order of exp(d * inv)) + noise[r][c]
 * replaces  _quickshift_cy.pyx, `# compute densities` (densities[r, c] += exp(dist * inv_kernel_size_sqr)) and `# this will break ties
 *           that otherwise would give us headache` (densities += random_state.normal(scale=0.00001, size=(height, width)));
 *           the draw itself stays on the host (xai_engine/quickshift.py, tie_noise), so any array can be passed
 *   features : [B][H][W][C] fp64;  noise, dens : [B][H][W] fp64
 *   exp is the device library's fp64 exp (1 ulp by its documentation); everything else is exact in the order stated, so a density is
 *   within n_terms * (2^-52 + ulp(max density)) of any other arithmetic whose exp is within 2 ulp.
 *   NULL -> XAI_E_NULL;  B, H, W or C <= 0, kernel_size < 1 (or NaN) -> XAI_E_SHAPE;
 *   the cap above, B > 65535, H * W > 2^31 - 1, H > 65535 * 16 -> XAI_E_UNSUPPORTED */
int xai_quickshift_density_f64(const double* features, const double* noise, int B, int H, int W, int C, double kernel_size, double* dens,
                               xai_stream_t stream);

/* K54 the nearest denser neighbour.  For pixel (r, c), over the window in scan order, among the neighbours with
 *       dens[r_][c_] > dens[r][c]:  the smallest d (the same sum as K53's, bit for bit) with a strict <, so the first neighbour in
 *       scan order wins an exact tie;  closest = that d, or DBL_MAX when no neighbour is denser (or none is nearer than DBL_MAX)
 *       tree[r][c]   = r_ * W + c_ of that neighbour, or r * W + c when there is none (what skimage returns with return_tree=True)
 *       dist[r][c]   = sqrt(closest), correctly rounded (sqrt(DBL_MAX) = 1.3407807929942596e154 without a denser neighbour)
 *       parent[r][c] = tree[r][c], or r * W + c when dist[r][c] > max_dist
 *     Comparisons with a NaN are false as in C: a pixel with a NaN density has no denser neighbour and is nobody's parent.
 * replaces  _quickshift_cy.pyx, `# find nearest node with higher density` (closest = DBL_MAX; ...; dist_parent[r, c] = sqrt(closest)) and `# remove parents with
 *           distance > max_dist` (too_far = dist_parent_flat > max_dist)
 *   features : [B][H][W][C] fp64;  dens, closest, dist : [B][H][W] fp64;  parent, tree : [B][H][W] int32 (tree may be NULL)
 *   refusals: K53's */
int xai_quickshift_parent_f64(const double* features, const double* dens, int B, int H, int W, int C, double kernel_size, double max_dist,
                              int32_t* parent, int32_t* tree, double* closest, double* dist, xai_stream_t stream);

/* K55 roots and labels, three launches.  xai_quickshift_workspace_bytes(B, H, W) = B * H * W * 2 int32 (0 for a refused shape).
 *   1. root[i] = the pixel reached from i by following parent until parent[j] == j.  parent is only read.  An entry outside
 *      [0, H * W) counts as a root, and a walk ends after H * W steps at the latest, so no parent array reads out of bounds or hangs.
 *   2. one workgroup per image: flag[i] = (root[i] == i);  scan[i] = the number of flags before i in pixel order (an exclusive integer
 *      prefix sum);  D = the number of flags
 *   3. labels[i] = scan[root[i]]
 * which is np.unique(roots, return_inverse=True)[1]: the roots numbered in ascending pixel order.
 * replaces  _quickshift_cy.pyx, `# flatten forest (mark each pixel with root of corresponding tree)` (while (old != parent_flat).any():
 *           parent_flat = parent_flat[parent_flat]) and np.unique(parent_flat, return_inverse=True)[1]
 *   parent, labels : [B][H][W] int32;  D : [B] int32;  ws : >= xai_quickshift_workspace_bytes(B, H, W) bytes, 4-byte aligned
 *   NULL -> XAI_E_NULL;  B, H or W <= 0, ws_bytes too small, ws not 4-byte aligned -> XAI_E_SHAPE;
 *   B > 65535, H * W > 2^31 - 1 -> XAI_E_UNSUPPORTED */
size_t xai_quickshift_workspace_bytes(int B, int H, int W);
int xai_quickshift_labels_i32(const int32_t* parent, int B, int H, int W, int32_t* labels, int32_t* D, void* ws, size_t ws_bytes,
                              xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT5_H */
