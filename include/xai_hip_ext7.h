/*
 * xai_hip_ext7.h -- C ABI of libxai_ext7.so, the seventh extension library beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11 and include/xai_hip_ext.h ... include/xai_hip_ext6.h are frozen or pinned by their tests, each
 * to its exact entry list; entry points added after that live here, in a library of their own with a version pair of its own.  The
 * grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int and
 * take the caller's stream last), so xai_engine/_lib.py binds this header with the same strict reader, and so are the conventions:
 * device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state, no
 * atomics (the same bytes on every run).  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch;
 * xai_strerror (libxai_hip.so) has the text.  Every argument check comes before the first HIP call, so a refused call needs no device.
 *
 * These are the device steps of the k-means of Transformer Input Sampling: the Euclidean Lloyd iteration the reference runs through
 * fast_pytorch_kmeans.KMeans (util/attribution_methods/TIS.py:150-155) and this project restates in torch ops in xai_engine/tis.py
 * (kmeans_centroids).  There the order of every sum is rocBLAS's and torch's and stated nowhere.  Here it is the interface.
 *
 * THE ARITHMETIC CONTRACT.  Everything is fp32 unless stated.  Products and sums round separately (no fused multiply-add).  Every sum
 * starts from +0 and runs sequentially in ascending index, one accumulator per result.
 *   inputs   X (n, d) fp32 contiguous;  first (k) indices into X;  max_iter;  tol (double).  The initial centroids are C = X[first].
 *   once     xx_i = sum_t X[i,t] * X[i,t]
 *   an iteration
 *     1. cc_j  = sum_t C[j,t] * C[j,t]
 *     2. dot_ij = sum_t X[i,t] * C[j,t]
 *     3. s_ij  = ((2 * dot_ij) - xx_i) - cc_j
 *     4. a_i   = the smallest j whose s_ij is maximal; NaN counts as maximal and the first NaN wins (np.argmax's rule and torch's)
 *     5. cnt_j = the number of points with a_i = j
 *     6. sum_jt = sum over i ascending with a_i = j of X[i,t]
 *     7. new_jt = sum_jt / float(cnt_j), a true division; every element that is NaN becomes +0 (`new[new != new] = 0`), so an empty
 *        cluster is a zero row
 *     8. q_jt = (new_jt - C_jt), squared in fp32;  e_j = sum_t (double) q_jt in fp64;  err = sum_j e_j in fp64
 *     9. C <- new; the iteration counter goes up by one
 *    10. stop if err <= tol, compared in fp64 (after step 9: the update is kept), or if the counter has reached max_iter
 * Once the loop has stopped every further launch of an iteration changes nothing: each kernel reads the `done` word of `state` and
 * returns.  A host may therefore issue iterations in chunks and read `state` once per chunk.  No kernel waits on another workgroup and
 * every loop is bounded by an extent.
 *
 * THE LIMITS: 1 <= k <= n <= XAI_KMEANS_MAX_POINTS, d <= XAI_KMEANS_MAX_FEATURES, k <= XAI_KMEANS_MAX_CLUSTERS.  K60 keeps one bit per
 * point (8 KB at the limit) and two floats per feature (32 KB) in the LDS of a workgroup.  TIS on ViT-B/16 has n = 9216 activation
 * channels, d = 196 tokens and k = 1024 masks.
 */
#ifndef XAI_HIP_EXT7_H
#define XAI_HIP_EXT7_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext7_version() = XAI_EXT7_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext7_version_minor() = XAI_EXT7_MINOR: bumped whenever entry points are added:
 *   0 = xai_kmeans_max_points, xai_kmeans_max_features, xai_kmeans_max_clusters, xai_kmeans_workspace_bytes, xai_kmeans_init_f32,
 *       xai_kmeans_assign_f32, xai_kmeans_update_f32, xai_kmeans_iterate_f32 */
#define XAI_EXT7_VERSION 1
#define XAI_EXT7_MINOR 0

int xai_ext7_version(void);
int xai_ext7_version_minor(void);

#define XAI_KMEANS_MAX_POINTS 65536
#define XAI_KMEANS_MAX_FEATURES 4096
#define XAI_KMEANS_MAX_CLUSTERS 16384
/* `state`: 6 int32 words, 8-byte aligned = { iterations run, done (0 / 1), status, 0, err as a double in words 4 and 5 } */
#define XAI_KMEANS_STATE_WORDS 6
/* state[2] */
#define XAI_KMEANS_OK 0
#define XAI_KMEANS_BAD_INDEX 1 /* an entry of `first` is outside [0, n): it was not followed, its centroid starts as a zero row */

/* = XAI_KMEANS_MAX_POINTS, XAI_KMEANS_MAX_FEATURES, XAI_KMEANS_MAX_CLUSTERS */
int xai_kmeans_max_points(void);
int xai_kmeans_max_features(void);
int xai_kmeans_max_clusters(void);

/* The bytes of `ws` every launch entry takes, 0 for extents outside THE LIMITS.  The layout:
 *   e  [k] float64   e_j of the iteration in flight
 *   xx [n] float32   written by the init entry
 *   cc [k] float32   of the centroids as they stand: written by the init entry, then by every update */
size_t xai_kmeans_workspace_bytes(int n, int d, int k);

/* K58 the start.  Two launches: xx_i, one lane per point, and state = { 0, 0, 0, 0, +0.0 };  then C[j] = X[first[j]] and cc_j, one
 * workgroup per centroid.
 * replaces  xai_engine/tis.py kmeans_centroids: `c = points[first].clone()`, `x_sq = (points * points).sum(1)` (TIS.py:150-155)
 *   X : [n][d] float32;  first : [k] int64 (device);  C : [k][d] float32, written;  ws : >= xai_kmeans_workspace_bytes(n, d, k) bytes
 *   NULL -> XAI_E_NULL;  an extent < 1, k > n, ws_bytes too small, ws or state not 8-byte aligned -> XAI_E_SHAPE;
 *   an extent over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_kmeans_init_f32(const float* X, const int64_t* first, int n, int d, int k, float* C, void* ws, size_t ws_bytes, int32_t* state,
                        xai_stream_t stream);

/* K59 the assignment: steps 2 - 4 from the centroids C and the cc of `ws`.  One workgroup per 32 points; the score matrix is never
 * stored.  Writes nothing when state[1] is set.
 * replaces  `sim = 2 * points @ c.T - x_sq - (c * c).sum(1)[None]`, `closest = sim.argmax(1)`
 *   assign : [n] int32, written;  refusals as xai_kmeans_init_f32 */
int xai_kmeans_assign_f32(const float* X, int n, int d, int k, const float* C, int32_t* assign, const void* ws, size_t ws_bytes,
                          const int32_t* state, xai_stream_t stream);

/* K60 and K61 the update: steps 5 - 10 and the next iteration's step 1.  K60, one workgroup per centroid, one lane per feature,
 * walks the assignments in ascending i and writes counts[j], the new row of C over the old one, e_j and cc_j;  K61, one workgroup, sums
 * the e_j in ascending j and writes `state`.  Both write nothing when state[1] is set.
 * replaces  `onehot @ points / onehot.sum(-1)[:, None]`, `new[new != new] = 0`, `err = (new - c).pow(2).sum()`, `c = new`,
 *           `if float(err) <= tol: break`
 *   C : [k][d] float32, read and written;  assign : [n] int32 of K59;  counts : [k] int32, written
 *   refusals as xai_kmeans_init_f32;  max_iter < 1 -> XAI_E_SHAPE */
int xai_kmeans_update_f32(const float* X, int n, int d, int k, float* C, const int32_t* assign, int32_t* counts, void* ws, size_t ws_bytes,
                          int32_t* state, int max_iter, double tol, xai_stream_t stream);

/* `iterations` Lloyd iterations, each K59 then K60 and K61, on one stream: 3 * iterations launches and no read-back.  The ones after
 * the stop change nothing, so the caller reads `state` when it likes.
 * replaces  the body of `for _ in range(max_iter)` of xai_engine/tis.py kmeans_centroids (TIS.py:150-155)
 *   refusals as xai_kmeans_update_f32;  iterations < 1 or iterations > max_iter -> XAI_E_SHAPE */
int xai_kmeans_iterate_f32(const float* X, int n, int d, int k, float* C, int32_t* assign, int32_t* counts, void* ws, size_t ws_bytes,
                           int32_t* state, int max_iter, double tol, int iterations, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT7_H */
