/*
 * xai_hip_ext6.h -- C ABI of libxai_ext6.so, the sixth extension library beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11, include/xai_hip_ext.h at 1.0, include/xai_hip_ext2.h at 1.1, include/xai_hip_ext3.h at 1.0,
 * include/xai_hip_ext4.h at 1.0 and include/xai_hip_ext5.h is pinned at 1.0 by its tests; entry points added after that live here, in a
 * library of their own with a version pair of its own.  The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch
 * entries end in _f32 / _f64 / _i32 / _u64, return int and take the caller's stream last), so xai_engine/_lib.py binds all seven
 * headers with the same strict reader, and so are the conventions: device pointers owned by the caller, asynchronous
 * graph-capturable launches, nothing allocated or retained, no global state, no atomics (the same bytes on every run).  Return values
 * are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so) has the text.  Every
 * argument check comes before the first HIP call, so a refused call needs no device.
 *
 * These are the two device steps of complete-linkage agglomerative clustering of a precomputed distance matrix as
 * scipy.cluster.hierarchy.linkage(y, "complete") computes it (scipy/cluster/_hierarchy.pyx: `nn_chain`, then in `linkage` a stable
 * argsort by height and `label`), which is what scikit-learn's AgglomerativeClustering(metric="precomputed", linkage="complete")
 * calls (sklearn/cluster/_agglomerative.py, linkage_tree), for ViT-CX's mask clustering (xai_engine/linkage.py, xai_engine/vit_cx.py).
 * The algorithm is restated, not repaired.  Complete linkage does no arithmetic on distances: the Lance-Williams update is `max`, so
 * every height is one of the float32 inputs and every fp32 comparison equals the libraries' fp64 comparison of the same values.  The
 * only floating-point operations on distances here are compare and select.
 *
 * THE CAP: 2 <= n <= XAI_LINKAGE_MAX_N = 2048.  K56 keeps `size` and the chain (2 int32 per point) and K57 the sort keys, the
 * merged pairs and the union-find (20 bytes per point) in the LDS of their one workgroup: 16 KB and 40 KB at the cap, inside the
 * 64 KB a workgroup may declare; the working copy is 16 MB there.  2048 covers every ViT width in use (768, 1024, 1280, 1408, 1664).
 */
#ifndef XAI_HIP_EXT6_H
#define XAI_HIP_EXT6_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext6_version() = XAI_EXT6_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext6_version_minor() = XAI_EXT6_MINOR: bumped whenever entry points are added:
 *   0 = xai_linkage_max_n, xai_linkage_workspace_bytes, xai_linkage_complete_f32, xai_linkage_sort_relabel_i32 */
#define XAI_EXT6_VERSION 1
#define XAI_EXT6_MINOR 0

int xai_ext6_version(void);
int xai_ext6_version_minor(void);

#define XAI_LINKAGE_MAX_N 2048
/* info[0]: 0, or why `merges` is not a dendrogram (the host raises; K57 then writes nothing) */
#define XAI_LINKAGE_OK 0
#define XAI_LINKAGE_NONFINITE 1 /* an entry above the diagonal is NaN or +-inf (sklearn's check_array refuses it) */
#define XAI_LINKAGE_BOUND 2     /* the chain loop hit one of its bounds, or K57 met a pair that is no merge: a logic error */

/* = XAI_LINKAGE_MAX_N */
int xai_linkage_max_n(void);

/* The bytes of `ws` both entries take, 0 for n outside [2, XAI_LINKAGE_MAX_N].  The layout, 4-byte words:
 *   W      [n][n] float32   the symmetric working copy
 *   flags  [n * ceil(n / 256)] int32   one word per workgroup of the copy: did it see a non-finite entry
 *   merges [n - 1][3]       x, y (int32, x < y) and the height (float32) of merge k, in the order the chain finds them */
size_t xai_linkage_workspace_bytes(int n);

/* K56 the working copy, the finite check and the nearest-neighbour chain.  Two launches.
 *   1. W[i][j] = W[j][i] = distance[i][j] for i < j, W[i][i] = 0.  Only the entries above the diagonal are read (sklearn takes
 *      X[np.triu_indices(n, 1)]; a matrix product need not be bit-symmetric).  A non-finite one sets info[0] =
 *      XAI_LINKAGE_NONFINITE and the chain does not start.
 *   2. One workgroup of `lanes` lanes.  size[i] = 1 for all i, the chain is empty.  For k = 0 .. n - 2:
 *        if the chain is empty, push the lowest i with size[i] > 0
 *        repeat: x = the chain's tip.  With at least 2 entries y = the entry below the tip and cur = W[x][y], else cur = +inf.
 *                Scan i = 0 .. n - 1 ascending, skipping size[i] == 0 and i == x: if W[x][i] < cur (strict) then cur = W[x][i], y = i.
 *                With at least 2 entries and y the entry below the tip: stop.  Else push y.
 *        pop two entries, order the pair so that x < y, merges[k] = (x, y, cur)
 *        size[y] += size[x], size[x] = 0;  for every i with size[i] > 0, i != y:  W[i][y] = W[y][i] = max(W[i][x], W[i][y])
 *      The scan is one pass of the workgroup over row x of W: the minimum of (W[x][i], i) in lexicographic order with the entry
 *      below the tip ranked before every index, which is the first index of the strict minimum with the chain predecessor
 *      preferred on equality.  max(a, b) is (b > a) ? b : a, so W[i][x] on a tie of +0 and -0, which compare equal everywhere.
 *      Bounded: after more than 4 n pushes, a chain of more than n entries or a scan that finds nothing, info[0] =
 *      XAI_LINKAGE_BOUND and the kernel returns; the loop over k ends after n - 1 merges.  No input can make it hang.
 * replaces  scipy/cluster/_hierarchy.pyx, `nn_chain` with method complete (new_dist = `_complete`), on sklearn's
 *           X[np.triu_indices(n, 1)] (sklearn/cluster/_agglomerative.py, linkage_tree)
 *   distance : [n][n] float32, only read;  ws : >= xai_linkage_workspace_bytes(n) bytes, 4-byte aligned
 *   info     : [4] int32 = { status, row scans, pushes, merges recorded }
 *   lanes    : 64, 256 or 1024, the width of the chain's workgroup; 0 = the default (256).  Every width writes the same bytes.
 *   NULL -> XAI_E_NULL;  n < 2, ws_bytes too small, ws not 4-byte aligned, another `lanes` -> XAI_E_SHAPE;
 *   n > XAI_LINKAGE_MAX_N -> XAI_E_UNSUPPORTED */
int xai_linkage_complete_f32(const float* distance, int n, void* ws, size_t ws_bytes, int32_t* info, int lanes, xai_stream_t stream);

/* K57 the stable sort by height and the relabelling, one workgroup.  Reads `merges` of the `ws` K56 has filled and info[0]; with
 * info[0] != 0 it writes nothing.
 *   order    = the merges sorted by height ascending, stably: equal heights (+0 and -0 are equal) keep the chain's order
 *   for k = 0 .. n - 2, (x, y, h) = merge order[k], over a union-find of the n points whose roots carry a cluster id (a point's
 *   own index at first):  a, b = the ids of x's and y's roots;  children[k] = (min(a, b), max(a, b));  heights[k] = h;  the united
 *   root gets id n + k
 *   A pair outside 0 <= x < y < n sets info[0] = XAI_LINKAGE_BOUND and ends the kernel.
 * replaces  scipy/cluster/hierarchy.py, linkage: `order = np.argsort(Z[:, 2], kind='mergesort')` and _hierarchy.pyx `label`
 *           (LinkageUnionFind); children and heights are sklearn's children_ and distances_
 *   children : [n - 1][2] int32;  heights : [n - 1] float32;  info : [4] int32, K56's
 *   NULL -> XAI_E_NULL;  n < 2, ws_bytes too small, ws not 4-byte aligned -> XAI_E_SHAPE;  n > XAI_LINKAGE_MAX_N -> XAI_E_UNSUPPORTED */
int xai_linkage_sort_relabel_i32(int n, const void* ws, size_t ws_bytes, int32_t* children, float* heights, int32_t* info,
                                 xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT6_H */
