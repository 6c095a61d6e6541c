/*
 * xai_conv.h -- C ABI of libxai_conv.so, the extension library of the 1x1 convolution backward-data GEMM beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11 and the extension headers before this one are frozen or pinned by their tests, each to
 * its exact entry list; entry points added after that live here, in a library of their own with a version pair of its own (its
 * record is the key `conv` of xai_engine/_lib.py's LIBRARIES; the source is csrc/conv/).  The
 * grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int and
 * take the caller's stream last), so xai_engine/_lib.py binds this header with the same strict reader, and so are the conventions:
 * device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state, no
 * atomics.  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so)
 * has the text.  Every argument check comes before the first HIP call, so a refused call needs no device.
 *
 * The input gradient of a kernel-1, stride-1, pad-0 convolution with K output and C input channels,
 *     gx[n][c][hw] = sum over k of gy[n][k][hw] * weight[k][c],
 * as an fp32 GEMM on v_mfma_f32_16x16x4_f32 whose order of summation is an argument (csrc/xai_conv_walk.h has the vocabulary and
 * the planner): K is cut into blocks of 16; the blocks are dealt to `splits` partial sums (`membership`); inside a partial sum the
 * blocks are taken in ascending order, each as four MFMAs of four k (`grouping`), an MFMA being the fmaf chain over its four k in
 * ascending order onto the accumulator, which starts at +0; the partial sums are then added one after the other (`order`), from
 * the first of them or from +0 (`from_zero`).  With the walk a split-K GEMM library uses for a shape, the result is that library's
 * bit for bit -- which the caller proves per site before relying on it (xai_engine/prepare.py) -- with no workspace and no second
 * kernel: the partial sums stay in registers.
 */
#ifndef XAI_CONV_H
#define XAI_CONV_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_conv_version() = XAI_CONV_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_conv_version_minor() = XAI_CONV_MINOR: bumped whenever entry points are added:
 *   0 = xai_conv1x1_bwd_data_f32, xai_conv1x1_bwd_data_simple_f32 */
#define XAI_CONV_VERSION 1
#define XAI_CONV_MINOR 0

int xai_conv_version(void);
int xai_conv_version_minor(void);

/* K78  gx = the sum above, walked as (splits, membership, grouping, order, from_zero) say.  Columns are the folded (n, hw) index,
 * rows are c: a workgroup owns tile_rows x 64 outputs and moves slabs of 16 k through LDS; tile_rows = 32 | 64, or 0 for the
 * library's choice.  The result does not depend on tile_rows.
 * replaces  MIOpen's backward-data of the 1x1 convolutions of layer4 (a split-K GEMM, its workspace and its reduction kernel)
 *           inside the autograd.grad of saliencyMethods.py:213
 *   gy : [N][K][HW];  weight : [K][C];  gx : [N][C][HW]
 *   membership: 0 contiguous, 1 round robin;  grouping: 0 consecutive fours, 1 stride 4;  order: 0 ascending, 1 descending
 *   an extent < 1, K % 16 != 0, splits outside 1 .. 32, an unknown membership / grouping / order / tile_rows, a pointer that is not
 *   4-byte aligned -> XAI_E_SHAPE;  N * HW, N * K * HW or N * C * HW > INT32_MAX -> XAI_E_UNSUPPORTED */
int xai_conv1x1_bwd_data_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int splits, int membership,
                             int grouping, int order, int from_zero, int tile_rows, float* gx, xai_stream_t stream);

/* K79  the same sum by the plainest kernel that can say it: one wavefront per 16 x 16 output tile, every operand straight from
 * global memory, no LDS.  It exists to be read: the experiment that finds a library's walk and the tests of K78 compare against it.
 * replaces  nothing on a hot path; the yardstick of K78 under saliencyMethods.py:213
 *   arguments and refusals as xai_conv1x1_bwd_data_f32 */
int xai_conv1x1_bwd_data_simple_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int splits, int membership,
                                    int grouping, int order, int from_zero, float* gx, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_CONV_H */
