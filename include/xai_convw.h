/*
 * xai_convw.h -- C ABI of libxai_convw.so, the extension library of the 1x1 convolution backward-data GEMM on large planes, beside
 * libxai_conv.so.
 *
 * include/xai_conv.h is pinned by its tests at 1.0 with exactly two entries; the entry points added after it live here, in a library of
 * their own with a version pair of its own (its record is the key `convw` of xai_engine/_lib.py's LIBRARIES; the source is csrc/conv/).
 * The grammar and the conventions are xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32, return int and
 * take the caller's stream last; device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or
 * retained, no global state, no atomics).  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch;
 * xai_strerror (libxai_hip.so) has the text.  Every argument check comes before the first HIP call, so a refused call needs no device.
 *
 * The input gradient of a kernel-1, stride-1, pad-0 convolution with K output and C input channels,
 *     gx[n][c][hw] = sum over k of gy[n][k][hw] * weight[k][c],
 * as an fp32 GEMM on v_mfma_f32_16x16x4_f32 in one partial sum whose order is an argument (csrc/xai_conv_walk.h has the vocabulary
 * and the planners): K is cut into blocks of 16, each taken as four MFMAs of four k (`grouping`), an MFMA being the fmaf chain over
 * its four k in ascending order onto the accumulator, which starts at +0 (`from_zero`: +0 is added to the sum once more).  The blocks
 * are taken in ascending order from a first block that depends on where the output lies, round to the block before it -- the
 * staggered start of a GEMM library's K loop: the loop runs K / depth iterations; the outputs are cut into tiles of `tile` along hw
 * (axis 0) or c (axis 1); tile number w starts at iteration (w & mask) << shift, where shift = log2(stride / (4 * depth)), or 0 if that
 * is less than one iteration, and mask + 1 is the largest power of two <= `stagger` with (mask + 1) << shift <= K / depth.
 * stagger = 0: every output starts at k = 0, the walk (1, 0, grouping, 0, from_zero) of xai_conv.h.
 */
#ifndef XAI_CONVW_H
#define XAI_CONVW_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_convw_version() = XAI_CONVW_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_convw_version_minor() = XAI_CONVW_MINOR: bumped whenever entry points are added:
 *   0 = xai_convw_bwd_data_f32, xai_convw_bwd_data_simple_f32 */
#define XAI_CONVW_VERSION 1
#define XAI_CONVW_MINOR 0

int xai_convw_version(void);
int xai_convw_version_minor(void);

/* K80  gx = the sum above.  A workgroup owns 64 or 128 rows (c) of 64 columns (hw) of one image -- 32 columns where the stagger's
 * tiles are no multiple of 64 -- and moves slabs of 16 k through LDS; every element of gy is read from global memory once and every
 * element of gx written once, except that for C > 128 with K > 128 (K > 64 at 32 columns) each 128 rows read gy again.  Loads are 16
 * bytes wide where HW % 4 == 0, C % 4 == 0 and gy and weight are 16-byte aligned, dwords otherwise; the result is the same.
 * replaces  MIOpen's backward-data of the stride-1 1x1 convolutions on planes larger than 64 positions (a GEMM per image on 32-wide
 *           tiles) inside the autograd.grad of saliencyMethods.py:213
 *   gy : [N][K][HW];  weight : [K][C];  gx : [N][C][HW]
 *   grouping: 0 consecutive fours, 1 stride 4;  axis: 0 tiles along hw, 1 along c
 *   an extent < 1, K or depth no multiple of 16, K % depth != 0, tile no positive multiple of 16, an unknown grouping or axis,
 *   stagger negative or no power of two, stride < 0, a pointer that is not 4-byte aligned -> XAI_E_SHAPE;
 *   a stagger (mask != 0) along c, or one whose tile is no multiple of 32; N > 65535; K * HW or C * HW > INT32_MAX -> XAI_E_UNSUPPORTED */
int xai_convw_bwd_data_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int grouping, int from_zero, int depth,
                           int tile, int axis, int stagger, int stride, float* gx, xai_stream_t stream);

/* K81  the same sum by the plainest kernel that can say it: one wavefront per 16 x 16 outputs of one image, every operand straight
 * from global memory, no LDS; both axes.  The experiment that finds a library's stagger and the tests of K80 compare against it.
 * replaces  nothing on a hot path; the yardstick of K80 under saliencyMethods.py:213
 *   arguments as xai_convw_bwd_data_f32; its XAI_E_UNSUPPORTED cases about the stagger do not apply; C > 16 * 65535 -> XAI_E_UNSUPPORTED */
int xai_convw_bwd_data_simple_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int grouping, int from_zero,
                                  int depth, int tile, int axis, int stagger, int stride, float* gx, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_CONVW_H */
