/*
 * xai_hip_compact.h -- C ABI of libxai_compact.so, the extension library of the compact-layout BN/ReLU kernels beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11 and include/xai_hip_ext.h ... include/xai_hip_ext7.h are frozen or pinned by their tests, each
 * to its exact entry list; entry points added after that live here, in a library of their own with a version pair of its own.  The
 * grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int and
 * take the caller's stream last), so xai_engine/_lib.py binds this header with the same strict reader, and so are the conventions:
 * device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state, no
 * atomics.  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so)
 * has the text.  Every argument check comes before the first HIP call, so a refused call needs no device.
 *
 * These are the fused BatchNorm + ReLU (+ add) kernels of xai_hip.h (xai_bn_relu_fwd_mask_f32, xai_bn_relu_bwd_mask_f32 and its
 * guided twin) with operands in other layouts, for the two places of a ResNet gradient pass (the autograd.grad of
 * saliencyMethods.py:213 through the classifiers of evaluatePerturbation.py:627-640) where a tensor exists only to change a layout
 * or to repeat what is known:
 *   - the strided 1x1 convolution of a down-sampling shortcut, which MIOpen runs as one GEMM on channel-major (CNHW) tensors between
 *     layout kernels, a zero-fill and a scatter.  K62 gathers its input once, the convolution runs at stride 1 on the compact tensor
 *     (MIOpen moves nothing there), K63 reads its output and K64 writes its output gradient in CNHW order, and K64 at the block
 *     before takes its compact input gradient in place of the dense, three-quarters-zero one;
 *   - the head, AdaptiveAvgPool2d(1) + Linear behind score[n] = logits[n][target[n]] (saliencyMethods.py:209), whose backward is a
 *     constant per (n, c): K64 forms it from grad_out, the Linear's weight and the targets.
 * Per element every expression, its order of operations and the gate-mask layout are those of the xai_hip.h entries; only where an
 * operand is read or written differs.  CNHW: element (n, c, r) of an [N][C][HW] tensor sits at (c * N + n) * HW + r.
 */
#ifndef XAI_HIP_COMPACT_H
#define XAI_HIP_COMPACT_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_compact_version() = XAI_COMPACT_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_compact_version_minor() = XAI_COMPACT_MINOR: bumped whenever entry points are added:
 *   0 = xai_stride_gather_cnhw_f32, xai_bn_relu_fwd_cnhw_f32, xai_bn_relu_bwd_compact_f32, xai_bn_relu_bwd_bcast_f32 */
#define XAI_COMPACT_VERSION 1
#define XAI_COMPACT_MINOR 0

int xai_compact_version(void);
int xai_compact_version_minor(void);

/* K62  out[c][n][ho][wo] = side[n][c][ho * stride][wo * stride],  Ho = (H - 1) / stride + 1, Wo likewise: the input of a
 * kernel-1, pad-0 convolution at `stride`, compact and channel-major.  16-byte stores where N*C*Ho*Wo % 4 == 0 and `out` is aligned.
 * replaces  the strided NCHW -> CNHW gather inside the down-sample convolutions of evaluatePerturbation.py:627-640
 *   side : [N][C][H][W];  out : [C][N][Ho][Wo];  an extent < 1 -> XAI_E_SHAPE;  N * C > INT32_MAX -> XAI_E_UNSUPPORTED */
int xai_stride_gather_cnhw_f32(const float* side, int N, int C, int H, int W, int stride, float* out, xai_stream_t stream);

/* K63  xai_bn_relu_fwd_mask_f32 with the identity operand (required) in CNHW order: y = relu(bn(x) + identity) or, with the
 * second BatchNorm (weight2 ... var2, nullable as a set), relu(bn(x) + bn2(identity)).  y is NCHW and the same bits.
 * `mask` as there, or NULL when no gradient will be taken (then no gate is written: xai_bn_act_fwd_f32's result).
 * replaces  the CNHW -> NCHW transpose behind the same convolutions, under saliencyMethods.py:213
 *   x, y : [N][C][HW];  identity_cnhw : [C][N][HW];  refusals as xai_bn_relu_fwd_mask_f32;  N * C > INT32_MAX -> XAI_E_UNSUPPORTED */
int xai_bn_relu_fwd_cnhw_f32(const float* x, const float* identity_cnhw, const float* weight, const float* bias, const float* mean,
                             const float* var, float eps, const float* weight2, const float* bias2, const float* mean2,
                             const float* var2, float eps2, int variant, int N, int C, int HW, float* y, void* mask,
                             xai_stream_t stream);

/* K64  xai_bn_relu_bwd_mask_f32 (guided != 0: xai_bn_relu_bwd_mask_guided_f32) where
 *   g_identity_cnhw != 0 : g_identity is written in CNHW order, [C][N][HW];
 *   gy2_compact != NULL  : the second gradient is [C][N][Ho][Wo], the input gradient of a kernel-1, pad-0 convolution at `stride`
 *                          over planes of width W (HW % W == 0): g = gy + gy2_compact[c][n][h / stride][w / stride] where stride
 *                          divides both h and w, g = gy + (+0) everywhere else (so -0 becomes +0 there, as with the dense
 *                          zero-filled tensor).  gy2 (dense) must then be NULL.
 * replaces  the zero-fill, the NCHW -> CNHW transpose and the strided scatter around the backward of the same convolutions, under
 *           saliencyMethods.py:213
 *   refusals as xai_bn_relu_bwd_mask_f32;  both gy2 forms, W or stride < 1, HW % W != 0 -> XAI_E_SHAPE;
 *   g_identity_cnhw without g_identity -> XAI_E_NULL */
int xai_bn_relu_bwd_compact_f32(const float* gy, const float* gy2, const float* gy2_compact, int W, int stride, const void* mask,
                                const float* weight, const float* var, float eps, const float* weight2, const float* var2,
                                float eps2, int variant, int guided, int N, int C, int HW, float* gx, float* g_identity,
                                int g_identity_cnhw, xai_stream_t stream);

/* K64  the same backward at the LAST block of a classifier whose head is AdaptiveAvgPool2d(1) + Linear and whose score is one logit
 * per image (saliencyMethods.py:209, :213).  gy is then no tensor: PyTorch's gather, Linear and mean backward hand on
 *     gy[n][c][hw] = (grad_out[n] * fc_weight[targets[n]][c]) * scale        divisor == 0  (PyTorch: scale = 1.0f / HW)
 *                  = (grad_out[n] * fc_weight[targets[n]][c]) / divisor      divisor != 0
 * for every hw, and the kernel forms that value per element, with those two roundings, instead of reading N*C*HW floats.
 * replaces  ones_like -> gather backward (fill, scatter) -> Linear backward (GEMM) -> mean backward (expand, scale)
 *   grad_out : [N];  fc_weight : [classes][C];  targets : [N] int64, values outside [0, classes) are clamped into it;
 *   gy2 (dense, nullable), mask ... g_identity (NCHW) as xai_bn_relu_bwd_mask_f32;  classes < 1 -> XAI_E_SHAPE */
int xai_bn_relu_bwd_bcast_f32(const float* grad_out, const float* fc_weight, const int64_t* targets, int classes, float scale,
                              float divisor, const float* gy2, const void* mask, const float* weight, const float* var, float eps,
                              const float* weight2, const float* var2, float eps2, int variant, int guided, int N, int C, int HW,
                              float* gx, float* g_identity, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_COMPACT_H */
