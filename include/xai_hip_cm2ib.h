/*
 * xai_hip_cm2ib.h -- C ABI of libxai_cm2ib.so: CLIP's M2IB row (m2ib; xai_engine/m2ib.py), K88-K90.
 *
 * The grammar and the conventions are xai_clip.h's: one extern "C" block, the stream typedef, launch entries return int, end in _f32
 * or _f16 and take the caller's stream last; device pointers owned by the caller, asynchronous graph-capturable launches, nothing
 * allocated or retained, no global state, no atomics, no memset, the same bytes on every run.  Return values: 0 = success, <0 =
 * XAI_E_*, >0 = hipError_t of the launch.  Every argument check comes before the first HIP call, so a refused call needs no device.
 * T is the model's dtype, float (_f32) or IEEE half (_f16): only x9, t and dL/dt are held in T; alpha, Adam's moments, the noise and
 * the capacity are fp32 in both, as they are in the reference (InformationBottleneck.alpha is an fp32 Parameter whatever the model).
 *
 * WHAT THE REFERENCE COMPUTES (util/attribution_methods/CLIP/M2IB/scripts/iba.py:89-194, methods.py:46-51).  Visual block `layer`
 * is followed by an information bottleneck: with x the block's output (a constant of the image, x9), per element
 *   lam = sigmoid(alpha),  mu = x * lam,  var = (1 - lam) ** 2,  t = mu + sqrt(var) * eps,  eps ~ N(0, 1)          (iba.py:121-128)
 *   cap = -0.5 * (1 + log(var) - mu ** 2 - var)                                                                     (iba.py:111-114)
 * and alpha (1, L, D), from 5, takes torch.optim.Adam(lr=1) steps on  beta * mean(cap) - mean_r cos(text, image(t_r))  over R = 10
 * noisy copies.  The map is nansum over D of the cap of the last forward, per patch token.  K88 is the sample, K89 the gradient that
 * autograd gives alpha from dL/dt plus the Adam step, K90 the capacity and its nansum.  What lies between K88 and K89, the blocks
 * behind the bottleneck and the cosine, is torch's (xai_engine/m2ib.py).
 *
 * THE ARITHMETIC RULE.  Every product, sum, difference, quotient, square root, expf and logf is an fp32 operation rounded once (the
 * library is compiled with -ffp-contract=off; division and square root are the correctly rounded ones).  Per element, a = alpha, x =
 * float(x9) (exact):
 *   lam = 1 / (1 + expf(-a));  om = 1 - lam;  var = om * om;  sd = sqrtf(var);  mu = x * lam
 *   rT(y): y rounded to T, to nearest even, once (the identity for float): where image_encoder_wrapper.forward casts the
 *     bottleneck's fp32 output with .to(self.dtype) (clip_wrapper.py:53)
 *   SUM(n; a_i), by one wave: lane l sums a_i over i = l, l + 64, ... < n in ascending i from +0; then the 64 lane sums are added by
 *     an xor butterfly, offsets 32, 16, 8, 4, 2, 1 (xai_clip.h's DOT without the product)
 * These orders are this library's, not torch's: the row is held to the reference's own fp32-to-fp64 gap (tests/test_gpu_m2ib.py),
 * the kernels to this header (tests/test_gpu_m2ib_edges.py).
 *
 * THE NaN RULE.  Where lam rounds to 1 (expf(-a) < 2^-24, a above about 16.7) om = var = sd = 0, and the reference's autograd
 * multiplies d sqrt / d var = 0.5 / 0 = Inf and d log / d var = 1 / 0 = Inf by d var / d lam = -2 * 0: the gradient of that element
 * is 0 * Inf = NaN, and Adam makes its moments and its alpha a NaN for good.  It is observable behaviour, K89 keeps it (q and gv
 * below); the element's cap is then a NaN and K90's nansum leaves it out, as torch.nansum does.
 *
 * THE BOUNDS BEHIND expf AND logf, u = 2^-24.  expf(-a) is the first operation of every kernel, so nothing precedes it; what the
 * tests hold bit for bit is every kernel GIVEN lam (they read the device's lam out of K88_f32 with x9 = 1 and eps = 0: t = lam * 1 + sd
 * * 0 = lam exactly; the same expression on the same input gives the same bits in the three kernels).  The device's expf and logf are
 * within 1 ulp (HIP's documented bound) and so are a restatement's:
 *   lam: two evaluations of e = expf(-a) differ by at most 2 ulp = 4u relatively; s = 1 + e by at most 4u e / (1 + e) + 2u <= 6u
 *     relatively (each side rounds the sum once), lam = 1 / s by 6u + 2u = 8u relatively.  Where e overflows to +Inf lam is +0 on both
 *     sides, where 1 + e rounds to 1 it is 1 on both unless e lies within 4u e of 2^-24.
 *   cap, GIVEN lam (var, mu exact): lg = logf(var) differs by at most 4u |lg|; s1 = 1 + lg, s2 = s1 - mu * mu, s3 = s2 - var each round
 *     once on either side, so cap = -0.5 * s3 differs by at most 0.5 * (4u |lg| + 2u (|s1| + |s2| + |s3|)) (the product by -0.5 is exact
 *     above the subnormal range).  K90's token sums GIVEN the cap it wrote (cap_out) are restated bit for bit.
 *
 * THE LIMITS: 1 <= B <= 65535, 2 <= L <= XAI_CM2IB_MAX_TOKENS (K88, K89: 1 <= L), 1 <= D <= XAI_CM2IB_MAX_WIDTH, 1 <= R <=
 * XAI_CM2IB_MAX_COPIES (grid extents).  Every flat index is formed in int64.  Every operand is contiguous.
 */
#ifndef XAI_HIP_CM2IB_H
#define XAI_HIP_CM2IB_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_cm2ib_version() = XAI_CM2IB_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_cm2ib_version_minor() = XAI_CM2IB_MINOR: bumped whenever entry points are added:
 *   0 = xai_cm2ib_max_tokens, xai_cm2ib_max_width, xai_cm2ib_max_copies, xai_cm2ib_sample_{f32,f16}, xai_cm2ib_adam_step_{f32,f16},
 *       xai_cm2ib_saliency_f32 */
#define XAI_CM2IB_VERSION 1
#define XAI_CM2IB_MINOR 0

int xai_cm2ib_version(void);
int xai_cm2ib_version_minor(void);

#define XAI_CM2IB_MAX_TOKENS 4096
#define XAI_CM2IB_MAX_WIDTH 8192
#define XAI_CM2IB_MAX_COPIES 1024

/* = XAI_CM2IB_MAX_TOKENS, XAI_CM2IB_MAX_WIDTH, XAI_CM2IB_MAX_COPIES */
int xai_cm2ib_max_tokens(void);
int xai_cm2ib_max_width(void);
int xai_cm2ib_max_copies(void);

/* K88 the sample of the bottleneck.  A lane per (b, l, d), which walks the R copies:
 *   t[b][r][l][d] = rT(mu + sd * eps[b][r][l][d])
 * replaces  InformationBottleneck.forward's sigmoid, expand, masked_mu, masked_var and _sample_t's arithmetic (iba.py:104-108,
 *           :122-127) and the cast in front of the next block (clip_wrapper.py:53); the draw of eps itself is the caller's
 *   alpha : [B][L][D] float;  x9 : [B][L][D] T;  eps : [B][R][L][D] float;  t : [B][R][L][D] T
 *   NULL alpha, x9, eps or t -> XAI_E_NULL;  B, R, L or D < 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_cm2ib_sample_f32(const float* alpha, const void* x9, const float* eps, int B, int R, int L, int D, void* t, xai_stream_t stream);
int xai_cm2ib_sample_f16(const float* alpha, const void* x9, const float* eps, int B, int R, int L, int D, void* t, xai_stream_t stream);

/* K89 the gradient of alpha and one step of Adam, in place.  A lane per (b, l, d); g_r = float(gt[b][r][l][d]), the gradient of
 * minus the fitting term with respect to t as autograd leaves it in T:
 *   lamp = lam * om;  xl = x * lamp;  q = (0.5 / sd) * (om + om);  ql = q * lamp      (q is d sqrt(var) / d var * -d var / d lam: 1 up
 *     to rounding, 0 * Inf = NaN under THE NaN RULE;  d t / d alpha = xl - ql * eps)
 *   fit = sum of g_r * (xl - ql * eps[b][r][l][d]) over r = 0 .. R-1 in ascending r from +0
 *   gv = -0.5 * (1 / var - 1);  dcap = mu * xl - (gv * (om + om)) * lamp               (d cap / d mu = mu, d cap / d var = gv)
 *   g = fit + (beta / float(L * D)) * dcap                                              (mean over the (R, L, D) equal copies)
 * then torch's single-tensor Adam (torch/optim/adam.py, _single_tensor_adam: exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2)
 * .addcmul_(grad, grad, value=1 - beta2); denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); param.addcdiv_(exp_avg,
 * denom, value=-step_size)), in this sequence:
 *   m = m + w1 * (g - m);  v = v * b2 + (w2 * g) * g;  den = sqrtf(v) / bc2s + adam_eps;  alpha = a - step_size * (m / den)
 * with the host-made fp32 scalars of step k = 1, 2, ...: w1 = float(1 - beta1), b2 = float(beta2), w2 = float(1 - beta2), bc2s =
 * float(sqrt(1 - beta2 ** k)), step_size = float(lr / (1 - beta1 ** k)), formed in double and rounded once.  At k = 1 from m = v = 0
 * this is alpha = a -+ lr up to adam_eps: Adam's first step is sign(g).
 * replaces  loss_t.backward() through InformationBottleneck.forward and calc_loss's compression term (iba.py:185, :189-194) and
 *           optimizer.step (iba.py:186)
 *   gt : [B][R][L][D] T;  eps : [B][R][L][D] float;  x9 : [B][L][D] T;  alpha, m, v : [B][L][D] float, updated in place
 *   NULL gt, eps, x9, alpha, m or v -> XAI_E_NULL;  B, R, L or D < 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_cm2ib_adam_step_f32(const void* gt, const float* eps, const void* x9, int B, int R, int L, int D, float beta, float w1, float b2,
                            float w2, float bc2s, float step_size, float adam_eps, float* alpha, float* m, float* v, xai_stream_t stream);
int xai_cm2ib_adam_step_f16(const void* gt, const float* eps, const void* x9, int B, int R, int L, int D, float beta, float w1, float b2,
                            float w2, float bc2s, float step_size, float adam_eps, float* alpha, float* m, float* v, xai_stream_t stream);

/* K90 the capacity and the map in front of the resize.  A wave per token (b, l):
 *   cap[l][d] = -0.5 * (((1 + logf(var)) - mu * mu) - var)
 *   out[b][l - 1] = SUM(D; cap[l][d] if it is not a NaN, else +0)   for l = 1 .. L-1 (token 0 is the class token, iba.py:154)
 * A token whose every term is a NaN gives +0; a +Inf term (var = 0 without a NaN, or x9 = +-Inf) stays in the sum.
 * replaces  _calc_capacity (iba.py:111-114) of the last forward that is read, the mean over its R equal copies (iba.py:171), and
 *           torch.nansum(saliency, -1)[1:] (iba.py:154)
 *   alpha : [B][L][D] float;  x9 : [B][L][D] float (_f32 only: K90 runs once per map, the caller converts a half x9, which is
 *   exact);  out : [B][L - 1] float;
 *   cap_out : [B][L][D] float, every cap[l][d], token 0 included, or NULL: not written (the tests read them)
 *   NULL alpha, x9 or out -> XAI_E_NULL;  B < 1, L < 2, D < 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_cm2ib_saliency_f32(const float* alpha, const float* x9, int B, int L, int D, float* cap_out, float* out, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_CM2IB_H */
