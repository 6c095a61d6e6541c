/*
 * xai_clip.h -- C ABI of libxai_clip.so: the row reductions of the Grad-ECLIP rows for CLIP (eclip, eclip_wo, eclip_nograd,
 * maskclip, selfattn; xai_engine/eclip.py), K75-K77.
 *
 * The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries return int and take the caller's stream last),
 * with one addition: the launch entries of this header end in _f32 or _f16.  Operands come in the model's dtype T, float (_f32) or
 * IEEE half (_f16), one template; their pointers are void* here.  The conventions are xai_hip.h's too: device pointers owned by the
 * caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state, no atomics, no memset, the same
 * bytes on every run.  Return values: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so) has
 * the text.  Every argument check comes before the first HIP call, so a refused call needs no device.
 *
 * WHAT THE REFERENCE COMPUTES (util/attribution_methods/CLIP/generate_emap.py): clip_encode_dense :309-376 runs the last visual
 * block as ONE head of width D over all L tokens (attention_layer :288-307), and grad_eclip :453-485, mask_clip :500-529 and the
 * selfattn row (evaluatePerturbation.py:424) read only the class-token row of it: grad[:1,0,:], q_out[:1,0,:], attn[0,:1,1:].
 * These kernels compute that row.
 *
 * THE ARITHMETIC RULE, both dtypes.  rT(x) is x rounded to T (to nearest, ties to even; the identity for float).  Every product,
 * sum, quotient, exp and square root is an fp32 operation rounded once (the library is compiled with -ffp-contract=off, and
 * division and square root are the correctly rounded ones).  A value passes through rT exactly where the reference materialises a
 * tensor of dtype T: `q * scaling`, the scores, the softmax, the attention output, a norm, each element-wise product or quotient,
 * each `.sum(-1)`, the min and max, the stacked `.sum(0)` over the texts.  The final maps are written as fp32.
 *   DOT(n; a_i, b_i), the sum over one row by one wave: lane l sums a_i * b_i over i = l, l + 64, l + 128, ... < n in ascending i
 *     from +0; then the 64 lane sums are added by an xor butterfly, offsets 32, 16, 8, 4, 2, 1 (v = v + partner's v)
 *   SUMSQ(n; a_i) = DOT(n; a_i, a_i);  SUM(n; a_i): the same tree over a_i alone
 *   NORMALIZE(a) (torch's F.normalize, `a / a.norm().clamp_min(1e-12)`): n = rT(sqrt(SUMSQ(a))), e = rT(1e-12) (which is 0 in half),
 *     m = n < e ? e : n (a NaN n stays), and a'_i = rT(a_i / m)
 *   BLOCKSUM(L; e_j), the softmax denominator by a workgroup of 1024 lanes: lane t sums e_j over j = t, t + 1024, ... < L in ascending
 *     j from +0; the butterfly above inside each wave; then the sixteen wave sums in ascending wave order from +0
 *
 * THE LIMITS: 2 <= L <= XAI_CLIP_MAX_TOKENS, 1 <= D <= XAI_CLIP_MAX_WIDTH, 1 <= E <= XAI_CLIP_MAX_WIDTH, 1 <= T <= XAI_CLIP_MAX_TEXTS,
 * 1 <= B <= 65535 (a grid extent).  A workgroup keeps one row of D floats and one of L floats in LDS: (8192 + 4096) * 4 bytes = 48 KiB
 * at the limits, inside the 64 KiB a workgroup may take on gfx950 (of 160 KiB per CU), with room for the reduction scratch.  Every
 * flat index is formed in int64.  Row strides are in elements; the last axis of every operand is contiguous.
 *
 * THE BOUND AFTER THE FIRST EXP (K75).  Everything before it (round(q * scaling), the scores, their max) is defined bit for bit by
 * the rule above.  e_j = expf(s_j - max): the device expf is within 1 ulp of exp (HIP's documented bound), and so is a restatement's
 * float32 exp, so two evaluations differ by at most 2 ulp = 4u relatively, u = 2^-24.  BLOCKSUM adds numbers that differ by that
 * much through a tree of depth n = ceil(L / 1024) + 6 + 16, each addition rounding differently by at most u on either side: the two
 * sums differ by at most (4 + 2n)u relatively.  p_j = rT(e_j / sum): (4 + 4 + 2n + 2)u = (10 + 2n)u relatively before rT, and rT may
 * move two such neighbours to adjacent values of T, one ulp of T apart.  att_output[d] = rT(sum_j p_j v_jd), in ascending j from +0:
 * the two sums differ by at most sum_j |dp_j| |v_jd| + 2 L u sum_j |p_j v_jd|, and again one ulp of T after rT.
 * The relative 1 ulp of expf holds in the normal range only: below 2^-126 one ulp is 2^-149 absolute.  So for float dp_j gains
 * 3 * 2^-149: the sum is at least 1 because the maximum contributes e = 1, so the quotient does not enlarge the two exps' 2 * 2^-149,
 * and the quotient's own rounding adds one more.  (The device's expf keeps subnormal results, it does not return 0 for them:
 * tests/test_gpu_clip_edges.py runs e_j down through the subnormal range to 0 and holds this term.)
 */
#ifndef XAI_CLIP_H
#define XAI_CLIP_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_clip_version() = XAI_CLIP_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_clip_version_minor() = XAI_CLIP_MINOR: bumped whenever entry points are added:
 *   0 = xai_clip_max_tokens, xai_clip_max_width, xai_clip_max_texts, xai_clip_cls_attention_f32, xai_clip_cls_attention_f16,
 *       xai_clip_eclip_map_f32, xai_clip_eclip_map_f16, xai_clip_maskclip_map_f32, xai_clip_maskclip_map_f16 */
#define XAI_CLIP_VERSION 1
#define XAI_CLIP_MINOR 0

int xai_clip_version(void);
int xai_clip_version_minor(void);

#define XAI_CLIP_MAX_TOKENS 4096
#define XAI_CLIP_MAX_WIDTH 8192
#define XAI_CLIP_MAX_TEXTS 1024

/* = XAI_CLIP_MAX_TOKENS, XAI_CLIP_MAX_WIDTH, XAI_CLIP_MAX_TEXTS */
int xai_clip_max_tokens(void);
int xai_clip_max_width(void);
int xai_clip_max_texts(void);

/* K75 the class-token row of the one-head attention.  One workgroup of 1024 lanes (16 waves) per image, a wave per key row:
 *   qs_d = rT(q0[b][d] * scaling);  s_j = rT(DOT(D; qs_d, k[j][b][d])), j < L;  m = max_j s_j;  e_j = expf(s_j - m);
 *   attn[b][j] = p_j = rT(e_j / BLOCKSUM(L; e_j));  att_out[b][d] = rT(sum_j p_j * v[j][b][d]), ascending j from +0, a lane per d.
 * K and V are read once.  `scaling` is the caller's float(D) ** -0.5 rounded to float.
 * replaces  attention_layer (generate_emap.py:288-307) for the query row 0, as clip_encode_dense :348 calls it (num_heads = 1)
 *   q0 : [B][D], the class row of q;  k, v : element (j, b, d) at j * ld_l + b * ld_b + d;  attn : [B][L] T;  att_out : [B][D] T;
 *   scores : [B][L] T, the s_j, or NULL: not written (the tests read them: they are the last values before the exp)
 *   NULL -> XAI_E_NULL;  B < 1, L < 2, D < 1, ld_l < D, ld_b < D with B > 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_clip_cls_attention_f32(const void* q0, const void* k, int64_t k_ld_l, int64_t k_ld_b, const void* v, int64_t v_ld_l,
                               int64_t v_ld_b, int B, int L, int D, float scaling, void* scores, void* attn, void* att_out,
                               xai_stream_t stream);
int xai_clip_cls_attention_f16(const void* q0, const void* k, int64_t k_ld_l, int64_t k_ld_b, const void* v, int64_t v_ld_l,
                               int64_t v_ld_b, int B, int L, int D, float scaling, void* scores, void* attn, void* att_out,
                               xai_stream_t stream);

/* K76 the Grad-ECLIP map.  One workgroup of 1024 lanes (16 waves) per image, a wave per patch row i = 1 .. L - 1:
 *   withksim:  q' = NORMALIZE(q_out0[b]), k'_i = NORMALIZE(k_out[i][b]), c_i = rT(SUM(D; rT(q'_d * k'_id)));  lo = min_i c_i,
 *     hi = max_i c_i (NaN if any c_i is NaN, as torch's min and max);  w_i = rT(rT(c_i - lo) / rT(hi - lo)), 0 / 0 = NaN kept
 *   per text t:  withgrad and withksim: m_ti = rT(SUM(D; rT(rT(g_td * v_id) * w_i)));  withgrad only: rT(SUM(D; rT(g_td * v_id)));
 *     withksim only: rT(SUM(D; rT(v_id * w_i)));  neither: rT(SUM(D; v_id));  g = grad_cls[b][t], v = v[i][b]
 *   out[b][i - 1] = float(rT(sum_t relu(m_ti))), ascending t from +0;  relu(x) = x > 0 ? x : +0, and a NaN stays
 * replaces  grad_eclip (generate_emap.py:453-485) after its autograd.grad, and the stack(...).sum(0) of evaluatePerturbation.py:402-409
 *   q_out0 : [B][D] (unread and may be NULL when withksim == 0);  k_out (the same), v : strided as in K75;  grad_cls : [B][T][D], may
 *   be NULL when withgrad == 0;  out : [B][L - 1] float
 *   a needed pointer NULL -> XAI_E_NULL;  extents and strides as K75, T < 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_clip_eclip_map_f32(const void* q_out0, const void* k_out, int64_t k_ld_l, int64_t k_ld_b, const void* v, int64_t v_ld_l,
                           int64_t v_ld_b, const void* grad_cls, int B, int L, int D, int T, int withksim, int withgrad, float* out,
                           xai_stream_t stream);
int xai_clip_eclip_map_f16(const void* q_out0, const void* k_out, int64_t k_ld_l, int64_t k_ld_b, const void* v, int64_t v_ld_l,
                           int64_t v_ld_b, const void* grad_cls, int B, int L, int D, int T, int withksim, int withgrad, float* out,
                           xai_stream_t stream);

/* K77 the MaskCLIP map.  One workgroup of 1024 lanes (16 waves) per image, a wave per patch row i = 1 .. L - 1:
 *   f' = NORMALIZE(v_final[b][i - 1]);  a_ti = rT(DOT(E; f'_e, txt[b][t][e])) (a matrix product: its products are not rounded to T);
 *   k'_0 = NORMALIZE(k_out[0][b]), k'_i = NORMALIZE(k_out[i][b]), c_i = rT(SUM(D; rT(k'_0d * k'_id)));
 *   out[b][i - 1] = float(rT(sum_t rT(a_ti * c_i))), ascending t from +0
 * replaces  mask_clip (generate_emap.py:500-529) and the .sum(0) of evaluatePerturbation.py:416-417
 *   v_final : [B][L - 1][E];  txt : text t of image b at b * txt_ld_b + t * E, txt_ld_b = 0 for texts shared by the images;
 *   k_out : strided as in K75;  out : [B][L - 1] float
 *   NULL -> XAI_E_NULL;  extents and strides as K75, E < 1, T < 1, txt_ld_b < 0 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_clip_maskclip_map_f32(const void* v_final, const void* txt, int64_t txt_ld_b, const void* k_out, int64_t k_ld_l, int64_t k_ld_b,
                              int B, int L, int D, int E, int T, float* out, xai_stream_t stream);
int xai_clip_maskclip_map_f16(const void* v_final, const void* txt, int64_t txt_ld_b, const void* k_out, int64_t k_ld_l, int64_t k_ld_b,
                              int B, int L, int D, int E, int T, float* out, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_CLIP_H */
