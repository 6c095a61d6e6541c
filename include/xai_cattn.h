/*
 * xai_cattn.h -- C ABI of libxai_cattn.so: the attention rows of CLIP (game, rollout, lrp; xai_engine/clip_attn.py), K82-K85.
 *
 * The grammar and the conventions are xai_clip.h's: one extern "C" block, the stream typedef, launch entries return int, end in _f32
 * or _f16 (one template, operands of the model's dtype T behind void*) and take the caller's stream last; device pointers owned by
 * the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global state, no atomics, no memset, the same
 * bytes on every run.  Return values: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch.  Every argument check comes before
 * the first HIP call, so a refused call needs no device.
 *
 * WHAT THE REFERENCE COMPUTES (util/attribution_methods/CLIP/generate_emap.py): mm_interpret :133-174, compute_rollout_attention
 * :269-285 and clip_lrp :207-239 read the attention probabilities A_i,h (L x L, block i, head h) of the visual tower and the
 * gradients G_i,h of the image-text logit with respect to them, nothing else:
 *   game     last block only:  R = I + mean_h clamp(G_h * A_h, min=0), the map is R[0, 1:], summed over the texts
 *   rollout  last block only:  avg = A.sum(0) / A.shape[0] over the T * H leading entries; (avg + I_fp32)[0] / its row sum, [1:]
 *   lrp      every block:      C_i = mean_h clamp(G_i,h * A_i,h, min=0);  R <- R + C_i @ R from R = I, i = 0 .. n-1; the map is R[0, 1:]
 * Behind the last attention every operation is token-wise and the tower reads token 0 only, so in the last block G is zero outside
 * row 0 and G_h[0][j] = <g_h, V_h[j]>, g the gradient of the logit with respect to row 0 of the attention output (D values, head h
 * owning d = D / H of them): game needs one row.  Only row 0 of lrp's final R is read, and e_0^T (I + C_n-1) ... (I + C_0) is a chain
 * of n vector-matrix products from the last block down: K85.  That chain associates the products differently from the reference's
 * matrix chain; it is held to the reference's own precision gap, not to its bits (tests/test_gpu_clip_attn.py).
 *
 * THE ARITHMETIC RULE, both dtypes, is xai_clip.h's.  rT(x) is x rounded to T (to nearest, ties to even; the identity for float).
 * Every product, sum and quotient is an fp32 operation rounded once (-ffp-contract=off; the division is the correctly rounded one).
 * A value passes through rT exactly where the reference materialises a tensor of dtype T: the gradient G (a matrix product of T), the
 * product G * A, the mean over the heads, the sum over the texts, the product C @ R and the sum R + C @ R.  The maps are written as fp32.
 *   DOT(n; a_i, b_i), by one wave: lane l sums a_i * b_i over i = l, l + 64, ... < n in ascending i from +0; then the 64 lane sums are
 *     added by an xor butterfly, offsets 32, 16, 8, 4, 2, 1 (xai_clip.h's DOT; a matrix product: its products are not rounded to T)
 *   relu(x) = x > 0 ? x : +0, and a NaN stays (torch's clamp(min=0))
 *   MEAN_h(x_h) = rT((sum of x_h over h = 0 .. H-1 in ascending h from +0) / float(H)): torch's half `mean` is an fp32 sum scaled once
 *     and rounded once; it is not rT(rT(sum) / H).  (For float this is the value K52 of libxai_ext4.so computes in its mode 0.)
 *
 * THE LIMITS: 2 <= L <= XAI_CATTN_MAX_TOKENS, 1 <= H, H divides D, D <= XAI_CATTN_MAX_WIDTH, 1 <= T <= XAI_CATTN_MAX_TEXTS,
 * 1 <= B <= 65535 and 1 <= n * B <= 65535 (grid extents).  Every flat index is formed in int64.
 */
#ifndef XAI_CATTN_H
#define XAI_CATTN_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_cattn_version() = XAI_CATTN_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_cattn_version_minor() = XAI_CATTN_MINOR: bumped whenever entry points are added:
 *   0 = xai_cattn_max_tokens, xai_cattn_max_width, xai_cattn_max_texts, xai_cattn_game_map_f32/_f16, xai_cattn_rollout_row_f32/_f16,
 *       xai_cattn_lrp_matrices_f32/_f16, xai_cattn_lrp_row_f32/_f16 */
#define XAI_CATTN_VERSION 1
#define XAI_CATTN_MINOR 0

int xai_cattn_version(void);
int xai_cattn_version_minor(void);

#define XAI_CATTN_MAX_TOKENS 4096
#define XAI_CATTN_MAX_WIDTH 8192
#define XAI_CATTN_MAX_TEXTS 1024

/* = XAI_CATTN_MAX_TOKENS, XAI_CATTN_MAX_WIDTH, XAI_CATTN_MAX_TEXTS */
int xai_cattn_max_tokens(void);
int xai_cattn_max_width(void);
int xai_cattn_max_texts(void);

/* K82 the game map.  One workgroup of 1024 lanes (16 waves) per image, a wave per patch column j = 1 .. L - 1; d = D / H:
 *   per text t and head h:  G = rT(DOT(d; g[b][t][h * d + i], v[j][b][h * d + i]));  p = rT(G * a0[b][h][j])
 *   m_tj = MEAN_h(relu(p));  out[b][j - 1] = float(rT(sum_t m_tj)), ascending t from +0
 * replaces  mm_interpret (generate_emap.py:133-174, start_layer = -1) after its autograd.grad, and the emap.sum(0) of
 *           evaluatePerturbation.py:414
 *   g : [B][T][D], the gradient of text t's logit with respect to row 0 of the last block's attention output;
 *   v : element (j, b, c) at j * v_ld_l + b * v_ld_b + c (the V third of the in-projection, as K75 reads it);
 *   a0 : [B][H][L], the class-token row of each head's attention;  out : [B][L - 1] float
 *   NULL -> XAI_E_NULL;  B < 1, L < 2, D < 1, H < 1, H not dividing D, T < 1, v_ld_l < D, v_ld_b < D with B > 1 -> XAI_E_SHAPE;
 *   over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_cattn_game_map_f32(const void* g, const void* v, int64_t v_ld_l, int64_t v_ld_b, const void* a0, int B, int L, int D, int H, int T,
                           float* out, xai_stream_t stream);
int xai_cattn_game_map_f16(const void* g, const void* v, int64_t v_ld_l, int64_t v_ld_b, const void* a0, int B, int L, int D, int H, int T,
                           float* out, xai_stream_t stream);

/* K83 the rollout row.  One workgroup of 256 lanes (4 waves) per image:
 *   s_j = rT(sum of a0[b][h][j], taken T times over, in ascending h inside ascending t, from +0)   (the reference repeats the image
 *     once per text, so its A.sum(0) runs over T * H entries);  avg_j = rT(s_j / float(T * H));
 *   a_j = float(avg_j) + (j == 0 ? 1.f : 0.f)   (the reference's eye is fp32);
 *   S = the sum of a_j over the row: lane l sums j = l, l + 256, ... < L in ascending j from +0, the butterfly of DOT inside each
 *     wave, then the four wave sums in ascending wave order from +0;  out[b][j - 1] = a_j / S, j = 1 .. L - 1
 * replaces  the attentions of mm_interpret(rollout=True) (:160-162) and compute_rollout_attention (:269-285) on their one matrix
 *   a0 : [B][H][L];  out : [B][L - 1] float
 *   NULL -> XAI_E_NULL;  B < 1, L < 2, H < 1, T < 1 -> XAI_E_SHAPE;  over THE LIMITS (H <= XAI_CATTN_MAX_WIDTH) -> XAI_E_UNSUPPORTED */
int xai_cattn_rollout_row_f32(const void* a0, int B, int H, int L, int T, float* out, xai_stream_t stream);
int xai_cattn_rollout_row_f16(const void* a0, int B, int H, int L, int T, float* out, xai_stream_t stream);

/* K84 the relevance matrices of lrp, every block in one launch; it reads 2 n H L^2 values once and writes n L^2.  A lane per element
 * (k, j) of a block's matrix, or per 16 bytes of them:
 *   c[b][i][k][j] = MEAN_h(relu(rT(grad[i][b][h][k][j] * attn[i][b][h][k][j])))
 * The 16-byte flavour runs when L * L is a multiple of 16 / sizeof(T) and the three pointers are 16-byte aligned, the scalar one
 * otherwise; both give the same bytes.
 * replaces  clip_lrp (generate_emap.py:231-237): grad * cam, clamp(min=0), mean over the heads
 *   attn, grad : [n][B][H][L][L] of T;  c : [B][n][L][L] of T
 *   NULL -> XAI_E_NULL;  n < 1, B < 1, H < 1, L < 2 -> XAI_E_SHAPE;  over THE LIMITS (H <= XAI_CATTN_MAX_WIDTH) -> XAI_E_UNSUPPORTED */
int xai_cattn_lrp_matrices_f32(const void* attn, const void* grad, int n, int B, int H, int L, void* c, xai_stream_t stream);
int xai_cattn_lrp_matrices_f16(const void* attn, const void* grad, int n, int B, int H, int L, void* c, xai_stream_t stream);

/* K85 the class-token row of lrp's relevance.  One workgroup of 1024 lanes per image, r (L values of T, held as floats) in LDS,
 * r = e_0 at the start; for i = n - 1 down to 0, a lane per column j:
 *   u_j = rT(sum of r_k * c[b][i][k][j] over k = 0 .. L-1 in ascending k from +0)   (a matrix product: its products are not rounded)
 *   r_j <- rT(r_j + u_j), every j from the r of the step before
 *   out[b][j - 1] = r_j, j = 1 .. L - 1
 * replaces  R = R + torch.bmm(cam, R) of clip_lrp (:238) for row 0 of the final R, and image_relevance = R[:, 0, 1:] (:239)
 *   c : [B][n][L][L] of T, as K84 writes it;  out : [B][L - 1] float
 *   NULL -> XAI_E_NULL;  n < 1, B < 1, L < 2 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_cattn_lrp_row_f32(const void* c, int n, int B, int L, float* out, xai_stream_t stream);
int xai_cattn_lrp_row_f16(const void* c, int n, int B, int L, float* out, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_CATTN_H */
