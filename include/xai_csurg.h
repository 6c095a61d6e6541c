/*
 * xai_csurg.h -- C ABI of libxai_csurg.so: the CLIP Surgery row (surgery; xai_engine/surgery.py), K86-K87.
 *
 * The grammar and the conventions are xai_clip.h's: one extern "C" block, the stream typedef, launch entries return int, end in _f32
 * and take the caller's stream last; device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or
 * retained, no global state, no atomics, no memset, the same bytes on every run.  Return values: 0 = success, <0 = XAI_E_*, >0 =
 * hipError_t of the launch.  Every argument check comes before the first HIP call, so a refused call needs no device.  The entries
 * come in _f32 only: the reference runs this row in fp32 (its build_model.py leaves convert_weights commented out).
 *
 * WHAT THE REFERENCE COMPUTES (util/attribution_methods/CLIP/CLIP_Surgery/clip/clip_surgery_model.py, clip.py:271-308,
 * generate_emap.py:117-129).  The last six visual blocks get a second path that never feeds back into the plain one:
 *   x_new = x_in + sum_i proj_i(softmax((v_i v_i^T) * scale) v_i),  v_i the V third of block i's in-projection of ln_1(x_ori),
 * per head, d = D / H, scale = d ** -0.5 (Attention.forward :71-103).  K86 is that v-v attention of all blocks, images and heads.
 * Behind ln_post and the projection, clip_surgery_map divides the (1, L, E) features by their norm over dim=1, the TOKENS, per
 * embedding channel (observable behaviour, kept), and clip_feature_surgery forms
 *   w = softmax(2 f_0 t^T) / mean,  feats[i][t][c] = f_ic t_tc w_t,  sim[i][t] = sum_c (feats[i][t][c] - mean_t feats[i][t][c])
 * whose (L, T, E) tensor is never needed: sim[i][t] = sum_c f_ic (w_t t_tc - r_c), r_c = mean_t w_t t_tc.  get_similarity_map
 * min-max-normalises sim over the patches i >= 1 per text.  K87 is everything from the features to that normalised map.
 *
 * THE ARITHMETIC RULE.  Every product, sum, difference, quotient, square root and exp is an fp32 operation rounded once (the
 * library is compiled with -ffp-contract=off; division and square root are the correctly rounded ones).
 *   DOT(n; a_i, b_i), by one wave: lane l sums a_i * b_i over i = l, l + 64, ... < n in ascending i from +0; then the 64 lane sums are
 *     added by an xor butterfly, offsets 32, 16, 8, 4, 2, 1 (xai_clip.h's DOT);  SUM(n; a_i): the same tree over a_i alone
 *   MAX(n; a_i): the largest a_i that is not a NaN (fmaxf from -Inf; -Inf if every a_i is a NaN).  It is a value, not an order: of
 *     -0 and +0 either may be returned, and what is computed from it below does not depend on which.
 * These orders of summation are this library's, not torch's: the row is held to the reference's own fp32-to-fp64 gap, not to its
 * bits (tests/test_gpu_surgery.py); the kernels are held to this header bit for bit up to the first exp and to the bounds below
 * after it (tests/test_gpu_surgery_edges.py).
 *
 * THE LIMITS: 2 <= L <= XAI_CSURG_MAX_TOKENS, 1 <= H, H divides D, D <= XAI_CSURG_MAX_WIDTH, 1 <= E <= XAI_CSURG_MAX_WIDTH,
 * 1 <= T <= XAI_CSURG_MAX_TEXTS, 1 <= B <= 65535, 1 <= H <= 65535 and 1 <= n * B <= 65535 (grid extents).  K86 keeps one head's V,
 * L rows of d floats at a row stride of d + 1, and one row of L probabilities per wave in LDS: with its XAI_CSURG_VV_WAVES = 4 waves
 * that is L * (d + 1) + 4 * L floats, which must fit XAI_CSURG_LDS_FLOATS = 16384 floats, the 64 KiB a workgroup may take on gfx950
 * (of 160 KiB per CU: at L = 197, d = 64 a workgroup takes 54 KiB and two of them share a CU).  So K86 takes
 * L * (d + 1 + XAI_CSURG_VV_WAVES) <= XAI_CSURG_LDS_FLOATS, L <= 237 at d = 64; anything above returns XAI_E_UNSUPPORTED.  K87
 * keeps 2 E + T floats in LDS (n_c, r_c, w_t), 68 KiB at the limits of E and T together, so it takes 2 * E + T <= XAI_CSURG_LDS_FLOATS.
 * Every flat index is formed in int64.  Row strides are in elements; the last axis of every operand is contiguous.
 *
 * THE BOUND AFTER THE FIRST EXP, K86.  The scores s_ij and their maximum are defined bit for bit by the rule above.  e_j =
 * expf(s_ij - m): the device expf is within 1 ulp of exp (HIP's documented bound) and so is a restatement's float32 exp, so two
 * evaluations differ by at most 2 ulp = 4u relatively, u = 2^-24.  SUM adds numbers that differ by that much through a tree of depth
 * n = ceil(L / 64) + 6, each addition rounding differently by at most u on either side: the sums differ by at most (4 + 2n)u.
 * p_j = e_j / sum: (4 + 4 + 2n + 2)u = (10 + 2n)u relatively.  o_ic = sum_j p_j v_jc in ascending j from +0: the two sums differ by at
 * most sum_j |dp_j| |v_jc| + 2 L u sum_j |p_j v_jc|.  The relative ulp of expf holds in the normal range only; below 2^-126 one ulp is
 * 2^-149 absolute, so dp_j gains 3 * 2^-149 (the sum is at least 1 because the maximum contributes e = 1; two exps and the quotient's
 * own rounding).  The device's expf keeps subnormal results.
 * THE BOUND OF K87's w.  prob_t and x_t = 2 prob_t are defined bit for bit.  With n = ceil(T / 64) + 6: p_t = e_t / SUM(e) differs by
 * (10 + 2n)u as above; P = SUM(T; p_t) by (10 + 2n + 2n)u; mean = P / float(T) by two more; w_t = p_t / mean by
 * (10 + 2n) + (12 + 4n) + 2 = (24 + 6n)u relatively, plus (3 T + 2) * 2^-149 absolute for the subnormal range (dp_t = 3 * 2^-149
 * enlarged by 1 / mean, which is about T, and the quotient's rounding).  Everything behind w is exact arithmetic on w again: K87 fed
 * the w it wrote is restated bit for bit.
 */
#ifndef XAI_CSURG_H
#define XAI_CSURG_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_csurg_version() = XAI_CSURG_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_csurg_version_minor() = XAI_CSURG_MINOR: bumped whenever entry points are added:
 *   0 = xai_csurg_max_tokens, xai_csurg_max_width, xai_csurg_max_texts, xai_csurg_lds_floats, xai_csurg_vv_waves,
 *       xai_csurg_vv_attention_f32, xai_csurg_similarity_map_f32 */
#define XAI_CSURG_VERSION 1
#define XAI_CSURG_MINOR 0

int xai_csurg_version(void);
int xai_csurg_version_minor(void);

#define XAI_CSURG_MAX_TOKENS 4096
#define XAI_CSURG_MAX_WIDTH 8192
#define XAI_CSURG_MAX_TEXTS 1024
#define XAI_CSURG_LDS_FLOATS 16384
#define XAI_CSURG_VV_WAVES 4

/* = XAI_CSURG_MAX_TOKENS, XAI_CSURG_MAX_WIDTH, XAI_CSURG_MAX_TEXTS, XAI_CSURG_LDS_FLOATS, XAI_CSURG_VV_WAVES */
int xai_csurg_max_tokens(void);
int xai_csurg_max_width(void);
int xai_csurg_max_texts(void);
int xai_csurg_lds_floats(void);
int xai_csurg_vv_waves(void);

/* K86 the v-v self-attention of n blocks x B images x H heads in one launch.  One workgroup of XAI_CSURG_VV_WAVES waves per (tile
 * of 16 query rows, head, block * B + image); the head's V is staged once in LDS, then a wave per query row i, d = D / H:
 *   s_ij = (sum of v_ic * v_jc over c = 0 .. d-1 in ascending c from +0) * scale, a lane per key j   (so s_ij == s_ji bit for bit);
 *   m = MAX(L; s_ij);  e_j = expf(s_ij - m);  p_j = e_j / SUM(L; e_j);
 *   out[blk][b][i][h * d + c] = sum of p_j * v_jc over j = 0 .. L-1 in ascending j from +0, a lane per column c
 * A NaN among the s_ij makes the row's sum and with it every p_j and o_ic a NaN, as torch's softmax does; so does a +Inf (Inf - Inf).
 * `scale` is the caller's float(d) ** -0.5 rounded to float.
 * replaces  the new path of Attention.forward (clip_surgery_model.py:82-99): q = k = v, (q @ k^T) * scale, softmax, attn @ v and the
 *           transpose(1, 2).reshape(B, N, C), for the six blocks at once
 *   v : element (blk, j, b, h * d + c) at blk * v_ld_n + j * v_ld_l + b * v_ld_b + h * d + c (the V third of each block's
 *       in-projection where it lies: v_ld_l = 3 D for one image's (L, 3 D) rows);  out : [n][B][L][D] float;
 *   scores : [n][B][H][L][L] float, the s_ij, or NULL: not written (the tests read them: they are the last values before the exp)
 *   NULL v or out -> XAI_E_NULL;  n < 1, B < 1, L < 2, D < 1, H < 1, H not dividing D, v_ld_l < D, v_ld_b < D with B > 1, v_ld_n < D
 *   with n > 1 -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_csurg_vv_attention_f32(const float* v, int64_t v_ld_n, int64_t v_ld_l, int64_t v_ld_b, int n, int B, int L, int D, int H,
                               float scale, float* scores, float* out, xai_stream_t stream);

/* K87 the min-max-normalised similarity map of the first T_out texts.  One workgroup of 1024 lanes (16 waves) per image:
 *   n_c = sqrt(sum of F[b][i][c] * F[b][i][c] over i = 0 .. L-1 in ascending i from +0), a lane per channel c   (the norm over the
 *     TOKENS);  f_ic = F[b][i][c] / n_c wherever it is read, 0 / 0 = NaN kept
 *   prob_t = DOT(E; f_0c, txt_tc), a wave per text;  x_t = 2 * prob_t;  m = MAX(T; x_t);  e_t = expf(x_t - m);
 *   p_t = e_t / SUM(T; e_t);  mean = SUM(T; p_t) / float(T);  w_t = p_t / mean   (by wave 0)
 *   r_c = (sum of w_t * txt_tc over t = 0 .. T-1 in ascending t from +0) / float(T), a lane per channel
 *   s_it = DOT(E; f_ic, w_t * txt_tc - r_c) for i = 1 .. L-1 and t < T_out, a wave per (t, i)
 *   lo_t = min_i s_it, hi_t = max_i s_it, both a NaN if any s_it is one (torch's min and max);
 *   out[b][t][i - 1] = (s_it - lo_t) / (hi_t - lo_t), 0 / 0 = NaN kept   (where the least s_it are -0 and +0 together, which of the
 *     two lo_t is, and with it the sign of a zero result, is the device's fminf's choice)
 * replaces  the normalisation of clip_surgery_map (generate_emap.py:121), clip_feature_surgery (clip.py:287-308) and the min-max of
 *           get_similarity_map (clip.py:274) for the texts that are read
 *   F : [B][L][E], the features before the normalisation;  txt : text t of image b at b * txt_ld_b + t * E, txt_ld_b = 0 for texts
 *   shared by the images;  out : [B][T_out][L - 1] float;  w : [B][T] float, the w_t, or NULL: not written (the last values that
 *   depend on expf: the tests feed them back into the restatement)
 *   NULL F, txt or out -> XAI_E_NULL;  B < 1, L < 2, E < 1, T < 1, T_out outside 1 .. T, txt_ld_b < 0, 0 < txt_ld_b < T * E
 *   -> XAI_E_SHAPE;  over THE LIMITS -> XAI_E_UNSUPPORTED */
int xai_csurg_similarity_map_f32(const float* F, const float* txt, int64_t txt_ld_b, int B, int L, int E, int T, int T_out,
                                 float* w, float* out, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_CSURG_H */
