/*
 * xai_hip_ext4.h -- C ABI of libxai_ext4.so, the fourth extension library beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11, include/xai_hip_ext.h at 1.0, include/xai_hip_ext2.h at 1.1 and include/xai_hip_ext3.h is
 * pinned at 1.0 by its tests; entry points added after that live here, in a library of their own with a version pair of its own.
 * The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 / _u64, return int
 * and take the caller's stream last), so xai_engine/_lib.py binds all five headers with the same strict reader, and so are the
 * conventions: device pointers owned by the caller, asynchronous graph-capturable launches, nothing allocated or retained, no global
 * state, no atomics (the same bytes on every run).  Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the
 * launch; xai_strerror (libxai_hip.so) has the text.  Every argument check comes before the first HIP call, so a refused call needs
 * no device.
 *
 * These are the element-wise steps of the relevance pass of Transformer Attribution (xai_engine/lrp.py; the reference's
 * LRP.generate_LRP with alpha = 1, util/attribution_methods/VIT_LRP/util/layers_ours.py and ViT_LRP_timm.py); its GEMMs stay with
 * rocBLAS.  Everything is fp32 and every product, sum and quotient is rounded once, in the order written (the library is compiled
 * with -ffp-contract=off).  Every entry takes a leading image count B; an image is what the reference's one-image call sees.
 *
 * Two expressions recur:
 *   cmin(x, c) = clamp(x, min=c) = x if x is NaN, else fmaxf(x, c);   cmax(x, c) = clamp(x, max=c) = x if x is NaN, else fminf(x, c)
 *   sd(a, b)   = safe_divide(a, b) of layers_ours.py:10-13, in its order:
 *                  den = cmin(b, 1e-9f) + cmax(b, 1e-9f);  den = den + (den == 0 ? 1.f : 0.f) * 1e-9f;  a / den * (b != 0 ? 1.f : 0.f)
 * 16-byte accesses where the element count is a multiple of 4 and every pointer is 16-byte aligned, scalar ones otherwise; the
 * values do not depend on the width.
 */
#ifndef XAI_HIP_EXT4_H
#define XAI_HIP_EXT4_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext4_version() = XAI_EXT4_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext4_version_minor() = XAI_EXT4_MINOR: bumped whenever entry points are added:
 *   0 = xai_lrp_split_f32, xai_lrp_ratio_f32, xai_lrp_gather_f32, xai_lrp_half_product_f32, xai_lrp_add_chunk, xai_lrp_add_workspace_bytes,
 *       xai_lrp_add_parts_f32, xai_lrp_add_scale_f32, xai_lrp_clone_f32, xai_lrp_attn_matrices_f32 */
#define XAI_EXT4_VERSION 1
#define XAI_EXT4_MINOR 0

int xai_ext4_version(void);
int xai_ext4_version_minor(void);

/* K46 pos = cmin(x, 0), neg = cmax(x, 0)
 * replaces  layers_ours.py:216-219 (torch.clamp(X, min=0), torch.clamp(X, max=0); for a weight, once per model)
 *   x, pos, neg : [B][n]
 *   NULL -> XAI_E_NULL;  B <= 0 or n <= 0 -> XAI_E_SHAPE */
int xai_lrp_split_f32(const float* x, int B, int64_t n, float* pos, float* neg, xai_stream_t stream);

/* K47 s = sd(r, z1 + z2), or sd(r, z1) when z2 is NULL
 * replaces  layers_ours.py:224 (safe_divide(R, Z1 + Z2)) and :51 (RelPropSimple)
 *   r, z1, z2, s : [B][n] (s may be r, z1 or z2) */
int xai_lrp_ratio_f32(const float* r, const float* z1, const float* z2, int B, int64_t n, float* s, xai_stream_t stream);

/* K48 out = cmin(x, 0) * g1 + cmax(x, 0) * g2: two products and one sum
 * replaces  layers_ours.py:226-229 (C1 = x1 * grad, C2 = x2 * grad, C1 + C2)
 *   x, g1, g2, out : [B][n] (out may be g1 or g2) */
int xai_lrp_gather_f32(const float* x, const float* g1, const float* g2, int B, int64_t n, float* out, xai_stream_t stream);

/* K49 out = x * c / 2: one product, then one true division
 * replaces  layers_ours.py:56-57 (X[i] * C[i]) with ViT_LRP_timm.py:362-363, :373-374 (cam /= 2) and the rearrange of :376
 *   x, c : [B][h][N][d].  slots == 1: out is [B][h][N][d] too (the plain mode; d = 1 serves any flat array).
 *   slots == 3: out is cam_qkv [B][N][3][h][d] and element (b, hh, t, e) goes to out[b][t][slot][hh][e]; nothing else is written.
 *   slots not 1 or 3, slot outside [0, slots) -> XAI_E_SHAPE */
int xai_lrp_half_product_f32(const float* x, const float* c, int B, int h, int N, int d, int slots, int slot, float* out,
                             xai_stream_t stream);

/* K50 Add.relprop (layers_ours.py:106-125) in two launches.
 * xai_lrp_add_chunk(): the elements of an image one workgroup sums (4096).  An image of n elements has P = ceil(n / chunk) chunks,
 * whatever the device.  xai_lrp_add_workspace_bytes(B, n) = B * P * 3 doubles (0 for a refused shape).
 *
 * pass 1 (xai_lrp_add_parts_f32):  s = sd(r, x0 + x1);  a = x0 * s;  b = x1 * s;  and per image and chunk p the fp64 sums
 *       part[img][p] = {sum a, sum b, sum r} over the chunk's elements, each fp32 value converted to fp64, in this fixed tree:
 *           lane t of 256 owns the chunk's elements i (counted from the chunk's start) with (i / 4) % 256 == t and adds them in
 *           ascending i, starting from +0.0;  the 64 lanes of a wave are combined by an xor butterfly with offsets 32, 16, 8, 4, 2, 1
 *           (a + b at both partners);  the 4 wave sums are added in ascending wave order, starting from +0.0.
 * pass 2 (xai_lrp_add_scale_f32):  per image  A, Bs, R = the chunks' parts added in ascending p, starting from +0.0, in fp64, each
 *       total rounded once to fp32;  then in fp32
 *           a_fact = sd(|A|, |A| + |Bs|) * R;  b_fact = sd(|Bs|, |A| + |Bs|) * R;  a = a * sd(a_fact, A);  b = b * sd(b_fact, Bs)
 * The reference's a.sum(), b.sum() and R.sum() are fp32 sums in torch's own order; these are the same sums, more exactly.
 *   x0, x1, r, a, b : [B][n];  ws : >= xai_lrp_add_workspace_bytes(B, n) bytes, 8-byte aligned, written by pass 1, read by pass 2
 *   n > 2^31 - 4096 or B > 65535 -> XAI_E_UNSUPPORTED;  ws_bytes too small -> XAI_E_SHAPE */
int xai_lrp_add_chunk(void);
size_t xai_lrp_add_workspace_bytes(int B, int64_t n);
int xai_lrp_add_parts_f32(const float* x0, const float* x1, const float* r, int B, int64_t n, float* a, float* b, void* ws,
                          size_t ws_bytes, xai_stream_t stream);
int xai_lrp_add_scale_f32(float* a, float* b, int B, int64_t n, const void* ws, size_t ws_bytes, xai_stream_t stream);

/* K51 out = x * (sd(r1, x) + sd(r2, x))
 * replaces  layers_ours.py:166-175 (Clone.relprop with num = 2)
 *   x, r1, r2, out : [B][n] (out may be r1 or r2) */
int xai_lrp_clone_f32(const float* x, const float* r1, const float* r2, int B, int64_t n, float* out, xai_stream_t stream);

/* K52 the attention matrices of all L blocks in one launch.  For block l, image b, row i, column j:
 *       m = (sum over heads hh = 0 .. h-1, ascending, starting from +0.f, of cmin(t, 0)) / h  (one true division),
 *           t = grad[l][b][hh][i][j] * cam[l][b][hh][i][j], or cam[l][b][hh][i][j] when grad is NULL
 *   mode 0: out[b][l][i][j] = m
 *   mode 1: m = m + (i == j ? 1.f : 0.f);  out[b][l][i][j] = m / rowsum, rowsum = the sum of the row's m over j in this fixed tree:
 *           lane t of 64 adds its columns j = t, t + 64, ... in ascending j, starting from +0.f; the lanes are combined by an xor
 *           butterfly with offsets 32, 16, 8, 4, 2, 1
 *   mode 2: out[b][l][j] = m of row i = 0 only (the CLS row)
 * replaces  ViT_LRP_timm.py:655-656, :666-678 (grad * cam, clamp(min=0), mean over heads), compute_rollout_attention :187-190 and
 *           :727-734 / :738-745 (last_layer, second_layer)
 *   cam, grad : [L][B][h][S][S];  out : [B][L][S][S] (the layout K19, xai_rollout_row_f32, reads), mode 2: [B][L][S]
 *   mode outside 0..2 -> XAI_E_SHAPE;  L or B > 65535 -> XAI_E_UNSUPPORTED */
int xai_lrp_attn_matrices_f32(const float* cam, const float* grad, int L, int B, int h, int S, int mode, float* out,
                              xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT4_H */
