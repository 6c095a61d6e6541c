/*
 * xai_hip.h -- C ABI of libxai_hip.so, the MI355X (gfx950) kernels behind the
 * saliency-attribution hot path of chasewalker26/Image-Classification-XAI.
 *
 * The reference is pure Python and has NO FFI for this path: its "interface" is a set of
 * torch / NumPy expressions inside util/attribution_methods and util/test_methods.  Each
 * entry point below names the reference expression (file:line, relative to the reference
 * root) it replaces; INTEGRATION.md shows the ctypes stub a maintainer would add at that
 * line.  The Python modules under image-classification-xai_amd/util/ keep the reference's
 * call signatures and are the only intended callers.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer owned by the caller (tensor.data_ptr() of a
 *     contiguous tensor); the library never allocates, frees or retains memory;
 *   - `stream` is the caller's hipStream_t (torch.cuda.current_stream().cuda_stream);
 *     launches are asynchronous on it and graph-capturable (no sync, no malloc inside);
 *   - float data is IEEE fp32, index data int32, layouts are dense row-major
 *     (NCHW for images, [image][step][C][H*W] for step batches);
 *   - return value: 0 = success; <0 = argument error (XAI_E_*); >0 = hipError_t of the launch;
 *   - no global mutable state beyond a per-device compute-unit count published once through a std::atomic;
 *     re-entrant from several host threads on different streams.
 */
#ifndef XAI_HIP_H
#define XAI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t */

/* xai_version() = XAI_ABI_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_version_minor() = XAI_ABI_MINOR: bumped whenever entry points are added or an accepted argument range grows, so a
 * host can tell an older libxai_hip.so from this one without probing symbols:
 *   1 = the round-1 set;  2 = + xai_ig_accum_timed_f32, xai_maxpool_bwd_f32 accepts more than 65 535 planes;
 *   3 = + xai_version_minor, xai_masked_sums_f32;
 *   4 = + xai_attn_head_importance_f32 (+ _workspace_bytes), xai_rave_matrices_f32, xai_rollout_row_f32,
 *         xai_residual_shares_f32, xai_attn_cam_f32;
 *   5 = + xai_gig_init_f32, xai_gig_step_f32;
 *   6 = + xai_agi_init_f32, xai_agi_step_f32, xai_agi_heatmap_f32;
 *   7 = + xai_ablate_features_f32, xai_ablate_windows_f32, xai_ablation_finish_features_f32, xai_ablation_finish_windows_f32;
 *   8 = + xai_bn_gate_mask_bytes, xai_bn_relu_fwd_mask_f32, xai_bn_relu_bwd_mask_f32, xai_bn_relu_maxpool_fwd_code_f32,
 *         xai_bn_relu_maxpool_bwd_f32;
 *   9 = + xai_bn_relu_bwd_mask_guided_f32, xai_bn_relu_maxpool_bwd_guided_f32, xai_guided_map_f32;
 *  10 = + xai_xrai_workspace_bytes, xai_xrai_pack_u64, xai_xrai_rank_f32;
 *  11 = + xai_lime_max_features, xai_lime_compose_f32, xai_lime_fit_f64, xai_lime_paint_f32 */
#define XAI_ABI_VERSION 1
#define XAI_ABI_MINOR 11
#define XAI_OK 0
#define XAI_E_NULL (-1)        /* required pointer is NULL                      */
#define XAI_E_SHAPE (-2)       /* non-positive / inconsistent extent, or misaligned */
#define XAI_E_UNSUPPORTED (-3) /* extent beyond what the kernel was built for   */

int xai_version(void);
int xai_version_minor(void);
/* static string for a code returned by any entry point (never NULL) */
const char* xai_strerror(int code);

/* ---- Integrated Gradients -------------------------------------------------------- */

/* K1  out[i][s][e] = b[i][e] + alpha[i][s] * (x[i][e] - b[i][e])   (mul, then add: no FMA)
 * replaces  saliencyMethods.py:38,44  (also :113, :169, :245)
 *   x, baseline : [n_img][n_elem]; baseline may be NULL -> every element = baseline_scalar
 *   alphas      : n_alpha values per image, image i at alphas + i*alpha_img_stride
 *                 (alpha_img_stride = 0 shares one schedule)
 *   out         : [n_img][n_alpha][n_elem] */
int xai_ig_interp_f32(const float* x, const float* baseline, float baseline_scalar,
                      const float* alphas, int64_t alpha_img_stride, int n_img, int n_alpha,
                      int64_t n_elem, float* out, xai_stream_t stream);

/* Left-IG cutoff: n_use[i] = first s with logit[i][s] > alpha_star * max_s logit[i][s];
 * none -> 1; 0 -> 1.   replaces  saliencyMethods.py:48-65   (alpha_star == 1 -> n_steps) */
int xai_ig_cutoff_f32(const float* logits, int n_img, int n_steps, float alpha_star,
                      int32_t* n_use, xai_stream_t stream);

/* K2  out[i][c][p] = ( sum_{s<n_use_i} w1[i][s]*w2[i][s]*g[i][s][c][p] ) / denom_i * (x - b)
 *     out_abs[i][p] = | sum_c out[i][c][p] |                     (optional, fused a5)
 * replaces  saliencyMethods.py:53,67,70 (IG / Left-IG), :125-135 (IDG, with w1 = slopes,
 *           w2 = alpha sub-step, denom = n_steps) and evaluatePerturbation.py:181 (abs-sum)
 *   grads      : [n_img][n_steps][C][hw]
 *   n_use_dev  : per-image count on the device (NULL -> n_use_host for every image);
 *                denom_i = n_use_i (mean over the prefix)
 *   step_w1/2  : [n_img][n_steps] optional per-step weights (NULL -> 1)
 *   out_chw    : [n_img][C][hw];  out_abs_hw : [n_img][hw] or NULL */
int xai_ig_accum_f32(const float* grads, int n_img, int n_steps, const int32_t* n_use_dev,
                     int n_use_host, const float* step_w1, const float* step_w2,
                     const float* x, const float* baseline, float baseline_scalar, int C,
                     int64_t hw, float* out_chw, float* out_abs_hw, xai_stream_t stream);

/* K2, the same launch (saliencyMethods.py:53,67,70), with the kernel's OWN start / stop timestamps recorded into two
 * caller-owned hipEvent_t (created with timing enabled) by the dispatch itself (hipExtLaunchKernel): hipEventElapsedTime of
 * the pair is the kernel's duration, without the dispatch latency that two events bracketing a launch include.  Used by
 * bench.py for roofline.achieved.  start_event / stop_event : hipEvent_t, both required */
int xai_ig_accum_timed_f32(const float* grads, int n_img, int n_steps, const int32_t* n_use_dev,
                           int n_use_host, const float* step_w1, const float* step_w2,
                           const float* x, const float* baseline, float baseline_scalar, int C,
                           int64_t hw, float* out_chw, float* out_abs_hw, void* start_event,
                           void* stop_event, xai_stream_t stream);

/* dst[e] = src[e] with non-temporal stores: files one classifier pass's step gradients into
 * the [n_img][n_steps][C][hw] buffer without leaving dirty lines in the Infinity Cache
 * replaces  `gradients[start:end] = ...` at saliencyMethods.py:46 */
int xai_ig_store_grads_f32(const float* src, float* dst, int64_t n_elem, xai_stream_t stream);

/* K2, streaming form: acc[e] += sum_{b<n_batch} grads[b][e]   (no [steps][N] buffer kept)
 * replaces  saliencyMethods.py:46 + :53 when alpha_star == 1 */
int xai_ig_accum_add_f32(const float* grads, int n_batch, float* acc, int64_t n_elem,
                         xai_stream_t stream);

/* finish of the streaming form: out = acc / n_steps * (x - b); optional abs-sum as above */
int xai_ig_finish_f32(const float* acc, int n_img, int n_steps, const float* x,
                      const float* baseline, float baseline_scalar, int C, int64_t hw,
                      float* out_chw, float* out_abs_hw, xai_stream_t stream);

/* IDGI  sumsq[s] = sum_e g[s][e]^2 ;  out[e] = sum_{s<n_steps-1} g[s][e]^2 * d[s] / sumsq[s]
 * replaces  saliencyMethods.py:172-179    (d[s] = logit[s+1]-logit[s], computed in-kernel) */
int xai_sumsq_f32(const float* grads, int n_rows, int64_t n_elem, float* sumsq,
                  xai_stream_t stream);
int xai_idgi_accum_f32(const float* grads, int n_steps, const float* logits,
                       const float* sumsq, int64_t n_elem, float* out, xai_stream_t stream);

/* ---- Grad-CAM --------------------------------------------------------------------- */

/* K3a  w[c] = mean_hw grad[b][c]; cam[b][p] = (relu) sum_c w[c]*act[b][c][p]
 * replaces  captum 0.7.0 LayerGradCam.attribute as called at evaluatePerturbation.py:149-151
 *   act, grad : [B][C][h*w];  cam : [B][h*w];  h*w <= 1024
 *   ws : optional device scratch of xai_gradcam_workspace_bytes(B,C,h,w) bytes; with it the channels
 *        of one image are reduced by several workgroups (partials summed in a fixed order);
 *        NULL -> one workgroup per image */
size_t xai_gradcam_workspace_bytes(int B, int C, int h, int w);
int xai_gradcam_f32(const float* act, const float* grad, int B, int C, int h, int w, int relu,
                    float* cam, void* ws, size_t ws_bytes, xai_stream_t stream);

/* K3b  bilinear up-sample, align_corners = False; dst = scale * up(src), |.| if take_abs
 * replaces  torchvision Resize((H,W), antialias=True) at evaluatePerturbation.py:153 and
 *           (scale = 3, take_abs = 1) the x ones(3,H,W) + abs-sum of :153,:181 */
int xai_bilinear_up_f32(const float* src, int B, int h, int w, int H, int W, float scale,
                        int take_abs, float* dst, xai_stream_t stream);

/* ---- RISE ------------------------------------------------------------------------- */

/* K4  mask_n = crop(upsample(grid_n, (s+1)*cell), shift_n, HxW);  masked_n = image * mask_n
 * replaces  generate_emap.py:72-80 (skimage resize order=1 'reflect' + shift crop) and :91
 *   grid : [n][s][s] uint8 {0,1};  shift : [n][2] int32 (row shift, col shift)
 *   image : [C][H][W];  masked_out : [n][C][H][W] or NULL;  masks_out : [n][H][W] or NULL
 *   Limits: s <= 64, n_masks <= 65535, H*W < 2^31 (XAI_E_UNSUPPORTED above); the crop must lie inside the up-sampled grid,
 *   H + cell_h - 1 <= (s+1)*cell_h and the same along W (XAI_E_SHAPE otherwise; cell = ceil(H/s) always fits). */
int xai_rise_apply_f32(const uint8_t* grid, const int32_t* shift, int n_masks, int s,
                       int cell_h, int cell_w, const float* image, int C, int H, int W,
                       float* masked_out, float* masks_out, xai_stream_t stream);

/* K5  acc[p] += scale * sum_n scores[n] * mask_n[p]     (masks regenerated from the grid;
 *     fp64 accumulator that may be carried over several calls; the caller rounds to fp32)
 * replaces  generate_emap.py:99-100  (scale = 1/N/p1)
 *   Limits: every s <= 64 that K4 accepts runs (XAI_E_UNSUPPORTED above).  The tap tables of the up-sampled grid,
 *   12 * (s+1) * (cell_h + cell_w) bytes, share 64 KiB of LDS with the staged masks: 256 masks of 16 bytes for s == 8 with an
 *   8-byte aligned grid, else as many masks of 20 + s*s bytes as fit, 256 at most (256 up to s = 14 at 224 x 224, 243 at
 *   s = 15, 14 at s = 64).  XAI_E_UNSUPPORTED only where not even one mask fits next to the tap tables (s = 64 needs
 *   cell_h + cell_w <= 78, images up to about 2500 x 2500); the same crop rule as K4 (XAI_E_SHAPE). */
int xai_rise_accum_f64(const uint8_t* grid, const int32_t* shift, const float* scores,
                       int n_masks, int s, int cell_h, int cell_w, int H, int W, double scale,
                       double* acc, xai_stream_t stream);

/* ---- insertion / deletion loop ------------------------------------------------------ */

/* K8  stable ascending argsort of each row (NumPy kind='stable': -0 == +0, NaN last) and its
 *     inverse permutation.   replaces  MASTestFunctions.py:209,212 (np.argsort / np.flip)
 *   sal : [n_seg][hw];  order, rank : [n_seg][hw] int32;  descending order = reverse of
 *   `order`.  ws : device scratch of at least xai_rank_workspace_bytes(n_seg, hw) bytes */
size_t xai_rank_workspace_bytes(int n_seg, int64_t hw);
int xai_rank_f32(const float* sal, int n_seg, int64_t hw, int32_t* order, int32_t* rank, void* ws,
                 size_t ws_bytes, xai_stream_t stream);

/* flip_step[p] = (descending ? hw-1-rank[p] : rank[p]) / step_size : the 0-based step at
 * which pixel p switches from `start` to `finish`   (MASTestFunctions.py:251) */
int xai_flip_steps_i32(const int32_t* rank, int64_t hw, int descending, int step_size,
                       int32_t* flip_step, xai_stream_t stream);

/* K6  out[k][c][p] = flip_step[p] <= first_step + k ? finish[c][p] : start[c][p]
 * replaces  MASTestFunctions.py:249-257 (and the same loop in RISE:181, AIC:179, PNP:141,
 *           MONO:173): the NumPy fancy-index copy + images[i] = start
 *   start, finish : [C][hw];  out : [n_batch][C][hw] */
int xai_perturb_batch_f32(const float* start, const float* finish, const int32_t* flip_step,
                          int C, int64_t hw, int first_step, int n_batch, float* out,
                          xai_stream_t stream);

/* K10 seg[t] = float32 sum of sal over the pixels of step t, i.e. positions
 *     [t*step_size, (t+1)*step_size) of the ascending `order` (read back to front when
 *     descending); total = float32 sum of the whole map; n_steps = ceil(hw/step_size)
 * replaces  MASTestFunctions.py:227,259   (density numerators) */
int xai_segment_sums_f32(const float* sal, const int32_t* order, int64_t hw, int descending,
                         int step_size, int n_steps, float* seg, float* total,
                         xai_stream_t stream);

/* K7  separable zero-padded blur: out = k1d (x) k1d applied per channel
 * replaces  conv2d(x, gkern(klen, nsig), padding=klen//2) at evaluatePerturbation.py:459
 *   x, out : [B][C][H][W];  k1d : [klen] on the device, klen odd <= 63
 *   Not in place: x == out is refused with XAI_E_SHAPE (a tile's halo belongs to its neighbours' outputs). */
int xai_blur_sep_f32(const float* x, const float* k1d, int klen, int B, int C, int H, int W,
                     float* out, xai_stream_t stream);

/* one zero-padded 1-D pass of the same blur along W (axis = 1) or H (axis = 0), any odd klen; two calls
 * (through a caller buffer, x != out) give the separable blur for the long kernels of the growing-kernel
 * search in the MDA branch, evaluatePerturbation.py:244-257 (klen += 4 up to 101) */
int xai_blur_1d_f32(const float* x, const float* k1d, int klen, int axis, int B, int C, int H,
                    int W, float* out, xai_stream_t stream);

/* K9  per row of logits: softmax[target], -sum p log2 p, argmax
 * replaces  MASTestFunctions.py:273-276, AICTestFunctions.py:191-192
 *   target_dev : device int32 (NULL -> target_host; target_host < 0 -> each row's argmax)
 *   any of p_target / entropy_bits / argmax may be NULL */
int xai_softmax_stats_f32(const float* logits, int B, int K, const int32_t* target_dev,
                          int target_host, float* p_target, float* entropy_bits,
                          int32_t* argmax, xai_stream_t stream);

/* ---- feature-map maskers of the RISE family (ViT-CX) ---------------------------------- */

/* K11 masks[r] = minmax_row( bilinear_up(src[r], (H,W), align_corners = False) ), one launch, the up-sampled
 *     maps never exist un-normalised in memory
 * replaces  ViT_CX/ViT_CX.py:82-84 (transforms.Resize(input_size, antialias=True), then norm_matrix :29-34)
 *   src : [R][h*w], h*w <= 4096, h*W <= 8192, H <= 1024;  out : [R][H*W];  a constant row gives 0/0 = NaN as in the reference
 *   H >= h and W >= w: the reference's antialias = True is the plain bilinear formula only when up-sampling (14x14 -> 7x7
 *   differs by 0.74 of the row span), so a target smaller than the source in either axis is XAI_E_UNSUPPORTED */
int xai_up_rownorm_f32(const float* src, int R, int h, int w, int H, int W, float* out,
                       xai_stream_t stream);

/* K12 out[r] = (x[r] - min x[r]) / (max x[r] - min x[r])      (in place allowed)
 * replaces  norm_matrix, ViT_CX/ViT_CX.py:29-34, as applied to the cluster sums at :109 */
int xai_rownorm_f32(const float* x, int R, int64_t P, float* out, xai_stream_t stream);

/* K13 out[k] = sum of rows[members[m]] for m in [offs[k], offs[k+1]), added in that order starting from 0
 * replaces  the `mask_clustering[cluster_labels[i]] += mask[i]` loop, ViT_CX/ViT_CX.py:105-106
 *   rows : [R][P];  members : int32 row ids grouped by cluster (ascending inside a cluster);
 *   offs : [K+1] int32;  out : [K][P] */
int xai_cluster_sum_f32(const float* rows, const int32_t* members, const int32_t* offs, int K,
                        int64_t P, float* out, xai_stream_t stream);

/* K14 add = (noise[n][c][p] * noise_scale) * (1 - masks[n][p]);
 *     stack[n][c][p] = x[c][p] * masks[n][p] + add;   stack[N + n][c][p] = x[c][p] + add
 * replaces  ViT_CX/causal_score.py:27-47 (masks_inverse, random_whole * 0.1, the per-mask loop, torch.cat)
 *   x : [C][HW];  masks : [N][HW];  noise : [N][C][HW] standard normal draws;  stack : [2N][C][HW] */
int xai_causal_apply_f32(const float* x, const float* masks, const float* noise, int N, int C,
                         int64_t HW, float noise_scale, float* stack, xai_stream_t stream);

/* K16 out_weighted[p] = (sum_n weights[n] * rows[n][p]) / N;  out_plain[p] = (sum_n rows[n][p]) / N   -- ONE read of the
 *     stored mask stack (n ascending, fp32, each product rounded before it is added)
 * replaces  (scores * masks).sum / masks.sum of TIS.generate_saliency, util/attribution_methods/TIS.py:331-366, and the
 *           matmul(p_final, masks / masks.sum(0)) of ViT_CX/causal_score.py:54-61 restricted to the one class row consumed
 *   rows : [N][P];  weights : [N];  out_weighted, out_plain : [P] */
int xai_masked_sums_f32(const float* rows, const float* weights, int N, int64_t P, float* out_weighted,
                        float* out_plain, xai_stream_t stream);

/* ---- ViT explainers: Baselines.generate_RAVE ("InFlow") and Baselines.generate_cam_attn ----------------------------
 * after the classifier's backward passes (util/attribution_methods/VIT_LRP/ViT_explanation_generator.py).  Per-block
 * tensors are separate allocations, so the multi-block entries take a DEVICE array of device pointers, one per block (and
 * operand), and cover all L blocks in one call.  No floating-point atomics: results are bit-identical from run to run. */

/* K17 workspace of xai_attn_head_importance_f32: L*H*ceil(S/32)^2 floats (the per-tile partials of
 * ViT_explanation_generator.py:268-271) */
size_t xai_attn_head_importance_workspace_bytes(int L, int H, int S);

/* K17 Ih[l][h] = m[l][h] / sum_h m[l][h],  m[l][h] = mean_ij |(A_lh^T G_lh)[i][j]|   (f32-input MFMA, f32 accumulation;
 *     the S x S product is never written: abs and the tile sums happen in the epilogue, the tile sums are added in tile order)
 * replaces  ViT_explanation_generator.py:268-271 (torch.matmul(attn^T, grad).abs().mean(dim=(-1,-2)), Ih / sum(Ih))
 *   attn_tab[l], grad_tab[l] : [H][S][S] attention map / its gradient of block l (image 0);  Ih : [L][H]
 *   ws : >= xai_attn_head_importance_workspace_bytes(L, H, S) bytes of device scratch (required) */
int xai_attn_head_importance_f32(const float* const* attn_tab, const float* const* grad_tab, int L, int H, int S,
                                 float* Ih, void* ws, size_t ws_bytes, xai_stream_t stream);

/* K18 aug[l] = row-normalised InFlow matrix of block l:
 *     M[i][j] = max_h A_lh[i][j] * Ih[l][h];  with bgrad: M = max(mean_h Gb_lh[i][j] * M, 0)
 *     r[i][j] = M[i][j] * b1[l][1][j] + (i == j) * b1[l][0][j]
 *     ablate == 0: r[i][j] *= ratio[j] * b2[l][1][j] + b2[l][0][j],  ratio = q / max(sum_j |q_j|, 1e-12),  q = b2[l][1] / b2[l][0]
 *     aug[l][i][j] = r[i][j] / sum_j r[i][j]
 * replaces  ViT_explanation_generator.py:272 (max over heads), :278-281 (bottom-up gradient), compute_RAVE :63-86 (the
 *           r1 @ r2 product is a column scale: r2 is diagonal)
 *   attn_tab[l], bgrad_tab[l] : [H][S][S] (bgrad_tab NULL = withgrad False);  Ih : [L][H];  b1, b2 : [L][2][S];
 *   ablate : 0 or 1;  aug : [L][S][S]
 *   NaN: the max over heads, the clamp at 0 and the clamp at 1e-12 carry a NaN as torch.max / clamp / F.normalize do (a NaN
 *   gradient entry makes its row NaN, as in the reference) */
int xai_rave_matrices_f32(const float* const* attn_tab, const float* const* bgrad_tab, const float* Ih, const float* b1,
                          const float* b2, int L, int H, int S, int ablate, float* aug, xai_stream_t stream);

/* K19 out[n] = row target_token of aug[n][L-1] . aug[n][L-2] ... aug[n][0], as L-1 vector-matrix products (all entries >= 0)
 * replaces  compute_RAVE, ViT_explanation_generator.py:84-88, and rollout[:, target_token] of :299
 *   aug : [n_img][L][S][S];  out : [n_img][S]
 *   one workgroup per image with 17 * S * 4 bytes of dynamic LDS: S <= 2409 (160 KiB), beyond that XAI_E_UNSUPPORTED.  Above
 *   64 KiB the limit is declared on the kernel (hipFuncAttributeMaxDynamicSharedMemorySize) at the first such call of the
 *   process; that call must not arrive on a capturing stream (XAI_E_UNSUPPORTED), later ones may */
int xai_rollout_row_f32(const float* aug, int n_img, int L, int S, int target_token, float* out, xai_stream_t stream);

/* K20 residual-stream 2-norm shares of every block, p=1-normalised with a max(., 1e-12) denominator:
 *     b1[l] = (|x|, |attn|) / max(|x| + |attn|, 1e-12),  b2[l] = (|x + attn|, |mlp|) / max(|x + attn| + |mlp|, 1e-12) per token
 * replaces  ViT_explanation_generator.py:286-297 (torch.linalg.norm x4, stack, normalize per block)
 *   tab[4l + 0..3] : block l's input, attention output, input + attention, MLP output, each [S][D] (image 0);
 *   b1, b2 : [L][2][S] */
int xai_residual_shares_f32(const float* const* tab, int L, int S, int D, float* b1, float* b2, xai_stream_t stream);

/* K21 out[n][p] = (c[p] - min c) / (max c - min c),  c[p] = max(mean_h A[n][h][0][1+p] * G[n][h][0][1+p], 0), p < S-1;
 *     a constant c gives NaN everywhere, as the reference's 0/0; so does a NaN in any c[p] of the image (torch's clamp, min
 *     and max carry it)
 * replaces  ViT_explanation_generator.py:167-177 (Baselines.generate_cam_attn after its backward)
 *   attn, grad : [n_img][H][S][S] of one block;  out : [n_img][S-1] */
int xai_attn_cam_f32(const float* attn, const float* grad, int n_img, int H, int S, float* out, xai_stream_t stream);

/* ---- Guided IG (util/attribution_methods/GIGBuilder.py:194-292) --------------------------------------------- */

/* Per-image state words of the Guided IG entries: int32 state[n_img][4] =
 *   { next step index, status, selections (quantile calls) of the last step, step at which the status was set }.
 * status: 0 ok; 1 a selection key is NaN (a NaN gradient off x_max: torch.quantile returns NaN and the reference loops
 * forever); 2 XAI_GIG_MAX_SELECTIONS selections did not reach the step's L1 target; 3 gamma <= 0 or NaN (the reference's
 * assert, :287); 4 more step launches than `steps`.  An image with a nonzero status is not touched again. */
#define XAI_GIG_MAX_SELECTIONS 64

/* K22 init: x = x_baseline, attr = 0, l1_total[i] = sum |x_input - x_baseline| (fp32 terms, one fixed fp64 sum order,
 * rounded to fp32), state = 0.  Replaces the set-up of guided_ig_impl, GIGBuilder.py:209-213; a kernel, not a memset,
 * so that it can sit in front of a captured graph.
 *   x_input, x_baseline, x, attr : [n_img][n_elem];  l1_total : [n_img];  state : [n_img][4]
 * n_elem above 16 777 216 (2^24) returns XAI_E_UNSUPPORTED, as xai_gig_step_f32 does. */
int xai_gig_init_f32(const float* x_input, const float* x_baseline, int n_img, int64_t n_elem, float* x, float* attr,
                     float* l1_total, int32_t* state, xai_stream_t stream);

/* K22 step: one outer step of guided_ig_impl (GIGBuilder.py:228-292) for every image, the whole inner
 * `while gamma > 1` loop (:246-291) on the device: clamp to x_min, l1_current and the math.isclose exit, the selection
 * of the features whose |grad| is at most the torch.quantile(..., fraction, interpolation='lower') order statistic
 * (rank floor(fp32(fraction) * fp32(n_elem - 1)), exact, keys = +inf where x == x_max), l1_s, gamma, the update of x and
 * attr += (x - x_old) * grad.  Infinite gradients are treated as the reference treats them: +inf is never selected
 * (:264, :268), -inf ranks with the infinities and is selected when the threshold itself is infinite.  One workgroup per image; the step index is read from and advanced in state[i][0], so the
 * same launch serves every step (graph-capturable).  Images whose l1_total is 0 keep attr = 0 (:222-225).
 *   grad : [n_img][n_elem], the gradient at the current x;  fraction in [0, 1];  max_dist as the reference's python float
 *   x, attr : updated in place;  l1_total, state : as left by xai_gig_init_f32
 * n_elem above 16 777 216 (2^24) returns XAI_E_UNSUPPORTED: torch.quantile refuses such inputs, so the reference has no
 * result there, and only up to 2^24 is fp32(n_elem - 1) exact and the rank below n_elem. */
int xai_gig_step_f32(const float* x_input, const float* x_baseline, const float* grad, int n_img, int64_t n_elem, int steps,
                     float fraction, double max_dist, float* x, float* attr, const float* l1_total, int32_t* state,
                     xai_stream_t stream);

/* ---- Adversarial Gradient Integration (util/attribution_methods/AGI.py:39-115, evaluatePerturbation.py:119-139) -- */

/* A pair is one (image, false class) attack: pair p = image * n_cls + k attacks classes[k]; x_cur, c_delta, g_adv, g_lab are
 * [n_img * n_cls][n_elem], data is [n_img][n_elem].  Per-pair state words int32 state[n_img * n_cls][4] =
 *   { active, iterations done (fgsm updates applied), stop reason, updated by the last step launch }.
 * stop reason: 0 running; 1 the argmax reached the class (the reference's break, AGI.py:64-65); 2 skipped, the class is
 * init_pred (:97-98); 3 max_iter updates done.  An inactive pair is not touched again. */

/* K23 init: init_pred[i] = the first maximal logit of logits[i] (NaN counted as maximal, as torch.max on the CPU; AGI.py:87),
 * the state words of every pair (active when classes[k] != init_pred), x_cur = data, c_delta = 0 (the int 0 of pgd_step, :55).
 * A kernel, not a memset, so that it can sit in front of a captured graph.
 *   logits : [n_img][n_out] of the forward of data;  classes : [n_cls] in [0, n_out);  init_pred : int64 [n_img] */
int xai_agi_init_f32(const float* logits, const float* data, const int32_t* classes, int n_img, int n_cls, int n_out, int64_t n_elem,
                     int64_t* init_pred, float* x_cur, float* c_delta, int32_t* state, xai_stream_t stream);

/* K24 step: one iteration of pgd_step (AGI.py:57-79) for every pair.  An active pair whose argmax of `logits` (the forward of
 * x_cur just run) is its class stops without an update; every other active pair gets fgsm_step (:39-49), from the ORIGINAL
 * image: x_cur = clamp(data + epsilon * sign(g_adv), 0, 1), c_delta += -g_lab * (x_cur - data), fp32 in the reference's order
 * (sign(NaN) = sign(-0) = +0), and stops after its max_iter-th update.  Two launches (decide, update): every block of a pair
 * acts on the same decision.  Graph-capturable: the iteration count lives in the state words.
 *   logits : [n_img * n_cls][n_out];  g_adv, g_lab : d softmax[class] / d x_cur and d softmax[init_pred] / d x_cur */
int xai_agi_step_f32(const float* logits, const float* g_adv, const float* g_lab, const float* data, const int32_t* classes,
                     int n_img, int n_cls, int n_out, int64_t n_elem, float epsilon, int max_iter, float* x_cur, float* c_delta,
                     int32_t* state, xai_stream_t stream);

/* K25 heatmap (evaluatePerturbation.py:132-139 after AGI.py:93-101): per image, step_grad = the sum of its pairs' c_delta in
 * class order from +0; hm = the channel mean (((c0 + c1) + c2) / C in fp32); q, u = NumPy 2's 'linear' percentiles q_lo,
 * q_hi of hm (float32 arithmetic, exact order statistics); hm < q -> q, hm > u -> u, out = (hm - q) / (u - q).  A NaN in hm
 * makes every output NaN (NumPy's NaN percentiles).  One workgroup per image.
 *   c_delta : [n_img * n_cls][C][HW];  out : [n_img][HW];  step_grad : [n_img][C][HW] or NULL;  qu : [n_img][2] (q, u) or NULL
 *   q_lo, q_hi in [0, 100];  HW < 2^24 */
int xai_agi_heatmap_f32(const float* c_delta, int n_img, int n_cls, int C, int64_t HW, double q_lo, double q_hi, float* out,
                        float* step_grad, float* qu, xai_stream_t stream);

/* ---- Feature Ablation / Occlusion (captum 0.7.0 as called at evaluatePerturbation.py:171-176) ------------------------ */

/* The altered images of a call form one flat list: row r = image * n_total + j, j = feature id - id_min (feature mode) or the
 * window index (occlusion mode).  A classifier pass is a run [first, first + n) of that list; it may cross from one image into
 * the next.  Scores are the target logits of those rows, [n_img][n_total].  Occlusion windows span all channels; over (H, W)
 * there are count = ceil((dim - window) / stride) + 1 shifts per axis (n_total = count_h * count_w, computed by the entries),
 * window j starts at row (j % count_h) * stride_h, column (j / count_h) * stride_w -- captum's order, the row shift fastest --
 * and is clipped to the image.  Per axis 1 <= window <= dim and 1 <= stride, stride <= window unless window == dim, as captum requires. */

/* K26 out[r - first][c][p] = x[b][c][p] * (1 - m) + baseline[c][p] * m,  m = (ids[c][p] == id_min + j) as 0.f / 1.f
 *     (captum's float expression, no select: -0 + 0 = +0, inf * 0 = NaN as there)
 * replaces  FeatureAblation._construct_ablated_input behind evaluatePerturbation.py:171-173, all n rows in one launch instead of
 *           one altered image per classifier call
 *   x : [B][C][H][W];  ids : int32 [H][W] (ids_C = 1) or [C][H][W] (ids_C = C);  baseline : [C][H][W] or NULL -> baseline_scalar;
 *   out : [n][C][H][W];  0 <= first, first + n <= B * n_total;  an id outside [id_min, id_min + n_total) is never ablated */
int xai_ablate_features_f32(const float* x, const int32_t* ids, int ids_C, int id_min, int n_total, const float* baseline,
                            float baseline_scalar, int B, int C, int H, int W, int64_t first, int n, float* out,
                            xai_stream_t stream);

/* K26, occlusion mode: the same expression with m = (pixel inside window j)
 * replaces  Occlusion._construct_ablated_input / _occlusion_mask behind evaluatePerturbation.py:174-176 */
int xai_ablate_windows_f32(const float* x, int win_h, int win_w, int stride_h, int stride_w, const float* baseline,
                           float baseline_scalar, int B, int C, int H, int W, int64_t first, int n, float* out,
                           xai_stream_t stream);

/* K27 attr[b][c][p] = +0 + (s0[b] - scores[b][ids[c][p] - id_min])   (captum's attr += (s0 - s_j) * m over ascending j, from +0)
 *     samples[b][c][i][j] = attr[b][c][floor((i + 0.5) * H / g)][floor((j + 0.5) * W / g)]   (nearest-exact, fp32 index
 *     arithmetic as F.interpolate; computed from the scores, attr need not be written)
 * replaces  the accumulation of FeatureAblation.attribute behind evaluatePerturbation.py:171-173 and `downsize`, :95
 *   s0 : [B];  scores : [B][n_total];  attr : [B][C][H][W] or NULL;  samples : [B][C][g][g] or NULL (one of the two required)
 * Finite scores only: captum's d * m turns one NaN or infinite score into NaN at EVERY element of the image (NaN * 0); the
 * gather confines it to the elements of that feature. */
int xai_ablation_finish_features_f32(const float* s0, const float* scores, const int32_t* ids, int ids_C, int id_min, int n_total,
                                     int B, int C, int H, int W, int g, float* attr, float* samples, xai_stream_t stream);

/* K27, occlusion mode: attr[b][c][p] = (sum over the windows k covering p, ascending k, from +0, of s0[b] - scores[b][k]) / their
 *     count as fp32 (captum's attr / weights; at most ceil(window / stride)^2 windows cover an element); samples as above
 * replaces  the accumulation and the division of Occlusion.attribute behind evaluatePerturbation.py:174-176 and `downsize`, :95
 * Finite scores only, as above. */
int xai_ablation_finish_windows_f32(const float* s0, const float* scores, int win_h, int win_w, int stride_h, int stride_w, int B,
                                    int C, int H, int W, int g, float* attr, float* samples, xai_stream_t stream);

/* ---- opt-in classifier-side fusion (xai_engine/prepare.py: fuse_bn_relu) --------------- */

/* y = act( bn(x) [+ identity] ), eval-mode BatchNorm2d with running statistics; act = ReLU when relu != 0 (required with
 * an identity).  Not a replacement of a reference expression: the reference's classifiers are torchvision modules
 * (XAI_Survey/evaluations/evaluatePerturbation.py:627-640) whose BatchNorm2d / ReLU / residual add run as separate
 * PyTorch kernels; this fuses them.   x, identity, y : [N][C][HW];  weight, bias, mean, var : [C]
 *   variant : ordering of the arithmetically equivalent BN expression (see csrc/bnrelu_kernels.hip)
 *   weight2 .. eps2 (nullable as a set): the identity operand is a raw convolution output with its own eval-mode
 *   BatchNorm (the down-sample branch): y = relu( bn(x) + bn2(identity) ) */
int xai_bn_act_fwd_f32(const float* x, const float* identity, const float* weight, const float* bias,
                       const float* mean, const float* var, float eps, const float* weight2,
                       const float* bias2, const float* mean2, const float* var2, float eps2, int variant,
                       int relu, int N, int C, int HW, float* y, xai_stream_t stream);

/* backward of the ReLU form, reached through the autograd.grad of saliencyMethods.py:213 (getGradientsParallel):
 * g = gy [+ gy2];  g1 = y > 0 ? g : 0;  gx = g1 * weight * invstd;  g_identity (nullable) = g1
 *   gy2 (nullable): the second gradient of a block output that feeds both the next convolution and the next identity path
 *   weight2, var2, eps2 (nullable as a set): g_identity = g1 * weight2 * invstd2, the gradient of the identity operand
 *   before its own BatchNorm */
int xai_bn_relu_bwd_f32(const float* gy, const float* gy2, const float* y, const float* weight, const float* var,
                        float eps, const float* weight2, const float* var2, float eps2, int variant, int N,
                        int C, int HW, float* gx, float* g_identity, xai_stream_t stream);

/* MaxPool2d backward from the forward's arg-max indices (int64, h * W + w within a plane), windows added in (ph, pw)
 * ascending order like PyTorch's max_pool_backward_nchw -> bit-identical; the stem of the classifiers instantiated at
 * XAI_Survey/evaluations/evaluatePerturbation.py:627-640.   gy, indices : [planes][PH*PW];  gx : [planes][H*W];
 * any plane count (more than 65 535 planes are launched in slabs) */
int xai_maxpool_bwd_f32(const float* gy, const int64_t* indices, int planes, int H, int W, int PH, int PW,
                        int kernel, int stride, int pad, float* gx, xai_stream_t stream);

/* inference-only stem: y = max_pool2d( relu( bn(x) ), kernel, stride, pad ) in one pass (no autograd; the un-pooled
 * activation is never written); same classifiers, evaluatePerturbation.py:627-640, as run by the forward-only loops of
 * MASTestFunctions.py:273 and generate_emap.py:91-97.   x : [N][C][H*W];  y : [N][C][PH*PW] */
int xai_bn_relu_maxpool_fwd_f32(const float* x, const float* weight, const float* bias, const float* mean,
                                const float* var, float eps, int variant, int N, int C, int H, int W, int PH,
                                int PW, int kernel, int stride, int pad, float* y, xai_stream_t stream);

/* ---- the same fusion when a gradient will be taken: 1-bit ReLU gates, and the stem as one kernel per direction ---- */

/* bytes of the gate mask of an n-element activation: one bit per element, in 64-bit words, four per group of 256
 * consecutive elements (flat index e: bit (e % 256) / 4 of word (e / 256) * 4 + e % 4; a partial last group is a whole
 * group).  The layout is private to the two entry points below, which serve the autograd.grad of saliencyMethods.py:213. */
size_t xai_bn_gate_mask_bytes(int64_t n);

/* xai_bn_act_fwd_f32 with relu != 0 that also writes the gate `y > 0` (NaN -> 0) of every element into `mask`
 * (xai_bn_gate_mask_bytes(N*C*HW) bytes, 8-byte aligned; every word is written, nothing needs a zero-fill), for the
 * backward pass of saliencyMethods.py:213 through the classifiers of evaluatePerturbation.py:627-640.  Same y, bit for bit. */
int xai_bn_relu_fwd_mask_f32(const float* x, const float* identity, const float* weight, const float* bias,
                             const float* mean, const float* var, float eps, const float* weight2,
                             const float* bias2, const float* mean2, const float* var2, float eps2, int variant,
                             int N, int C, int HW, float* y, void* mask, xai_stream_t stream);

/* xai_bn_relu_bwd_f32 with the gate mask written by xai_bn_relu_fwd_mask_f32 in place of y (1/32 of its bytes): same gx and
 * g_identity, bit for bit; reached through the autograd.grad of saliencyMethods.py:213 (getGradientsParallel) */
int xai_bn_relu_bwd_mask_f32(const float* gy, const float* gy2, const void* mask, const float* weight,
                             const float* var, float eps, const float* weight2, const float* var2, float eps2,
                             int variant, int N, int C, int HW, float* gx, float* g_identity, xai_stream_t stream);

/* the stem with autograd, forward: y = max_pool2d( relu( bn(x) ), kernel, stride, pad ) as xai_bn_relu_maxpool_fwd_f32, plus
 * one byte per pooled output for the backward: the arg-max position a * kernel + b inside its window (PyTorch's rule: h
 * then w ascending, update on val > max || isnan(val)), or 255 when the pooled value is <= 0 (ReLU gate closed; a NaN
 * passes the ReLU and keeps its gate open, as in PyTorch).  Classifiers of evaluatePerturbation.py:627-640 under the
 * gradient passes of saliencyMethods.py:213.   x : [N][C][H*W];  y, code : [N][C][PH*PW]
 * Accepted: 2*pad <= kernel, kernel <= 15, ceil(kernel/stride) <= 2, N*C <= 65535, PH / PW the pooled extents of H / W,
 * a tile of 7*stride+kernel padded rows within 48 KiB of LDS; anything else XAI_E_SHAPE / XAI_E_UNSUPPORTED */
int xai_bn_relu_maxpool_fwd_code_f32(const float* x, const float* weight, const float* bias, const float* mean,
                                     const float* var, float eps, int variant, int N, int C, int H, int W, int PH,
                                     int PW, int kernel, int stride, int pad, float* y, uint8_t* code,
                                     xai_stream_t stream);

/* the stem with autograd, backward, one kernel for max_pool_backward + threshold_backward + the BatchNorm gradient:
 * gx[p] = ( (sum over the windows q whose code selects p, (ph, pw) ascending, from +0, of gy[q] [+ gy2[q]]) * weight ) * invstd;
 * a window with code 255 contributes nothing.  gy2 (nullable): the second gradient of the pooled tensor (it feeds the first
 * block's convolution AND its down-sample branch).  Reached through the autograd.grad of saliencyMethods.py:213.
 * Same geometry as the forward.   gy, gy2, code : [N][C][PH*PW];  gx : [N][C][H*W] */
int xai_bn_relu_maxpool_bwd_f32(const float* gy, const float* gy2, const uint8_t* code, const float* weight,
                                const float* var, float eps, int variant, int N, int C, int H, int W, int PH,
                                int PW, int kernel, int stride, int pad, float* gx, xai_stream_t stream);

/* ---- Guided Backprop / Guided Grad-CAM (xai_engine/guided.py) ---------------------------- */

/* xai_bn_relu_bwd_mask_f32 in guided mode: the backward of captum's GuidedBackprop(model).attribute(x, target) behind
 * evaluatePerturbation.py:154-158 at a fused BN(+add)+ReLU site.  g = gy [+ gy2] (one fp32 add), g = g <= 0 ? +0 : g (relu of the
 * COMPLETE gradient of the ReLU's output: at a residual join the sum of both branches; NaN kept as by F.relu), then the gate and
 * the BatchNorm gradients exactly as the unguided entry.  Same arguments. */
int xai_bn_relu_bwd_mask_guided_f32(const float* gy, const float* gy2, const void* mask, const float* weight,
                                    const float* var, float eps, const float* weight2, const float* var2, float eps2,
                                    int variant, int N, int C, int HW, float* gx, float* g_identity, xai_stream_t stream);

/* xai_bn_relu_maxpool_bwd_f32 in guided mode (the stem's ReLU under evaluatePerturbation.py:154-158): the sum over the windows
 * whose code selects p -- the max-pool's complete scattered gradient at p -- is clamped, g <= 0 ? +0 : g, AFTER the last window
 * was added and before (g * weight) * invstd; never per window.  Same arguments. */
int xai_bn_relu_maxpool_bwd_guided_f32(const float* gy, const float* gy2, const uint8_t* code, const float* weight,
                                       const float* var, float eps, int variant, int N, int C, int H, int W, int PH,
                                       int PW, int kernel, int stride, int pad, float* gx, xai_stream_t stream);

/* K28 attr[b][c][y][x] = grad[b][c][y][x] * cam[b][sy][sx]          (cam NULL: attr = grad)
 *     map[b][y][x]     = | ((a_0 + a_1) + a_2 + ...) |,  a_c = attr[b][c][y][x], channels left to right from the first
 *     sy = min((int)floorf(y * ((float)h / H)), h - 1), sx likewise: F.interpolate(mode="nearest"), the legacy rule
 * replaces  captum's GuidedGradCam product gbp * interpolate(cam) behind evaluatePerturbation.py:159-163 and the harness's
 *           np.abs(np.sum(., axis=0)), :181 (for gbp, :154-158, with cam NULL)
 *   grad : [B][C][H][W];  cam : [B][h][w] or NULL (h, w then ignored);  attr : [B][C][H][W] or NULL;  map : [B][H][W] or NULL
 *   (one of the two outputs required); product and sums round separately; 16-byte accesses when W % 4 == 0 and grad, attr, map
 *   are 16-byte aligned */
int xai_guided_map_f32(const float* grad, const float* cam, int B, int C, int H, int W, int h, int w, float* attr,
                       float* map, xai_stream_t stream);

/* ---- XRAI (xai_engine/xrai.py) ---------------------------------------------------------- */

/* Bit planes: mask m is n_words = ceil(H*W / 64) uint64 words; pixel p = y*W + x is bit p % 64 of word p / 64; the bits at
 * positions >= H*W are zero.
 *
 * K29 bits[m] = dilate(mask m, disk(radius)), span[m] = (first, last) non-empty word of it, (n_words, -1) when it is empty
 * replaces  XRAIBuilder.py:287-292 (_unpack_segs_to_masks) and the dilation of :256-258
 *   label mode (labels != NULL, masks == NULL): labels : [S][H][W] int32;  label_min, label_max : [S] (device).  Map s gives one
 *     mask per integer l in [label_min[s], label_max[s]], in that order, the maps one after the other; an absent label is an
 *     empty mask that keeps its index; a label outside the stated range of its map belongs to no mask.
 *     M must be the sum of label_max[s] - label_min[s] + 1.
 *   mask mode (masks != NULL, labels == NULL): masks : [M][H][W] uint8, non-zero = set
 *   out[y][x] = OR of in[y + dy][x + dx] over the offsets dx*dx + dy*dy <= radius*radius that stay inside the image (skimage's
 *     disk(radius) footprint, 81 offsets at radius 5; a neighbour outside the image counts as false, which for this footprint
 *     equals skimage's reflecting border); radius 0 only packs; radius <= 64, above it XAI_E_UNSUPPORTED
 *   bits : [M][n_words] (zeroed here);  span : [M][2] int32 */
int xai_xrai_pack_u64(const int32_t* labels, const int32_t* label_min, const int32_t* label_max, int S, const uint8_t* masks,
                      int64_t M, int H, int W, int radius, uint64_t* bits, int32_t* span, xai_stream_t stream);

/* bytes of workspace xai_xrai_rank_f32 needs (16-byte aligned; nothing has to be zeroed); 0 for a non-positive extent.  It holds
 * what the reference keeps in `remaining_masks` (XRAIBuilder.py:656): per mask a cached remainder count and gain, and the order of
 * the fast mode (:754-755) */
size_t xai_xrai_workspace_bytes(int n_img, int H, int W, int64_t M_total);

/* K30 the greedy region ranking of n_img images in one launch, one workgroup per image
 * replaces  XRAIBuilder.py:619-711 (XRAI._xrai; fast != 0: _xrai_fast, :714-789) with _gain_density / _get_diff_cnt, :266-284
 *   attr : [n_img][H*W];  bits, span : the planes of all images, image i owns the masks [mask_first[i], mask_first[i + 1])
 *   (mask_first : [n_img + 1] int32 on the device, ascending, last entry M_total; an image may own none)
 *   Every iteration takes the remaining masks in ascending index: cnt = popcount(mask & ~current); cnt < min_pixel_diff drops
 *   the mask for good; else gain = (float)(fp64 sum of attr over those pixels / cnt).  The FIRST mask with the strictly
 *   greatest gain is selected (a tie goes to the lowest index): out over its remainder = gain, pixel_iter = the selection's
 *   number, current |= mask.  The loop ends when no mask remains or count(current) / (H*W) > area_threshold (fp64).  The pixels
 *   never covered get (float)(fp64 sum of attr over them / their count) and keep pixel_iter -1.
 *   fast: full-mask gains once, stable order by descending gain, one pass with the same drop rule; area_threshold is ignored.
 *   out : [n_img][H*W] fp32;  pixel_iter : [n_img][H*W] int32;  sel_key, sel_gain : [M_total], image i's selections in order from
 *   mask_first[i] on, keys relative to the image's first mask;  state : [n_img][4] int32 = selections, uncomputed pixels,
 *   status, covered pixels.  status 1: masks remain but none has a gain above -inf (NaN or -inf attr) -- the reference dies
 *   there with KeyError (remaining_masks[None], :682); status 2 (fast): a full-mask gain is NaN, the reference's sort order is
 *   then undefined.  The sums are taken in one fixed order, there are no floating-point atomics: two runs give the same bits.
 *   Limits: H*W <= 262144 (512 x 512: `current` is held in 32 KiB of LDS), above it XAI_E_UNSUPPORTED; min_pixel_diff < 1
 *   (the reference then loops over empty masks and crashes) XAI_E_UNSUPPORTED; bits, span, sel_key, sel_gain may be NULL when
 *   M_total == 0. */
int xai_xrai_rank_f32(const float* attr, const uint64_t* bits, const int32_t* span, const int32_t* mask_first, int n_img,
                      int64_t M_total, int H, int W, int min_pixel_diff, double area_threshold, int fast, float* out,
                      int32_t* pixel_iter, int32_t* sel_key, float* sel_gain, int32_t* state, void* workspace,
                      size_t workspace_bytes, xai_stream_t stream);

/* ---- LIME for images (xai_engine/lime.py) ------------------------------------------------- */

/* A sample is a row of bits, one per superpixel: bit z % 64 of word z / 64 of the row is 1 where superpixel z keeps the image
 * and 0 where it is replaced; a row has words >= ceil(D / 64) uint64 words, the bits at positions >= D are ignored.  The
 * samples of all images form one flat list, row r = image * n_samples + sample.
 *
 * K31 out[k][c][p] = bit(rows[first + k], seg[b][p]) ? x[b][c][p] : (fudged ? fudged[b][c][p] : hide[c]),  b = (first + k) / n_samples
 * replaces  lime_image.py:255-262 (data_labels: one deepcopy and one full-image compare per switched-off superpixel, per sample)
 *           and the transpose / stack of limeAttr.py:8-13
 *   x : [B][C][H][W];  seg : [B][H][W] int32;  rows : [B * n_samples][words];  D : [B] int32 (device), the superpixels of every
 *   image;  hide : [C] or NULL;  fudged : [B][C][H][W] or NULL (one of the two required; fudged wins);  out : [n][C][H][W]
 *   The value is selected, never blended: NaN and Inf of a kept superpixel pass through, those of a replaced one vanish.  An id
 *   outside [0, D[b]) belongs to no superpixel a row can switch off and keeps the image.  16-byte accesses when C*H*W % 4 == 0
 *   and x, fudged, out are 16-byte aligned, else the scalar flavour.  words <= 2048, above it XAI_E_UNSUPPORTED. */
int xai_lime_compose_f32(const float* x, const int32_t* seg, const uint64_t* rows, const int32_t* D, int words, const float* hide,
                         const float* fudged, int B, int C, int H, int W, int n_samples, int64_t first, int n, float* out,
                         xai_stream_t stream);

/* the largest D[b] xai_lime_fit_f64 fits (lime_base.py:78-80 and :189-193 put no bound on it; the caller fits larger images itself) */
int xai_lime_max_features(void);

/* K32 distances, kernel weights and both weighted ridge fits of every label of every image in one launch, one workgroup per image
 * replaces  lime_image.py:202-206 (cosine distances to row 0), :120-121 (the exponential kernel) and lime_base.py:181-207
 *           (explain_instance_with_data with feature_selection 'highest_weights': Ridge(alpha_select) at :78-80, the order of
 *           :109-114, Ridge(alpha) at :189-193, score, local_pred and the sorted explanation of :205-206)
 *   rows as for K31, N = n_samples;  Y : [B][N][L] float32, the label columns of the classifier's probabilities
 *   k_n = popcount of the first D bits of row n;  dist = 1 - sqrt(k_n / D);  weight = sqrt(exp(-dist^2 / kernel_width^2))
 *   mean_j = sum_n w x_nj / sum_n w,  ybar likewise;  A = sum_n w (x_n - mean)(x_n - mean)^T;  rhs = sum_n w (x_n - mean)(y_n - ybar)
 *   c1 = (A + alpha_select I)^-1 rhs;  position of feature j among the used features = its rank by |c1_j * x_0j| descending,
 *   ties to the lower j;  coef = (A + alpha I)^-1 rhs;  intercept = ybar - mean . coef;  local_pred = intercept + x_0 . coef;
 *   score = 1 - sum w (y - pred)^2 / sum w (y - ybar)^2 (NaN for N < 2; a zero denominator gives 1 when the numerator is 0,
 *   else 0, as sklearn's r2_score);  order = the features by |coef_j| descending, ties to the earlier position
 *   coef : [B][L][d_stride] fp64, indexed by feature, 0 at j >= D;  order : [B][L][d_stride] int32, -1 at j >= D;
 *   intercept, score, local_pred : [B][L] fp64;  dist, weight : [B][N] fp64
 *   All arithmetic is fp64 (Cholesky, packed lower triangles in LDS); every sum has one fixed order and there are no floating-point
 *   atomics: two runs give the same bits.  An image with D[b] outside [1, min(xai_lime_max_features(), d_stride, 64 * words)] is
 *   skipped: none of its outputs is written.  NaN in Y leaves `order` of that label unspecified. */
int xai_lime_fit_f64(const uint64_t* rows, int words, const int32_t* D, const float* Y, int B, int N, int L, int d_stride,
                     double kernel_width, double alpha_select, double alpha, double* coef, double* intercept, double* score,
                     double* local_pred, int32_t* order, double* dist, double* weight, xai_stream_t stream);

/* K33 out[b][p] = table[b][seg[b][p]], 0 for an id outside [0, d_stride)
 * replaces  lime_image.py:74-76 (get_image_and_mask: mask[segments == f] = 1 per chosen feature) with the harness's
 *           broadcast to three channels and |sum|, evaluatePerturbation.py:181, for a table that holds 3 on the chosen segments
 *   table : [B][d_stride] float32;  seg : [B][H][W] int32;  out : [B][H][W] float32 */
int xai_lime_paint_f32(const float* table, const int32_t* seg, int B, int d_stride, int H, int W, float* out, xai_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* XAI_HIP_H */
