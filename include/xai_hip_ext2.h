/*
 * xai_hip_ext2.h -- C ABI of libxai_ext2.so, the second extension library beside libxai_hip.so.
 *
 * include/xai_hip.h is frozen at ABI 1.11 and include/xai_hip_ext.h at 1.0 (GradientShap); entry
 * points added after that live here, in a library of their own with a version pair of its own.
 * Unlike the other two this header is open: a later feature adds its entries below and bumps
 * XAI_EXT2_MINOR.  The grammar is xai_hip.h's (one extern "C" block, the stream typedef, launch
 * entries end in _f32 / _f64 / _i32 / _u64, return int and take the caller's stream last), so
 * xai_engine/_lib.py binds all three headers with the same strict reader, and so are the
 * conventions: device pointers owned by the caller, asynchronous graph-capturable launches,
 * nothing allocated or retained, no global state.  Return values are xai_hip.h's: 0 = success,
 * <0 = XAI_E_*, >0 = hipError_t of the launch; xai_strerror (libxai_hip.so) has the text.
 */
#ifndef XAI_HIP_EXT2_H
#define XAI_HIP_EXT2_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext2_version() = XAI_EXT2_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext2_version_minor() = XAI_EXT2_MINOR: bumped whenever entry points are added:
 *   0 = xai_mda_max_segments, xai_mda_max_width, xai_mda_compose_f32, xai_mda_select_f32, xai_mda_commit_f32
 *   1 = xai_sanity_normalize_f32, xai_ssim_tile, xai_ssim_workspace_bytes, xai_ssim_f32, xai_tie_ranks_chunk, xai_tie_ranks_i32,
 *       xai_rank_corr_max_n, xai_rank_corr_f64, xai_hog_workspace_bytes, xai_hog_f32 */
#define XAI_EXT2_VERSION 1
#define XAI_EXT2_MINOR 1

int xai_ext2_version(void);
int xai_ext2_version_minor(void);

/* ---- MDA (xai_engine/mda.py): the greedy patch search of MDAFunctions.py ------------------- */

/* the largest number of segments S of one image K37 takes (>= 1024), and the largest sub-search width L (one wave) */
int xai_mda_max_segments(void);
int xai_mda_max_width(void);

/* K36 out[img][r][c][p] = (seg[img][p] == cand[img][r]) ? finish[img][c][p] : start[img][c][p]   for every r < L
 *     a select: the bits of either source pass through (NaN payloads, -0).  A row whose candidate is a label no pixel
 *     carries (K37 writes -1 at and above the step's n_cand) is a copy of start.
 * replaces  MDAFunctions.py:154-162 (and :224-233, :395-404, :463-472): start.clone() with the candidate segment's pixels taken
 *           from finish, one image per candidate
 *   start, finish : [n_img][C][HW];  seg : [n_img][HW] labels;  cand : [n_img][L];  out : [n_img][L][C][HW]
 *   16-byte accesses when HW % 4 == 0 and start, finish, seg, out are 16-byte aligned, scalar ones otherwise */
int xai_mda_compose_f32(const float* start, const float* finish, const int32_t* seg, const int32_t* cand, int n_img, int L,
                        int C, int64_t HW, float* out, xai_stream_t stream);

/* K37 one search step's decision per image, everything between the classifier pass and the next one.
 *     state[img] = {steps taken, done, last winner's segment (-1: none), plan rows};  plan[img][step] = {slot, n_cand, cutoff_slot}.
 *     An image with done != 0 or steps taken >= plan rows is left untouched.  Otherwise, with the plan row of `steps taken`:
 *       w = the first NaN of resp[img][0 .. n_cand), else its first maximum (mode 1) / first minimum (mode 0)   -- torch.argmax /
 *           torch.argmin on the CPU;   s = cand[img][w]
 *       mr[img][slot] = resp[img][w];  chosen[img][slot] = s;  taken[img][s] = 1;  last winner = s
 *       mode 1 and stop_test != 0:  if ((resp[img][w] - stop_ref[img][0]) / stop_ref[img][1] >= cutoff)  -- a difference and a true
 *           division, each rounded to fp32, as torch computes it on a 0-d float32 tensor and Python floats --
 *           mr[img][cutoff_slot] = cutoff and done = 1
 *       cand[img][0 .. n_next) = the first n_next entries of order[img] whose segment is not taken, n_next = the next plan row's
 *           n_cand (0 after a stop or past the last row);  cand[img][n_next .. L) = -1
 *       steps taken += 1
 *     A plan row or candidate outside its range (slot not in [0, S), n_cand not in [1, L], s not in [0, S)) sets done = 2 and
 *     writes nothing else.
 * replaces  MDAFunctions.py:129-139 and :177-192 (and :198-208, :247-262, :369-379, :418-422, :437-447, :487-491)
 *   resp : [n_img][L];  order : [n_img][S];  plan : [n_img][plan_stride][3];  stop_ref : [n_img][2] or NULL when not tested
 *   mr : [n_img][S];  chosen, taken : [n_img][S];  cand : [n_img][L];  state : [n_img][4]
 *   S > xai_mda_max_segments() or L > xai_mda_max_width() -> XAI_E_UNSUPPORTED */
int xai_mda_select_f32(const float* resp, const int32_t* order, const int32_t* plan, const float* stop_ref, int n_img, int S,
                       int L, int plan_stride, int mode, int stop_test, float cutoff, float* mr, int32_t* chosen,
                       int32_t* taken, int32_t* cand, int32_t* state, xai_stream_t stream);

/* K38 start[img][c][p] = finish[img][c][p] where seg[img][p] == state[img][2] (the last winner; < 0: nothing)
 * replaces  MDAFunctions.py:187-188 (and :257-258, :424-425, :493-494): the winner's pixels committed into start
 *   finish, start : [n_img][C][HW];  seg : [n_img][HW];  state : [n_img][4] */
int xai_mda_commit_f32(const float* finish, const int32_t* seg, const int32_t* state, int n_img, int C, int64_t HW,
                       float* start, xai_stream_t stream);

/* ---- sanity test (xai_engine/sanity.py): the map comparison of evaluateSanity.py get_sanity ---- */

/* K39 out[m] = normalize_image(x[m]) for every map m < n, in fp32 and in the reference's order:
 *       mn, mx = min, max of the map with NumPy's NaN rule (one NaN makes both NaN)
 *       guard != 0 and mx - mn == 0: the map is copied through unchanged
 *       every +Inf and -Inf becomes 0;  mn, mx again on the fixed map;  out = (x - mn) / (mx - mn), a true fp32 division
 *     so a map that is constant once its Inf are gone becomes all NaN (0 / 0).
 * replaces  evaluateSanity.py:68-79 normalize_image (guard = 1);  util/test_methods/sanityForMethods.py:60-72 (guard = 0)
 *   x, out : [n][hw] (out may be x);  16-byte accesses when hw % 4 == 0 and both are 16-byte aligned */
int xai_sanity_normalize_f32(const float* x, int n, int64_t hw, int guard, float* out, xai_stream_t stream);

/* the extent of K40's square output tile */
int xai_ssim_tile(void);
/* bytes of K40's scratch: one fp64 partial sum per tile and pair (0: an extent is not positive or the count leaves int) */
int xai_ssim_workspace_bytes(int n, int H, int W);

/* K40 mean[p] = structural_similarity(x[p], y[p], gaussian_weights=True) of skimage on one fp32 channel, for every pair p < n.
 *     The filter is scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5, mode='reflect') (radius 5) on x, y, x*x, y*y, x*y (each
 *     product one fp32 multiply): along axis 0, rounded to fp32, then along axis 1; every sample accumulates in fp64 in scipy's
 *     symmetric order, centre * w5 then (in[i+j] + in[i-j]) * w(j+5) for j = -5 .. -1; indices reflect as d c b a | a b c d | d c b a.
 *     w0 .. w5 are scipy's weights exp(-0.5 / sigma^2 * k^2) / sum for k = -5 .. 0, computed by the caller; the kernel calls no exp.
 *     Then in fp32, every operation rounded, with cov_norm = 121 / 120:
 *       vx = cov_norm * (uxx - ux * ux), vy and vxy likewise
 *       S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
 *     C1 = (0.01 R)^2 and C2 = (0.03 R)^2 of the data range R come from the caller.
 *     mean[p] is the fp64 mean of S over the interior (5 pixels cropped on every side): fp64 partial sums per tile in one fixed
 *     tree, the tiles added in ascending order.  S, when not NULL, receives the full uncropped map (skimage's full=True).
 * replaces  evaluateSanity.py:89 and :93 (sanityForMethods.py:82 and :86): ssim(..., gaussian_weights=True) per channel
 *   x, y : [n][H][W];  mean : [n] fp64;  S : [n][H][W] or NULL;  ws : xai_ssim_workspace_bytes(n, H, W) bytes, 8-byte aligned
 *   H < 11 or W < 11 -> XAI_E_SHAPE (skimage raises);  n > 65535 or more than 65535 tile rows -> XAI_E_UNSUPPORTED */
int xai_ssim_f32(const float* x, const float* y, int n, int H, int W, double w0, double w1, double w2, double w3, double w4,
                 double w5, float C1, float C2, double* mean, float* S, void* ws, size_t ws_bytes, xai_stream_t stream);

/* the number of sorted positions one workgroup of K41 handles */
int xai_tie_ranks_chunk(void);

/* K41 ranks2[r][i] = 2 * rankdata(vals[r], method='average')[i] = lo + hi + 2, an exact integer, where lo .. hi are the sorted
 *     positions of the elements equal (==, so -0 ties with +0) to vals[r][i].  `order` is the stable ascending argsort of each row,
 *     as K8 (xai_rank_f32) writes it.  A tie group may have any length up to the whole row.  A row with a NaN gets ranks that mean
 *     nothing (K42 answers NaN for it).
 * replaces  evaluateSanity.py:97-98 (sanityForMethods.py:79, :90): the rankdata inside scipy.stats.spearmanr
 *   vals : [n_rows][n];  order, ranks2 : [n_rows][n] int32;  n > 2^30 or n_rows > 65535 -> XAI_E_UNSUPPORTED */
int xai_tie_ranks_i32(const float* vals, const int32_t* order, int n_rows, int64_t n, int32_t* ranks2, xai_stream_t stream);

/* the largest row length K42 takes: 131072 */
int xai_rank_corr_max_n(void);

/* K42 out[p] = scipy.stats.spearmanr(a[p], b[p]).statistic from the doubled ranks ra[p], rb[p] of K41, bit for bit:
 *       d = r - (n + 1);  Saa, Sbb, Sab = the exact int64 sums of da * da, db * db, da * db
 *       inv = 1.0 / (n - 1);  c.. = (S.. / 4) * inv;  r = (cab / sqrt(cbb)) / sqrt(caa), clipped to [-1, 1]   -- numpy.corrcoef in fp64
 *     A constant row gives 0 / 0 = NaN.  a, b are the ranked values (either may be NULL: not tested): a NaN in a[p] or b[p] makes
 *     out[p] NaN, spearmanr's nan_policy='propagate'.
 * replaces  evaluateSanity.py:97-98 (sanityForMethods.py:79, :90): spr(...) on the pixels and on the HOG vectors
 *   ra, rb : [n_pairs][n] int32;  a, b : [n_pairs][n] or NULL;  out : [n_pairs] fp64
 *   n < 2 -> XAI_E_SHAPE;  n > xai_rank_corr_max_n() -> XAI_E_UNSUPPORTED */
int xai_rank_corr_f64(const int32_t* ra, const int32_t* rb, const float* a, const float* b, int n_pairs, int64_t n, double* out,
                      xai_stream_t stream);

/* bytes of K43's scratch: the fp64 cell histograms (0: an extent is not positive or the count leaves int) */
int xai_hog_workspace_bytes(int n, int H, int W, int ch, int cw);

/* K43 out[m] = skimage.feature.hog(img[m], orientations=9, pixels_per_cell=(ch, cw), cells_per_block=(3, 3), block_norm='L2-Hys')
 *     on one fp32 channel:
 *       g_row[1:-1, :] = img[2:, :] - img[:-2, :] in fp32, rows 0 and H-1 zero; g_col likewise along columns; both widened to fp64
 *       mag = hypot(g_col, g_row);  ori = rad2deg(atan2(g_row, g_col)) modulo 180 by Python's rule (fmod, then + 180 if negative);
 *           a value that rounds to exactly 180.0 falls in no bin
 *       cells tile the top-left (H / ch) ch x (W / cw) cw pixels (a gradient at the last used row or column still reads the pixel
 *           beyond it where there is one); bin i of a cell = the fp64 sum of mag over its pixels with 20 i <= ori < 20 (i + 1),
 *           divided by ch * cw
 *       every 3 x 3 block of cells at stride 1, in fp64:  v = b / sqrt(sum(b^2) + 1e-10);  v = min(v, 0.2);
 *           v = v / sqrt(sum(v^2) + 1e-10);  stored as fp32
 *     The sums are fixed trees, not row-major chains: a feature may differ from a NumPy restatement in the last fp32 bit.
 * replaces  evaluateSanity.py:90-91 and :94-95 (sanityForMethods.py:83-84, :87-88): feature.hog(..., pixels_per_cell=(16, 16))
 *   img : [n][H][W];  out : [n][H/ch - 2][W/cw - 2][3][3][9];  ws : xai_hog_workspace_bytes(n, H, W, ch, cw) bytes, 8-byte aligned
 *   fewer than 3 cells on an axis -> XAI_E_SHAPE;  n or H / ch above 65535 -> XAI_E_UNSUPPORTED */
int xai_hog_f32(const float* img, int n, int H, int W, int ch, int cw, float* out, void* ws, size_t ws_bytes, xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT2_H */
