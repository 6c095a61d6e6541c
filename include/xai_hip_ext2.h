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
 *   0 = xai_mda_max_segments, xai_mda_max_width, xai_mda_compose_f32, xai_mda_select_f32, xai_mda_commit_f32 */
#define XAI_EXT2_VERSION 1
#define XAI_EXT2_MINOR 0

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

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT2_H */
