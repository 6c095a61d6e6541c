/*
 * xai_hip_ext.h -- C ABI of libxai_ext.so, the extension library beside libxai_hip.so.
 *
 * include/xai_hip.h and the exports of libxai_hip.so are frozen at ABI 1.11; entry points added
 * after that live here, in a library of their own with a version pair of its own.  The grammar is
 * xai_hip.h's (one extern "C" block, the stream typedef, launch entries end in _f32 / _f64 / _i32 /
 * _u64, return int and take the caller's stream last), so xai_engine/_lib.py binds both headers
 * with the same strict reader, and so are the conventions: device pointers owned by the caller,
 * asynchronous graph-capturable launches, nothing allocated or retained, no global state.
 * Return values are xai_hip.h's: 0 = success, <0 = XAI_E_*, >0 = hipError_t of the launch;
 * xai_strerror (libxai_hip.so) has the text for all of them.
 */
#ifndef XAI_HIP_EXT_H
#define XAI_HIP_EXT_H

#include <stddef.h>
#include <stdint.h>

#include "xai_hip.h" /* XAI_OK, XAI_E_NULL, XAI_E_SHAPE, XAI_E_UNSUPPORTED */

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */

/* xai_ext_version() = XAI_EXT_VERSION: bumped when an existing prototype or its documented meaning changes.
 * xai_ext_version_minor() = XAI_EXT_MINOR: bumped whenever entry points are added:
 *   0 = xai_gshap_scale_f32, xai_gshap_finish_f32 */
#define XAI_EXT_VERSION 1
#define XAI_EXT_MINOR 0

int xai_ext_version(void);
int xai_ext_version_minor(void);

/* ---- GradientShap (xai_engine/gshap.py) ------------------------------------------------- */

/* K34 out[r][e] = alpha[r] * xr[r][e] + (1.0f - alpha[r]) * baselines[idx[r]][e]
 *     two products and one sum, each rounded to fp32 (no FMA); xr[r] = x[r / n_samples] when
 *     x_per_row == 0 (one input per image, n_samples rows each: repeat_interleave) and x[r] otherwise
 * replaces  captum's GradientShap interpolants behind evaluatePerturbation.py:164-167
 *           (rand_coefficient * input + (1 - rand_coefficient) * baseline on the randomly chosen baselines)
 *   x         : [n_rows / n_samples][n_elem] or, x_per_row != 0, [n_rows][n_elem]
 *   baselines : [n_base][n_elem];  idx : n_rows values in [0, n_base) (a value outside is clamped into it)
 *   alpha     : n_rows values;  out : [n_rows][n_elem];  n_rows must be a multiple of n_samples
 *   16-byte accesses when n_elem % 4 == 0 and x, baselines, out are 16-byte aligned */
int xai_gshap_scale_f32(const float* x, const float* baselines, const float* alpha, const int64_t* idx, int n_rows,
                        int n_samples, int64_t n_elem, int n_base, int x_per_row, float* out, xai_stream_t stream);

/* K35 attr[b][c][p] = (+0 + sum over s = 0 .. n_samples-1, ascending, of (xr[r][c][p] - baselines[idx[r]][c][p]) * grads[r][c][p])
 *                     / (float)n_samples,   r = b * n_samples + s;  difference, product, sums and the division round separately
 *     map[b][p]     = | ((a_0 + a_1) + a_2 + ...) |,  a_c = attr[b][c][p], channels left to right from the first
 * replaces  captum's GradientShap tail behind evaluatePerturbation.py:164-167 (grads * (input - baseline), the mean over the
 *           n_samples rows of an image) and the harness's np.abs(np.sum(., axis=0)), :181
 *   grads : [B * n_samples][C][HW];  x : [B][C][HW] or, x_per_row != 0, [B * n_samples][C][HW];  baselines : [n_base][C][HW]
 *   idx   : B * n_samples values as for K34;  attr : [B][C][HW] or NULL;  map : [B][HW] or NULL (one of the two required;
 *   nothing is written through a NULL output); 16-byte accesses when HW % 4 == 0 and every array is 16-byte aligned */
int xai_gshap_finish_f32(const float* grads, const float* x, const float* baselines, const int64_t* idx, int B,
                         int n_samples, int C, int64_t HW, int n_base, int x_per_row, float* attr, float* map,
                         xai_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XAI_HIP_EXT_H */
