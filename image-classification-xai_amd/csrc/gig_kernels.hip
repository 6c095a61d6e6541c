// K22: Guided IG (GIGBuilder.py:194-292) for gfx950 -- one outer step of guided_ig_impl per launch, B images per launch.
//
// One workgroup of 1024 lanes per image runs the whole `while gamma > 1` loop of a step (:246-291) with no host round
// trip.  An iteration is five sweeps over the image's N features (all read x, x_input, x_baseline, grad; L2-resident for
// a 224^2 image):
//   A   clamp to x_min (:249-253, recomputed on the fly, x is written only by the last sweep), l1_current, and the
//       histogram of the top 11 key bits;
//   B,C the next 11 and the last 10 key bits of the keys still in the running (a 3-pass radix select of the exact order
//       statistic torch.quantile(..., interpolation='lower') returns, :267);
//   D   l1_s (:272);
//   E   the update of x (:282-289) and attr (:292).
// A key is the gradient's bit pattern rotated left by one: |grad| in the upper 31 bits (non-negative floats order like their
// bit patterns), the sign below it.  The key of +inf (kOutKey) also marks x == x_max (:264): never selected, as the reference
// never selects grad == +inf (:268); -inf is the one key above it and is selected exactly when the threshold is infinite.
// The histograms count with LDS atomics (integer counts do not depend on arrival order).  l1_total, l1_current and l1_s
// are summed by one fixed tree (lane t takes elements t, t+1024, ... in order, fp64 per lane, wave butterfly, waves in
// order) and rounded to fp32: two runs give the same bytes, and on the last step, where every remaining feature is
// selected, l1_current and l1_s add the same terms in the same order and gamma is exactly 1.
// Capturable: the step index lives in the per-image state words and is advanced by the kernel, the init entry replaces
// every memset, and no host value changes from step to step.
#include "xai_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kBins = 2048;                  // 11-bit digits: bits [21,32), [10,21), [0,10)
constexpr int kMaxSelections = XAI_GIG_MAX_SELECTIONS;   // per step; the reference needed 51 for 50 steps on a toy net
constexpr uint32_t kOutKey = 0xff000000u;     // +inf rotated: x == x_max or grad == +inf
constexpr uint32_t kNegInfKey = 0xff000001u;  // -inf rotated; every NaN is above it
constexpr int64_t kMaxElems = int64_t{1} << 24;   // torch.quantile's own limit; up to it fp32(n_elem - 1) is exact

enum : int32_t { kOk = 0, kNanKey = 1, kCap = 2, kGamma = 3, kSteps = 4 };

// x after the clamp of :249-253, and x_max (translate_alpha_to_x, :183).  torch rounds every operation to fp32 and
// compares with the fp32 value of a python-float scalar; -ffp-contract=off keeps a*b+c two roundings.
__device__ __forceinline__ float clamped_x(float x, float xi, float xb, float amin, float amax, float& xmax) {
  const float d = xi - xb;
  const float xmin = xb + d * amin;
  xmax = xb + d * amax;
  float xa = d != 0.f ? (x - xb) / d : __builtin_nanf("");   // translate_x_to_alpha, :170
  if (xa != xa) xa = amax;                                    // :250
  return xa < amin ? xmin : x;
}

__device__ __forceinline__ uint32_t sel_key(float xc, float xmax, float g) {
  const uint32_t b = __float_as_uint(g);
  return xc == xmax ? kOutKey : (b << 1) | (b >> 31);          // +x and -x are neighbours: 2k and 2k + 1
}

// Python's math.isclose(a, b, rel_tol=1e-9, abs_tol=1e-9) on the fp32 values, in double (:258)
__device__ __forceinline__ bool py_isclose(float a32, float b32) {
  const double a = a32, b = b32;
  if (a == b) return true;
  if (isinf(a) || isinf(b)) return false;
  const double diff = fabs(a - b);
  return diff <= fmax(1e-9 * fmax(fabs(a), fabs(b)), 1e-9);
}

template <int V>
__global__ __launch_bounds__(kThreads) void gig_init_kernel(const float* __restrict__ xin_all, const float* __restrict__ xb_all, int64_t N,
                                                            float* __restrict__ x_all, float* __restrict__ attr_all,
                                                            float* __restrict__ l1_total, int32_t* __restrict__ state) {
  __shared__ double red[kWaves];
  const int64_t off = static_cast<int64_t>(blockIdx.x) * N;
  const float* xin = xin_all + off;
  const float* xb = xb_all + off;
  double s = 0.0;
  for (int64_t i = static_cast<int64_t>(threadIdx.x) * V; i < N; i += static_cast<int64_t>(kThreads) * V) {
    const Pack<V> a = ldp<V>(xin + i), b = ldp<V>(xb + i);
    Pack<V> z;
#pragma unroll
    for (int u = 0; u < V; ++u) {
      s += static_cast<double>(fabsf(a.v[u] - b.v[u]));       // l1_distance(x_input, x_baseline), :212
      z.v[u] = 0.f;
    }
    stp<V>(x_all + off + i, b);
    stp<V>(attr_all + off + i, z);
  }
  const double tot = block_sum<kWaves>(s, red);
  if (threadIdx.x == 0) {
    l1_total[blockIdx.x] = static_cast<float>(tot);
    int32_t* st = state + 4 * blockIdx.x;
    st[0] = 0; st[1] = kOk; st[2] = 0; st[3] = 0;
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void gig_step_kernel(const float* __restrict__ xin_all, const float* __restrict__ xb_all,
                                                            const float* __restrict__ g_all, int64_t N, int steps, double max_dist,
                                                            uint32_t rank, float* __restrict__ x_all, float* __restrict__ attr_all,
                                                            const float* __restrict__ l1_total, int32_t* __restrict__ state) {
  __shared__ uint32_t hist[kBins];
  __shared__ double red[kWaves];
  __shared__ uint32_t wsum[kWaves];
  __shared__ uint32_t pick[2];
  __shared__ uint32_t nan_seen;
  const int tid = threadIdx.x;
  int32_t* st = state + 4 * blockIdx.x;
  const int32_t step = st[0];
  if (st[1] != kOk) return;                                    // a failed image is left as it stands
  __syncthreads();                                             // every lane has read the state before lane 0 may write it
  if (step >= steps) {
    if (tid == 0) { st[1] = kSteps; st[3] = step; }
    return;
  }
  const float l1t = l1_total[blockIdx.x];
  if (l1t == 0.f) {                                            // input == baseline: attr stays zero (:222-225)
    if (tid == 0) { st[0] = step + 1; st[2] = 0; }
    return;
  }
  // :235-244 -- python floats (double), rounded to fp32 where torch meets them
  const double alpha = (step + 1.0) / steps;
  const float amin = static_cast<float>(fmax(alpha - max_dist, 0.0));
  const float amax = static_cast<float>(fmin(alpha + max_dist, 1.0));
  const float l1_target = l1t * static_cast<float>(1.0 - static_cast<double>(step + 1) / steps);

  const int64_t off = static_cast<int64_t>(blockIdx.x) * N;
  const float* xin = xin_all + off;
  const float* xb = xb_all + off;
  const float* g = g_all + off;
  float* x = x_all + off;
  float* attr = attr_all + off;
  const int64_t i0 = static_cast<int64_t>(tid) * V, di = static_cast<int64_t>(kThreads) * V;

  int selections = 0;
  for (;;) {
    // ---- A: clamp, l1_current, top digit
    select_zero_hist(hist);
    if (tid == 0) nan_seen = 0u;
    __syncthreads();
    double s = 0.0;
    for (int64_t i = i0; i < N; i += di) {
      const Pack<V> px = ldp<V>(x + i), pi = ldp<V>(xin + i), pb = ldp<V>(xb + i), pg = ldp<V>(g + i);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        float xmax;
        const float xc = clamped_x(px.v[u], pi.v[u], pb.v[u], amin, amax, xmax);
        s += static_cast<double>(fabsf(xc - pi.v[u]));
        const uint32_t key = sel_key(xc, xmax, pg.v[u]);
        if (key > kNegInfKey) nan_seen = 1u;
        else atomicAdd(&hist[key >> 21], 1u);
      }
    }
    const float l1_current = static_cast<float>(block_sum<kWaves>(s, red));   // (block_sum synchronises: hist and nan_seen are complete)
    const bool close = py_isclose(l1_target, l1_current);
    if (!close) {
      int32_t err = kOk;
      if (nan_seen) err = kNanKey;                              // torch.quantile would return NaN and the loop never ends
      else if (selections == kMaxSelections) err = kCap;
      if (err != kOk) {
        if (tid == 0) { st[1] = err; st[2] = selections; st[3] = step; }
        return;
      }
    }
    float gamma = 0.f;
    uint32_t thr = 0u;
    if (!close) {
      ++selections;
      // ---- B, C: radix select of the key of rank `rank`
      uint32_t k = rank;
      const uint32_t d1 = select_digit<kThreads>(hist, k, wsum, pick);
      select_zero_hist(hist);
      __syncthreads();
      for (int64_t i = i0; i < N; i += di) {
        const Pack<V> px = ldp<V>(x + i), pi = ldp<V>(xin + i), pb = ldp<V>(xb + i), pg = ldp<V>(g + i);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float xmax;
          const float xc = clamped_x(px.v[u], pi.v[u], pb.v[u], amin, amax, xmax);
          const uint32_t key = sel_key(xc, xmax, pg.v[u]);
          if ((key >> 21) == d1) atomicAdd(&hist[(key >> 10) & 0x7FFu], 1u);
        }
      }
      __syncthreads();
      const uint32_t d2 = select_digit<kThreads>(hist, k, wsum, pick);
      const uint32_t hi = (d1 << 11) | d2;
      select_zero_hist(hist);
      __syncthreads();
      for (int64_t i = i0; i < N; i += di) {
        const Pack<V> px = ldp<V>(x + i), pi = ldp<V>(xin + i), pb = ldp<V>(xb + i), pg = ldp<V>(g + i);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float xmax;
          const float xc = clamped_x(px.v[u], pi.v[u], pb.v[u], amin, amax, xmax);
          const uint32_t key = sel_key(xc, xmax, pg.v[u]);
          if ((key >> 10) == hi) atomicAdd(&hist[key & 0x3FFu], 1u);
        }
      }
      __syncthreads();
      thr = (hi << 10) | select_digit<kThreads>(hist, k, wsum, pick) | 1u;   // | 1: |grad| <= threshold takes -x with +x
      // ---- D: l1_s = sum |x - x_max| over the selection s = |grad| <= threshold && grad != inf (:268, :272)
      s = 0.0;
      for (int64_t i = i0; i < N; i += di) {
        const Pack<V> px = ldp<V>(x + i), pi = ldp<V>(xin + i), pb = ldp<V>(xb + i), pg = ldp<V>(g + i);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float xmax;
          const float xc = clamped_x(px.v[u], pi.v[u], pb.v[u], amin, amax, xmax);
          const uint32_t key = sel_key(xc, xmax, pg.v[u]);
          if (key <= thr && key != kOutKey) s += static_cast<double>(fabsf(xc - xmax));
        }
      }
      const float l1_s = static_cast<float>(block_sum<kWaves>(s, red));
      gamma = l1_s > 0.f ? (l1_current - l1_target) / l1_s : __builtin_inff();    // :277-280
      if (!(gamma > 1.f) && !(gamma > 0.f)) {                                      // the reference's assert (:287)
        if (tid == 0) { st[1] = kGamma; st[2] = selections; st[3] = step; }
        return;
      }
    }
    // ---- E: x <- clamped x, then the selection moves to x_max (gamma > 1) or by gamma toward it; attr += (x - x_old) * grad
    for (int64_t i = i0; i < N; i += di) {
      const Pack<V> px = ldp<V>(x + i), pi = ldp<V>(xin + i), pb = ldp<V>(xb + i), pg = ldp<V>(g + i);
      Pack<V> pa = ldp<V>(attr + i), pn;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        float xmax;
        const float xc = clamped_x(px.v[u], pi.v[u], pb.v[u], amin, amax, xmax);
        float xn = xc;
        if (!close) {
          const uint32_t key = sel_key(xc, xmax, pg.v[u]);
          if (key <= thr && key != kOutKey) xn = gamma > 1.f ? xmax : xc + (xmax - xc) * gamma;
        }
        pn.v[u] = xn;
        pa.v[u] = pa.v[u] + (xn - px.v[u]) * pg.v[u];
      }
      stp<V>(x + i, pn);
      stp<V>(attr + i, pa);
    }
    if (close || !(gamma > 1.f)) break;
    __syncthreads();                                           // this sweep's writes of x before the next iteration reads them
  }
  if (tid == 0) { st[0] = step + 1; st[2] = selections; }
}

}  // namespace

XAI_EXPORT int xai_gig_init_f32(const float* x_input, const float* x_baseline, int n_img, int64_t n_elem, float* x, float* attr,
                                float* l1_total, int32_t* state, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x_input); XAI_REQUIRE_PTR(x_baseline); XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(attr); XAI_REQUIRE_PTR(l1_total);
  XAI_REQUIRE_PTR(state);
  XAI_REQUIRE(n_img > 0 && n_elem > 0, XAI_E_SHAPE);
  XAI_REQUIRE(n_img <= 65535 && n_elem <= kMaxElems, XAI_E_UNSUPPORTED);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(xai_can_vec4(n_elem, {x_input, x_baseline, x, attr}), [&](auto V4) {
    hipLaunchKernelGGL(gig_init_kernel<V4 ? 4 : 1>, dim3(n_img), dim3(kThreads), 0, st, x_input, x_baseline, n_elem, x, attr, l1_total, state);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_gig_step_f32(const float* x_input, const float* x_baseline, const float* grad, int n_img, int64_t n_elem, int steps,
                                float fraction, double max_dist, float* x, float* attr, const float* l1_total, int32_t* state,
                                xai_stream_t stream) {
  XAI_REQUIRE_PTR(x_input); XAI_REQUIRE_PTR(x_baseline); XAI_REQUIRE_PTR(grad); XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(attr);
  XAI_REQUIRE_PTR(l1_total); XAI_REQUIRE_PTR(state);
  XAI_REQUIRE(n_img > 0 && n_elem > 0 && steps > 0, XAI_E_SHAPE);
  XAI_REQUIRE(fraction >= 0.f && fraction <= 1.f && max_dist == max_dist, XAI_E_SHAPE);
  XAI_REQUIRE(n_img <= 65535 && n_elem <= kMaxElems, XAI_E_UNSUPPORTED);
  // torch.quantile: rank = floor(q * (n - 1)) with q an fp32 tensor, so the product rounds to fp32 first (n_elem - 1 < 2^24 is
  // exact in fp32, so the rank is at most n_elem - 1)
  const float r = fraction * static_cast<float>(n_elem - 1);
  const uint32_t rank = static_cast<uint32_t>(floorf(r));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(xai_can_vec4(n_elem, {x_input, x_baseline, grad, x, attr}), [&](auto V4) {
    hipLaunchKernelGGL(gig_step_kernel<V4 ? 4 : 1>, dim3(n_img), dim3(kThreads), 0, st, x_input, x_baseline, grad, n_elem, steps, max_dist,
                       rank, x, attr, l1_total, state);
  });
  return xai_launch_status();
}
