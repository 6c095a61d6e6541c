// K65-K68: SLIC superpixels as scikit-image 0.18.3 computes them (slic_superpixels.py:298-328, _slic.pyx), for gfx950.  libxai_slic.so;
// include/xai_hip_slic.h states the contract (the k-means in T = float or double with every operation rounded once, the regular
// case of the connectivity pass).
//
//   K65 assign      one lane per pixel, a workgroup per 16 x 16 tile.  256 clusters at a time, in ascending k, the workgroup lists
//                   those whose window meets the tile (centre and integer bounds in LDS, placed by a ballot and a prefix of the
//                   waves' counts); each lane walks the list with its own containment test and `dist > d`.
//   K66 update      one wave per cluster walks the cluster's window in raster order, 64 pixels at a time: a ballot of the members,
//                   their (y, x, features) staged in LDS, lane f adding feature f of the members in ascending lane order -- the
//                   sequential chain that gives skimage's float sums.  Then the division, over the old centre.
//   K67 components  one workgroup per image: least-root sweeps between two arrays until nothing changes, the sizes, the regular test
//   K68 numbering   one workgroup per image: an integer prefix scan of the first pixels in pixel order, then the renumbering
// Nothing waits on another workgroup and every loop has a bound fixed at launch.  The only atomics are integer ones whose result does
// not depend on their order (an OR into the status word, an add into a component's size).
#include "xai_common.h"
#include "xai_hip_slic.h"

#include <float.h>
#include <math.h>

XAI_VERSION_ENTRIES(xai_slic_version, XAI_SLIC_VERSION, XAI_SLIC_MINOR)

namespace {

constexpr int kSlicTile = 16;                       // K65: a workgroup is a 16 x 16 block of pixels
constexpr int kSlicList = kSlicTile * kSlicTile;    // clusters tested, and at the most listed, per pass: one per lane
constexpr int kSlicMaxF = 2 + XAI_SLIC_MAX_CHANNELS;
constexpr int kSlicCc = 1024;                       // lanes of the one workgroup K67 / K68 give an image

template <typename T>
__device__ __forceinline__ T slic_far();
template <>
__device__ __forceinline__ float slic_far<float>() { return INFINITY; }        // (float)DBL_MAX
template <>
__device__ __forceinline__ double slic_far<double>() { return DBL_MAX; }

// [lo, hi) of a window along an axis of n pixels: trunc(max(c - 2 step, 0)), trunc(min(c + 2 step + 1, n)), in T; both clamped to
// [0, n], which changes no window that holds a pixel and keeps the conversion defined; a NaN centre has the empty window.
template <typename T>
__device__ __forceinline__ void slic_bounds(T c, T two_step, int n, int& lo, int& hi) {
  if (c != c) {
    lo = hi = 0;
    return;
  }
  const T fn = static_cast<T>(n);
  T a = c - two_step;
  a = a > T(0) ? a : T(0);
  a = a < fn ? a : fn;
  T b = (c + two_step) + T(1);
  b = b < fn ? b : fn;
  b = b > T(0) ? b : T(0);
  lo = static_cast<int>(a);
  hi = static_cast<int>(b);
}

// ------------------------------------------------------------------------------------------------ K65
template <typename T>
__global__ __launch_bounds__(kSlicList) void slic_assign_kernel(const T* __restrict__ features, const T* __restrict__ centres, int H, int W,
                                                                int C, int S, int step, int32_t* __restrict__ labels,
                                                                int32_t* __restrict__ status) {
  __shared__ T cen[kSlicList][kSlicMaxF];
  __shared__ int win[kSlicList][4];
  __shared__ int ks[kSlicList];
  __shared__ int wcount[kSlicList / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const int b = blockIdx.z, F = 2 + C;
  const int ty0 = blockIdx.y * kSlicTile, tx0 = blockIdx.x * kSlicTile;
  const int y = ty0 + t / kSlicTile, x = tx0 + t % kSlicTile;
  const bool in = y < H && x < W;
  const size_t pix = (static_cast<size_t>(b) * H + (in ? y : 0)) * W + (in ? x : 0);
  T f[XAI_SLIC_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < XAI_SLIC_MAX_CHANNELS; ++c) f[c] = (in && c < C) ? features[pix * C + c] : T(0);
  const T fstep = static_cast<T>(step);
  const T two_step = static_cast<T>(2 * step);
  const T sw = T(1) / (fstep * fstep);
  const T fy = static_cast<T>(y), fx = static_cast<T>(x);

  T best = slic_far<T>();
  int label = -1;
  for (int base = 0; base < S; base += kSlicList) {
    const int k = base + t;
    bool meets = false;
    int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    const T* row = centres + (static_cast<size_t>(b) * S + (k < S ? k : 0)) * F;
    if (k < S) {
      slic_bounds<T>(row[0], two_step, H, y0, y1);
      slic_bounds<T>(row[1], two_step, W, x0, x1);
      meets = y0 < y1 && x0 < x1 && y0 < ty0 + kSlicTile && y1 > ty0 && x0 < tx0 + kSlicTile && x1 > tx0;
    }
    const uint64_t bits = __ballot(meets);
    if (lane == 0) wcount[wave] = __popcll(bits);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSlicList / kWave; ++w) {
      if (w < wave) off += wcount[w];
      total += wcount[w];
    }
    if (meets) {                                     // ascending k: the waves in order, the lanes of a wave in order
      const int slot = off + __popcll(bits & ((uint64_t(1) << lane) - 1));
      ks[slot] = k;
      win[slot][0] = y0; win[slot][1] = y1; win[slot][2] = x0; win[slot][3] = x1;
      for (int c = 0; c < F; ++c) cen[slot][c] = row[c];
    }
    __syncthreads();
    if (in) {
      for (int e = 0; e < total; ++e) {
        if (y < win[e][0] || y >= win[e][1] || x < win[e][2] || x >= win[e][3]) continue;
        const T dy = cen[e][0] - fy, dx = cen[e][1] - fx;
        T dc = T(0);
#pragma unroll
        for (int c = 0; c < XAI_SLIC_MAX_CHANNELS; ++c) {
          if (c < C) {
            const T q = f[c] - cen[e][2 + c];
            dc = dc + q * q;
          }
        }
        const T d = ((dy * dy) + (dx * dx)) * sw + dc;
        if (best > d) {
          best = d;
          label = ks[e];
        }
      }
    }
    __syncthreads();                                 // the list is free again
  }
  if (in) {
    labels[pix] = label;
    if (label < 0) atomicOr(&status[b], XAI_SLIC_UNCOVERED);
  }
}

// ------------------------------------------------------------------------------------------------ K66
template <typename T>
__global__ __launch_bounds__(kWave) void slic_update_kernel(const T* __restrict__ features, const int32_t* __restrict__ labels, int H, int W,
                                                            int C, int S, int step, T* centres, int32_t* __restrict__ status) {
  __shared__ T stage[kWave][kSlicMaxF];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, F = 2 + C;
  T* row = centres + (static_cast<size_t>(b) * S + k) * F;
  const T two_step = static_cast<T>(2 * step);
  int y0, y1, x0, x1;
  slic_bounds<T>(row[0], two_step, H, y0, y1);
  slic_bounds<T>(row[1], two_step, W, x0, x1);
  const int wh = y1 - y0, ww = x1 - x0;
  const int n = (wh > 0 && ww > 0) ? wh * ww : 0;
  const size_t image = static_cast<size_t>(b) * H * W;
  T acc = T(0);
  int cnt = 0;
  for (int i = 0; i < n; i += kWave) {               // the window in raster order, 64 pixels at a time
    const int idx = i + lane;
    bool member = false;
    if (idx < n) {
      const int y = y0 + idx / ww, x = x0 + idx % ww;
      const size_t p = image + static_cast<size_t>(y) * W + x;
      member = labels[p] == k;
      if (member) {
        stage[lane][0] = static_cast<T>(y);
        stage[lane][1] = static_cast<T>(x);
        for (int c = 0; c < C; ++c) stage[lane][2 + c] = features[p * C + c];
      }
    }
    uint64_t bits = __ballot(member);
    __syncthreads();
    cnt += __popcll(bits);
    if (lane < F) {
      while (bits) {                                 // ascending lane = ascending pixel: at the most 64 turns
        const int l = __ffsll(static_cast<unsigned long long>(bits)) - 1;
        bits &= bits - 1;
        acc = acc + stage[l][lane];
      }
    }
    __syncthreads();
  }
  if (lane < F) row[lane] = acc / static_cast<T>(cnt);                 // 0 / 0 for a cluster without a pixel, reported
  if (lane == 0 && cnt == 0) atomicOr(&status[b], XAI_SLIC_EMPTY);
}

// ------------------------------------------------------------------------------------------------ K67
__global__ __launch_bounds__(kSlicCc) void slic_components_kernel(const int32_t* __restrict__ labels, int H, int W, int min_size, int max_size,
                                                                  int32_t* __restrict__ comp, int32_t* __restrict__ status, int32_t* side_a,
                                                                  int32_t* side_b, int32_t* sizes) {
  __shared__ int changed;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1);
  const int n = H * W;
  const size_t image = static_cast<size_t>(b) * n;
  const int32_t* lab = labels + image;
  int32_t* src = side_a + image;
  int32_t* dst = side_b + image;
  int32_t* size = sizes + image;
  for (int p = t; p < n; p += kSlicCc) {
    src[p] = p;
    size[p] = 0;
  }
  __threadfence();                                   // the zeroed sizes are at the device's level before any lane adds to them
  __syncthreads();
  bool settled = false;
  for (int sweep = 0; sweep < XAI_SLIC_MAX_SWEEPS; ++sweep) {
    if (t == 0) changed = 0;
    __syncthreads();
    bool any = false;
    for (int p = t; p < n; p += kSlicCc) {
      const int l = lab[p], mine = src[p];
      int best = src[mine];                          // a root is in its pixel's component and not above it, so this follows it once
      const int y = p / W, x = p - y * W;
      if (y > 0 && lab[p - W] == l) best = min(best, src[src[p - W]]);
      if (x > 0 && lab[p - 1] == l) best = min(best, src[src[p - 1]]);
      if (x + 1 < W && lab[p + 1] == l) best = min(best, src[src[p + 1]]);
      if (y + 1 < H && lab[p + W] == l) best = min(best, src[src[p + W]]);
      dst[p] = best;
      any |= best != mine;
    }
    if (any) changed = 1;                            // every writer writes the same word
    __syncthreads();
    const int c = changed;
    int32_t* const swap = src;
    src = dst;
    dst = swap;
    __syncthreads();
    if (!c) {
      settled = true;
      break;
    }
  }
  if (!settled) {
    if (t == 0) atomicOr(&status[b], XAI_SLIC_IRREGULAR);
    for (int p = t; p < n; p += kSlicCc) comp[image + p] = src[p];
    return;
  }
  // sizes: a run of equal roots inside a wave's 64 consecutive pixels adds its length once, by its first lane
  for (int base = 0; base < n; base += kSlicCc) {
    const int p = base + t;
    const int r = p < n ? src[p] : -1;
    const int before = __shfl_up(r, 1, kWave);
    const bool head = p < n && (lane == 0 || before != r);
    const uint64_t heads = __ballot(head), live = __ballot(p < n);
    if (p < n) comp[image + p] = r;
    if (head) {
      const uint64_t above = lane == kWave - 1 ? 0 : (heads >> (lane + 1)) << (lane + 1);
      const int end = above ? __ffsll(static_cast<unsigned long long>(above)) - 1 : __popcll(live);
      atomicAdd(&size[r], end - lane);
    }
  }
  __threadfence();
  __syncthreads();
  bool bad = false;
  for (int p = t; p < n; p += kSlicCc) {
    if (src[p] == p) {
      const int s = __hip_atomic_load(&size[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bad |= s < min_size || s >= max_size;
    }
  }
  if (bad) atomicOr(&status[b], XAI_SLIC_IRREGULAR);
}

// ------------------------------------------------------------------------------------------------ K68
__global__ __launch_bounds__(kSlicCc) void slic_number_kernel(const int32_t* __restrict__ comp, int n, int start_label, int32_t* __restrict__ out,
                                                              int32_t* __restrict__ nlabels, int32_t* ranks) {
  __shared__ uint32_t wsum[kSlicCc / kWave];
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t image = static_cast<size_t>(b) * n;
  const int32_t* cm = comp + image;
  int32_t* rank = ranks + image;
  uint32_t run = 0;                                  // the first pixels below this pass
  for (int base = 0; base < n; base += kSlicCc) {
    const int p = base + t;
    const uint32_t flag = (p < n && cm[p] == p) ? 1u : 0u;
    const uint32_t below = block_scan_excl<kSlicCc>(flag, run, wsum);
    if (flag) rank[p] = static_cast<int32_t>(below);
    __syncthreads();
  }
  if (t == 0) nlabels[b] = static_cast<int32_t>(run);
  for (int p = t; p < n; p += kSlicCc) {
    int c = cm[p];
    if (c < 0 || c >= n || cm[c] != c) c = -1;        // never followed: not a first pixel
    out[image + p] = c < 0 ? -1 : start_label + rank[c];
  }
}

// ------------------------------------------------------------------------------------------------ host side
int slic_check(int B, int H, int W, int C, int S, int step) {
  XAI_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && S >= 1 && step >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && S <= XAI_SLIC_MAX_CLUSTERS && C <= XAI_SLIC_MAX_CHANNELS, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(static_cast<int64_t>(H) * W <= XAI_SLIC_MAX_PIXELS && step <= XAI_SLIC_MAX_PIXELS, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(xai_ceil_div(H, kSlicTile) <= 65535, XAI_E_UNSUPPORTED);          // K65's rows of tiles are a grid extent in y
  return XAI_OK;
}

int slic_check_image(int B, int H, int W, const void* ws, size_t ws_bytes) {
  XAI_REQUIRE(B >= 1 && H >= 1 && W >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && static_cast<int64_t>(H) * W <= XAI_SLIC_MAX_PIXELS, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= xai_slic_workspace_bytes(B, H, W) && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, XAI_E_SHAPE);
  return XAI_OK;
}

template <typename T>
int slic_assign(const T* features, const T* centres, int B, int H, int W, int C, int S, int step, int32_t* labels, int32_t* status,
                hipStream_t s) {
  const dim3 grid(unsigned(xai_ceil_div(W, kSlicTile)), unsigned(xai_ceil_div(H, kSlicTile)), unsigned(B));
  slic_assign_kernel<T><<<grid, kSlicList, 0, s>>>(features, centres, H, W, C, S, step, labels, status);
  return xai_launch_status();
}

template <typename T>
int slic_update(const T* features, const int32_t* labels, int B, int H, int W, int C, int S, int step, T* centres, int32_t* status,
                hipStream_t s) {
  slic_update_kernel<T><<<dim3(unsigned(S), unsigned(B)), kWave, 0, s>>>(features, labels, H, W, C, S, step, centres, status);
  return xai_launch_status();
}

template <typename T>
int slic_assign_entry(const T* features, const T* centres, int B, int H, int W, int C, int S, int step, int32_t* labels, int32_t* status,
                      xai_stream_t stream) {
  XAI_REQUIRE_PTR(features);
  XAI_REQUIRE_PTR(centres);
  XAI_REQUIRE_PTR(labels);
  XAI_REQUIRE_PTR(status);
  const int rc = slic_check(B, H, W, C, S, step);
  if (rc != XAI_OK) return rc;
  return slic_assign<T>(features, centres, B, H, W, C, S, step, labels, status, static_cast<hipStream_t>(stream));
}

template <typename T>
int slic_update_entry(const T* features, const int32_t* labels, int B, int H, int W, int C, int S, int step, T* centres, int32_t* status,
                      xai_stream_t stream) {
  XAI_REQUIRE_PTR(features);
  XAI_REQUIRE_PTR(labels);
  XAI_REQUIRE_PTR(centres);
  XAI_REQUIRE_PTR(status);
  const int rc = slic_check(B, H, W, C, S, step);
  if (rc != XAI_OK) return rc;
  return slic_update<T>(features, labels, B, H, W, C, S, step, centres, status, static_cast<hipStream_t>(stream));
}

template <typename T>
int slic_iterate_entry(const T* features, int B, int H, int W, int C, int S, int step, int iterations, T* centres, int32_t* labels,
                       int32_t* status, xai_stream_t stream) {
  XAI_REQUIRE_PTR(features);
  XAI_REQUIRE_PTR(centres);
  XAI_REQUIRE_PTR(labels);
  XAI_REQUIRE_PTR(status);
  const int rc = slic_check(B, H, W, C, S, step);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(iterations >= 1, XAI_E_SHAPE);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int st = xai_clear_i32(status, B, s);
  for (int it = 0; it < iterations && st == XAI_OK; ++it) {
    st = slic_assign<T>(features, centres, B, H, W, C, S, step, labels, status, s);
    if (st == XAI_OK) st = slic_update<T>(features, labels, B, H, W, C, S, step, centres, status, s);
  }
  return st;
}

}  // namespace

XAI_EXPORT int xai_slic_max_clusters(void) { return XAI_SLIC_MAX_CLUSTERS; }
XAI_EXPORT int xai_slic_max_channels(void) { return XAI_SLIC_MAX_CHANNELS; }
XAI_EXPORT int xai_slic_max_pixels(void) { return XAI_SLIC_MAX_PIXELS; }

XAI_EXPORT size_t xai_slic_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || B > 65535 || static_cast<int64_t>(H) * W > XAI_SLIC_MAX_PIXELS) return 0;
  return static_cast<size_t>(3) * B * H * W * sizeof(int32_t);
}

XAI_EXPORT int xai_slic_clear_i32(int32_t* status, int B, xai_stream_t stream) {
  XAI_REQUIRE_PTR(status);
  XAI_REQUIRE(B >= 1, XAI_E_SHAPE);
  return xai_clear_i32(status, B, static_cast<hipStream_t>(stream));
}

XAI_EXPORT int xai_slic_assign_f32(const float* features, const float* centres, int B, int H, int W, int C, int S, int step, int32_t* labels,
                                   int32_t* status, xai_stream_t stream) {
  return slic_assign_entry<float>(features, centres, B, H, W, C, S, step, labels, status, stream);
}
XAI_EXPORT int xai_slic_assign_f64(const double* features, const double* centres, int B, int H, int W, int C, int S, int step,
                                   int32_t* labels, int32_t* status, xai_stream_t stream) {
  return slic_assign_entry<double>(features, centres, B, H, W, C, S, step, labels, status, stream);
}
XAI_EXPORT int xai_slic_update_f32(const float* features, const int32_t* labels, int B, int H, int W, int C, int S, int step, float* centres,
                                   int32_t* status, xai_stream_t stream) {
  return slic_update_entry<float>(features, labels, B, H, W, C, S, step, centres, status, stream);
}
XAI_EXPORT int xai_slic_update_f64(const double* features, const int32_t* labels, int B, int H, int W, int C, int S, int step,
                                   double* centres, int32_t* status, xai_stream_t stream) {
  return slic_update_entry<double>(features, labels, B, H, W, C, S, step, centres, status, stream);
}
XAI_EXPORT int xai_slic_iterate_f32(const float* features, int B, int H, int W, int C, int S, int step, int iterations, float* centres,
                                    int32_t* labels, int32_t* status, xai_stream_t stream) {
  return slic_iterate_entry<float>(features, B, H, W, C, S, step, iterations, centres, labels, status, stream);
}
XAI_EXPORT int xai_slic_iterate_f64(const double* features, int B, int H, int W, int C, int S, int step, int iterations, double* centres,
                                    int32_t* labels, int32_t* status, xai_stream_t stream) {
  return slic_iterate_entry<double>(features, B, H, W, C, S, step, iterations, centres, labels, status, stream);
}

XAI_EXPORT int xai_slic_components_i32(const int32_t* labels, int B, int H, int W, int min_size, int max_size, int32_t* comp,
                                       int32_t* status, void* ws, size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(labels);
  XAI_REQUIRE_PTR(comp);
  XAI_REQUIRE_PTR(status);
  XAI_REQUIRE_PTR(ws);
  const int rc = slic_check_image(B, H, W, ws, ws_bytes);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(min_size >= 0 && max_size >= min_size, XAI_E_SHAPE);
  int32_t* side_a = static_cast<int32_t*>(ws);
  const size_t pixels = static_cast<size_t>(B) * H * W;
  slic_components_kernel<<<unsigned(B), kSlicCc, 0, static_cast<hipStream_t>(stream)>>>(labels, H, W, min_size, max_size, comp, status,
                                                                                         side_a, side_a + pixels, side_a + 2 * pixels);
  return xai_launch_status();
}

XAI_EXPORT int xai_slic_number_i32(const int32_t* comp, int B, int H, int W, int start_label, int32_t* out, int32_t* nlabels, void* ws,
                                   size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(comp);
  XAI_REQUIRE_PTR(out);
  XAI_REQUIRE_PTR(nlabels);
  XAI_REQUIRE_PTR(ws);
  const int rc = slic_check_image(B, H, W, ws, ws_bytes);
  if (rc != XAI_OK) return rc;
  slic_number_kernel<<<unsigned(B), kSlicCc, 0, static_cast<hipStream_t>(stream)>>>(comp, H * W, start_label, out, nlabels,
                                                                                    static_cast<int32_t*>(ws));
  return xai_launch_status();
}
