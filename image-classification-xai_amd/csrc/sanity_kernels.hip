// K39-K43: the map comparison of the model-randomisation sanity test (evaluateSanity.py:68-106 normalize_image and get_sanity;
// util/test_methods/sanityForMethods.py:60-92) for gfx950.  Part of libxai_ext2.so (include/xai_hip_ext2.h).
//
// The reference compares the attribution of the trained model with the one of a randomised copy on the host: skimage's SSIM with
// Gaussian weights, scipy's spearmanr over all pixels, and spearmanr over the two skimage HOG vectors.  Here the maps stay on the
// device and a batch of pairs is compared by:
//   K39 normalize   one workgroup per map: min / max with NumPy's NaN rule, the +-Inf -> 0 fix, min / max again, (x - mn) / (mx - mn)
//   K40 ssim        one workgroup per 32 x 32 tile of a pair: both images with a halo of 5 in LDS (indices reflected), scipy's
//                   Gaussian filter along axis 0 on x, y, x*x, y*y, x*y (fp64 accumulation in scipy's symmetric order, rounded to
//                   fp32), then along axis 1, then skimage's S in fp32; the tile's interior sum in fp64 goes to the workspace and a
//                   second launch adds the tiles of a pair in ascending order
//   K41 tie ranks   one lane per sorted position: the first and last position of its tie group by two binary searches over the
//                   sorted values (skipped where a neighbour differs), twice the average rank = lo + hi + 2 written at the element
//   K42 rank corr   one workgroup per pair: exact int64 sums of the products of doubled rank deviations, then NumPy's corrcoef
//                   sequence in fp64 by lane 0
//   K43 hog         one workgroup per cell: central differences in fp32, hypot / atan2 in fp64, nine fp64 bin sums in one fixed
//                   tree each; then one wave per 3 x 3 block of cells for the L2-Hys normalisation
// Every sum has one fixed order, so a result is the same bits on every run.  Capturable: no allocation, no memset, no atomics.
#include "xai_common.h"
#include "xai_hip_ext2.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ K39
constexpr int kNormThreads = 1024;
constexpr int kNormWaves = kNormThreads / kWave;

__device__ __forceinline__ float inf_to_zero(float v) { return (v == INFINITY || v == -INFINITY) ? 0.f : v; }

template <int V>
__global__ __launch_bounds__(kNormThreads) void sanity_normalize_kernel(const float* __restrict__ x_all, int64_t hw, int guard,
                                                                        float* __restrict__ out_all) {
  __shared__ float red[2 * kNormWaves];
  const float* x = x_all + static_cast<int64_t>(blockIdx.x) * hw;
  float* out = out_all + static_cast<int64_t>(blockIdx.x) * hw;
  const int64_t first = static_cast<int64_t>(threadIdx.x) * V, stride = static_cast<int64_t>(kNormThreads) * V;
  float lo1 = INFINITY, hi1 = -INFINITY, lo2 = INFINITY, hi2 = -INFINITY;   // of the map as given; with +-Inf replaced by 0
  int nan = 0;
  for (int64_t i = first; i < hw; i += stride) {
    const Pack<V> p = ldp<V>(x + i);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float v = p.v[k], f = inf_to_zero(v);
      nan |= v != v;
      lo1 = fminf(lo1, v); hi1 = fmaxf(hi1, v);
      lo2 = fminf(lo2, f); hi2 = fmaxf(hi2, f);
    }
  }
  block_min_max<kNormWaves>(lo1, hi1, red);
  block_min_max<kNormWaves>(lo2, hi2, red);
  if (__syncthreads_or(nan)) lo1 = hi1 = lo2 = hi2 = NAN;                   // NumPy: one NaN makes min and max NaN
  const bool through = guard && (hi1 - lo1) == 0.f;
  const float den = hi2 - lo2;
  for (int64_t i = first; i < hw; i += stride) {
    Pack<V> p = ldp<V>(x + i);
    if (!through) {
#pragma unroll
      for (int k = 0; k < V; ++k) p.v[k] = (inf_to_zero(p.v[k]) - lo2) / den;
    }
    stp<V>(out + i, p);
  }
}

// ------------------------------------------------------------------------------------------------ K40
constexpr int kSsimTile = 32;                        // outputs of a workgroup along each axis
constexpr int kSsimR = 5;                            // int(truncate * sigma + 0.5) = int(3.5 * 1.5 + 0.5)
constexpr int kSsimIn = kSsimTile + 2 * kSsimR;
constexpr int kSsimThreads = 256;

struct SsimWeights {
  double w[kSsimR + 1];                              // w[0]: the outermost tap ... w[5]: the centre
};

// scipy's mode='reflect' (d c b a | a b c d | d c b a); one fold is enough for a halo of 5 on an axis of at least 11.  The clamp
// only keeps the loads of a tile that hangs over the image inside it; what they fetch is never used.
__device__ __forceinline__ int reflect_index(int i, int n) {
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - i - 1;
  return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(kSsimThreads) void ssim_tile_kernel(const float* __restrict__ x_all, const float* __restrict__ y_all,
                                                                 int H, int W, SsimWeights wt, float C1, float C2,
                                                                 float* __restrict__ S_all, double* __restrict__ partial) {
  __shared__ float sx[kSsimIn][kSsimIn + 1], sy[kSsimIn][kSsimIn + 1];
  __shared__ float mid[5][kSsimTile][kSsimIn + 1];   // x, y, x*x, y*y, x*y filtered along axis 0
  __shared__ double red[kSsimThreads / kWave];
  const int pair = blockIdx.z, t = threadIdx.x;
  const int r0 = blockIdx.y * kSsimTile, c0 = blockIdx.x * kSsimTile;
  const int64_t plane = static_cast<int64_t>(H) * W;
  const float* x = x_all + pair * plane;
  const float* y = y_all + pair * plane;
  for (int e = t; e < kSsimIn * kSsimIn; e += kSsimThreads) {
    const int i = e / kSsimIn, j = e - i * kSsimIn;
    const int64_t at = static_cast<int64_t>(reflect_index(r0 - kSsimR + i, H)) * W + reflect_index(c0 - kSsimR + j, W);
    sx[i][j] = x[at];
    sy[i][j] = y[at];
  }
  __syncthreads();
  // axis 0: scipy's correlate1d, symmetric branch: centre * w[5], then (in[i+j] + in[i-j]) * w[j+5] for j = -5 .. -1
  for (int e = t; e < kSsimTile * kSsimIn; e += kSsimThreads) {
    const int i = e / kSsimIn, j = e - i * kSsimIn;
    const float xc = sx[i + kSsimR][j], yc = sy[i + kSsimR][j];
    double ax = double(xc) * wt.w[kSsimR], ay = double(yc) * wt.w[kSsimR];
    double axx = double(xc * xc) * wt.w[kSsimR], ayy = double(yc * yc) * wt.w[kSsimR], axy = double(xc * yc) * wt.w[kSsimR];
#pragma unroll
    for (int k = 0; k < kSsimR; ++k) {
      const float xa = sx[i + k][j], xb = sx[i + 2 * kSsimR - k][j];
      const float ya = sy[i + k][j], yb = sy[i + 2 * kSsimR - k][j];
      ax += (double(xa) + double(xb)) * wt.w[k];
      ay += (double(ya) + double(yb)) * wt.w[k];
      axx += (double(xa * xa) + double(xb * xb)) * wt.w[k];
      ayy += (double(ya * ya) + double(yb * yb)) * wt.w[k];
      axy += (double(xa * ya) + double(xb * yb)) * wt.w[k];
    }
    mid[0][i][j] = static_cast<float>(ax);
    mid[1][i][j] = static_cast<float>(ay);
    mid[2][i][j] = static_cast<float>(axx);
    mid[3][i][j] = static_cast<float>(ayy);
    mid[4][i][j] = static_cast<float>(axy);
  }
  __syncthreads();
  const float cov_norm = static_cast<float>(121.0 / 120.0);
  double sum = 0.0;
  for (int e = t; e < kSsimTile * kSsimTile; e += kSsimThreads) {
    const int i = e / kSsimTile, j = e - i * kSsimTile;
    const int r = r0 + i, c = c0 + j;
    if (r >= H || c >= W) continue;
    float u[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const float* m = &mid[q][i][j + kSsimR];
      double a = double(m[0]) * wt.w[kSsimR];
#pragma unroll
      for (int k = 0; k < kSsimR; ++k) a += (double(m[k - kSsimR]) + double(m[kSsimR - k])) * wt.w[k];
      u[q] = static_cast<float>(a);
    }
    const float ux = u[0], uy = u[1];
    const float vx = cov_norm * (u[2] - ux * ux);
    const float vy = cov_norm * (u[3] - uy * uy);
    const float vxy = cov_norm * (u[4] - ux * uy);
    const float A1 = 2.f * ux * uy + C1, A2 = 2.f * vxy + C2;
    const float B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    const float S = (A1 * A2) / (B1 * B2);
    if (S_all) S_all[pair * plane + static_cast<int64_t>(r) * W + c] = S;
    if (r >= kSsimR && r < H - kSsimR && c >= kSsimR && c < W - kSsimR) sum += double(S);
  }
  sum = block_sum<kSsimThreads / kWave>(sum, red);
  if (t == 0) partial[(static_cast<int64_t>(pair) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
}

// the tiles of a pair in ascending order, from +0
__global__ __launch_bounds__(kWave) void ssim_mean_kernel(const double* __restrict__ partial, int n, int tiles, double count,
                                                          double* __restrict__ mean) {
  const int pair = blockIdx.x * kWave + threadIdx.x;
  if (pair >= n) return;
  const double* p = partial + static_cast<int64_t>(pair) * tiles;
  double s = 0.0;
  for (int i = 0; i < tiles; ++i) s += p[i];
  mean[pair] = s / count;
}

// ------------------------------------------------------------------------------------------------ K41
constexpr int kTieChunk = 256;                       // sorted positions of a workgroup, one per lane

// the value at sorted position q; an `order` entry outside the row (never written by K8) reads the row's last element
__device__ __forceinline__ float sorted_value(const float* vals, const int32_t* order, int64_t n, int64_t q) {
  const uint32_t i = static_cast<uint32_t>(order[q]);
  return vals[i < n ? i : n - 1];
}

__global__ __launch_bounds__(kTieChunk) void tie_ranks_kernel(const float* __restrict__ vals_all, const int32_t* __restrict__ order_all,
                                                              int64_t n, int32_t* __restrict__ out_all) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kTieChunk + threadIdx.x;
  if (p >= n) return;
  const float* vals = vals_all + blockIdx.y * n;
  const int32_t* order = order_all + blockIdx.y * n;
  const uint32_t idx = static_cast<uint32_t>(order[p]);
  if (idx >= n) return;
  const float v = vals[idx];
  int64_t lo = p, hi = p;
  if (p > 0 && sorted_value(vals, order, n, p - 1) == v) {       // the first position of [0, p) that holds v
    int64_t a = 0, b = p - 1;
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (sorted_value(vals, order, n, m) < v) a = m + 1; else b = m;
    }
    lo = a;
  }
  if (p + 1 < n && sorted_value(vals, order, n, p + 1) == v) {   // the last position of (p, n) that holds v
    int64_t a = p + 1, b = n - 1;
    while (a < b) {
      const int64_t m = (a + b + 1) >> 1;
      if (v < sorted_value(vals, order, n, m)) b = m - 1; else a = m;
    }
    hi = a;
  }
  out_all[blockIdx.y * n + idx] = static_cast<int32_t>(lo + hi + 2);
}

// ------------------------------------------------------------------------------------------------ K42
constexpr int kCorrThreads = 1024;
constexpr int kCorrWaves = kCorrThreads / kWave;
constexpr int64_t kCorrMaxN = 131072;                // every int64 sum below stays under 2^51

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__global__ __launch_bounds__(kCorrThreads) void rank_corr_kernel(const int32_t* __restrict__ ra_all, const int32_t* __restrict__ rb_all,
                                                                 const float* __restrict__ a_all, const float* __restrict__ b_all,
                                                                 int64_t n, double* __restrict__ out) {
  __shared__ long long red[3][kCorrWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * n;
  const int32_t* ra = ra_all + base;
  const int32_t* rb = rb_all + base;
  const long long mid = n + 1;                       // twice the mean rank
  long long saa = 0, sbb = 0, sab = 0;
  int nan = 0;
  for (int64_t i = threadIdx.x; i < n; i += kCorrThreads) {
    const long long da = ra[i] - mid, db = rb[i] - mid;
    saa += da * da; sbb += db * db; sab += da * db;
    if (a_all) { const float v = a_all[base + i]; nan |= v != v; }
    if (b_all) { const float v = b_all[base + i]; nan |= v != v; }
  }
  saa = wave_sum_i64(saa); sbb = wave_sum_i64(sbb); sab = wave_sum_i64(sab);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[0][threadIdx.x / kWave] = saa; red[1][threadIdx.x / kWave] = sbb; red[2][threadIdx.x / kWave] = sab;
  }
  nan = __syncthreads_or(nan);
  if (threadIdx.x != 0) return;
  saa = sbb = sab = 0;
  for (int w = 0; w < kCorrWaves; ++w) { saa += red[0][w]; sbb += red[1][w]; sab += red[2][w]; }
  // numpy.corrcoef: cov = dot(X, X.T) * (1 / (n - 1)) on rank deviations (ours are doubled: / 4), c /= stddev[:, None], c /= stddev[None, :]
  const double inv = 1.0 / static_cast<double>(n - 1);
  const double caa = (static_cast<double>(saa) / 4.0) * inv;
  const double cbb = (static_cast<double>(sbb) / 4.0) * inv;
  const double cab = (static_cast<double>(sab) / 4.0) * inv;
  double r = (cab / sqrt(cbb)) / sqrt(caa);
  if (r > 1.0) r = 1.0;                              // np.clip: a NaN stays
  if (r < -1.0) r = -1.0;
  out[blockIdx.x] = nan ? static_cast<double>(NAN) : r;
}

// ------------------------------------------------------------------------------------------------ K43
constexpr int kHogThreads = 256;
constexpr int kHogBins = 9;
constexpr int kHogBlock = 3;                         // cells per block along each axis
constexpr int kHogFeat = kHogBlock * kHogBlock * kHogBins;

// grid = (cells along W, cells along H, maps)
__global__ __launch_bounds__(kHogThreads) void hog_cells_kernel(const float* __restrict__ img_all, int H, int W, int ch, int cw,
                                                                double* __restrict__ hist) {
  __shared__ double red[kHogThreads / kWave];
  const float* img = img_all + static_cast<int64_t>(blockIdx.z) * H * W;
  const int r_first = blockIdx.y * ch, c_first = blockIdx.x * cw;
  double acc[kHogBins];
#pragma unroll
  for (int i = 0; i < kHogBins; ++i) acc[i] = 0.0;
  for (int p = threadIdx.x; p < ch * cw; p += kHogThreads) {
    const int r = r_first + p / cw, c = c_first + p % cw;
    const int64_t at = static_cast<int64_t>(r) * W + c;
    const float g_row = (r > 0 && r < H - 1) ? img[at + W] - img[at - W] : 0.f;
    const float g_col = (c > 0 && c < W - 1) ? img[at + 1] - img[at - 1] : 0.f;
    const double mag = hypot(static_cast<double>(g_col), static_cast<double>(g_row));
    const double deg = atan2(static_cast<double>(g_row), static_cast<double>(g_col)) * (180.0 / 3.141592653589793);
    double m = fmod(deg, 180.0);                     // Python's %: the sign of the divisor, and +0 for a zero remainder
    if (m != 0.0) { if (m < 0.0) m += 180.0; } else m = 0.0;
#pragma unroll
    for (int i = 0; i < kHogBins; ++i) acc[i] += (m >= 20.0 * i && m < 20.0 * (i + 1)) ? mag : 0.0;
  }
  const double area = static_cast<double>(ch) * cw;
  double* h = hist + ((static_cast<int64_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kHogBins;
#pragma unroll
  for (int i = 0; i < kHogBins; ++i) {
    const double s = block_sum<kHogThreads / kWave>(acc[i], red);
    if (threadIdx.x == 0) h[i] = s / area;
  }
}

// np.minimum(v, 0.2): a NaN stays
__device__ __forceinline__ double hys_clip(double v) { return v > 0.2 ? 0.2 : v; }

// grid = (blocks along W, blocks along H, maps), one wave: lane e and lane e + 64 hold elements e of the block's 81
__global__ __launch_bounds__(kWave) void hog_blocks_kernel(const double* __restrict__ hist, int cells_r, int cells_c,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x;
  const double* h = hist + static_cast<int64_t>(blockIdx.z) * cells_r * cells_c * kHogBins;
  double b[2];
  bool live[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int e = lane + k * kWave;
    live[k] = e < kHogFeat;
    const int cy = e / (kHogBlock * kHogBins), cx = (e / kHogBins) % kHogBlock, o = e % kHogBins;
    b[k] = live[k] ? h[(static_cast<int64_t>(blockIdx.y + cy) * cells_c + blockIdx.x + cx) * kHogBins + o] : 0.0;
  }
  const double n1 = sqrt(wave_sum(b[0] * b[0] + b[1] * b[1]) + 1e-10);
  b[0] = hys_clip(b[0] / n1);
  b[1] = hys_clip(b[1] / n1);
  const double n2 = sqrt(wave_sum(b[0] * b[0] + b[1] * b[1]) + 1e-10);
  float* o = out + ((static_cast<int64_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kHogFeat;
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (live[k]) o[lane + k * kWave] = static_cast<float>(b[k] / n2);
}

inline int ssim_tiles(int extent) { return (extent + kSsimTile - 1) / kSsimTile; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

XAI_EXPORT int xai_sanity_normalize_f32(const float* x, int n, int64_t hw, int guard, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n > 0 && hw > 0, XAI_E_SHAPE);
  const bool vec = xai_can_vec4(hw, {x, out});
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(sanity_normalize_kernel<V4 ? 4 : 1>, dim3(static_cast<unsigned>(n)), dim3(kNormThreads), 0, st, x, hw,
                       guard != 0 ? 1 : 0, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_ssim_tile(void) { return kSsimTile; }

XAI_EXPORT int xai_ssim_workspace_bytes(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t bytes = static_cast<int64_t>(n) * ssim_tiles(H) * ssim_tiles(W) * static_cast<int64_t>(sizeof(double));
  return bytes <= INT32_MAX ? static_cast<int>(bytes) : 0;
}

XAI_EXPORT int xai_ssim_f32(const float* x, const float* y, int n, int H, int W, double w0, double w1, double w2, double w3, double w4,
                            double w5, float C1, float C2, double* mean, float* S, void* ws, size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(y); XAI_REQUIRE_PTR(mean); XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE(n > 0 && H >= 2 * kSsimR + 1 && W >= 2 * kSsimR + 1, XAI_E_SHAPE);
  const int need = xai_ssim_workspace_bytes(n, H, W);
  XAI_REQUIRE(need > 0 && n <= 65535 && ssim_tiles(H) <= 65535, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= static_cast<size_t>(need) && aligned8(ws), XAI_E_SHAPE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SsimWeights wt{{w0, w1, w2, w3, w4, w5}};
  const dim3 grid(static_cast<unsigned>(ssim_tiles(W)), static_cast<unsigned>(ssim_tiles(H)), static_cast<unsigned>(n));
  double* partial = static_cast<double*>(ws);
  hipLaunchKernelGGL(ssim_tile_kernel, grid, dim3(kSsimThreads), 0, st, x, y, H, W, wt, C1, C2, S, partial);
  const double count = static_cast<double>(H - 2 * kSsimR) * static_cast<double>(W - 2 * kSsimR);
  hipLaunchKernelGGL(ssim_mean_kernel, dim3(static_cast<unsigned>(xai_ceil_div(n, kWave))), dim3(kWave), 0, st, partial, n,
                     ssim_tiles(H) * ssim_tiles(W), count, mean);
  return xai_launch_status();
}

XAI_EXPORT int xai_tie_ranks_chunk(void) { return kTieChunk; }

XAI_EXPORT int xai_tie_ranks_i32(const float* vals, const int32_t* order, int n_rows, int64_t n, int32_t* ranks2, xai_stream_t stream) {
  XAI_REQUIRE_PTR(vals); XAI_REQUIRE_PTR(order); XAI_REQUIRE_PTR(ranks2);
  XAI_REQUIRE(n_rows > 0 && n > 0, XAI_E_SHAPE);
  XAI_REQUIRE(n <= (int64_t(1) << 30) && n_rows <= 65535, XAI_E_UNSUPPORTED);
  const dim3 grid(static_cast<unsigned>(xai_ceil_div(n, kTieChunk)), static_cast<unsigned>(n_rows));
  hipLaunchKernelGGL(tie_ranks_kernel, grid, dim3(kTieChunk), 0, static_cast<hipStream_t>(stream), vals, order, n, ranks2);
  return xai_launch_status();
}

XAI_EXPORT int xai_rank_corr_max_n(void) { return static_cast<int>(kCorrMaxN); }

XAI_EXPORT int xai_rank_corr_f64(const int32_t* ra, const int32_t* rb, const float* a, const float* b, int n_pairs, int64_t n,
                                 double* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(ra); XAI_REQUIRE_PTR(rb); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n_pairs > 0 && n >= 2, XAI_E_SHAPE);
  XAI_REQUIRE(n <= kCorrMaxN, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(rank_corr_kernel, dim3(static_cast<unsigned>(n_pairs)), dim3(kCorrThreads), 0, static_cast<hipStream_t>(stream),
                     ra, rb, a, b, n, out);
  return xai_launch_status();
}

XAI_EXPORT int xai_hog_workspace_bytes(int n, int H, int W, int ch, int cw) {
  if (n <= 0 || H <= 0 || W <= 0 || ch <= 0 || cw <= 0) return 0;
  const int64_t bytes = static_cast<int64_t>(n) * (H / ch) * (W / cw) * kHogBins * static_cast<int64_t>(sizeof(double));
  return bytes <= INT32_MAX ? static_cast<int>(bytes) : 0;
}

XAI_EXPORT int xai_hog_f32(const float* img, int n, int H, int W, int ch, int cw, float* out, void* ws, size_t ws_bytes,
                           xai_stream_t stream) {
  XAI_REQUIRE_PTR(img); XAI_REQUIRE_PTR(out); XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE(n > 0 && H > 0 && W > 0 && ch > 0 && cw > 0, XAI_E_SHAPE);
  const int cells_r = H / ch, cells_c = W / cw;
  XAI_REQUIRE(cells_r >= kHogBlock && cells_c >= kHogBlock, XAI_E_SHAPE);
  const int need = xai_hog_workspace_bytes(n, H, W, ch, cw);
  XAI_REQUIRE(need > 0 && n <= 65535 && cells_r <= 65535 && static_cast<int64_t>(ch) * cw <= INT32_MAX, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= static_cast<size_t>(need) && aligned8(ws), XAI_E_SHAPE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* hist = static_cast<double*>(ws);
  hipLaunchKernelGGL(hog_cells_kernel, dim3(static_cast<unsigned>(cells_c), static_cast<unsigned>(cells_r), static_cast<unsigned>(n)),
                     dim3(kHogThreads), 0, st, img, H, W, ch, cw, hist);
  hipLaunchKernelGGL(hog_blocks_kernel, dim3(static_cast<unsigned>(cells_c - kHogBlock + 1), static_cast<unsigned>(cells_r - kHogBlock + 1),
                                             static_cast<unsigned>(n)),
                     dim3(kWave), 0, st, hist, cells_r, cells_c, out);
  return xai_launch_status();
}
