// K53-K55: quickshift superpixels as scikit-image 0.18.3 computes them (skimage/segmentation/_quickshift_cy.pyx) for gfx950.  Part of
// libxai_ext5.so (include/xai_hip_ext5.h, which states every expression, the scan order and the cap).
//
// skimage walks the pixels one after the other on one host thread: per pixel a (2 kw + 1)^2 window of fp64 exp for the density, the
// same window again for the nearest denser neighbour, then a pointer-doubling loop and np.unique.  Here
//   K53 density   one lane per pixel, the window in skimage's scan order, the features of the tile plus halo staged in LDS
//   K54 parent    the same walk over the denser neighbours; the squared distance is K53's sum bit for bit
//   K55 labels    every pixel follows `parent` to its root; an exclusive prefix sum of the root flags numbers the roots in pixel
//                 order (one workgroup per image); labels[i] = scan[root[i]]
// Every output element has one owner: no atomics, nothing to zero beforehand, the same bytes on every run.  Capturable: nothing is
// allocated.
#include "xai_common.h"
#include "xai_hip_ext5.h"

#include <float.h>
#include <math.h>

// the version pair of libxai_ext5.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext5_version, XAI_EXT5_VERSION, XAI_EXT5_MINOR)

namespace {

constexpr int kQsTile = 16;            // a workgroup is a kQsTile x kQsTile block of pixels, one lane each
constexpr size_t kQsLdsCap = 65536;
constexpr double kQsMaxKernelSize = 10000.0;
constexpr int kQsThreads = 256;     // K55's element-wise launches
constexpr int kQsScanThreads = 1024;  // K55's one workgroup per image

// The tile plus halo of one workgroup: plane ch of `lds` is [TW][TW] doubles, TW = kQsTile + 2 kw, origin at pixel (r0, c0) of the image.
// Cells outside the image are never read by a window (it is clipped to the image); they are set to 0.
__device__ __forceinline__ void stage_tile(const double* __restrict__ f, int H, int W, int C, int kw, int r0, int c0, double* lds) {
  const int TW = kQsTile + 2 * kw;
  const int cells = TW * TW * C;
  for (int idx = threadIdx.x; idx < cells; idx += kQsTile * kQsTile) {
    const int ch = idx % C, p = idx / C, tc = p % TW, tr = p / TW;   // ch fastest: consecutive lanes read consecutive doubles
    const int r = r0 + tr, c = c0 + tc;
    double v = 0.0;
    if (r >= 0 && r < H && c >= 0 && c < W) v = f[(static_cast<int64_t>(r) * W + c) * C + ch];
    lds[(ch * TW + tr) * TW + tc] = v;
  }
}

// d of the header: channels ascending from +0, then the row term, then the column term; each product and each sum rounded once.
// own / other: the two pixels' cells of plane 0; plane: doubles from one plane to the next.
__device__ __forceinline__ double qs_dist(const double* own, const double* other, int C, int plane, int dr, int dc) {
  double d = 0.0;
  for (int ch = 0; ch < C; ++ch) {
    const double t = own[ch * plane] - other[ch * plane];
    d += t * t;
  }
  double t = static_cast<double>(dr);
  d += t * t;
  t = static_cast<double>(dc);
  d += t * t;
  return d;
}

struct QsWindow {
  int r, c, r_min, r_max, c_min, c_max;
};

__device__ __forceinline__ bool qs_window(int H, int W, int kw, QsWindow* w) {
  w->r = blockIdx.y * kQsTile + threadIdx.x / kQsTile;
  w->c = blockIdx.x * kQsTile + threadIdx.x % kQsTile;
  if (w->r >= H || w->c >= W) return false;
  w->r_min = max(w->r - kw, 0);
  w->r_max = min(w->r + kw + 1, H);
  w->c_min = max(w->c - kw, 0);
  w->c_max = min(w->c + kw + 1, W);
  return true;
}

// ------------------------------------------------------------------------------------------------ K53
__global__ __launch_bounds__(kQsTile * kQsTile) void density_kernel(const double* __restrict__ features, const double* __restrict__ noise, int H,
                                                        int W, int C, int kw, double inv, double* __restrict__ dens) {
  extern __shared__ double lds[];
  const int TW = kQsTile + 2 * kw, plane = TW * TW;
  const int r0 = blockIdx.y * kQsTile - kw, c0 = blockIdx.x * kQsTile - kw;
  const int64_t n = static_cast<int64_t>(H) * W;
  stage_tile(features + blockIdx.z * n * C, H, W, C, kw, r0, c0, lds);
  __syncthreads();
  QsWindow w;
  if (!qs_window(H, W, kw, &w)) return;
  const double* own = lds + (w.r - r0) * TW + (w.c - c0);
  double sum = 0.0;
  for (int r_ = w.r_min; r_ < w.r_max; ++r_) {
    const int row = (r_ - r0) * TW - c0;          // row + c_ >= 0: the cell of pixel (r_, c_) in plane 0
    for (int c_ = w.c_min; c_ < w.c_max; ++c_) sum += exp(qs_dist(own, lds + (row + c_), C, plane, w.r - r_, w.c - c_) * inv);
  }
  const int64_t i = blockIdx.z * n + static_cast<int64_t>(w.r) * W + w.c;
  dens[i] = sum + noise[i];
}

// ------------------------------------------------------------------------------------------------ K54
__global__ __launch_bounds__(kQsTile * kQsTile) void parent_kernel(const double* __restrict__ features, const double* __restrict__ dens, int H, int W,
                                                       int C, int kw, double max_dist, int32_t* __restrict__ parent,
                                                       int32_t* __restrict__ tree, double* __restrict__ closest_out,
                                                       double* __restrict__ dist_out) {
  extern __shared__ double lds[];
  const int TW = kQsTile + 2 * kw, plane = TW * TW;
  const int r0 = blockIdx.y * kQsTile - kw, c0 = blockIdx.x * kQsTile - kw;
  const int64_t n = static_cast<int64_t>(H) * W;
  stage_tile(features + blockIdx.z * n * C, H, W, C, kw, r0, c0, lds);
  __syncthreads();
  QsWindow w;
  if (!qs_window(H, W, kw, &w)) return;
  const double* own = lds + (w.r - r0) * TW + (w.c - c0);
  const double* dimg = dens + blockIdx.z * n;
  const int self = w.r * W + w.c;
  const double current = dimg[self];
  double closest = DBL_MAX;
  int best = self;
  for (int r_ = w.r_min; r_ < w.r_max; ++r_) {
    const int row = (r_ - r0) * TW - c0;          // row + c_ >= 0: the cell of pixel (r_, c_) in plane 0
    const double* drow = dimg + static_cast<int64_t>(r_) * W;
    for (int c_ = w.c_min; c_ < w.c_max; ++c_) {
      if (drow[c_] > current) {                 // false for a NaN on either side
        const double d = qs_dist(own, lds + (row + c_), C, plane, w.r - r_, w.c - c_);
        if (d < closest) {                      // strict: the first in scan order keeps an exact tie
          closest = d;
          best = r_ * W + c_;
        }
      }
    }
  }
  const double dist = __dsqrt_rn(closest);
  const int64_t i = blockIdx.z * n + self;
  if (tree) tree[i] = best;
  parent[i] = dist > max_dist ? self : best;
  closest_out[i] = closest;
  dist_out[i] = dist;
}

// ------------------------------------------------------------------------------------------------ K55
__global__ __launch_bounds__(kQsThreads) void roots_kernel(const int32_t* __restrict__ parent, int n, int32_t* __restrict__ root) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kQsThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t* par = parent + static_cast<int64_t>(blockIdx.y) * n;
  int j = static_cast<int>(i);
  for (int step = 0; step < n; ++step) {        // a chain of distinct pixels has at most n - 1 links: a cycle ends here too
    const int p = par[j];
    if (p == j || p < 0 || p >= n) break;
    j = p;
  }
  root[static_cast<int64_t>(blockIdx.y) * n + i] = j;
}

__global__ __launch_bounds__(kQsScanThreads) void scan_kernel(const int32_t* __restrict__ root, int n, int32_t* __restrict__ scan,
                                                              int32_t* __restrict__ D) {
  __shared__ uint32_t wsum[kQsScanThreads / kWave];
  const int t = threadIdx.x;
  const int32_t* rt = root + static_cast<int64_t>(blockIdx.x) * n;
  int32_t* sc = scan + static_cast<int64_t>(blockIdx.x) * n;
  uint32_t carry = 0;
  for (int64_t base = 0; base < n; base += kQsScanThreads) {
    const int64_t i = base + t;
    const uint32_t flag = (i < n && rt[i] == static_cast<int32_t>(i)) ? 1u : 0u;
    const uint32_t below = block_scan_excl<kQsScanThreads>(flag, carry, wsum);
    if (i < n) sc[i] = static_cast<int32_t>(below);
    __syncthreads();
  }
  if (t == 0) D[blockIdx.x] = static_cast<int32_t>(carry);
}

__global__ __launch_bounds__(kQsThreads) void relabel_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ scan, int n,
                                                             int32_t* __restrict__ labels) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kQsThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t at = static_cast<int64_t>(blockIdx.y) * n;
  labels[at + i] = scan[at + root[at + i]];
}

// ------------------------------------------------------------------------------------------------ host side
// The checks K53 and K54 share, in the header's order -> XAI_OK and (*kw, *lds_bytes), or the refusal.
int qs_check(int B, int H, int W, int C, double kernel_size, int* kw, size_t* lds_bytes) {
  XAI_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, XAI_E_SHAPE);
  const size_t bytes = xai_quickshift_lds_bytes(C, kernel_size);
  XAI_REQUIRE(bytes != 0, XAI_E_SHAPE);
  XAI_REQUIRE(bytes <= kQsLdsCap, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(B <= 65535 && static_cast<int64_t>(H) * W <= INT32_MAX && xai_ceil_div(H, kQsTile) <= 65535, XAI_E_UNSUPPORTED);
  *kw = static_cast<int>(ceil(3.0 * kernel_size));
  *lds_bytes = bytes;
  return XAI_OK;
}

int qs_shape(int B, int H, int W) {
  XAI_REQUIRE(B > 0 && H > 0 && W > 0, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && static_cast<int64_t>(H) * W <= INT32_MAX, XAI_E_UNSUPPORTED);
  return XAI_OK;
}

}  // namespace

XAI_EXPORT size_t xai_quickshift_lds_bytes(int C, double kernel_size) {
  if (C <= 0 || !(kernel_size >= 1.0)) return 0;
  if (kernel_size > kQsMaxKernelSize) return SIZE_MAX;
  const size_t side = static_cast<size_t>(kQsTile) + 2 * static_cast<size_t>(ceil(3.0 * kernel_size));
  return side * side * static_cast<size_t>(C) * sizeof(double);
}

XAI_EXPORT int xai_quickshift_density_f64(const double* features, const double* noise, int B, int H, int W, int C, double kernel_size,
                                          double* dens, xai_stream_t stream) {
  XAI_REQUIRE_PTR(features);
  XAI_REQUIRE_PTR(noise);
  XAI_REQUIRE_PTR(dens);
  int kw;
  size_t lds;
  const int rc = qs_check(B, H, W, C, kernel_size, &kw, &lds);
  if (rc != XAI_OK) return rc;
  const double inv = -0.5 / (kernel_size * kernel_size);
  const dim3 grid(unsigned(xai_ceil_div(W, kQsTile)), unsigned(xai_ceil_div(H, kQsTile)), unsigned(B));
  hipStream_t s = static_cast<hipStream_t>(stream);
  density_kernel<<<grid, kQsTile * kQsTile, lds, s>>>(features, noise, H, W, C, kw, inv, dens);
  return xai_launch_status();
}

XAI_EXPORT int xai_quickshift_parent_f64(const double* features, const double* dens, int B, int H, int W, int C, double kernel_size,
                                         double max_dist, int32_t* parent, int32_t* tree, double* closest, double* dist,
                                         xai_stream_t stream) {
  XAI_REQUIRE_PTR(features);
  XAI_REQUIRE_PTR(dens);
  XAI_REQUIRE_PTR(parent);
  XAI_REQUIRE_PTR(closest);
  XAI_REQUIRE_PTR(dist);
  int kw;
  size_t lds;
  const int rc = qs_check(B, H, W, C, kernel_size, &kw, &lds);
  if (rc != XAI_OK) return rc;
  const dim3 grid(unsigned(xai_ceil_div(W, kQsTile)), unsigned(xai_ceil_div(H, kQsTile)), unsigned(B));
  hipStream_t s = static_cast<hipStream_t>(stream);
  parent_kernel<<<grid, kQsTile * kQsTile, lds, s>>>(features, dens, H, W, C, kw, max_dist, parent, tree, closest, dist);
  return xai_launch_status();
}

XAI_EXPORT size_t xai_quickshift_workspace_bytes(int B, int H, int W) {
  if (qs_shape(B, H, W) != XAI_OK) return 0;
  return static_cast<size_t>(B) * static_cast<size_t>(H) * static_cast<size_t>(W) * 2 * sizeof(int32_t);
}

XAI_EXPORT int xai_quickshift_labels_i32(const int32_t* parent, int B, int H, int W, int32_t* labels, int32_t* D, void* ws,
                                         size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(parent);
  XAI_REQUIRE_PTR(labels);
  XAI_REQUIRE_PTR(D);
  XAI_REQUIRE_PTR(ws);
  const int rc = qs_shape(B, H, W);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(ws_bytes >= xai_quickshift_workspace_bytes(B, H, W) && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, XAI_E_SHAPE);
  const int n = H * W;
  int32_t* root = static_cast<int32_t*>(ws);
  int32_t* scan = root + static_cast<size_t>(B) * n;
  const dim3 grid(unsigned(xai_ceil_div(n, kQsThreads)), unsigned(B));
  hipStream_t s = static_cast<hipStream_t>(stream);
  roots_kernel<<<grid, kQsThreads, 0, s>>>(parent, n, root);
  int st = xai_launch_status();
  if (st != XAI_OK) return st;
  scan_kernel<<<unsigned(B), kQsScanThreads, 0, s>>>(root, n, scan, D);
  st = xai_launch_status();
  if (st != XAI_OK) return st;
  relabel_kernel<<<grid, kQsThreads, 0, s>>>(root, scan, n, labels);
  return xai_launch_status();
}
