// K44-K45: the per-image scoring of the ImageNet-segmentation evaluation (evaluateImageNetSeg.py:215-217, :332-334, :463-465 and
// eval_batch :470-507 with utils/metrices.py) for gfx950.  Part of libxai_ext3.so (include/xai_hip_ext3.h).
//
// The reference normalises every attribution map on the host, thresholds it at its mean and hands the two masks to sklearn.  All
// four scores are functions of a small integer table: per image row, label (0 / 1) and prediction state (<= thr, > thr, neither),
// the number of pixels.  Here a batch of maps stays on the device and is scored by:
//   K44 normalize   one workgroup of 1024 lanes per map: min / max with torch's NaN rule, (x - mn) / (mx - mn) in fp32, and the
//                   fp64 sum of the written values in one fixed tree (xai_hip_ext3.h states it) for the mean threshold
//   K45 counts      one wave per image row: a lane holds up to 4 pixels and their labels in registers (256 pixels of the row per
//                   pass: W = 224 is one pass of 3.5 waves' worth, the missing half wave is masked), and for every threshold the six
//                   cells of the row are wave ballots counted by the scalar unit; lanes 0-5 store them as one 24-byte row.  A row
//                   wider than 256 pixels takes more passes, the same wave adding to the cells it wrote itself.  A second launch
//                   of one workgroup per map counts the labels that are neither 0 nor 1.
// Every cell has exactly one owner: no atomics, no memset, the same bytes on every run.  Capturable: nothing is allocated.
#include "xai_common.h"
#include "xai_hip_ext3.h"

#include <math.h>

// the version pair of libxai_ext3.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext3_version, XAI_EXT3_VERSION, XAI_EXT3_MINOR)

namespace {

constexpr int64_t kSegMaxHw = int64_t(1) << 30;
constexpr int kSegMaxThresholds = 16;

// ------------------------------------------------------------------------------------------------ K44
constexpr int kSegThreads = 1024;
constexpr int kSegWaves = kSegThreads / kWave;
constexpr int kSegQuad = 4;                          // consecutive elements of one lane: the unit of the stated sum tree

// the up to four elements x[i .. i + 4) that lie below hw -> how many there are
template <bool VEC>
__device__ __forceinline__ int load_quad(const float* x, int64_t i, int64_t hw, float (&v)[kSegQuad]) {
  if constexpr (VEC) {
    const float4 t = ld4(x + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    return kSegQuad;
  } else {
    const int live = static_cast<int>(hw - i < kSegQuad ? hw - i : kSegQuad);
#pragma unroll
    for (int k = 0; k < kSegQuad; ++k) v[k] = k < live ? x[i + k] : 0.f;
    return live;
  }
}

// x and out may be the same array: a lane reads only the elements it writes, and the barriers of the reductions lie between
// its last read of pass 1 and its first write
template <bool VEC>
__global__ __launch_bounds__(kSegThreads) void seg_normalize_kernel(const float* x_all, int64_t hw, float* out_all,
                                                                    float* __restrict__ thr, float* __restrict__ stats) {
  __shared__ float red[2 * kSegWaves];
  __shared__ double dred[kSegWaves];
  const float* x = x_all + static_cast<int64_t>(blockIdx.x) * hw;
  float* out = out_all + static_cast<int64_t>(blockIdx.x) * hw;
  const int64_t first = static_cast<int64_t>(threadIdx.x) * kSegQuad, stride = static_cast<int64_t>(kSegThreads) * kSegQuad;
  float lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  for (int64_t i = first; i < hw; i += stride) {
    float v[kSegQuad];
    const int live = load_quad<VEC>(x, i, hw, v);
#pragma unroll
    for (int k = 0; k < kSegQuad; ++k)
      if (k < live) {
        nan |= v[k] != v[k];
        lo = fminf(lo, v[k]); hi = fmaxf(hi, v[k]);
      }
  }
  block_min_max<kSegWaves>(lo, hi, red);
  if (__syncthreads_or(nan)) lo = hi = NAN;          // torch: one NaN makes min and max NaN
  const float den = hi - lo;
  double s = 0.0;
  for (int64_t i = first; i < hw; i += stride) {
    float v[kSegQuad];
    const int live = load_quad<VEC>(x, i, hw, v);
#pragma unroll
    for (int k = 0; k < kSegQuad; ++k) {
      v[k] = (v[k] - lo) / den;
      if (k < live) s += static_cast<double>(v[k]);
    }
    if constexpr (VEC) {
      st4(out + i, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
      for (int k = 0; k < kSegQuad; ++k)
        if (k < live) out[i + k] = v[k];
    }
  }
  s = block_sum<kSegWaves>(s, dred);
  if (threadIdx.x == 0) {
    thr[blockIdx.x] = static_cast<float>(s / static_cast<double>(hw));
    stats[2 * blockIdx.x] = lo;
    stats[2 * blockIdx.x + 1] = hi;
  }
}

// ------------------------------------------------------------------------------------------------ K45
constexpr int kCntThreads = 256;
constexpr int kCntRows = kCntThreads / kWave;        // image rows of a workgroup, one wave each
constexpr int kCntPix = 4;                           // pixels a lane holds per pass
constexpr int kCntCells = 6;                         // [label 0 / 1][<= thr, > thr, neither]

__device__ __forceinline__ int ballot_count(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(kCntThreads) void seg_counts_kernel(const float* __restrict__ res, const int32_t* __restrict__ labels,
                                                                 const float* __restrict__ thr, int H, int W, int T,
                                                                 int32_t* __restrict__ counts) {
  const int m = blockIdx.y, lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * kCntRows + threadIdx.x / kWave;
  if (r >= H) return;                                // the whole wave leaves; the kernel has no barrier
  const int64_t row = (static_cast<int64_t>(m) * H + r) * W;
  const float* thr_m = thr + static_cast<int64_t>(m) * T;
  for (int c0 = 0; c0 < W; c0 += kCntPix * kWave) {
    float v[kCntPix];
    int l[kCntPix];
#pragma unroll
    for (int k = 0; k < kCntPix; ++k) {
      const int c = c0 + k * kWave + lane;
      const bool live = c < W;
      v[k] = live ? res[row + c] : 0.f;
      l[k] = live ? labels[row + c] : -1;            // past the row's end: a label that enters no cell
    }
    for (int t = 0; t < T; ++t) {
      const float th = thr_m[t];
      int cnt[kCntCells] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < kCntPix; ++k) {
        const bool le = v[k] <= th, gt = v[k] > th, ne = !(le || gt);
        const bool l0 = l[k] == 0, l1 = l[k] == 1;
        cnt[0] += ballot_count(l0 && le); cnt[1] += ballot_count(l0 && gt); cnt[2] += ballot_count(l0 && ne);
        cnt[3] += ballot_count(l1 && le); cnt[4] += ballot_count(l1 && gt); cnt[5] += ballot_count(l1 && ne);
      }
      int mine = cnt[0];
#pragma unroll
      for (int j = 1; j < kCntCells; ++j) mine = lane == j ? cnt[j] : mine;
      int32_t* cell = counts + ((static_cast<int64_t>(m) * T + t) * H + r) * kCntCells;
      if (lane < kCntCells) cell[lane] = c0 == 0 ? mine : cell[lane] + mine;
    }
  }
}

__global__ __launch_bounds__(kSegThreads) void seg_other_kernel(const int32_t* __restrict__ labels, int64_t hw,
                                                                int32_t* __restrict__ other) {
  __shared__ int part[kSegWaves];
  const int32_t* lab = labels + static_cast<int64_t>(blockIdx.x) * hw;
  int c = 0;
  for (int64_t i = threadIdx.x; i < hw; i += kSegThreads) {
    const int32_t l = lab[i];
    c += (l != 0 && l != 1) ? 1 : 0;
  }
  c = wave_sum(c);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kSegWaves; ++w) s += part[w];
    other[blockIdx.x] = s;
  }
}

}  // namespace

XAI_EXPORT int xai_seg_max_hw(void) { return static_cast<int>(kSegMaxHw); }
XAI_EXPORT int xai_seg_max_thresholds(void) { return kSegMaxThresholds; }

XAI_EXPORT int xai_seg_normalize_f32(const float* x, int n, int64_t hw, float* out, float* thr, float* stats, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(out); XAI_REQUIRE_PTR(thr); XAI_REQUIRE_PTR(stats);
  XAI_REQUIRE(n > 0 && hw > 0, XAI_E_SHAPE);
  XAI_REQUIRE(hw <= kSegMaxHw, XAI_E_UNSUPPORTED);
  const bool vec = xai_can_vec4(hw, {x, out});
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(seg_normalize_kernel<V4>, dim3(static_cast<unsigned>(n)), dim3(kSegThreads), 0, st, x, hw, out, thr, stats);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_seg_counts_i32(const float* res, const int32_t* labels, const float* thr, int n, int H, int W, int T,
                                  int32_t* counts, int32_t* other, xai_stream_t stream) {
  XAI_REQUIRE_PTR(res); XAI_REQUIRE_PTR(labels); XAI_REQUIRE_PTR(thr); XAI_REQUIRE_PTR(counts); XAI_REQUIRE_PTR(other);
  XAI_REQUIRE(n > 0 && H > 0 && W > 0 && T > 0, XAI_E_SHAPE);
  const int64_t hw = static_cast<int64_t>(H) * W;
  XAI_REQUIRE(T <= kSegMaxThresholds && n <= 65535 && hw <= kSegMaxHw, XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(seg_counts_kernel, dim3(static_cast<unsigned>(xai_ceil_div(H, kCntRows)), static_cast<unsigned>(n)),
                     dim3(kCntThreads), 0, st, res, labels, thr, H, W, T, counts);
  const int status = xai_launch_status();
  if (status != XAI_OK) return status;
  hipLaunchKernelGGL(seg_other_kernel, dim3(static_cast<unsigned>(n)), dim3(kSegThreads), 0, st, labels, hw, other);
  return xai_launch_status();
}
