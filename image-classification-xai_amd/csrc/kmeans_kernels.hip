// K58-K61: the Euclidean Lloyd iteration of TIS's k-means (TIS.py:150-155, xai_engine/tis.py kmeans_centroids) for gfx950, in a stated
// arithmetic order.  Part of libxai_ext7.so (include/xai_hip_ext7.h, which states the contract: every sum from +0, sequential in
// ascending index, one accumulator per result, products and sums rounded separately).
//
//   K58 norms     xx_i once, one lane per point; then C = X[first] and cc_j, one workgroup per centroid
//   K59 assign    one workgroup of 8 waves per 32 points.  The centroids stream through LDS 256 at a time, the features 32 at a time,
//                 the global loads of the next tile in flight while this one is computed on; a lane keeps a 4 x 4 register tile of
//                 (point, centroid) dot products, 16 independent sequential chains over t, and a running (best score, best index)
//                 per point; the 64 lanes of the wave that shares 4 points merge by (score, lower index).  The score matrix never
//                 exists in memory.  No MFMA: its summation order cannot be stated.
//   K60 update    one workgroup per centroid, one lane per feature.  The workgroup turns the assignments into one bit per point (a
//                 ballot per 64), then every lane walks the set bits in ascending i and adds its feature of row i.  The same
//                 workgroup divides, replaces NaN by +0, writes the new row over the old one (no other workgroup reads row j here),
//                 and one lane sums e_j (fp64) and the next iteration's cc_j in ascending t.
//   K61 finish    one workgroup: err = the e_j in ascending j (fp64), the iteration counter, the `done` word
// Every kernel of an iteration reads state[1] (`done`) first and returns when it is set, so launches issued after the stop change
// nothing.  Nothing waits on another workgroup; every output word has one owner: no atomics, the same bytes on every run.
#include "xai_common.h"
#include "xai_hip_ext7.h"

#include <math.h>

// the version pair of libxai_ext7.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext7_version, XAI_EXT7_VERSION, XAI_EXT7_MINOR)

namespace {

constexpr int kKmMaxN = XAI_KMEANS_MAX_POINTS;
constexpr int kKmMaxD = XAI_KMEANS_MAX_FEATURES;
constexpr int kKmMaxK = XAI_KMEANS_MAX_CLUSTERS;
constexpr int kKmThreads = 256;
constexpr int kKmAssign = 512;          // lanes of a K59 workgroup: 8 waves, one per group of 4 points
constexpr int kKmPT = 4 * (kKmAssign / kWave);      // points of one K59 workgroup: 32
constexpr int kKmCT = 4 * kWave;        // centroids of one LDS tile: 4 per lane of a wave, 256
constexpr int kKmLR = kKmAssign / 32;   // rows of a tile the lanes load at a time
constexpr int kKmTT = 32;               // features of one LDS tile
constexpr int kKmXW = kKmPT + 4;        // LDS row pitches in floats: a multiple of 4 keeps the 16-byte reads aligned, the + 4 spreads
constexpr int kKmCW = kKmCT + 4;        // the transposing writes over the banks
constexpr int kKmFinish = 1024;         // e_j staged per pass of K61

// The words of `ws` (the header's layout).
struct KmWs {
  double* e;
  float* xx;
  float* cc;
};

// ------------------------------------------------------------------------------------------------ K58
__global__ __launch_bounds__(kKmThreads) void kmeans_norms_kernel(const float* __restrict__ X, int n, int d, float* __restrict__ xx,
                                                                  int32_t* __restrict__ state) {
  const int i = blockIdx.x * kKmThreads + threadIdx.x;
  if (i == 0) {
#pragma unroll
    for (int w = 0; w < XAI_KMEANS_STATE_WORDS; ++w) state[w] = 0;       // iterations, done, status, 0, err = +0.0
  }
  if (i >= n) return;
  const float* row = X + static_cast<size_t>(i) * d;
  float s = 0.f;
  for (int t = 0; t < d; ++t) s = s + row[t] * row[t];
  xx[i] = s;
}

__global__ __launch_bounds__(kKmThreads) void kmeans_gather_kernel(const float* __restrict__ X, const int64_t* __restrict__ first, int n, int d,
                                                                   float* __restrict__ C, float* __restrict__ cc, int32_t* __restrict__ state) {
  const int j = blockIdx.x;
  const int64_t at = first[j];
  const bool ok = at >= 0 && at < n;                                     // an index outside X is never followed: a zero row and a status
  const float* row = X + (ok ? static_cast<size_t>(at) * d : 0);
  float* out = C + static_cast<size_t>(j) * d;
  for (int t = threadIdx.x; t < d; t += kKmThreads) out[t] = ok ? row[t] : 0.f;
  if (threadIdx.x == 0) {
    float s = 0.f;
    if (ok)
      for (int t = 0; t < d; ++t) s = s + row[t] * row[t];
    cc[j] = s;
    if (!ok) state[2] = XAI_KMEANS_BAD_INDEX;                             // every writer writes the same word
  }
}

// ------------------------------------------------------------------------------------------------ K59
// The global loads of one LDS tile pair, held in registers while the tile before it is computed on: lane (lt, lr) loads feature lt of
// rows lr, lr + 16, ... of the point tile and of the centroid tile.  Outside the extents it loads +0, which the compute loop never reads.
struct KmStage {
  float x[kKmPT / kKmLR];
  float c[kKmCT / kKmLR];
};

__device__ __forceinline__ void km_stage_load(KmStage& st, const float* __restrict__ X, const float* __restrict__ C, int n, int d, int k, int i0,
                                              int j0, int t0, int lt, int lr) {
  const bool tin = t0 + lt < d;
#pragma unroll
  for (int u = 0; u < kKmPT / kKmLR; ++u) {
    const int i = i0 + lr + kKmLR * u;
    st.x[u] = (tin && i < n) ? X[static_cast<size_t>(i) * d + t0 + lt] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < kKmCT / kKmLR; ++u) {
    const int j = j0 + lr + kKmLR * u;
    st.c[u] = (tin && j < k) ? C[static_cast<size_t>(j) * d + t0 + lt] : 0.f;
  }
}

__global__ __launch_bounds__(kKmAssign) void kmeans_assign_kernel(const float* __restrict__ X, const float* __restrict__ C,
                                                                   const float* __restrict__ xx, const float* __restrict__ cc, int n, int d, int k,
                                                                   int32_t* __restrict__ assign, const int32_t* __restrict__ state) {
  if (state[1]) return;
  __shared__ __align__(16) float Xs[kKmTT * kKmXW];
  __shared__ __align__(16) float Cs[kKmTT * kKmCW];
  const int t = threadIdx.x;
  const int cg = t & (kWave - 1), pg = t / kWave;     // the lane's 4 centroids of a tile (4 cg .. + 3), its wave's 4 points
  const int lt = t & 31, lr = t >> 5;                 // as a loader: feature lt of the tile, rows lr, lr + 16, ...
  const int i0 = blockIdx.x * kKmPT;

  float xxi[4], bv[4];
  int bi[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + 4 * pg + p;
    xxi[p] = i < n ? xx[i] : 0.f;
    bv[p] = -INFINITY;                                // (-inf, INT32_MAX) loses to every candidate, -inf and NaN included
    bi[p] = INT32_MAX;
  }

  KmStage st;
  km_stage_load(st, X, C, n, d, k, i0, 0, 0, lt, lr);
  for (int j0 = 0; j0 < k; j0 += kKmCT) {
    float acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[p][c] = 0.f;
    for (int t0 = 0; t0 < d; t0 += kKmTT) {
      const int tn = min(kKmTT, d - t0);
      __syncthreads();                                // the readers of the tile before this one are done
#pragma unroll
      for (int u = 0; u < kKmPT / kKmLR; ++u) Xs[lt * kKmXW + lr + kKmLR * u] = st.x[u];
#pragma unroll
      for (int u = 0; u < kKmCT / kKmLR; ++u) Cs[lt * kKmCW + lr + kKmLR * u] = st.c[u];
      __syncthreads();
      {                                               // the next tile pair is on its way while this one is computed on
        const bool more_t = t0 + kKmTT < d;
        const int nj0 = more_t ? j0 : j0 + kKmCT, nt0 = more_t ? t0 + kKmTT : 0;
        if (nj0 < k) km_stage_load(st, X, C, n, d, k, i0, nj0, nt0, lt, lr);
      }
#pragma unroll 4
      for (int s = 0; s < tn; ++s) {                  // ascending t: the 16 chains of the lane advance together
        const float4 xv = *reinterpret_cast<const float4*>(&Xs[s * kKmXW + 4 * pg]);      // one address per wave: a broadcast
        const float4 cv = *reinterpret_cast<const float4*>(&Cs[s * kKmCW + 4 * cg]);
        const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ca[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[p][c] = acc[p][c] + xa[p] * ca[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {                     // ascending j within the lane; the order among lanes is settled by the index
      const int j = j0 + 4 * cg + c;
      if (j < k) {
        const float ccj = cc[j];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float s = ((2.f * acc[p][c]) - xxi[p]) - ccj;
          if (argmax_beats(s, j, bv[p], bi[p])) {
            bv[p] = s;
            bi[p] = j;
          }
        }
      }
    }
  }
  // the lanes of a point group are one wave.  The order is total, so partners agree.
#pragma unroll
  for (int p = 0; p < 4; ++p) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv[p], off, kWave);
      const int oi = __shfl_xor(bi[p], off, kWave);
      if (argmax_beats(ov, oi, bv[p], bi[p])) {
        bv[p] = ov;
        bi[p] = oi;
      }
    }
    const int i = i0 + 4 * pg + p;
    if (cg == 0 && i < n) assign[i] = bi[p];
  }
}

// ------------------------------------------------------------------------------------------------ K60
__global__ __launch_bounds__(kKmThreads) void kmeans_update_kernel(const float* __restrict__ X, const int32_t* __restrict__ assign, int n, int d,
                                                                   float* C, float* __restrict__ cc, int32_t* __restrict__ counts,
                                                                   double* __restrict__ e, const int32_t* __restrict__ state) {
  if (state[1]) return;
  __shared__ uint64_t member[kKmMaxN / kWave];        // bit l of word m: point 64 m + l is assigned to this centroid
  __shared__ float news[kKmMaxD];
  __shared__ float qs[kKmMaxD];
  const int j = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1);
  const int nm = (n + kWave - 1) / kWave;
  for (int m = t / kWave; m < nm; m += kKmThreads / kWave) {
    const int i = m * kWave + lane;
    const int a = i < n ? assign[i] : -1;
    const uint64_t bits = __ballot(a == j);
    if (lane == 0) member[m] = bits;
  }
  __syncthreads();
  int cnt = 0;
  for (int m = 0; m < nm; ++m) cnt += __popcll(member[m]);
  const float fcnt = static_cast<float>(cnt);
  float* crow = C + static_cast<size_t>(j) * d;
  for (int tt = t; tt < d; tt += kKmThreads) {
    float acc = 0.f;
    for (int m = 0; m < nm; ++m) {                    // ascending i: the words in order, the bits of a word from the lowest
      uint64_t bits = member[m];
      while (bits) {
        const int l = __ffsll(static_cast<unsigned long long>(bits)) - 1;
        bits &= bits - 1;
        acc = acc + X[static_cast<size_t>(m * kWave + l) * d + tt];
      }
    }
    float nw = acc / fcnt;                            // 0 / 0 for an empty cluster
    if (nw != nw) nw = 0.f;
    const float q = nw - crow[tt];
    news[tt] = nw;
    qs[tt] = q * q;
    crow[tt] = nw;
  }
  __syncthreads();
  if (t == 0) {
    double es = 0.0;
    float cs = 0.f;
    for (int tt = 0; tt < d; ++tt) {
      es = es + static_cast<double>(qs[tt]);
      cs = cs + news[tt] * news[tt];
    }
    e[j] = es;
    cc[j] = cs;
    counts[j] = cnt;
  }
}

// ------------------------------------------------------------------------------------------------ K61
__global__ __launch_bounds__(kKmThreads) void kmeans_finish_kernel(const double* __restrict__ e, int k, int max_iter, double tol, int32_t* state) {
  if (state[1]) return;
  __shared__ double es[kKmFinish];
  double err = 0.0;
  for (int base = 0; base < k; base += kKmFinish) {
    const int m = min(kKmFinish, k - base);
    for (int j = threadIdx.x; j < m; j += kKmThreads) es[j] = e[base + j];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < m; ++j) err = err + es[j];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int it = state[0] + 1;
    state[0] = it;
    *reinterpret_cast<double*>(state + 4) = err;
    state[1] = (err <= tol || it >= max_iter) ? 1 : 0;                  // a NaN err compares false, as float(err) <= tol does
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The checks every entry shares, in the header's order -> XAI_OK and the layout, or the refusal.
int km_check(int n, int d, int k, const void* ws, size_t ws_bytes, const void* state, KmWs* lay) {
  XAI_REQUIRE(n >= 1 && d >= 1 && k >= 1 && k <= n, XAI_E_SHAPE);
  XAI_REQUIRE(n <= kKmMaxN && d <= kKmMaxD && k <= kKmMaxK, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= xai_kmeans_workspace_bytes(n, d, k), XAI_E_SHAPE);
  XAI_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(state) & 7u) == 0, XAI_E_SHAPE);
  lay->e = static_cast<double*>(const_cast<void*>(ws));
  lay->xx = reinterpret_cast<float*>(lay->e + k);
  lay->cc = lay->xx + n;
  return XAI_OK;
}

int km_assign(const float* X, int n, int d, int k, const float* C, int32_t* assign, const KmWs& lay, const int32_t* state, hipStream_t s) {
  kmeans_assign_kernel<<<unsigned(xai_ceil_div(n, kKmPT)), kKmAssign, 0, s>>>(X, C, lay.xx, lay.cc, n, d, k, assign, state);
  return xai_launch_status();
}

int km_update(const float* X, int n, int d, int k, float* C, const int32_t* assign, int32_t* counts, const KmWs& lay, int32_t* state,
              int max_iter, double tol, hipStream_t s) {
  kmeans_update_kernel<<<unsigned(k), kKmThreads, 0, s>>>(X, assign, n, d, C, lay.cc, counts, lay.e, state);
  const int st = xai_launch_status();
  if (st != XAI_OK) return st;
  kmeans_finish_kernel<<<1, kKmThreads, 0, s>>>(lay.e, k, max_iter, tol, state);
  return xai_launch_status();
}

}  // namespace

XAI_EXPORT int xai_kmeans_max_points(void) { return kKmMaxN; }
XAI_EXPORT int xai_kmeans_max_features(void) { return kKmMaxD; }
XAI_EXPORT int xai_kmeans_max_clusters(void) { return kKmMaxK; }

XAI_EXPORT size_t xai_kmeans_workspace_bytes(int n, int d, int k) {
  if (n < 1 || d < 1 || k < 1 || k > n || n > kKmMaxN || d > kKmMaxD || k > kKmMaxK) return 0;
  return static_cast<size_t>(k) * sizeof(double) + (static_cast<size_t>(n) + static_cast<size_t>(k)) * sizeof(float);
}

XAI_EXPORT int xai_kmeans_init_f32(const float* X, const int64_t* first, int n, int d, int k, float* C, void* ws, size_t ws_bytes,
                                   int32_t* state, xai_stream_t stream) {
  XAI_REQUIRE_PTR(X);
  XAI_REQUIRE_PTR(first);
  XAI_REQUIRE_PTR(C);
  XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE_PTR(state);
  KmWs lay;
  const int rc = km_check(n, d, k, ws, ws_bytes, state, &lay);
  if (rc != XAI_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  kmeans_norms_kernel<<<unsigned(xai_ceil_div(n, kKmThreads)), kKmThreads, 0, s>>>(X, n, d, lay.xx, state);
  const int st = xai_launch_status();
  if (st != XAI_OK) return st;
  kmeans_gather_kernel<<<unsigned(k), kKmThreads, 0, s>>>(X, first, n, d, C, lay.cc, state);
  return xai_launch_status();
}

XAI_EXPORT int xai_kmeans_assign_f32(const float* X, int n, int d, int k, const float* C, int32_t* assign, const void* ws, size_t ws_bytes,
                                     const int32_t* state, xai_stream_t stream) {
  XAI_REQUIRE_PTR(X);
  XAI_REQUIRE_PTR(C);
  XAI_REQUIRE_PTR(assign);
  XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE_PTR(state);
  KmWs lay;
  const int rc = km_check(n, d, k, ws, ws_bytes, state, &lay);
  if (rc != XAI_OK) return rc;
  return km_assign(X, n, d, k, C, assign, lay, state, static_cast<hipStream_t>(stream));
}

XAI_EXPORT int xai_kmeans_update_f32(const float* X, int n, int d, int k, float* C, const int32_t* assign, int32_t* counts, void* ws,
                                     size_t ws_bytes, int32_t* state, int max_iter, double tol, xai_stream_t stream) {
  XAI_REQUIRE_PTR(X);
  XAI_REQUIRE_PTR(C);
  XAI_REQUIRE_PTR(assign);
  XAI_REQUIRE_PTR(counts);
  XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE_PTR(state);
  KmWs lay;
  const int rc = km_check(n, d, k, ws, ws_bytes, state, &lay);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(max_iter >= 1, XAI_E_SHAPE);
  return km_update(X, n, d, k, C, assign, counts, lay, state, max_iter, tol, static_cast<hipStream_t>(stream));
}

XAI_EXPORT int xai_kmeans_iterate_f32(const float* X, int n, int d, int k, float* C, int32_t* assign, int32_t* counts, void* ws,
                                      size_t ws_bytes, int32_t* state, int max_iter, double tol, int iterations, xai_stream_t stream) {
  XAI_REQUIRE_PTR(X);
  XAI_REQUIRE_PTR(C);
  XAI_REQUIRE_PTR(assign);
  XAI_REQUIRE_PTR(counts);
  XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE_PTR(state);
  KmWs lay;
  const int rc = km_check(n, d, k, ws, ws_bytes, state, &lay);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(max_iter >= 1 && iterations >= 1 && iterations <= max_iter, XAI_E_SHAPE);
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int it = 0; it < iterations; ++it) {
    int st = km_assign(X, n, d, k, C, assign, lay, state, s);
    if (st != XAI_OK) return st;
    st = km_update(X, n, d, k, C, assign, counts, lay, state, max_iter, tol, s);
    if (st != XAI_OK) return st;
  }
  return XAI_OK;
}
