// LIME for images (reference util/attribution_methods/lime: lime_image.py, lime_base.py) for gfx950: the builder of the perturbed
// images (K31), the kernel weights and the two weighted ridge fits of every label of every image (K32), and the painter that
// turns a per-segment table into a dense map (K33).
//
// The perturbed images of a call form one flat list, row r = image * n_samples + sample; a classifier pass is a run
// [first, first + n) of that list and may cross from one image into the next (as K26's list, ablation_kernels.hip).  A sample is a
// row of bits, one per superpixel: bit z of word z / 64 is 1 where superpixel z keeps the image, 0 where it is replaced.
//
// K31 is write-bound like K26 (n * C * H * W * 4 B out; image, ids and fill values read once per lane and image): a lane keeps its 4
// elements of the flattened (C, H, W) image, their segment ids and fill values in registers and emits one 16-byte store per row;
// the bit words of a workgroup's rows are staged in LDS once, so a pixel costs one LDS read per row, no global one.  The value
// stored is a select (lime_image.py:261 `temp[mask] = fudged_image[mask]`), never a blend: NaN and Inf of an "on" segment pass.
//
// K32 is small dense fp64 work, one workgroup per image: the weights and the centred Gram matrix depend only on the image's rows,
// so they are built once, both regularised copies are factored once (Cholesky, packed lower triangles in LDS) and every label
// costs two triangular solves.  Every sum runs in one fixed order and there are no floating-point atomics: two runs give the
// same bits.
#include "xai_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRowWordsLds = 2048;             // bit words of one workgroup's rows staged in LDS (16 KiB)

constexpr int kFitThreads = 512;
constexpr int kFitWaves = kFitThreads / kWave;
constexpr int kMaxD = 128;                     // superpixels per image K32 fits: two packed triangles of 66 048 B in 160 KiB of LDS
constexpr int kSlots = kMaxD / kWave;          // features a lane owns in the per-label part: lane, lane + 64
constexpr int kTri = kMaxD * (kMaxD + 1) / 2;
static_assert(kSlots == 2, "the per-label part keeps a lane's features in two named registers");

// is superpixel `id` kept by the row whose words are `bits`: an id outside [0, D) -- or beyond the words -- belongs to no
// superpixel the row could switch off
__device__ __forceinline__ bool seg_on(const uint64_t* bits, int id, int D, int words) {
  if (id < 0 || id >= D || (id >> 6) >= words) return true;
  return (bits[id >> 6] >> (id & 63)) & 1ull;
}

// grid = (tiles of the flattened C*H*W image, row chunks); a lane handles V consecutive elements for every row of its chunk
template <int V>
__global__ __launch_bounds__(kBlock) void compose_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg,
                                                         const uint64_t* __restrict__ rows, const int32_t* __restrict__ Dv, int words,
                                                         const float* __restrict__ hide, const float* __restrict__ fudged, int C,
                                                         int64_t hw, int n_samples, int first, int n, int per, float* __restrict__ out) {
  __shared__ uint64_t sb[kRowWordsLds];
  const int k0 = blockIdx.y * per;
  const int k1 = min(k0 + per, n);
  const int staged = (k1 - k0) * words;          // <= kRowWordsLds: the launcher caps `per`
  const uint64_t* src = rows + static_cast<int64_t>(first + k0) * words;
  for (int i = threadIdx.x; i < staged; i += kBlock) sb[i] = src[i];
  __syncthreads();
  const int64_t chw = static_cast<int64_t>(C) * hw;
  const int64_t e = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (e >= chw) return;
  int64_t pix[V];
  float hv[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int64_t c = (e + i) / hw;
    pix[i] = (e + i) - c * hw;
    hv[i] = hide ? hide[c] : 0.f;
  }
  int idv[V];
  float xv[V], fv[V], o4[V];
  int cur_b = -1, Db = 0;
  float* o = out + k0 * chw + e;
  for (int k = k0; k < k1; ++k, o += chw) {
    const int b = (first + k) / n_samples;
    if (b != cur_b) {                            // the next image of the flat list: at most once per image and chunk
      const float* xs = x + b * chw + e;
      if constexpr (V == 4) {
        const float4 t = ld4(xs);
        xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
      } else {
        xv[0] = xs[0];
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        idv[i] = seg[b * hw + pix[i]];
        fv[i] = fudged ? fudged[b * chw + e + i] : hv[i];
      }
      Db = Dv[b];
      cur_b = b;
    }
    const uint64_t* bits = sb + (k - k0) * words;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float keep = xv[i], fill = fv[i];    // by value: a select between the two ARRAYS would move them to scratch
      o4[i] = seg_on(bits, idv[i], Db, words) ? keep : fill;
    }
    if constexpr (V == 4) st4(o, make_float4(o4[0], o4[1], o4[2], o4[3]));
    else *o = o4[0];
  }
}

__global__ __launch_bounds__(kBlock) void paint_kernel(const float* __restrict__ table, const int32_t* __restrict__ seg, int d_stride,
                                                       int64_t hw, int64_t total, float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / hw;
  const int id = seg[i];
  out[i] = (id >= 0 && id < d_stride) ? table[b * d_stride + id] : 0.f;
}

// ---- K32
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // j <= i

__device__ __forceinline__ double bit_of(const uint64_t* row, int j) {
  return static_cast<double>((row[j >> 6] >> (j & 63)) & 1ull);
}

// (i, j), j <= i, of the e-th element of a packed lower triangle
__device__ __forceinline__ void tri_decode(int e, int& i, int& j) {
  i = static_cast<int>((sqrtf(8.f * static_cast<float>(e) + 1.f) - 1.f) * 0.5f);
  while (i * (i + 1) / 2 > e) --i;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

// value of feature c (lane c % 64, slot c / 64) on every lane
__device__ __forceinline__ double lane_value(double v0, double v1, int c) { return __shfl(c < kWave ? v0 : v1, c & (kWave - 1), kWave); }
__device__ __forceinline__ int lane_value(int v0, int v1, int c) { return __shfl(c < kWave ? v0 : v1, c & (kWave - 1), kWave); }

// L L^T v = rhs for the packed factor `Lm` of order D by one wave, a lane holding rows lane and lane + 64 in (v0, v1); in place
__device__ __forceinline__ void chol_solve(const double* Lm, int D, int lane, double& v0, double& v1) {
  const int i0 = lane, i1 = lane + kWave;
  for (int c = 0; c < D; ++c) {                  // L z = rhs, column by column
    const double zc = lane_value(v0, v1, c) / Lm[tri(c, c)];
    if (i0 == c) v0 = zc;
    if (i1 == c) v1 = zc;
    if (i0 > c && i0 < D) v0 -= Lm[tri(i0, c)] * zc;
    if (i1 > c && i1 < D) v1 -= Lm[tri(i1, c)] * zc;
  }
  for (int c = D - 1; c >= 0; --c) {             // L^T v = z
    const double xc = lane_value(v0, v1, c) / Lm[tri(c, c)];
    if (i0 == c) v0 = xc;
    if (i1 == c) v1 = xc;
    if (i0 < c) v0 -= Lm[tri(c, i0)] * xc;
    if (i1 < c) v1 -= Lm[tri(c, i1)] * xc;
  }
}

// one workgroup per image
__global__ __launch_bounds__(kFitThreads) void fit_kernel(const uint64_t* __restrict__ rows, int words, const int32_t* __restrict__ Dv,
                                                          const float* __restrict__ Y, int N, int L, int d_stride, double kernel_width,
                                                          double alpha_select, double alpha, double* __restrict__ coef,
                                                          double* __restrict__ intercept, double* __restrict__ score,
                                                          double* __restrict__ local_pred, int32_t* __restrict__ order,
                                                          double* dist, double* weight) {
  __shared__ double triA[kTri];                  // the centred Gram matrix, then the factor of A + alpha I
  __shared__ double triF[kTri];                  // the factor of A + alpha_select I
  __shared__ double xbar[kMaxD + 1];             // weighted column sums (entry D: the sum of the weights), then the means
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const int D = Dv[b];
  if (D < 1 || D > kMaxD || D > d_stride || D > words * 64) return;          // not this kernel's image: its outputs stay as they are
  const uint64_t* R = rows + static_cast<int64_t>(b) * N * words;
  double* dv = dist + static_cast<int64_t>(b) * N;
  double* wv = weight + static_cast<int64_t>(b) * N;

  // cosine distance of a 0/1 row with k ones to the all-ones row: 1 - k / (sqrt(k) sqrt(D)) = 1 - sqrt(k / D), 1 for k = 0
  for (int n = t; n < N; n += kFitThreads) {
    int k = 0;
    for (int wi = 0; wi * 64 < D; ++wi) {
      const int left = D - wi * 64;
      const uint64_t m = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
      k += __popcll(R[static_cast<int64_t>(n) * words + wi] & m);
    }
    const double d = 1.0 - sqrt(static_cast<double>(k) / static_cast<double>(D));
    dv[n] = d;
    wv[n] = sqrt(exp(-(d * d) / (kernel_width * kernel_width)));
  }
  __syncthreads();                               // the weights are read back below, by other lanes of this workgroup only

  // S_j = sum_n w_n x_nj, and with j == D the same sum over an all-ones column: a column of ones then has the mean 1 exactly
  for (int j = wave; j <= D; j += kFitWaves) {
    double p = 0.0;
    for (int n = lane; n < N; n += kWave) {
      const double xv = j < D ? bit_of(R + static_cast<int64_t>(n) * words, j) : 1.0;
      p += wv[n] * xv;
    }
    p = wave_sum(p);
    if (lane == 0) xbar[j] = p;
  }
  __syncthreads();
  const double sw = xbar[D];
  __syncthreads();
  for (int j = t; j < D; j += kFitThreads) xbar[j] = xbar[j] / sw;
  __syncthreads();

  // A_jk = sum_n w_n (x_nj - mean_j)(x_nk - mean_k), n ascending
  const int n_tri = D * (D + 1) / 2;
  for (int e = t; e < n_tri; e += kFitThreads) {
    int j, k;
    tri_decode(e, j, k);
    const double mj = xbar[j], mk = xbar[k];
    double acc = 0.0;
    for (int n = 0; n < N; ++n) {
      const uint64_t* row = R + static_cast<int64_t>(n) * words;
      acc += wv[n] * ((bit_of(row, j) - mj) * (bit_of(row, k) - mk));
    }
    triA[e] = acc;
    triF[e] = acc;
  }
  __syncthreads();
  for (int j = t; j < D; j += kFitThreads) {
    triF[tri(j, j)] += alpha_select;
    triA[tri(j, j)] += alpha;
  }
  __syncthreads();

  // right-looking Cholesky of both matrices, column by column
  for (int c = 0; c < D; ++c) {
    const double dF = sqrt(triF[tri(c, c)]), dA = sqrt(triA[tri(c, c)]);
    __syncthreads();
    if (t == 0) {
      triF[tri(c, c)] = dF;
      triA[tri(c, c)] = dA;
    }
    for (int i = c + 1 + t; i < D; i += kFitThreads) {
      triF[tri(i, c)] /= dF;
      triA[tri(i, c)] /= dA;
    }
    __syncthreads();
    const int m = D - 1 - c;
    for (int e = t; e < m * (m + 1) / 2; e += kFitThreads) {
      int ii, jj;
      tri_decode(e, ii, jj);
      const int i = c + 1 + ii, j = c + 1 + jj;
      triF[tri(i, j)] -= triF[tri(i, c)] * triF[tri(j, c)];
      triA[tri(i, j)] -= triA[tri(i, c)] * triA[tri(j, c)];
    }
    __syncthreads();
  }

  // a wave per label; a lane owns the features j0 = lane and j1 = lane + 64
  const int j0 = lane, j1 = lane + kWave;
  const bool has0 = j0 < D, has1 = j1 < D;
  const double m0 = has0 ? xbar[j0] : 0.0, m1 = has1 ? xbar[j1] : 0.0;
  const double x00 = has0 ? bit_of(R, j0) : 0.0, x01 = has1 ? bit_of(R, j1) : 0.0;      // row 0, the instance explained
  for (int l = wave; l < L; l += kFitWaves) {
    const float* y = Y + static_cast<int64_t>(b) * N * L + l;
    double p = 0.0;
    for (int n = lane; n < N; n += kWave) p += wv[n] * static_cast<double>(y[static_cast<int64_t>(n) * L]);
    const double ybar = wave_sum(p) / sw;
    double r0 = 0.0, r1 = 0.0;                   // sum_n w_n (x_nj - mean_j)(y_n - ybar), n ascending
    for (int n = 0; n < N; ++n) {
      const uint64_t* row = R + static_cast<int64_t>(n) * words;
      const double yc = static_cast<double>(y[static_cast<int64_t>(n) * L]) - ybar;
      if (has0) r0 += wv[n] * ((bit_of(row, j0) - m0) * yc);
      if (has1) r1 += wv[n] * ((bit_of(row, j1) - m1) * yc);
    }
    double s0 = r0, s1 = r1;                     // the selection fit, lime_base.py:78-80
    chol_solve(triF, D, lane, s0, s1);
    chol_solve(triA, D, lane, r0, r1);           // the explanation fit, lime_base.py:189-193
    if (!has0) r0 = 0.0;
    if (!has1) r1 = 0.0;

    // lime_base.py:109-114: sorted(|coef * data[0]|, reverse=True), stable -> position of a feature among the used features
    const double k0 = fabs(s0 * x00), k1 = fabs(s1 * x01);
    int p0 = 0, p1 = 0;
    for (int i = 0; i < D; ++i) {
      const double ki = lane_value(k0, k1, i);
      p0 += (ki > k0 || (ki == k0 && i < j0)) ? 1 : 0;
      p1 += (ki > k1 || (ki == k1 && i < j1)) ? 1 : 0;
    }
    // lime_base.py:205-206: sorted(zip(used_features, coef), key=|coef|, reverse=True), stable
    const double a0 = fabs(r0), a1 = fabs(r1);
    int q0 = 0, q1 = 0;
    for (int i = 0; i < D; ++i) {
      const double ai = lane_value(a0, a1, i);
      const int pi = lane_value(p0, p1, i);
      q0 += (ai > a0 || (ai == a0 && pi < p0)) ? 1 : 0;
      q1 += (ai > a1 || (ai == a1 && pi < p1)) ? 1 : 0;
    }
    const int64_t row_out = (static_cast<int64_t>(b) * L + l) * d_stride;
    if (has0) { coef[row_out + j0] = r0; order[row_out + q0] = j0; }
    if (has1) { coef[row_out + j1] = r1; order[row_out + q1] = j1; }
    for (int j = D + lane; j < d_stride; j += kWave) { coef[row_out + j] = 0.0; order[row_out + j] = -1; }

    double dot = 0.0, at0 = 0.0;                 // mean . coef and data[0] . coef, features ascending
    for (int j = 0; j < D; ++j) {
      const double cj = lane_value(r0, r1, j);
      dot += xbar[j] * cj;
      at0 += bit_of(R, j) * cj;
    }
    const double icpt = ybar - dot;
    double num = 0.0, den = 0.0;                 // weighted R^2 of the explanation fit
    for (int n0 = 0; n0 < N; n0 += kWave) {
      const int n = n0 + lane;
      const bool valid = n < N;
      const uint64_t* row = R + static_cast<int64_t>(valid ? n : 0) * words;
      double pred = icpt;
      for (int j = 0; j < D; ++j) {
        const double cj = lane_value(r0, r1, j);
        if ((row[j >> 6] >> (j & 63)) & 1ull) pred += cj;
      }
      if (valid) {
        const double yn = static_cast<double>(y[static_cast<int64_t>(n) * L]);
        num += wv[n] * ((yn - pred) * (yn - pred));
        den += wv[n] * ((yn - ybar) * (yn - ybar));
      }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) {
      const int64_t o = static_cast<int64_t>(b) * L + l;
      intercept[o] = icpt;
      local_pred[o] = icpt + at0;
      // sklearn's r2_score: undefined below two samples; a constant target scores 1 when it is met exactly, else 0
      score[o] = N < 2 ? static_cast<double>(NAN) : (den == 0.0 ? (num == 0.0 ? 1.0 : 0.0) : 1.0 - num / den);
    }
  }
}

}  // namespace

XAI_EXPORT int xai_lime_max_features(void) { return kMaxD; }

XAI_EXPORT int xai_lime_compose_f32(const float* x, const int32_t* seg, const uint64_t* rows, const int32_t* D, int words,
                                    const float* hide, const float* fudged, int B, int C, int H, int W, int n_samples, int64_t first,
                                    int n, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(seg); XAI_REQUIRE_PTR(rows); XAI_REQUIRE_PTR(D); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(hide != nullptr || fudged != nullptr, XAI_E_NULL);
  XAI_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && n_samples > 0 && n > 0 && first >= 0 && words > 0, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(B) * n_samples <= INT32_MAX, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(first + n <= static_cast<int64_t>(B) * n_samples, XAI_E_SHAPE);
  XAI_REQUIRE(words <= kRowWordsLds, XAI_E_UNSUPPORTED);
  const int64_t hw = static_cast<int64_t>(H) * W, chw = hw * C;
  const bool vec = xai_can_vec4(chw, {x, out, fudged});
  // the row spans the channels; HBM-sized pass (64 MiB): two rows per lane.  The rows of a chunk must also fit the LDS stage.
  const XaiRowPlan plan = xai_row_chunk_plan(chw, kBlock, vec, n, 1, 1, int64_t(64) << 20, false);
  const int per = std::max(1, std::min(plan.per, kRowWordsLds / words));
  const int64_t chunks = xai_ceil_div(n, per);
  XAI_REQUIRE(chunks <= 65535 && plan.tiles <= INT32_MAX, XAI_E_UNSUPPORTED);
  const dim3 grid(static_cast<unsigned>(plan.tiles), static_cast<unsigned>(chunks));
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(compose_kernel<V4 ? 4 : 1>, grid, dim3(kBlock), 0, st, x, seg, rows, D, words, hide, fudged, C, hw, n_samples,
                       static_cast<int>(first), n, per, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lime_fit_f64(const uint64_t* rows, int words, const int32_t* D, const float* Y, int B, int N, int L, int d_stride,
                                double kernel_width, double alpha_select, double alpha, double* coef, double* intercept, double* score,
                                double* local_pred, int32_t* order, double* dist, double* weight, xai_stream_t stream) {
  XAI_REQUIRE_PTR(rows); XAI_REQUIRE_PTR(D); XAI_REQUIRE_PTR(Y); XAI_REQUIRE_PTR(coef); XAI_REQUIRE_PTR(intercept);
  XAI_REQUIRE_PTR(score); XAI_REQUIRE_PTR(local_pred); XAI_REQUIRE_PTR(order); XAI_REQUIRE_PTR(dist); XAI_REQUIRE_PTR(weight);
  XAI_REQUIRE(B > 0 && N > 0 && L > 0 && words > 0 && d_stride > 0, XAI_E_SHAPE);
  XAI_REQUIRE(kernel_width > 0.0 && alpha_select > 0.0 && alpha > 0.0, XAI_E_SHAPE);          // false for NaN too
  XAI_REQUIRE(static_cast<int64_t>(B) * N <= INT32_MAX, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(fit_kernel, dim3(B), dim3(kFitThreads), 0, static_cast<hipStream_t>(stream), rows, words, D, Y, N, L, d_stride,
                     kernel_width, alpha_select, alpha, coef, intercept, score, local_pred, order, dist, weight);
  return xai_launch_status();
}

XAI_EXPORT int xai_lime_paint_f32(const float* table, const int32_t* seg, int B, int d_stride, int H, int W, float* out,
                                  xai_stream_t stream) {
  XAI_REQUIRE_PTR(table); XAI_REQUIRE_PTR(seg); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(B > 0 && d_stride > 0 && H > 0 && W > 0, XAI_E_SHAPE);
  const int64_t hw = static_cast<int64_t>(H) * W, total = hw * B;
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(total, kBlock, &blocks), XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(paint_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), table, seg, d_stride, hw, total, out);
  return xai_launch_status();
}
