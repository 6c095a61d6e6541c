// K17-K21: the post-backward arithmetic of Baselines.generate_RAVE ("InFlow") and Baselines.generate_cam_attn for gfx950.
//
// Per-block tensors are separate allocations of the classifier's forward / backward, so the multi-block kernels take a
// DEVICE table of pointers (one per block and operand) and cover every block in one launch.  No atomics anywhere: every
// sum has one fixed order, so two calls on the same inputs give the same bytes.
//
// K17 head importance: Ih[l][h] = mean_ij |(A_h^T G_h)[i][j]| / sum_h(...).  One wave per 32x32 tile of A_h^T G_h on
//     v_mfma_f32_32x32x2_f32 (exact f32, operands straight from global memory: lane l reads A[k][i0 + (l&31)] and
//     G[k][j0 + (l&31)] for k = k0 + (l>>5), two 128-B row segments per operand), abs + tile sum in the epilogue; the
//     S x S product is never written.  Out-of-range rows/columns/k load 0 and so add exact zeros.  The tile partials go to
//     caller scratch and a one-workgroup launch sums them in tile order, divides by S^2 and normalises over heads.
// K18 RAVE matrices: one wave per (block, row i); max over heads, bottom-up gradient, residual shares, row normalisation.
// K19 rollout row: one workgroup per image, v in LDS, L-1 vector-matrix products.
// K20 residual shares: one wave per (block, token), four token 2-norms.
// K21 cam_attn: one workgroup per image.
//
// NaN: the reference's expressions are torch.max, clamp, min and F.normalize, which carry a NaN to their result; fmaxf / fminf
// return the other operand.  K18's max over heads and clamps, K20's clamped denominators and K21's clamp, min and max follow
// torch (max_nan, relu_nan, the NaN flag of K21): a NaN gradient gives a NaN row, block or image, as in the reference.
#include "xai_common.h"

#include <math.h>

#include <atomic>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;
constexpr int kK17Waves = 4;
constexpr int kKUnroll = 8;                        // k-steps of 2 whose loads are issued before their MFMAs

// torch.max / torch.clamp carry a NaN to the result; fmaxf returns the other operand.  IEEE 754-2019 maximum carries it, orders
// -0 below +0 and is fmaxf on every other pair; on gfx950 it is one instruction (v_maximum3_f32), as v_max_f32 is for fmaxf.
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float relu_nan(float v) { return max_nan(v, 0.f); }

inline int k17_tiles(int S) {
  const int t = (S + kTile - 1) / kTile;
  return t * t;
}

// grid (ceil(tiles / 4), L*H); wave w of workgroup x takes tile x*4 + w of block-head blockIdx.y
__global__ __launch_bounds__(kK17Waves* kWave) void head_importance_tiles_kernel(const float* const* __restrict__ A_tab,
                                                                                const float* const* __restrict__ G_tab, int H,
                                                                                int S, float* __restrict__ part) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nt = (S + kTile - 1) / kTile;
  const int tile = blockIdx.x * kK17Waves + wave;
  if (tile >= nt * nt) return;
  const int lh = blockIdx.y, l = lh / H, h = lh - l * H;
  const int64_t plane = static_cast<int64_t>(S) * S;
  const float* A = A_tab[l] + h * plane;
  const float* G = G_tab[l] + h * plane;
  const int i = (tile / nt) * kTile + (lane & 31);   // row of A^T = column of A
  const int j = (tile % nt) * kTile + (lane & 31);   // column of G
  const int kh = lane >> 5;
  const bool iok = i < S, jok = j < S;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < S; k0 += 2 * kKUnroll) {
    float a[kKUnroll], b[kKUnroll];
#pragma unroll
    for (int u = 0; u < kKUnroll; ++u) {
      const int k = k0 + 2 * u + kh;
      const bool kok = k < S;
      a[u] = (kok && iok) ? A[static_cast<int64_t>(k) * S + i] : 0.f;
      b[u] = (kok && jok) ? G[static_cast<int64_t>(k) * S + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kKUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += fabsf(acc[r]);   // padded rows / columns hold exact zeros
  s = wave_sum(s);
  if (lane == 0) part[static_cast<int64_t>(lh) * nt * nt + tile] = s;
}

// one workgroup; thread l*H + h sums the tiles of (l, h) in tile order, then per block the H means are normalised
__global__ __launch_bounds__(1024) void head_importance_finish_kernel(const float* __restrict__ part, int L, int H, int S, int tiles,
                                                                      float* __restrict__ Ih) {
  extern __shared__ float mean[];   // [L*H]
  const float n = static_cast<float>(S) * static_cast<float>(S);
  for (int lh = threadIdx.x; lh < L * H; lh += blockDim.x) {
    const float* p = part + static_cast<int64_t>(lh) * tiles;
    float s = 0.f;
    for (int t = 0; t < tiles; ++t) s += p[t];
    mean[lh] = s / n;
  }
  __syncthreads();
  for (int lh = threadIdx.x; lh < L * H; lh += blockDim.x) {
    const int l = lh / H;
    float tot = 0.f;
    for (int h = 0; h < H; ++h) tot += mean[l * H + h];
    Ih[lh] = mean[lh] / tot;
  }
}

// grid (ceil(S / 4), L), 4 waves: wave w owns row i = blockIdx.x*4 + w of block l
__global__ __launch_bounds__(256) void rave_matrices_kernel(const float* const* __restrict__ A_tab, const float* const* __restrict__ Gb_tab,
                                                            const float* __restrict__ Ih, const float* __restrict__ b1,
                                                            const float* __restrict__ b2, int H, int S, int ablate,
                                                            float* __restrict__ aug) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave, l = blockIdx.y;
  if (i >= S) return;
  const int64_t plane = static_cast<int64_t>(S) * S;
  const float* A = A_tab[l] + static_cast<int64_t>(i) * S;
  const float* Gb = Gb_tab ? Gb_tab[l] + static_cast<int64_t>(i) * S : nullptr;
  const float* ih = Ih + static_cast<int64_t>(l) * H;
  const float* b1l = b1 + static_cast<int64_t>(l) * 2 * S;   // [0] = input share, [1] = attention share
  const float* b2l = b2 + static_cast<int64_t>(l) * 2 * S;   // [0] = resid_1 share, [1] = mlp share
  // F.normalize(q, p=1): q / max(sum |q|, 1e-12), q = mlp share / resid_1 share
  float qs = 0.f;
  if (ablate == 0) {
    for (int j = lane; j < S; j += kWave) qs += fabsf(b2l[S + j] / b2l[j]);
    qs = max_nan(wave_sum(qs), 1e-12f);
  }
  float* out = aug + l * plane + static_cast<int64_t>(i) * S;
  float rs = 0.f;
  for (int j = lane; j < S; j += kWave) {
    float m = A[j] * ih[0];
    for (int h = 1; h < H; ++h) m = max_nan(m, A[h * plane + j] * ih[h]);
    if (Gb) {
      float g = 0.f;
      for (int h = 0; h < H; ++h) g += Gb[h * plane + j];
      m = relu_nan((g / static_cast<float>(H)) * m);
    }
    float r = m * b1l[S + j];
    if (j == i) r = r + b1l[j];
    if (ablate == 0) {
      const float ratio = (b2l[S + j] / b2l[j]) / qs;
      r = r * (ratio * b2l[S + j] + b2l[j]);   // r1 @ diag(d2): a column scale, exact
    }
    out[j] = r;
    rs += r;
  }
  rs = wave_sum(rs);
  for (int j = lane; j < S; j += kWave) out[j] = out[j] / rs;   // each lane re-reads only what it wrote
}

// one workgroup per image: v = aug[L-1][t], then v <- v . aug[l] for l = L-2 .. 0.  Wave w sums k in [w*kc, (w+1)*kc) for
// columns j = lane + 64q; the 16 wave partials are added in wave order.
constexpr int kRollWaves = 16;
__global__ __launch_bounds__(kRollWaves* kWave) void rollout_row_kernel(const float* __restrict__ aug, int L, int S, int t,
                                                                        float* __restrict__ out) {
  extern __shared__ float sm[];                    // v[S], part[kRollWaves][S]
  float* v = sm;
  float* part = sm + S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t plane = static_cast<int64_t>(S) * S;
  const float* img = aug + static_cast<int64_t>(blockIdx.x) * L * plane;
  for (int j = threadIdx.x; j < S; j += blockDim.x) v[j] = img[(L - 1) * plane + static_cast<int64_t>(t) * S + j];
  __syncthreads();
  const int kc = (S + kRollWaves - 1) / kRollWaves;
  const int kb = wave * kc, ke = min(S, kb + kc);
  for (int l = L - 2; l >= 0; --l) {
    const float* M = img + l * plane;
    for (int j = lane; j < S; j += kWave) {
      float s = 0.f;
      for (int k = kb; k < ke; ++k) s += v[k] * M[static_cast<int64_t>(k) * S + j];
      part[wave * S + j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < S; j += blockDim.x) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kRollWaves; ++w) s += part[w * S + j];
      v[j] = s;
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < S; j += blockDim.x) out[static_cast<int64_t>(blockIdx.x) * S + j] = v[j];
}

// K19 is the one kernel here that asks for more than 64 KiB of dynamic LDS (17 * S * 4 bytes, up to the CU's 160 KiB at
// S = 2409).  The limit is declared on the function the first time such a launch is asked for, never inside a stream capture
// (a first large launch that arrives while its stream is capturing is refused), and an error of the call is returned.
constexpr size_t kRollMaxLds = 160 * 1024;
std::atomic<int> g_roll_lds_status{-1};            // -1: not declared yet, else the hipError_t of the declaration
inline int rollout_row_allow_large_lds(hipStream_t st) {
  int s = g_roll_lds_status.load(std::memory_order_acquire);
  if (s < 0) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return XAI_E_UNSUPPORTED;
    s = static_cast<int>(hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_row_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kRollMaxLds)));
    g_roll_lds_status.store(s, std::memory_order_release);
  }
  return s == static_cast<int>(hipSuccess) ? XAI_OK : s;
}

// grid (ceil(S / 4), L), 4 waves: wave w owns token s = blockIdx.x*4 + w of block l.
// tab[4l + 0..3] = input, attention output, input + attention, MLP output of block l, each [S][D] (image 0)
__global__ __launch_bounds__(256) void residual_shares_kernel(const float* const* __restrict__ tab, int S, int D, float* __restrict__ b1,
                                                              float* __restrict__ b2) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + wave, l = blockIdx.y;
  if (s >= S) return;
  float q[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float* x = tab[4 * l + o] + static_cast<int64_t>(s) * D;
    float a = 0.f;
    for (int d = lane; d < D; d += kWave) a += x[d] * x[d];
    q[o] = sqrtf(wave_sum(a));
  }
  if (lane == 0) {
    const float d1 = max_nan(q[0] + q[1], 1e-12f), d2 = max_nan(q[2] + q[3], 1e-12f);
    float* o1 = b1 + static_cast<int64_t>(l) * 2 * S;
    float* o2 = b2 + static_cast<int64_t>(l) * 2 * S;
    o1[s] = q[0] / d1;
    o1[S + s] = q[1] / d1;
    o2[s] = q[2] / d2;
    o2[S + s] = q[3] / d2;
  }
}

// one workgroup per image: cam[p] = max(sum_h A[h][0][1+p] G[h][0][1+p] / H, 0), then (cam - min) / (max - min)
constexpr int kCamThreads = 1024;
__global__ __launch_bounds__(kCamThreads) void attn_cam_kernel(const float* __restrict__ attn, const float* __restrict__ grad, int H, int S,
                                                               float* __restrict__ out) {
  __shared__ float red[2 * (kCamThreads / kWave)];
  const int P = S - 1;
  const int64_t plane = static_cast<int64_t>(S) * S;
  const float* A = attn + static_cast<int64_t>(blockIdx.x) * H * plane;
  const float* G = grad + static_cast<int64_t>(blockIdx.x) * H * plane;
  float* o = out + static_cast<int64_t>(blockIdx.x) * P;
  float lo = INFINITY, hi = -INFINITY;
  int has_nan = 0;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += A[h * plane + 1 + p] * G[h * plane + 1 + p];
    const float c = relu_nan(s / static_cast<float>(H));
    o[p] = c;
    has_nan |= isnan(c);
    lo = fminf(lo, c);
    hi = fmaxf(hi, c);
  }
  block_min_max<kCamThreads / kWave>(lo, hi, red);
  if (__syncthreads_or(has_nan)) lo = hi = NAN;   // the reference's min() and max() of a map with a NaN are NaN: all NaN
  for (int p = threadIdx.x; p < P; p += blockDim.x) o[p] = (o[p] - lo) / (hi - lo);   // constant map: 0/0 = NaN, as the reference
}

}  // namespace

XAI_EXPORT size_t xai_attn_head_importance_workspace_bytes(int L, int H, int S) {
  if (L <= 0 || H <= 0 || S <= 0) return 0;
  return static_cast<size_t>(L) * H * k17_tiles(S) * sizeof(float);
}

XAI_EXPORT int xai_attn_head_importance_f32(const float* const* attn_tab, const float* const* grad_tab, int L, int H, int S, float* Ih,
                                            void* ws, size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(attn_tab); XAI_REQUIRE_PTR(grad_tab); XAI_REQUIRE_PTR(Ih); XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE(L > 0 && H > 0 && S > 0, XAI_E_SHAPE);
  XAI_REQUIRE(ws_bytes >= xai_attn_head_importance_workspace_bytes(L, H, S), XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(L) * H <= 4096 && S <= 4096, XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = k17_tiles(S);
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(head_importance_tiles_kernel, dim3((tiles + kK17Waves - 1) / kK17Waves, L * H), dim3(kK17Waves * kWave), 0, st,
                     attn_tab, grad_tab, H, S, part);
  hipLaunchKernelGGL(head_importance_finish_kernel, dim3(1), dim3(1024), static_cast<size_t>(L) * H * sizeof(float), st,
                     static_cast<const float*>(part), L, H, S, tiles, Ih);
  return xai_launch_status();
}

XAI_EXPORT int xai_rave_matrices_f32(const float* const* attn_tab, const float* const* bgrad_tab, const float* Ih, const float* b1,
                                     const float* b2, int L, int H, int S, int ablate, float* aug, xai_stream_t stream) {
  XAI_REQUIRE_PTR(attn_tab); XAI_REQUIRE_PTR(Ih); XAI_REQUIRE_PTR(b1); XAI_REQUIRE_PTR(b2); XAI_REQUIRE_PTR(aug);
  XAI_REQUIRE(L > 0 && H > 0 && S > 0 && (ablate == 0 || ablate == 1), XAI_E_SHAPE);
  XAI_REQUIRE(L <= 65535 && S <= 65535 * 4, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(rave_matrices_kernel, dim3((S + 3) / 4, L), dim3(256), 0, static_cast<hipStream_t>(stream), attn_tab, bgrad_tab, Ih,
                     b1, b2, H, S, ablate, aug);
  return xai_launch_status();
}

XAI_EXPORT int xai_rollout_row_f32(const float* aug, int n_img, int L, int S, int target_token, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(aug); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n_img > 0 && L > 0 && S > 0 && target_token >= 0 && target_token < S, XAI_E_SHAPE);
  const size_t lds = static_cast<size_t>(kRollWaves + 1) * S * sizeof(float);
  XAI_REQUIRE(lds <= kRollMaxLds && n_img <= 65535, XAI_E_UNSUPPORTED);
  if (lds > 64 * 1024) {
    const int e = rollout_row_allow_large_lds(static_cast<hipStream_t>(stream));
    if (e != XAI_OK) return e;
  }
  hipLaunchKernelGGL(rollout_row_kernel, dim3(n_img), dim3(kRollWaves * kWave), lds, static_cast<hipStream_t>(stream), aug, L, S,
                     target_token, out);
  return xai_launch_status();
}

XAI_EXPORT int xai_residual_shares_f32(const float* const* tab, int L, int S, int D, float* b1, float* b2, xai_stream_t stream) {
  XAI_REQUIRE_PTR(tab); XAI_REQUIRE_PTR(b1); XAI_REQUIRE_PTR(b2);
  XAI_REQUIRE(L > 0 && S > 0 && D > 0, XAI_E_SHAPE);
  XAI_REQUIRE(L <= 65535 && S <= 65535 * 4, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(residual_shares_kernel, dim3((S + 3) / 4, L), dim3(256), 0, static_cast<hipStream_t>(stream), tab, S, D, b1, b2);
  return xai_launch_status();
}

XAI_EXPORT int xai_attn_cam_f32(const float* attn, const float* grad, int n_img, int H, int S, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(attn); XAI_REQUIRE_PTR(grad); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n_img > 0 && H > 0 && S > 1, XAI_E_SHAPE);
  XAI_REQUIRE(n_img <= 65535, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(attn_cam_kernel, dim3(n_img), dim3(kCamThreads), 0, static_cast<hipStream_t>(stream), attn, grad, H, S, out);
  return xai_launch_status();
}
