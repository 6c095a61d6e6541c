// K88-K90: CLIP's M2IB row (libxai_cm2ib.so): the sample of the information bottleneck, the gradient of alpha with its Adam step,
// and the capacity with its nansum per token.  include/xai_hip_cm2ib.h states the arithmetic: every operation and the order of every sum.
#include "xai_common.h"
#include "xai_hip_cm2ib.h"
#include "clip_device.h"

XAI_VERSION_ENTRIES(xai_cm2ib_version, XAI_CM2IB_VERSION, XAI_CM2IB_MINOR)
XAI_EXPORT int xai_cm2ib_max_tokens(void) { return XAI_CM2IB_MAX_TOKENS; }
XAI_EXPORT int xai_cm2ib_max_width(void) { return XAI_CM2IB_MAX_WIDTH; }
XAI_EXPORT int xai_cm2ib_max_copies(void) { return XAI_CM2IB_MAX_COPIES; }

namespace {

constexpr int kThreads = 256;  // K88, K89: streaming, a lane per (l, d);  K90: 4 waves, a wave per token
constexpr int kWaves = kThreads / kWave;

// the header's per-element values
struct Gate {
  float lam, om, var, sd, mu;
};
__device__ __forceinline__ Gate gate(float a, float x) {
  Gate g;
  g.lam = 1.f / (1.f + expf(-a));
  g.om = 1.f - g.lam;
  g.var = g.om * g.om;
  g.sd = sqrtf(g.var);
  g.mu = x * g.lam;
  return g;
}

// K88: grid (ceil(L D / kThreads), B)
template <typename T>
__global__ __launch_bounds__(kThreads) void sample_kernel(const float* __restrict__ alpha, const T* __restrict__ x9,
                                                          const float* __restrict__ eps, int R, int64_t LD, T* __restrict__ t) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= LD) return;
  const int64_t b = blockIdx.y, e = b * LD + i;
  const Gate g = gate(alpha[e], ld(x9 + e));
  for (int r = 0; r < R; ++r) {
    const int64_t k = (b * R + r) * LD + i;
    st(t + k, g.mu + g.sd * eps[k]);
  }
}

// K89: grid (ceil(L D / kThreads), B)
template <typename T>
__global__ __launch_bounds__(kThreads) void adam_step_kernel(const T* __restrict__ gt, const float* __restrict__ eps, const T* __restrict__ x9,
                                                             int R, int64_t LD, float cscale, float w1, float b2, float w2, float bc2s,
                                                             float step_size, float adam_eps, float* __restrict__ alpha,
                                                             float* __restrict__ m, float* __restrict__ v) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= LD) return;
  const int64_t b = blockIdx.y, e = b * LD + i;
  const float a = alpha[e], x = ld(x9 + e);
  const Gate s = gate(a, x);
  const float lamp = s.lam * s.om;
  const float xl = x * lamp;
  const float q = (0.5f / s.sd) * (s.om + s.om);
  const float ql = q * lamp;
  float fit = 0.f;
  for (int r = 0; r < R; ++r) {
    const int64_t k = (b * R + r) * LD + i;
    fit = fit + ld(gt + k) * (xl - ql * eps[k]);
  }
  const float gv = -0.5f * (1.f / s.var - 1.f);
  const float dcap = s.mu * xl - (gv * (s.om + s.om)) * lamp;
  const float g = fit + cscale * dcap;
  const float mk = m[e] + w1 * (g - m[e]);
  const float vk = v[e] * b2 + (w2 * g) * g;
  const float den = sqrtf(vk) / bc2s + adam_eps;
  m[e] = mk;
  v[e] = vk;
  alpha[e] = a - step_size * (mk / den);
}

// K90: grid (ceil(L / kWaves), B)
__global__ __launch_bounds__(kThreads) void saliency_kernel(const float* __restrict__ alpha, const float* __restrict__ x9, int L, int D,
                                                            float* __restrict__ cap_out, float* __restrict__ out) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int l = blockIdx.x * kWaves + wave;  // the same in all lanes of a wave: a wave leaves whole
  if (l >= L || (l == 0 && !cap_out)) return;
  const int64_t b = blockIdx.y, row = (b * L + l) * D;
  float part = 0.f;
  for (int d = lane; d < D; d += kWave) {
    const Gate s = gate(alpha[row + d], x9[row + d]);
    const float cap = -0.5f * (((1.f + logf(s.var)) - s.mu * s.mu) - s.var);
    if (cap_out) cap_out[row + d] = cap;
    part = part + (cap != cap ? 0.f : cap);
  }
  part = wave_sum(part);
  if (lane == 0 && l >= 1) out[b * (L - 1) + (l - 1)] = part;
}

bool extents_ok(int B, int R, int L, int D) { return B >= 1 && R >= 1 && L >= 1 && D >= 1; }
bool limits_ok(int B, int R, int L, int D) {
  return B <= 65535 && R <= XAI_CM2IB_MAX_COPIES && L <= XAI_CM2IB_MAX_TOKENS && D <= XAI_CM2IB_MAX_WIDTH;
}

template <typename T>
int sample(const float* alpha, const void* x9, const float* eps, int B, int R, int L, int D, void* t, xai_stream_t stream) {
  XAI_REQUIRE_PTR(alpha); XAI_REQUIRE_PTR(x9); XAI_REQUIRE_PTR(eps); XAI_REQUIRE_PTR(t);
  XAI_REQUIRE(extents_ok(B, R, L, D), XAI_E_SHAPE);
  XAI_REQUIRE(limits_ok(B, R, L, D), XAI_E_UNSUPPORTED);
  const int64_t LD = int64_t(L) * D;
  hipLaunchKernelGGL(sample_kernel<T>, dim3(unsigned(xai_ceil_div(LD, kThreads)), unsigned(B)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), alpha, static_cast<const T*>(x9), eps, R, LD, static_cast<T*>(t));
  return xai_launch_status();
}

template <typename T>
int adam_step(const void* gt, const float* eps, const void* x9, int B, int R, int L, int D, float beta, float w1, float b2, float w2,
              float bc2s, float step_size, float adam_eps, float* alpha, float* m, float* v, xai_stream_t stream) {
  XAI_REQUIRE_PTR(gt); XAI_REQUIRE_PTR(eps); XAI_REQUIRE_PTR(x9); XAI_REQUIRE_PTR(alpha); XAI_REQUIRE_PTR(m); XAI_REQUIRE_PTR(v);
  XAI_REQUIRE(extents_ok(B, R, L, D), XAI_E_SHAPE);
  XAI_REQUIRE(limits_ok(B, R, L, D), XAI_E_UNSUPPORTED);
  const int64_t LD = int64_t(L) * D;
  const float cscale = beta / float(LD);  // L * D <= 2^25 is exact in a float
  hipLaunchKernelGGL(adam_step_kernel<T>, dim3(unsigned(xai_ceil_div(LD, kThreads)), unsigned(B)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const T*>(gt), eps, static_cast<const T*>(x9), R, LD, cscale, w1, b2, w2,
                     bc2s, step_size, adam_eps, alpha, m, v);
  return xai_launch_status();
}

}  // namespace

#define XAI_CM2IB_ENTRIES(suffix, T)                                                                                                      \
  XAI_EXPORT int xai_cm2ib_sample_##suffix(const float* alpha, const void* x9, const float* eps, int B, int R, int L, int D, void* t,     \
                                           xai_stream_t stream) {                                                                         \
    return sample<T>(alpha, x9, eps, B, R, L, D, t, stream);                                                                              \
  }                                                                                                                                       \
  XAI_EXPORT int xai_cm2ib_adam_step_##suffix(const void* gt, const float* eps, const void* x9, int B, int R, int L, int D, float beta,   \
                                              float w1, float b2, float w2, float bc2s, float step_size, float adam_eps, float* alpha,    \
                                              float* m, float* v, xai_stream_t stream) {                                                  \
    return adam_step<T>(gt, eps, x9, B, R, L, D, beta, w1, b2, w2, bc2s, step_size, adam_eps, alpha, m, v, stream);                       \
  }
XAI_CM2IB_ENTRIES(f32, float)
XAI_CM2IB_ENTRIES(f16, __half)

XAI_EXPORT int xai_cm2ib_saliency_f32(const float* alpha, const float* x9, int B, int L, int D, float* cap_out, float* out,
                                      xai_stream_t stream) {
  XAI_REQUIRE_PTR(alpha); XAI_REQUIRE_PTR(x9); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(B >= 1 && L >= 2 && D >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(limits_ok(B, 1, L, D), XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(saliency_kernel, dim3(unsigned(xai_ceil_div(L, kWaves)), unsigned(B)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), alpha, x9, L, D, cap_out, out);
  return xai_launch_status();
}
