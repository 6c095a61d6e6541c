// K82-K85: the attention rows of CLIP (game, rollout, lrp) from the attention probabilities and their gradients (libxai_cattn.so).
// include/xai_cattn.h states the arithmetic: what is rounded to the operand dtype T and where, and the order of every sum.
#include "xai_common.h"
#include "xai_cattn.h"
#include "clip_device.h"

XAI_VERSION_ENTRIES(xai_cattn_version, XAI_CATTN_VERSION, XAI_CATTN_MINOR)
XAI_EXPORT int xai_cattn_max_tokens(void) { return XAI_CATTN_MAX_TOKENS; }
XAI_EXPORT int xai_cattn_max_width(void) { return XAI_CATTN_MAX_WIDTH; }
XAI_EXPORT int xai_cattn_max_texts(void) { return XAI_CATTN_MAX_TEXTS; }

namespace {

constexpr int kThreads = 1024;  // K82, K85: 16 waves, a wave per patch column (K82) or a lane per column (K85)
constexpr int kWaves = kThreads / kWave;
constexpr int kRowThreads = 256;  // K83: a row of L <= 4096 values is at most 16 per lane
constexpr int kRowWaves = kRowThreads / kWave;
constexpr int kMatThreads = 256;  // K84: streaming, a lane per 16 bytes
constexpr int kRowUnroll = 8;     // K85: loads in flight per lane

// the header's relu: a NaN stays, -0 becomes +0
__device__ __forceinline__ float relu_keep_nan(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }

// V values of T in one access: 16 bytes when V * sizeof(T) == 16, one value when V == 1
template <typename T, int V>
struct Vec {
  float v[V];
};
template <typename T, int V>
__device__ __forceinline__ Vec<T, V> ldv(const T* p) {
  Vec<T, V> r;
  if constexpr (V == 1) {
    r.v[0] = ld(p);
  } else {
    static_assert(V * sizeof(T) == 16, "one 16-byte access");
    union { uint4 raw; T e[V]; } u;
    u.raw = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = ld(&u.e[i]);
  }
  return r;
}
template <typename T, int V>
__device__ __forceinline__ void stv(T* p, const Vec<T, V>& a) {
  if constexpr (V == 1) {
    st(p, a.v[0]);
  } else {
    union { uint4 raw; T e[V]; } u;
#pragma unroll
    for (int i = 0; i < V; ++i) st(&u.e[i], a.v[i]);
    *reinterpret_cast<uint4*>(p) = u.raw;
  }
}

// K82
template <typename T>
__global__ __launch_bounds__(kThreads) void game_map_kernel(const T* __restrict__ g, const T* __restrict__ v, int64_t v_ld_l, int64_t v_ld_b,
                                                            const T* __restrict__ a0, int L, int D, int H, int Tn,
                                                            float* __restrict__ out) {
  const int b = blockIdx.x, wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int d = D / H;
  const float heads_f = float(H);
  for (int j = 1 + wave; j < L; j += kWaves) {
    const T* vrow = v + j * v_ld_l + b * v_ld_b;
    float acc = 0.f;
    for (int t = 0; t < Tn; ++t) {
      const T* gt = g + (int64_t(b) * Tn + t) * D;
      float heads = 0.f;
      for (int h = 0; h < H; ++h) {
        float s = 0.f;
        for (int i = lane; i < d; i += kWave) s = s + ld(gt + h * d + i) * ld(vrow + h * d + i);
        const float grad = rT<T>(wave_sum(s));
        const float p = rT<T>(grad * ld(a0 + (int64_t(b) * H + h) * L + j));
        heads = heads + relu_keep_nan(p);
      }
      acc = acc + rT<T>(heads / heads_f);
    }
    if (lane == 0) out[int64_t(b) * (L - 1) + j - 1] = rT<T>(acc);
  }
}

// K83
template <typename T>
__global__ __launch_bounds__(kRowThreads) void rollout_row_kernel(const T* __restrict__ a0, int H, int L, int Tn, float* __restrict__ out) {
  __shared__ float red[kRowWaves];
  const int b = blockIdx.x, t = threadIdx.x, wave = t / kWave, lane = t & (kWave - 1);
  const float count = float(Tn * H);
  float part = 0.f;
  for (int j = t; j < L; j += kRowThreads) {
    float s = 0.f;
    for (int x = 0; x < Tn; ++x)
      for (int h = 0; h < H; ++h) s = s + ld(a0 + (int64_t(b) * H + h) * L + j);
    const float a = rT<T>(rT<T>(s) / count) + (j == 0 ? 1.f : 0.f);
    part = part + a;
  }
  part = wave_sum(part);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  float sum = 0.f;
  for (int w = 0; w < kRowWaves; ++w) sum = sum + red[w];
  // the a_j again, by the lanes that summed them: the same operations give the same bits, and no row of L floats in LDS is needed
  for (int j = t; j < L; j += kRowThreads) {
    if (j == 0) continue;
    float s = 0.f;
    for (int x = 0; x < Tn; ++x)
      for (int h = 0; h < H; ++h) s = s + ld(a0 + (int64_t(b) * H + h) * L + j);
    out[int64_t(b) * (L - 1) + j - 1] = rT<T>(rT<T>(s) / count) / sum;
  }
}

// K84: plane q = i * B + b of the operands, plane b * n + i of the result; LL = L * L values per head
template <typename T, int V>
__global__ __launch_bounds__(kMatThreads) void lrp_matrices_kernel(const T* __restrict__ attn, const T* __restrict__ grad, int n, int B, int H,
                                                                  int64_t LL, T* __restrict__ c) {
  const int q = blockIdx.y, i = q / B, b = q - i * B;
  const int64_t p = (int64_t(blockIdx.x) * kMatThreads + threadIdx.x) * V;
  if (p >= LL) return;
  const int64_t in = int64_t(q) * H * LL + p;
  const float heads_f = float(H);
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  for (int h = 0; h < H; ++h) {
    const Vec<T, V> a = ldv<T, V>(attn + in + h * LL), gr = ldv<T, V>(grad + in + h * LL);
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = acc[e] + relu_keep_nan(rT<T>(gr.v[e] * a.v[e]));
  }
  Vec<T, V> r;
#pragma unroll
  for (int e = 0; e < V; ++e) r.v[e] = rT<T>(acc[e] / heads_f);
  stv<T, V>(c + (int64_t(b) * n + i) * LL + p, r);
}

// K85
template <typename T>
__global__ __launch_bounds__(kThreads) void lrp_row_kernel(const T* __restrict__ c, int n, int L, float* __restrict__ out) {
  extern __shared__ float lds[];  // 2 L: r of this step and of the next
  float* cur = lds;
  float* nxt = lds + L;
  const int b = blockIdx.x, t = threadIdx.x;
  for (int j = t; j < L; j += kThreads) cur[j] = j == 0 ? 1.f : 0.f;
  __syncthreads();
  for (int i = n - 1; i >= 0; --i) {
    const T* m = c + (int64_t(b) * n + i) * L * L;
    for (int j = t; j < L; j += kThreads) {
      // the column is a chain of dependent additions, so eight loads are issued before the eight additions that use them: the order
      // of the sum stays ascending k, and the chain no longer waits for one load at a time (at L = 197, n = 12: 231 -> 61 us)
      float s = 0.f;
      int k = 0;
      for (; k + kRowUnroll <= L; k += kRowUnroll) {
        float cv[kRowUnroll];
#pragma unroll
        for (int u = 0; u < kRowUnroll; ++u) cv[u] = ld(m + int64_t(k + u) * L + j);
#pragma unroll
        for (int u = 0; u < kRowUnroll; ++u) s = s + cur[k + u] * cv[u];
      }
      for (; k < L; ++k) s = s + cur[k] * ld(m + int64_t(k) * L + j);
      nxt[j] = rT<T>(cur[j] + rT<T>(s));
    }
    __syncthreads();
    float* swap = cur;
    cur = nxt;
    nxt = swap;
  }
  for (int j = 1 + t; j < L; j += kThreads) out[int64_t(b) * (L - 1) + j - 1] = cur[j];
}

template <typename T>
int game_map(const void* g, const void* v, int64_t v_ld_l, int64_t v_ld_b, const void* a0, int B, int L, int D, int H, int Tn, float* out,
             xai_stream_t stream) {
  XAI_REQUIRE_PTR(g); XAI_REQUIRE_PTR(v); XAI_REQUIRE_PTR(a0); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(B >= 1 && L >= 2 && D >= 1 && H >= 1 && Tn >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(D % H == 0 && v_ld_l >= D && (B == 1 || v_ld_b >= D), XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && L <= XAI_CATTN_MAX_TOKENS && D <= XAI_CATTN_MAX_WIDTH && Tn <= XAI_CATTN_MAX_TEXTS, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(game_map_kernel<T>, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), static_cast<const T*>(g),
                     static_cast<const T*>(v), v_ld_l, v_ld_b, static_cast<const T*>(a0), L, D, H, Tn, out);
  return xai_launch_status();
}

template <typename T>
int rollout_row(const void* a0, int B, int H, int L, int Tn, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(a0); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(B >= 1 && L >= 2 && H >= 1 && Tn >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && L <= XAI_CATTN_MAX_TOKENS && H <= XAI_CATTN_MAX_WIDTH && Tn <= XAI_CATTN_MAX_TEXTS, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(rollout_row_kernel<T>, dim3(B), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream), static_cast<const T*>(a0), H, L,
                     Tn, out);
  return xai_launch_status();
}

template <typename T>
int lrp_matrices(const void* attn, const void* grad, int n, int B, int H, int L, void* c, xai_stream_t stream) {
  XAI_REQUIRE_PTR(attn); XAI_REQUIRE_PTR(grad); XAI_REQUIRE_PTR(c);
  XAI_REQUIRE(n >= 1 && B >= 1 && H >= 1 && L >= 2, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && int64_t(n) * B <= 65535 && L <= XAI_CATTN_MAX_TOKENS && H <= XAI_CATTN_MAX_WIDTH, XAI_E_UNSUPPORTED);
  constexpr int kVec = 16 / int(sizeof(T));
  const int64_t LL = int64_t(L) * L;
  const bool vec = LL % kVec == 0 && xai_can_vec4(0, {attn, grad, c});
  xai_dispatch(vec, [&](auto wide) {
    constexpr int V = decltype(wide)::value ? kVec : 1;
    const dim3 grid(unsigned(xai_ceil_div(LL, int64_t(kMatThreads) * V)), unsigned(n * B));
    hipLaunchKernelGGL((lrp_matrices_kernel<T, V>), grid, dim3(kMatThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const T*>(attn), static_cast<const T*>(grad), n, B, H, LL, static_cast<T*>(c));
  });
  return xai_launch_status();
}

template <typename T>
int lrp_row(const void* c, int n, int B, int L, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(c); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n >= 1 && B >= 1 && L >= 2, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && int64_t(n) * B <= 65535 && L <= XAI_CATTN_MAX_TOKENS, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(lrp_row_kernel<T>, dim3(B), dim3(kThreads), sizeof(float) * 2 * size_t(L), static_cast<hipStream_t>(stream),
                     static_cast<const T*>(c), n, L, out);
  return xai_launch_status();
}

}  // namespace

#define XAI_CATTN_ENTRIES(suffix, T)                                                                                                    \
  XAI_EXPORT int xai_cattn_game_map_##suffix(const void* g, const void* v, int64_t v_ld_l, int64_t v_ld_b, const void* a0, int B, int L, \
                                             int D, int H, int T_, float* out, xai_stream_t stream) {                                   \
    return game_map<T>(g, v, v_ld_l, v_ld_b, a0, B, L, D, H, T_, out, stream);                                                          \
  }                                                                                                                                     \
  XAI_EXPORT int xai_cattn_rollout_row_##suffix(const void* a0, int B, int H, int L, int T_, float* out, xai_stream_t stream) {         \
    return rollout_row<T>(a0, B, H, L, T_, out, stream);                                                                                \
  }                                                                                                                                     \
  XAI_EXPORT int xai_cattn_lrp_matrices_##suffix(const void* attn, const void* grad, int n, int B, int H, int L, void* c,               \
                                                 xai_stream_t stream) {                                                                 \
    return lrp_matrices<T>(attn, grad, n, B, H, L, c, stream);                                                                          \
  }                                                                                                                                     \
  XAI_EXPORT int xai_cattn_lrp_row_##suffix(const void* c, int n, int B, int L, float* out, xai_stream_t stream) {                      \
    return lrp_row<T>(c, n, B, L, out, stream);                                                                                         \
  }
XAI_CATTN_ENTRIES(f32, float)
XAI_CATTN_ENTRIES(f16, __half)
