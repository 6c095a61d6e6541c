// K75-K77: the class-token row of CLIP's last visual block and the Grad-ECLIP / MaskCLIP maps read from it (libxai_clip.so).
// include/xai_clip.h states the arithmetic: what is rounded to the operand dtype T and where, and the order of every sum.
#include "xai_common.h"
#include "xai_clip.h"
#include "clip_device.h"

XAI_VERSION_ENTRIES(xai_clip_version, XAI_CLIP_VERSION, XAI_CLIP_MINOR)
XAI_EXPORT int xai_clip_max_tokens(void) { return XAI_CLIP_MAX_TOKENS; }
XAI_EXPORT int xai_clip_max_width(void) { return XAI_CLIP_MAX_WIDTH; }
XAI_EXPORT int xai_clip_max_texts(void) { return XAI_CLIP_MAX_TEXTS; }

namespace {

constexpr int kThreads = 1024;  // 16 waves: a wave per token row, so L = 197 rows are 13 rounds (measured against 4 waves: profiles/r21_eclip.txt)
constexpr int kWaves = kThreads / kWave;

// the header's SUM over one row by one wave (DOT and SUMSQ are SUM over the products); every lane gets the result
template <typename F>
__device__ __forceinline__ float row_sum(int n, F term) {
  float s = 0.f;
  for (int i = threadIdx.x & (kWave - 1); i < n; i += kWave) s = s + term(i);
  return wave_sum(s);
}

// the denominator of the header's NORMALIZE
template <typename T>
__device__ __forceinline__ float norm_denominator(const T* row, int n) {
  const float sq = row_sum(n, [&](int i) { const float x = ld(row + i); return x * x; });
  const float norm = rT<T>(sqrtf(sq));
  const float eps = rT<T>(1e-12f);
  return norm < eps ? eps : norm;
}

// NORMALIZE(row) into LDS by the whole workgroup: every wave computes the same denominator, the lanes share the elements
template <typename T>
__device__ __forceinline__ void normalize_to_lds(const T* row, int n, float* dst) {
  const float m = norm_denominator<T>(row, n);
  for (int d = threadIdx.x; d < n; d += kThreads) dst[d] = rT<T>(ld(row + d) / m);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cls_attention_kernel(const T* __restrict__ q0, const T* __restrict__ k, int64_t k_ld_l,
                                                                 int64_t k_ld_b, const T* __restrict__ v, int64_t v_ld_l,
                                                                 int64_t v_ld_b, int L, int D, float scaling, T* __restrict__ scores,
                                                                 T* __restrict__ attn, T* __restrict__ att_out) {
  extern __shared__ float lds[];
  float* qs = lds;      // D: round(q * scaling)
  float* sc = lds + D;  // L: the scores, then exp, then the softmax
  __shared__ float red[kWaves];
  const int b = blockIdx.x, t = threadIdx.x, wave = t / kWave, lane = t & (kWave - 1);
  for (int d = t; d < D; d += kThreads) qs[d] = rT<T>(ld(q0 + int64_t(b) * D + d) * scaling);
  __syncthreads();
  for (int j = wave; j < L; j += kWaves) {
    const T* row = k + j * k_ld_l + b * k_ld_b;
    const float s = row_sum(D, [&](int d) { return qs[d] * ld(row + d); });
    if (lane == 0) {
      sc[j] = rT<T>(s);
      if (scores) st(scores + int64_t(b) * L + j, sc[j]);
    }
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = t; j < L; j += kThreads) m = fmaxf(m, sc[j]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
  for (int w = 1; w < kWaves; ++w) m = fmaxf(m, red[w]);
  __syncthreads();
  float part = 0.f;
  for (int j = t; j < L; j += kThreads) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    part = part + e;
  }
  part = wave_sum(part);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  float sum = 0.f;
  for (int w = 0; w < kWaves; ++w) sum = sum + red[w];
  for (int j = t; j < L; j += kThreads) {
    const float p = rT<T>(sc[j] / sum);
    sc[j] = p;
    st(attn + int64_t(b) * L + j, p);
  }
  __syncthreads();
  for (int d = t; d < D; d += kThreads) {
    const T* col = v + b * v_ld_b + d;
    float acc = 0.f;
    for (int j = 0; j < L; ++j) acc = acc + sc[j] * ld(col + j * v_ld_l);
    st(att_out + int64_t(b) * D + d, rT<T>(acc));
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void eclip_map_kernel(const T* __restrict__ q_out0, const T* __restrict__ k_out, int64_t k_ld_l,
                                                             int64_t k_ld_b, const T* __restrict__ v, int64_t v_ld_l, int64_t v_ld_b,
                                                             const T* __restrict__ grad_cls, int L, int D, int Tn, int withksim,
                                                             int withgrad, float* __restrict__ out) {
  extern __shared__ float lds[];
  float* qn = lds;     // D: NORMALIZE(q_out0)
  float* w = lds + D;  // L: the cosines, then their min-max; index 0 unused
  __shared__ float red[2 * kWaves];
  const int b = blockIdx.x, t = threadIdx.x, wave = t / kWave, lane = t & (kWave - 1);
  if (withksim) {
    normalize_to_lds<T>(q_out0 + int64_t(b) * D, D, qn);
    __syncthreads();
    for (int i = 1 + wave; i < L; i += kWaves) {
      const T* row = k_out + i * k_ld_l + b * k_ld_b;
      const float m = norm_denominator<T>(row, D);
      const float c = row_sum(D, [&](int d) { return rT<T>(qn[d] * rT<T>(ld(row + d) / m)); });
      if (lane == 0) w[i] = rT<T>(c);
    }
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int i = 1 + t; i < L; i += kThreads) {
      const float c = w[i];
      bad |= c != c;
      lo = fminf(lo, c);
      hi = fmaxf(hi, c);
    }
    block_min_max<kWaves>(lo, hi, red);
    if (__syncthreads_or(bad)) lo = hi = NAN;  // torch's min and max return a NaN that is there
    const float den = rT<T>(hi - lo);
    for (int i = 1 + t; i < L; i += kThreads) w[i] = rT<T>(rT<T>(w[i] - lo) / den);
    __syncthreads();
  }
  for (int i = 1 + wave; i < L; i += kWaves) {
    const T* vrow = v + i * v_ld_l + b * v_ld_b;
    const float wi = withksim ? w[i] : 0.f;
    float acc = 0.f;
    for (int x = 0; x < Tn; ++x) {
      const T* g = withgrad ? grad_cls + (int64_t(b) * Tn + x) * D : nullptr;
      float s;
      if (withgrad && withksim) s = row_sum(D, [&](int d) { return rT<T>(rT<T>(ld(g + d) * ld(vrow + d)) * wi); });
      else if (withgrad) s = row_sum(D, [&](int d) { return rT<T>(ld(g + d) * ld(vrow + d)); });
      else if (withksim) s = row_sum(D, [&](int d) { return rT<T>(ld(vrow + d) * wi); });
      else s = row_sum(D, [&](int d) { return ld(vrow + d); });
      s = rT<T>(s);
      acc = acc + (s > 0.f ? s : (s != s ? s : 0.f));
    }
    if (lane == 0) out[int64_t(b) * (L - 1) + i - 1] = rT<T>(acc);
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void maskclip_map_kernel(const T* __restrict__ v_final, const T* __restrict__ txt,
                                                                int64_t txt_ld_b, const T* __restrict__ k_out, int64_t k_ld_l,
                                                                int64_t k_ld_b, int L, int D, int E, int Tn, float* __restrict__ out) {
  extern __shared__ float lds[];
  float* k0 = lds;  // D: NORMALIZE(k_out[0])
  const int b = blockIdx.x, wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  normalize_to_lds<T>(k_out + b * k_ld_b, D, k0);
  __syncthreads();
  for (int i = 1 + wave; i < L; i += kWaves) {
    const T* krow = k_out + i * k_ld_l + b * k_ld_b;
    const float mk = norm_denominator<T>(krow, D);
    const float c = rT<T>(row_sum(D, [&](int d) { return rT<T>(k0[d] * rT<T>(ld(krow + d) / mk)); }));
    const T* frow = v_final + (int64_t(b) * (L - 1) + i - 1) * E;
    const float mf = norm_denominator<T>(frow, E);
    float acc = 0.f;
    for (int x = 0; x < Tn; ++x) {
      const T* trow = txt + b * txt_ld_b + int64_t(x) * E;
      const float a = rT<T>(row_sum(E, [&](int e) { return rT<T>(ld(frow + e) / mf) * ld(trow + e); }));
      acc = acc + rT<T>(a * c);
    }
    if (lane == 0) out[int64_t(b) * (L - 1) + i - 1] = rT<T>(acc);
  }
}

// the checks K75-K77 share: the extents, and the (L, B, D) strides of one operand
int check_extents(int B, int L, int D) {
  XAI_REQUIRE(B >= 1 && L >= 2 && D >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && L <= XAI_CLIP_MAX_TOKENS && D <= XAI_CLIP_MAX_WIDTH, XAI_E_UNSUPPORTED);
  return XAI_OK;
}
bool strides_ok(int64_t ld_l, int64_t ld_b, int B, int D) { return ld_l >= D && (B == 1 || ld_b >= D); }

template <typename T>
int cls_attention(const void* q0, const void* k, int64_t k_ld_l, int64_t k_ld_b, const void* v, int64_t v_ld_l, int64_t v_ld_b, int B,
                  int L, int D, float scaling, void* scores, void* attn, void* att_out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(q0); XAI_REQUIRE_PTR(k); XAI_REQUIRE_PTR(v); XAI_REQUIRE_PTR(attn); XAI_REQUIRE_PTR(att_out);
  if (const int e = check_extents(B, L, D)) return e;
  XAI_REQUIRE(strides_ok(k_ld_l, k_ld_b, B, D) && strides_ok(v_ld_l, v_ld_b, B, D), XAI_E_SHAPE);
  const size_t lds = sizeof(float) * (size_t(D) + L);
  hipLaunchKernelGGL(cls_attention_kernel<T>, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), static_cast<const T*>(q0),
                     static_cast<const T*>(k), k_ld_l, k_ld_b, static_cast<const T*>(v), v_ld_l, v_ld_b, L, D, scaling,
                     static_cast<T*>(scores), static_cast<T*>(attn), static_cast<T*>(att_out));
  return xai_launch_status();
}

template <typename T>
int eclip_map(const void* q_out0, const void* k_out, int64_t k_ld_l, int64_t k_ld_b, const void* v, int64_t v_ld_l, int64_t v_ld_b,
              const void* grad_cls, int B, int L, int D, int Tn, int withksim, int withgrad, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(v); XAI_REQUIRE_PTR(out);
  if (withksim) { XAI_REQUIRE_PTR(q_out0); XAI_REQUIRE_PTR(k_out); }
  if (withgrad) XAI_REQUIRE_PTR(grad_cls);
  if (const int e = check_extents(B, L, D)) return e;
  XAI_REQUIRE(Tn >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(Tn <= XAI_CLIP_MAX_TEXTS, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(strides_ok(v_ld_l, v_ld_b, B, D) && (!withksim || strides_ok(k_ld_l, k_ld_b, B, D)), XAI_E_SHAPE);
  const size_t lds = sizeof(float) * (size_t(D) + L);
  hipLaunchKernelGGL(eclip_map_kernel<T>, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream),
                     static_cast<const T*>(q_out0), static_cast<const T*>(k_out), k_ld_l, k_ld_b, static_cast<const T*>(v), v_ld_l,
                     v_ld_b, static_cast<const T*>(grad_cls), L, D, Tn, withksim != 0, withgrad != 0, out);
  return xai_launch_status();
}

template <typename T>
int maskclip_map(const void* v_final, const void* txt, int64_t txt_ld_b, const void* k_out, int64_t k_ld_l, int64_t k_ld_b, int B, int L,
                 int D, int E, int Tn, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(v_final); XAI_REQUIRE_PTR(txt); XAI_REQUIRE_PTR(k_out); XAI_REQUIRE_PTR(out);
  if (const int e = check_extents(B, L, D)) return e;
  XAI_REQUIRE(E >= 1 && Tn >= 1 && txt_ld_b >= 0, XAI_E_SHAPE);
  XAI_REQUIRE(E <= XAI_CLIP_MAX_WIDTH && Tn <= XAI_CLIP_MAX_TEXTS, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(strides_ok(k_ld_l, k_ld_b, B, D), XAI_E_SHAPE);
  hipLaunchKernelGGL(maskclip_map_kernel<T>, dim3(B), dim3(kThreads), sizeof(float) * size_t(D), static_cast<hipStream_t>(stream),
                     static_cast<const T*>(v_final), static_cast<const T*>(txt), txt_ld_b, static_cast<const T*>(k_out), k_ld_l, k_ld_b,
                     L, D, E, Tn, out);
  return xai_launch_status();
}

}  // namespace

#define XAI_CLIP_ENTRIES(suffix, T)                                                                                                     \
  XAI_EXPORT int xai_clip_cls_attention_##suffix(const void* q0, const void* k, int64_t k_ld_l, int64_t k_ld_b, const void* v,          \
                                                 int64_t v_ld_l, int64_t v_ld_b, int B, int L, int D, float scaling, void* scores,      \
                                                 void* attn, void* att_out, xai_stream_t stream) {                                      \
    return cls_attention<T>(q0, k, k_ld_l, k_ld_b, v, v_ld_l, v_ld_b, B, L, D, scaling, scores, attn, att_out, stream);                 \
  }                                                                                                                                     \
  XAI_EXPORT int xai_clip_eclip_map_##suffix(const void* q_out0, const void* k_out, int64_t k_ld_l, int64_t k_ld_b, const void* v,      \
                                             int64_t v_ld_l, int64_t v_ld_b, const void* grad_cls, int B, int L, int D, int T_,         \
                                             int withksim, int withgrad, float* out, xai_stream_t stream) {                             \
    return eclip_map<T>(q_out0, k_out, k_ld_l, k_ld_b, v, v_ld_l, v_ld_b, grad_cls, B, L, D, T_, withksim, withgrad, out, stream);      \
  }                                                                                                                                     \
  XAI_EXPORT int xai_clip_maskclip_map_##suffix(const void* v_final, const void* txt, int64_t txt_ld_b, const void* k_out,              \
                                                int64_t k_ld_l, int64_t k_ld_b, int B, int L, int D, int E, int T_, float* out,         \
                                                xai_stream_t stream) {                                                                  \
    return maskclip_map<T>(v_final, txt, txt_ld_b, k_out, k_ld_l, k_ld_b, B, L, D, E, T_, out, stream);                                 \
  }
XAI_CLIP_ENTRIES(f32, float)
XAI_CLIP_ENTRIES(f16, __half)
