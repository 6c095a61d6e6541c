// K86-K87: the CLIP Surgery row (libxai_csurg.so): the v-v self-attention of the dual path and the similarity map of feature surgery.
// include/xai_csurg.h states the arithmetic: the order of every sum, and the bounds behind the first exp.
#include "xai_common.h"
#include "xai_csurg.h"

XAI_VERSION_ENTRIES(xai_csurg_version, XAI_CSURG_VERSION, XAI_CSURG_MINOR)
XAI_EXPORT int xai_csurg_max_tokens(void) { return XAI_CSURG_MAX_TOKENS; }
XAI_EXPORT int xai_csurg_max_width(void) { return XAI_CSURG_MAX_WIDTH; }
XAI_EXPORT int xai_csurg_max_texts(void) { return XAI_CSURG_MAX_TEXTS; }
XAI_EXPORT int xai_csurg_lds_floats(void) { return XAI_CSURG_LDS_FLOATS; }

namespace {

// K86: waves per workgroup.  XAI_CSURG_ALT_WAVES builds the alternative that profiles/bench_surgery.py measures against it
// (DESIGN.md 4n); the library of the package is always built without it.
#ifdef XAI_CSURG_ALT_WAVES
constexpr int kVvWaves = XAI_CSURG_ALT_WAVES;
#else
constexpr int kVvWaves = XAI_CSURG_VV_WAVES;
#endif
constexpr int kVvThreads = kVvWaves * kWave;
constexpr int kVvTile = 4 * kVvWaves;  // query rows per workgroup: four per wave, so V is staged once per 16 rows
constexpr int kMapThreads = 1024;      // K87: 16 waves, a wave per (text, patch) row
constexpr int kMapWaves = kMapThreads / kWave;

// K86
__global__ __launch_bounds__(kVvThreads) void vv_attention_kernel(const float* __restrict__ v, int64_t v_ld_n, int64_t v_ld_l, int64_t v_ld_b,
                                                                  int B, int L, int D, int H, float scale, float* __restrict__ scores,
                                                                  float* __restrict__ out) {
  extern __shared__ float lds[];  // L * (d + 1): the head's V;  kVvWaves * L: a row of probabilities per wave
  const int d = D / H, ldv = d + 1;
  float* vs = lds;
  const int h = blockIdx.y, q = blockIdx.z, blk = q / B, b = q - blk * B;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  float* p = lds + L * ldv + wave * L;
  const float* vh = v + blk * v_ld_n + b * v_ld_b + int64_t(h) * d;
  for (int idx = threadIdx.x; idx < L * d; idx += kVvThreads) {
    const int j = idx / d, c = idx - j * d;
    vs[j * ldv + c] = vh[j * v_ld_l + c];
  }
  __syncthreads();
  const int i0 = blockIdx.x * kVvTile;
  const int i1 = i0 + kVvTile < L ? i0 + kVvTile : L;
  // no workgroup barrier below: the waves take different numbers of rows in the last tile, and a wave reads only its own p
  for (int i = i0 + wave; i < i1; i += kVvWaves) {
    const float* vi = vs + i * ldv;
    float mx = -INFINITY;
    for (int j = lane; j < L; j += kWave) {
      const float* vj = vs + j * ldv;
      float s = 0.f;
#pragma unroll 8
      for (int c = 0; c < d; ++c) s = s + vi[c] * vj[c];
      s = s * scale;
      p[j] = s;
      mx = fmaxf(mx, s);
      if (scores) scores[((int64_t(q) * H + h) * L + i) * L + j] = s;
    }
    mx = wave_max(mx);
    float part = 0.f;
    for (int j = lane; j < L; j += kWave) {
      const float e = expf(p[j] - mx);
      p[j] = e;
      part = part + e;
    }
    const float sum = wave_sum(part);
    for (int j = lane; j < L; j += kWave) p[j] = p[j] / sum;
    __builtin_amdgcn_wave_barrier();  // the lanes of this wave read each other's p_j from here on
    for (int c = lane; c < d; c += kWave) {
      float o = 0.f;
#pragma unroll 8
      for (int j = 0; j < L; ++j) o = o + p[j] * vs[j * ldv + c];
      out[(int64_t(q) * L + i) * D + h * d + c] = o;
    }
    __builtin_amdgcn_wave_barrier();  // the next row's scores overwrite p
  }
}

// K87
__global__ __launch_bounds__(kMapThreads) void similarity_map_kernel(const float* __restrict__ F, const float* __restrict__ txt,
                                                                     int64_t txt_ld_b, int L, int E, int T, int T_out, float* __restrict__ w_out,
                                                                     float* out) {
  extern __shared__ float lds[];  // E: n_c;  E: r_c;  T: x_t, then e_t, p_t, w_t in place
  float* nc = lds;
  float* rc = lds + E;
  float* wt = lds + 2 * E;
  const int b = blockIdx.x, t = threadIdx.x, wave = t / kWave, lane = t & (kWave - 1);
  const float* Fb = F + int64_t(b) * L * E;
  const float* tb = txt + b * txt_ld_b;
  const float texts_f = float(T);
  for (int c = t; c < E; c += kMapThreads) {
    float s = 0.f;
    for (int i = 0; i < L; ++i) {
      const float x = Fb[int64_t(i) * E + c];
      s = s + x * x;
    }
    nc[c] = sqrtf(s);
  }
  __syncthreads();
  for (int k = wave; k < T; k += kMapWaves) {
    float s = 0.f;
    for (int c = lane; c < E; c += kWave) s = s + (Fb[c] / nc[c]) * tb[int64_t(k) * E + c];
    s = wave_sum(s);
    if (lane == 0) wt[k] = 2.f * s;
  }
  __syncthreads();
  if (wave == 0) {
    float mx = -INFINITY;
    for (int k = lane; k < T; k += kWave) mx = fmaxf(mx, wt[k]);
    mx = wave_max(mx);
    float part = 0.f;
    for (int k = lane; k < T; k += kWave) {
      const float e = expf(wt[k] - mx);
      wt[k] = e;
      part = part + e;
    }
    const float sum = wave_sum(part);
    part = 0.f;
    for (int k = lane; k < T; k += kWave) {
      const float pk = wt[k] / sum;
      wt[k] = pk;
      part = part + pk;
    }
    const float mean = wave_sum(part) / texts_f;
    for (int k = lane; k < T; k += kWave) {
      const float wk = wt[k] / mean;
      wt[k] = wk;
      if (w_out) w_out[int64_t(b) * T + k] = wk;
    }
  }
  __syncthreads();
  for (int c = t; c < E; c += kMapThreads) {
    float s = 0.f;
    for (int k = 0; k < T; ++k) s = s + wt[k] * tb[int64_t(k) * E + c];
    rc[c] = s / texts_f;
  }
  __syncthreads();
  const int rows = L - 1;
  float* ob = out + int64_t(b) * T_out * rows;
  for (int64_t u = wave; u < int64_t(T_out) * rows; u += kMapWaves) {
    const int k = int(u / rows), i = 1 + int(u - int64_t(k) * rows);
    const float wk = wt[k];
    float s = 0.f;
    for (int c = lane; c < E; c += kWave) s = s + (Fb[int64_t(i) * E + c] / nc[c]) * (wk * tb[int64_t(k) * E + c] - rc[c]);
    s = wave_sum(s);
    if (lane == 0) ob[u] = s;
  }
  __syncthreads();  // the s_it of every wave, in global memory, are visible to the workgroup behind it
  for (int k = wave; k < T_out; k += kMapWaves) {
    float* o = ob + int64_t(k) * rows;
    float lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    for (int i = lane; i < rows; i += kWave) {
      const float x = o[i];
      nan |= x != x;
      lo = fminf(lo, x);
      hi = fmaxf(hi, x);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (wave_max(nan)) lo = hi = NAN;
    const float range = hi - lo;
    for (int i = lane; i < rows; i += kWave) o[i] = (o[i] - lo) / range;
  }
}

}  // namespace

XAI_EXPORT int xai_csurg_vv_waves(void) { return kVvWaves; }

XAI_EXPORT int xai_csurg_vv_attention_f32(const float* v, int64_t v_ld_n, int64_t v_ld_l, int64_t v_ld_b, int n, int B, int L, int D, int H,
                                          float scale, float* scores, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(v); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n >= 1 && B >= 1 && L >= 2 && D >= 1 && H >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(D % H == 0 && v_ld_l >= D && (B == 1 || v_ld_b >= D) && (n == 1 || v_ld_n >= D), XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && H <= 65535 && int64_t(n) * B <= 65535 && L <= XAI_CSURG_MAX_TOKENS && D <= XAI_CSURG_MAX_WIDTH,
              XAI_E_UNSUPPORTED);
  const int64_t floats = int64_t(L) * (D / H + 1 + kVvWaves);
  XAI_REQUIRE(floats <= XAI_CSURG_LDS_FLOATS, XAI_E_UNSUPPORTED);
  const dim3 grid(unsigned(xai_ceil_div(L, kVvTile)), unsigned(H), unsigned(n * B));
  hipLaunchKernelGGL(vv_attention_kernel, grid, dim3(kVvThreads), sizeof(float) * size_t(floats), static_cast<hipStream_t>(stream), v, v_ld_n,
                     v_ld_l, v_ld_b, B, L, D, H, scale, scores, out);
  return xai_launch_status();
}

XAI_EXPORT int xai_csurg_similarity_map_f32(const float* F, const float* txt, int64_t txt_ld_b, int B, int L, int E, int T, int T_out,
                                            float* w, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(F); XAI_REQUIRE_PTR(txt); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(B >= 1 && L >= 2 && E >= 1 && T >= 1 && T_out >= 1 && T_out <= T, XAI_E_SHAPE);
  XAI_REQUIRE(txt_ld_b == 0 || txt_ld_b >= int64_t(T) * E, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && L <= XAI_CSURG_MAX_TOKENS && E <= XAI_CSURG_MAX_WIDTH && T <= XAI_CSURG_MAX_TEXTS, XAI_E_UNSUPPORTED);
  const int64_t floats = 2 * int64_t(E) + T;
  XAI_REQUIRE(floats <= XAI_CSURG_LDS_FLOATS, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(similarity_map_kernel, dim3(B), dim3(kMapThreads), sizeof(float) * size_t(floats), static_cast<hipStream_t>(stream), F,
                     txt, txt_ld_b, L, E, T, T_out, w, out);
  return xai_launch_status();
}
