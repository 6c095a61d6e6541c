// Classifier-side fusion (opt-in, xai_engine/prepare.py): eval-mode BatchNorm2d + ReLU (+ residual add) as ONE
// element-wise kernel per direction instead of PyTorch's three to five.
//
//   forward   y  = relu( bn(x) [+ identity] ),   bn(x) = ((x - mean) * invstd) * weight + bias
//   backward  g1 = y > 0 ? gy : 0;   gx = (g1 * weight) * invstd;   g_identity = g1
//
// NCHW, flat indexing: a lane owns 4 consecutive elements when HW % 4 == 0 (they share a channel).  `variant` selects
// among arithmetically equivalent orderings of the BN expression (bit 0: rsqrt instead of 1/sqrt; bits 1-2: grouping;
// bit 3: fused multiply-add for the last step); xai_engine/prepare.py uses the one that reproduces PyTorch-ROCm's own
// eval-mode kernels bit for bit (found by profiles/experiments/exp_bn_variants.py).
#include "xai_bn_device.h"

namespace {

// o[k] = act( bn(x[i+k]) [+ identity[i+k] | + bn2(identity[i+k])] ), stored to y as one float4; i + 3 < n
template <bool ADD, bool RELU>
__device__ __forceinline__ void flat_fwd4(const float* __restrict__ x, const float* __restrict__ idt, const float* __restrict__ w,
                                          const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ var,
                                          float eps, const BnParams& bn2, int variant, int C, int HW, int64_t n, int64_t i,
                                          float* __restrict__ y, float (&o)[4]) {
  const XaiBnLane s = xai_bn_lane_first(i, n, HW, C);
  BnChannel p[4];
  lane_channels(p, s, HW, C, [&](int c) { return BnChannel{mean[c], inv_std(var[c], eps, variant), w[c], b[c]}; });
  const float4 v = ld4_nt(x + i);
  const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = bn_value(xv[k], p[k].m, p[k].is, p[k].w, p[k].b, variant);
  if (ADD) {
    const float4 t = ld4_nt(idt + i);
    float a[4] = {t.x, t.y, t.z, t.w};
    if (bn2.w != nullptr) {
      BnChannel q[4];
      lane_channels(q, s, HW, C, [&](int c) { return BnChannel{bn2.mean[c], inv_std(bn2.var[c], bn2.eps, variant), bn2.w[c], bn2.b[c]}; });
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = bn_value(a[k], q[k].m, q[k].is, q[k].w, q[k].b, variant);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] += a[k];
  }
  if (RELU) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
  }
  st4(y + i, make_float4(o[0], o[1], o[2], o[3]));
}

// g = gy (+ gy2) [guided clamp];  g1 = open[k] ? g : 0;  gx = bn_grad(g1);  g_identity = g1 | bn_grad through bn2;  i + 3 < n
template <bool ADD, bool GUIDED>
__device__ __forceinline__ void flat_bwd4(const float* __restrict__ gy, const float* __restrict__ gy2, const bool (&open)[4],
                                          const float* __restrict__ w, const float* __restrict__ var, float eps, const BnParams& bn2,
                                          int variant, int C, int HW, int64_t n, int64_t i, float* __restrict__ gx,
                                          float* __restrict__ gid) {
  const XaiBnLane s = xai_bn_lane_first(i, n, HW, C);
  BnChannel p[4];
  lane_channels(p, s, HW, C, [&](int c) { return BnChannel{0.f, inv_std(var[c], eps, variant), w[c], 0.f}; });
  const float4 t = ld4_nt(gy + i);
  float g[4] = {t.x, t.y, t.z, t.w};
  if (gy2 != nullptr) {
    const float4 h = ld4_nt(gy2 + i);
    g[0] += h.x; g[1] += h.y; g[2] += h.z; g[3] += h.w;
  }
  float g1[4], o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (GUIDED) g[k] = guided_clamp(g[k]);
    g1[k] = open[k] ? g[k] : 0.f;
    o[k] = bn_grad(g1[k], p[k].is, p[k].w, variant);
  }
  st4(gx + i, make_float4(o[0], o[1], o[2], o[3]));
  if (ADD) {
    if (bn2.w != nullptr) {                             // g_identity goes through the identity operand's own BatchNorm
      BnChannel q[4];
      lane_channels(q, s, HW, C, [&](int c) { return BnChannel{0.f, inv_std(bn2.var[c], bn2.eps, variant), bn2.w[c], 0.f}; });
#pragma unroll
      for (int k = 0; k < 4; ++k) g1[k] = bn_grad(g1[k], q[k].is, q[k].w, variant);
    }
    st4(gid + i, make_float4(g1[0], g1[1], g1[2], g1[3]));
  }
}

template <bool VEC, bool ADD, bool RELU>
__global__ __launch_bounds__(kBlock) void bn_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ idt,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                            BnParams bn2, int variant, int C, int HW, int64_t n, int flat,
                                                            float* __restrict__ y) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * (VEC ? 4 : flat ? 4 : 1);
  if (i >= n) return;
  if (!VEC && flat) {
    float o[4];
    flat_fwd4<ADD, RELU>(x, idt, w, b, mean, var, eps, bn2, variant, C, HW, n, i, y, o);
    return;
  }
  const int c = static_cast<int>((i / HW) % C);
  const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
  const bool second = ADD && bn2.w != nullptr;
  float m2 = 0.f, is2 = 1.f, w2 = 1.f, b2 = 0.f;
  if (second) { m2 = bn2.mean[c]; is2 = inv_std(bn2.var[c], bn2.eps, variant); w2 = bn2.w[c]; b2 = bn2.b[c]; }
  if (VEC) {
    const float4 v = ld4_nt(x + i);
    float4 o = make_float4(bn_value(v.x, m, is, wc, bc, variant), bn_value(v.y, m, is, wc, bc, variant),
                           bn_value(v.z, m, is, wc, bc, variant), bn_value(v.w, m, is, wc, bc, variant));
    if (ADD) {
      float4 a = ld4_nt(idt + i);
      if (second)
        a = make_float4(bn_value(a.x, m2, is2, w2, b2, variant), bn_value(a.y, m2, is2, w2, b2, variant),
                        bn_value(a.z, m2, is2, w2, b2, variant), bn_value(a.w, m2, is2, w2, b2, variant));
      o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
    }
    if (RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    st4(y + i, o);
  } else {
    float o = bn_value(x[i], m, is, wc, bc, variant);
    if (ADD) o += second ? bn_value(idt[i], m2, is2, w2, b2, variant) : idt[i];
    if (RELU) o = fmaxf(o, 0.f);
    y[i] = o;
  }
}

// gy2 (nullable): a second incoming gradient of the same output, summed first -- the residual join (the block output feeds
// the next block's first convolution AND its identity path), which autograd would otherwise add in a kernel of its own.
template <bool VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void bn_relu_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ gy2,
                                                             const float* __restrict__ y, const float* __restrict__ w,
                                                             const float* __restrict__ var, float eps, BnParams bn2, int variant,
                                                             int C, int HW, int64_t n, int flat, float* __restrict__ gx,
                                                             float* __restrict__ gid) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * (VEC ? 4 : flat ? 4 : 1);
  if (i >= n) return;
  if (!VEC && flat) {
    const float4 o = ld4_nt(y + i);
    const bool open[4] = {o.x > 0.f, o.y > 0.f, o.z > 0.f, o.w > 0.f};
    flat_bwd4<ADD, false>(gy, gy2, open, w, var, eps, bn2, variant, C, HW, n, i, gx, gid);
    return;
  }
  const int c = static_cast<int>((i / HW) % C);
  const float is = inv_std(var[c], eps, variant), wc = w[c];
  const bool second = ADD && bn2.w != nullptr;          // g_identity then goes through the identity operand's own BatchNorm
  float is2 = 1.f, w2 = 1.f;
  if (second) { is2 = inv_std(bn2.var[c], bn2.eps, variant); w2 = bn2.w[c]; }
  if (VEC) {
    float4 g = ld4_nt(gy + i);
    if (gy2 != nullptr) {
      const float4 h = ld4_nt(gy2 + i);
      g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w;
    }
    const float4 o = ld4_nt(y + i);
    const float4 g1 = make_float4(o.x > 0.f ? g.x : 0.f, o.y > 0.f ? g.y : 0.f, o.z > 0.f ? g.z : 0.f, o.w > 0.f ? g.w : 0.f);
    st4(gx + i, make_float4(bn_grad(g1.x, is, wc, variant), bn_grad(g1.y, is, wc, variant), bn_grad(g1.z, is, wc, variant),
                            bn_grad(g1.w, is, wc, variant)));
    if (ADD)
      st4(gid + i, second ? make_float4(bn_grad(g1.x, is2, w2, variant), bn_grad(g1.y, is2, w2, variant), bn_grad(g1.z, is2, w2, variant),
                                        bn_grad(g1.w, is2, w2, variant))
                          : g1);
  } else {
    float g = gy[i];
    if (gy2 != nullptr) g += gy2[i];
    const float g1 = y[i] > 0.f ? g : 0.f;
    gx[i] = bn_grad(g1, is, wc, variant);
    if (ADD) gid[i] = second ? bn_grad(g1, is2, w2, variant) : g1;
  }
}

}  // namespace

XAI_EXPORT int xai_bn_act_fwd_f32(const float* x, const float* identity, const float* weight, const float* bias, const float* mean,
                                  const float* var, float eps, const float* weight2, const float* bias2, const float* mean2,
                                  const float* var2, float eps2, int variant, int relu, int N, int C, int HW, float* y,
                                  xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(bias); XAI_REQUIRE_PTR(mean); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(y);
  XAI_REQUIRE(N > 0 && C > 0 && HW > 0 && variant >= 0 && variant < 16, XAI_E_SHAPE);
  if (weight2 != nullptr) {
    XAI_REQUIRE_PTR(identity); XAI_REQUIRE_PTR(bias2); XAI_REQUIRE_PTR(mean2); XAI_REQUIRE_PTR(var2);
  }
  const BnParams bn2{weight2, bias2, mean2, var2, eps2};
  const int64_t n = static_cast<int64_t>(N) * C * HW;
  const XaiBnPath path = xai_bn_path(n, HW, bn_low_bits({x, y, identity}));
  const bool vec = path == XAI_BN_VEC4;
  const int flat = path == XAI_BN_FLAT4;                // taken inside the VEC = false instantiations
  const unsigned grid = static_cast<unsigned>(xai_ceil_div(n, static_cast<int64_t>(kBlock) * (path == XAI_BN_SCALAR ? 1 : 4)));
  hipStream_t st = static_cast<hipStream_t>(stream);
#define XAI_BN_FWD(V, A, R) \
  hipLaunchKernelGGL((bn_act_fwd_kernel<V, A, R>), dim3(grid), dim3(kBlock), 0, st, x, identity, weight, bias, mean, var, eps, bn2, variant, C, HW, n, flat, y)
  if (identity != nullptr) {
    XAI_REQUIRE(relu != 0, XAI_E_UNSUPPORTED);
    if (vec) XAI_BN_FWD(true, true, true); else XAI_BN_FWD(false, true, true);
  } else if (relu) {
    if (vec) XAI_BN_FWD(true, false, true); else XAI_BN_FWD(false, false, true);
  } else {
    if (vec) XAI_BN_FWD(true, false, false); else XAI_BN_FWD(false, false, false);
  }
#undef XAI_BN_FWD
  return xai_launch_status();
}

XAI_EXPORT int xai_bn_relu_bwd_f32(const float* gy, const float* gy2, const float* y, const float* weight, const float* var, float eps,
                                   const float* weight2, const float* var2, float eps2, int variant, int N, int C, int HW, float* gx,
                                   float* g_identity, xai_stream_t stream) {
  XAI_REQUIRE_PTR(gy); XAI_REQUIRE_PTR(y); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(gx);
  XAI_REQUIRE(N > 0 && C > 0 && HW > 0 && variant >= 0 && variant < 16, XAI_E_SHAPE);
  const int64_t n = static_cast<int64_t>(N) * C * HW;
  if (weight2 != nullptr) {
    XAI_REQUIRE_PTR(g_identity); XAI_REQUIRE_PTR(var2);
  }
  const BnParams bn2{weight2, nullptr, nullptr, var2, eps2};
  const XaiBnPath path = xai_bn_path(n, HW, bn_low_bits({gy, y, gx, g_identity, gy2}));
  const bool vec = path == XAI_BN_VEC4;
  const int flat = path == XAI_BN_FLAT4;
  const unsigned grid = static_cast<unsigned>(xai_ceil_div(n, static_cast<int64_t>(kBlock) * (path == XAI_BN_SCALAR ? 1 : 4)));
  hipStream_t st = static_cast<hipStream_t>(stream);
#define XAI_BN_BWD(V, A) \
  hipLaunchKernelGGL((bn_relu_bwd_kernel<V, A>), dim3(grid), dim3(kBlock), 0, st, gy, gy2, y, weight, var, eps, bn2, variant, C, HW, n, flat, gx, g_identity)
  if (g_identity != nullptr) {
    if (vec) XAI_BN_BWD(true, true); else XAI_BN_BWD(false, true);
  } else {
    if (vec) XAI_BN_BWD(true, false); else XAI_BN_BWD(false, false);
  }
#undef XAI_BN_BWD
  return xai_launch_status();
}

// ---- the same pair with a 1-bit ReLU gate in place of y in the backward ----------------------------------------------
// The backward above loads y only to evaluate `y > 0`.  The forward form below also writes that bit per element (NaN -> 0)
// into a caller-provided mask, and the backward form reads the mask instead of y: 1/32 of the bytes.
//
// Mask layout, by flat element index e of the [N][C][HW] tensor (private to this pair; xai_bn_gate_mask_bytes(n)):
// 64-bit words, four per group of 256 consecutive elements;  the gate of e is
//     bit (e % 256) / 4  of word  (e / 256) * 4 + e % 4.
// A lane owns elements 4t .. 4t+3, so a wavefront owns exactly one group and word c of the group is the wave ballot of
// component c; lanes 0..3 store the four words with ordinary vector stores.  Every word of the mask is written, the tail
// group's bits of elements >= n as 0: nothing relies on a zero-fill.  When HW % 4 != 0 (layer4: HW = 49) the four
// elements of a lane can straddle two channels and any n is allowed: with n % 4 == 0 and aligned tensors they take the flat
// 16-byte path above (`flat`), otherwise they are loaded one by one with the channel taken per element -- same arithmetic
// per element, same layout.
namespace {

template <bool VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void bn_relu_fwd_mask_kernel(const float* __restrict__ x, const float* __restrict__ idt,
                                                                  const float* __restrict__ w, const float* __restrict__ b,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  float eps, BnParams bn2, int variant, int C, int HW, int64_t n,
                                                                  int flat, float* __restrict__ y, uint64_t* __restrict__ mask) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t group = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (group * kGateGroup >= n) return;                  // wave-uniform: this wavefront owns no element and no mask word
  const int64_t i = group * kGateGroup + lane * 4;
  const bool second = ADD && bn2.w != nullptr;
  float o[4] = {0.f, 0.f, 0.f, 0.f};                    // elements >= n keep +0: gate bit 0
  if (VEC) {                                            // HW % 4 == 0, so n % 4 == 0: a lane is inside or outside as a whole
    if (i < n) {
      const int c = static_cast<int>((i / HW) % C);
      const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
      const float4 v = ld4_nt(x + i);
      o[0] = bn_value(v.x, m, is, wc, bc, variant); o[1] = bn_value(v.y, m, is, wc, bc, variant);
      o[2] = bn_value(v.z, m, is, wc, bc, variant); o[3] = bn_value(v.w, m, is, wc, bc, variant);
      if (ADD) {
        float4 a = ld4_nt(idt + i);
        if (second) {
          const float m2 = bn2.mean[c], is2 = inv_std(bn2.var[c], bn2.eps, variant), w2 = bn2.w[c], b2 = bn2.b[c];
          a = make_float4(bn_value(a.x, m2, is2, w2, b2, variant), bn_value(a.y, m2, is2, w2, b2, variant),
                          bn_value(a.z, m2, is2, w2, b2, variant), bn_value(a.w, m2, is2, w2, b2, variant));
        }
        o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
      st4(y + i, make_float4(o[0], o[1], o[2], o[3]));
    }
  } else if (flat) {                                    // n % 4 == 0 here too: a lane is inside or outside as a whole
    if (i < n) flat_fwd4<ADD, true>(x, idt, w, b, mean, var, eps, bn2, variant, C, HW, n, i, y, o);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t e = i + k;
      if (e < n) {
        const int c = static_cast<int>((e / HW) % C);
        float v = bn_value(x[e], mean[c], inv_std(var[c], eps, variant), w[c], b[c], variant);
        if (ADD) v += second ? bn_value(idt[e], bn2.mean[c], inv_std(bn2.var[c], bn2.eps, variant), bn2.w[c], bn2.b[c], variant) : idt[e];
        v = fmaxf(v, 0.f);
        y[e] = v;
        o[k] = v;
      }
    }
  }
  store_gate_words(mask, group, lane, o[0] > 0.f, o[1] > 0.f, o[2] > 0.f, o[3] > 0.f);
}

// GUIDED: the clamp above on g = gy (+ gy2), then the gate; nothing else differs
template <bool VEC, bool ADD, bool GUIDED>
__global__ __launch_bounds__(kBlock) void bn_relu_bwd_mask_kernel(const float* __restrict__ gy, const float* __restrict__ gy2,
                                                                  const uint64_t* __restrict__ mask, const float* __restrict__ w,
                                                                  const float* __restrict__ var, float eps, BnParams bn2, int variant,
                                                                  int C, int HW, int64_t n, int flat, float* __restrict__ gx,
                                                                  float* __restrict__ gid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t group = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (group * kGateGroup >= n) return;
  const int64_t i = group * kGateGroup + lane * 4;
  if (i >= n) return;
  const uint64_t* mw = mask + group * 4;                // wave-uniform address: four words shared by the whole wavefront
  const bool open[4] = {((mw[0] >> lane) & 1) != 0, ((mw[1] >> lane) & 1) != 0, ((mw[2] >> lane) & 1) != 0, ((mw[3] >> lane) & 1) != 0};
  const bool second = ADD && bn2.w != nullptr;          // g_identity then goes through the identity operand's own BatchNorm
  if (VEC) {
    const int c = static_cast<int>((i / HW) % C);
    const float is = inv_std(var[c], eps, variant), wc = w[c];
    float is2 = 1.f, w2 = 1.f;
    if (second) { is2 = inv_std(bn2.var[c], bn2.eps, variant); w2 = bn2.w[c]; }
    float4 g = ld4_nt(gy + i);
    if (gy2 != nullptr) {
      const float4 h = ld4_nt(gy2 + i);
      g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w;
    }
    if (GUIDED) g = make_float4(guided_clamp(g.x), guided_clamp(g.y), guided_clamp(g.z), guided_clamp(g.w));
    const float4 g1 = make_float4(open[0] ? g.x : 0.f, open[1] ? g.y : 0.f, open[2] ? g.z : 0.f, open[3] ? g.w : 0.f);
    st4(gx + i, make_float4(bn_grad(g1.x, is, wc, variant), bn_grad(g1.y, is, wc, variant), bn_grad(g1.z, is, wc, variant),
                            bn_grad(g1.w, is, wc, variant)));
    if (ADD)
      st4(gid + i, second ? make_float4(bn_grad(g1.x, is2, w2, variant), bn_grad(g1.y, is2, w2, variant), bn_grad(g1.z, is2, w2, variant),
                                        bn_grad(g1.w, is2, w2, variant))
                          : g1);
  } else if (flat) {
    flat_bwd4<ADD, GUIDED>(gy, gy2, open, w, var, eps, bn2, variant, C, HW, n, i, gx, gid);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t e = i + k;
      if (e < n) {
        const int c = static_cast<int>((e / HW) % C);
        float g = gy[e];
        if (gy2 != nullptr) g += gy2[e];
        if (GUIDED) g = guided_clamp(g);
        const float g1 = open[k] ? g : 0.f;
        gx[e] = bn_grad(g1, inv_std(var[c], eps, variant), w[c], variant);
        if (ADD) gid[e] = second ? bn_grad(g1, inv_std(bn2.var[c], bn2.eps, variant), bn2.w[c], variant) : g1;
      }
    }
  }
}

}  // namespace

XAI_EXPORT size_t xai_bn_gate_mask_bytes(int64_t n) {
  return n <= 0 ? 0 : static_cast<size_t>(xai_ceil_div(n, kGateGroup)) * 4 * sizeof(uint64_t);
}

XAI_EXPORT int xai_bn_relu_fwd_mask_f32(const float* x, const float* identity, const float* weight, const float* bias, const float* mean,
                                        const float* var, float eps, const float* weight2, const float* bias2, const float* mean2,
                                        const float* var2, float eps2, int variant, int N, int C, int HW, float* y, void* mask,
                                        xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(bias); XAI_REQUIRE_PTR(mean); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(y);
  XAI_REQUIRE_PTR(mask);
  XAI_REQUIRE(N > 0 && C > 0 && HW > 0 && variant >= 0 && variant < 16, XAI_E_SHAPE);
  XAI_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 7u) == 0, XAI_E_SHAPE);
  if (weight2 != nullptr) {
    XAI_REQUIRE_PTR(identity); XAI_REQUIRE_PTR(bias2); XAI_REQUIRE_PTR(mean2); XAI_REQUIRE_PTR(var2);
  }
  const BnParams bn2{weight2, bias2, mean2, var2, eps2};
  const int64_t n = static_cast<int64_t>(N) * C * HW;
  const XaiBnPath path = xai_bn_path(n, HW, bn_low_bits({x, y, identity}));
  const bool vec = path == XAI_BN_VEC4;
  const int flat = path == XAI_BN_FLAT4;
  const unsigned grid = static_cast<unsigned>(xai_ceil_div(n, static_cast<int64_t>(kBlock) * 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint64_t* mk = static_cast<uint64_t*>(mask);
#define XAI_BN_FWDM(V, A) \
  hipLaunchKernelGGL((bn_relu_fwd_mask_kernel<V, A>), dim3(grid), dim3(kBlock), 0, st, x, identity, weight, bias, mean, var, eps, bn2, variant, C, HW, n, flat, y, mk)
  if (identity != nullptr) {
    if (vec) XAI_BN_FWDM(true, true); else XAI_BN_FWDM(false, true);
  } else {
    if (vec) XAI_BN_FWDM(true, false); else XAI_BN_FWDM(false, false);
  }
#undef XAI_BN_FWDM
  return xai_launch_status();
}

template <bool GUIDED>
static int bn_relu_bwd_mask_launch(const float* gy, const float* gy2, const void* mask, const float* weight, const float* var, float eps,
                                   const float* weight2, const float* var2, float eps2, int variant, int N, int C, int HW, float* gx,
                                   float* g_identity, xai_stream_t stream) {
  XAI_REQUIRE_PTR(gy); XAI_REQUIRE_PTR(mask); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(gx);
  XAI_REQUIRE(N > 0 && C > 0 && HW > 0 && variant >= 0 && variant < 16, XAI_E_SHAPE);
  XAI_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 7u) == 0, XAI_E_SHAPE);
  const int64_t n = static_cast<int64_t>(N) * C * HW;
  if (weight2 != nullptr) {
    XAI_REQUIRE_PTR(g_identity); XAI_REQUIRE_PTR(var2);
  }
  const BnParams bn2{weight2, nullptr, nullptr, var2, eps2};
  const XaiBnPath path = xai_bn_path(n, HW, bn_low_bits({gy, gx, g_identity, gy2}));
  const bool vec = path == XAI_BN_VEC4;
  const int flat = path == XAI_BN_FLAT4;
  const unsigned grid = static_cast<unsigned>(xai_ceil_div(n, static_cast<int64_t>(kBlock) * 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint64_t* mk = static_cast<const uint64_t*>(mask);
#define XAI_BN_BWDM(V, A) \
  hipLaunchKernelGGL((bn_relu_bwd_mask_kernel<V, A, GUIDED>), dim3(grid), dim3(kBlock), 0, st, gy, gy2, mk, weight, var, eps, bn2, variant, C, HW, n, flat, gx, g_identity)
  if (g_identity != nullptr) {
    if (vec) XAI_BN_BWDM(true, true); else XAI_BN_BWDM(false, true);
  } else {
    if (vec) XAI_BN_BWDM(true, false); else XAI_BN_BWDM(false, false);
  }
#undef XAI_BN_BWDM
  return xai_launch_status();
}

XAI_EXPORT int xai_bn_relu_bwd_mask_f32(const float* gy, const float* gy2, const void* mask, const float* weight, const float* var,
                                        float eps, const float* weight2, const float* var2, float eps2, int variant, int N, int C, int HW,
                                        float* gx, float* g_identity, xai_stream_t stream) {
  return bn_relu_bwd_mask_launch<false>(gy, gy2, mask, weight, var, eps, weight2, var2, eps2, variant, N, C, HW, gx, g_identity, stream);
}

XAI_EXPORT int xai_bn_relu_bwd_mask_guided_f32(const float* gy, const float* gy2, const void* mask, const float* weight, const float* var,
                                               float eps, const float* weight2, const float* var2, float eps2, int variant, int N, int C,
                                               int HW, float* gx, float* g_identity, xai_stream_t stream) {
  return bn_relu_bwd_mask_launch<true>(gy, gy2, mask, weight, var, eps, weight2, var2, eps2, variant, N, C, HW, gx, g_identity, stream);
}

// ---- MaxPool2d backward (stem) ------------------------------------------------------------------------------------
// gx[plane][h][w] = sum of gy[plane][ph][pw] over the pooling windows (ph, pw ascending) whose arg-max index (from
// PyTorch's own forward, int64 = h * W + w) is this position -- the loop and the accumulation order of PyTorch's
// max_pool_backward_nchw, so the result is bit-identical; one lane per input element, coalesced stores, the window
// reads hit L1 / L2 (PyTorch's kernel takes 611 us for the benchmark's 100 x 64 x 112 x 112 stem activation).
namespace {

// grid = (ceil(H*W / 256), planes), 32-bit index arithmetic.  NW = windows per axis that can cover one input position
// (ceil(kernel / stride)); for NW <= 2 all candidate indices AND gradients are loaded unconditionally up front and then
// selected -- with the load of gy behind the index comparison, every lane walked a chain of up to 8 dependent memory
// latencies and the kernel took as long as PyTorch's (570 us for the benchmark's stem activation).
template <int NW>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ gy, const int64_t* __restrict__ idx, int H, int W,
                                                          int PH, int PW, int k, int stride, int pad, float* __restrict__ gx) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int h = p / W, w = p - h * W;
  const int ph0 = (h + pad < k) ? 0 : (h + pad - k) / stride + 1;
  const int ph1 = min((h + pad) / stride + 1, PH);
  const int pw0 = (w + pad < k) ? 0 : (w + pad - k) / stride + 1;
  const int pw1 = min((w + pad) / stride + 1, PW);
  const int64_t off = static_cast<int64_t>(blockIdx.y) * PH * PW;
  const int64_t* ip = idx + off;
  const float* gp = gy + off;
  float g = 0.f;
  if (NW > 0) {
    constexpr int M = NW > 0 ? NW : 1;
    int hit[M][M];
    float val[M][M];
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
      for (int b = 0; b < NW; ++b) {
        const int ph = ph0 + a, pw = pw0 + b;
        const bool in = ph < ph1 && pw < pw1;
        const int q = in ? ph * PW + pw : 0;
        hit[a][b] = in ? static_cast<int>(ip[q]) : -1;
        val[a][b] = gp[q];
      }
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
      for (int b = 0; b < NW; ++b)
        if (hit[a][b] == p) g += val[a][b];
  } else {
    for (int ph = ph0; ph < ph1; ++ph)
      for (int pw = pw0; pw < pw1; ++pw) {
        const int q = ph * PW + pw;
        if (static_cast<int>(ip[q]) == p) g += gp[q];
      }
  }
  gx[static_cast<int64_t>(blockIdx.y) * H * W + p] = g;
}

// Tiled form of the same gather: a workgroup owns kBwdRows input rows of one plane; the pooled rows whose windows can
// reach them (indices truncated to int32, and gradients) are staged in LDS with coalesced loads, 8 in flight per lane, and
// every lane then walks its (at most NW x NW) candidate windows in LDS in the same (ph, pw) order.
constexpr int kBwdRows = 16;

template <int NW>
__global__ __launch_bounds__(256) void maxpool_bwd_tiled_kernel(const float* __restrict__ gy, const int64_t* __restrict__ idx, int H, int W,
                                                                int PH, int PW, int k, int stride, int pad, float* __restrict__ gx) {
  extern __shared__ int lds_i[];                         // [rows][PW] indices, then [rows][PW] gradients
  const int h0 = blockIdx.x * kBwdRows;
  const int h_last = min(h0 + kBwdRows, H) - 1;
  const int pr0 = (h0 + pad < k) ? 0 : (h0 + pad - k) / stride + 1;           // first pooled row that can cover row h0
  const int pr1 = min((h_last + pad) / stride + 1, PH);                         // one past the last that can cover h_last
  const int rows = pr1 - pr0;
  float* lds_g = reinterpret_cast<float*>(lds_i + rows * PW);
  const int64_t off = static_cast<int64_t>(blockIdx.y) * PH * PW + static_cast<int64_t>(pr0) * PW;
  const int total = rows * PW;
  for (int base = threadIdx.x; base < total; base += 256 * 8) {
    int iv[8];
    float gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      iv[u] = i < total ? static_cast<int>(idx[off + i]) : -1;
      gv[u] = i < total ? gy[off + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      if (i < total) { lds_i[i] = iv[u]; lds_g[i] = gv[u]; }
    }
  }
  __syncthreads();
  const int n_rows = h_last - h0 + 1;
  for (int q = threadIdx.x; q < n_rows * W; q += 256) {
    const int r = q / W, w = q - r * W;
    const int h = h0 + r, p = h * W + w;
    const int ph0 = (h + pad < k) ? 0 : (h + pad - k) / stride + 1;
    const int ph1 = min((h + pad) / stride + 1, PH);
    const int pw0 = (w + pad < k) ? 0 : (w + pad - k) / stride + 1;
    const int pw1 = min((w + pad) / stride + 1, PW);
    float g = 0.f;
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
      for (int b = 0; b < NW; ++b) {
        const int ph = ph0 + a, pw = pw0 + b;
        if (ph < ph1 && pw < pw1) {
          const int t = (ph - pr0) * PW + pw;
          if (lds_i[t] == p) g += lds_g[t];
        }
      }
    gx[static_cast<int64_t>(blockIdx.y) * H * W + p] = g;
  }
}

}  // namespace

XAI_EXPORT int xai_maxpool_bwd_f32(const float* gy, const int64_t* indices, int planes, int H, int W, int PH, int PW, int kernel,
                                   int stride, int pad, float* gx, xai_stream_t stream) {
  XAI_REQUIRE_PTR(gy); XAI_REQUIRE_PTR(indices); XAI_REQUIRE_PTR(gx);
  XAI_REQUIRE(planes > 0 && H > 0 && W > 0 && PH > 0 && PW > 0 && kernel > 0 && stride > 0 && pad >= 0, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(H) * W <= INT32_MAX, XAI_E_UNSUPPORTED);
  const int nw = (kernel + stride - 1) / stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int pooled_rows = (kBwdRows + kernel - 2) / stride + 2;                   // upper bound of the pooled rows one tile needs
  const size_t lds = static_cast<size_t>(pooled_rows) * PW * 8;
  // planes ride on grid.y (<= 65535): larger batches (1024 images x 64 stem channels and up) go in slabs of planes
  constexpr int kMaxPlanes = 65535;
  for (int p0 = 0; p0 < planes; p0 += kMaxPlanes) {
    const int np = planes - p0 < kMaxPlanes ? planes - p0 : kMaxPlanes;
    const float* gy_s = gy + static_cast<int64_t>(p0) * PH * PW;
    const int64_t* idx_s = indices + static_cast<int64_t>(p0) * PH * PW;
    float* gx_s = gx + static_cast<int64_t>(p0) * H * W;
    if (nw <= 2 && lds <= 48 * 1024) {
      dim3 tgrid(static_cast<unsigned>(xai_ceil_div(H, kBwdRows)), np);
      if (nw == 1)
        hipLaunchKernelGGL(maxpool_bwd_tiled_kernel<1>, tgrid, dim3(256), lds, st, gy_s, idx_s, H, W, PH, PW, kernel, stride, pad, gx_s);
      else
        hipLaunchKernelGGL(maxpool_bwd_tiled_kernel<2>, tgrid, dim3(256), lds, st, gy_s, idx_s, H, W, PH, PW, kernel, stride, pad, gx_s);
    } else {
      dim3 grid(static_cast<unsigned>(xai_ceil_div(static_cast<int64_t>(H) * W, 256)), np);
      if (nw == 1)
        hipLaunchKernelGGL(maxpool_bwd_kernel<1>, grid, dim3(256), 0, st, gy_s, idx_s, H, W, PH, PW, kernel, stride, pad, gx_s);
      else if (nw == 2)
        hipLaunchKernelGGL(maxpool_bwd_kernel<2>, grid, dim3(256), 0, st, gy_s, idx_s, H, W, PH, PW, kernel, stride, pad, gx_s);
      else
        hipLaunchKernelGGL(maxpool_bwd_kernel<0>, grid, dim3(256), 0, st, gy_s, idx_s, H, W, PH, PW, kernel, stride, pad, gx_s);
    }
    const int rc = xai_launch_status();
    if (rc != XAI_OK) return rc;
  }
  return XAI_OK;
}

// ---- inference-only stem: max_pool( relu( bn(x) ) ) in one pass --------------------------------------------------------
// One lane per pooled output: the (up to k x k) inputs of its window go through the BN expression and ReLU in registers and
// only the maximum is written -- the 4x larger un-pooled activation is never stored.  Forward-only loops (RISE, the
// insertion / deletion sequences) run the classifier without autograd, so nothing downstream needs that activation.
// Values are those of PyTorch's three kernels (a maximum has no rounding); NaN wins like in max_pool_forward_nchw.
namespace {

__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, const float* __restrict__ mean,
                                                              const float* __restrict__ var, float eps, int variant, int C, int H, int W,
                                                              int PH, int PW, int k, int stride, int pad, float* __restrict__ y) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= PH * PW) return;
  const int plane = blockIdx.y;
  const int c = plane % C;
  const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
  const int ph = q / PW, pw = q - ph * PW;
  const int h0 = max(ph * stride - pad, 0), h1 = min(ph * stride - pad + k, H);
  const int w0 = max(pw * stride - pad, 0), w1 = min(pw * stride - pad + k, W);
  const float* src = x + static_cast<int64_t>(plane) * H * W;
  float best = -INFINITY;
  for (int h = h0; h < h1; ++h)
    for (int ww = w0; ww < w1; ++ww) {
      const float v = fmaxf(bn_value(src[h * W + ww], m, is, wc, bc, variant), 0.f);
      if (v > best || v != v) best = v;
    }
  y[static_cast<int64_t>(plane) * PH * PW + q] = best;
}

// Tiled form: a workgroup owns kPoolRows pooled rows of one plane; the input rows they cover are read once, coalesced, put
// through BN + ReLU and parked in LDS (out-of-range positions as -inf), then every lane takes the maximum of its window
// from LDS.  The direct form above reads each input up to (k/stride)^2 times with a stride-2 lane pattern and ran at
// 1.6 TB/s on the benchmark's stem (803 MB for 250 images).
constexpr int kPoolRows = 8;

__global__ __launch_bounds__(256) void bn_relu_maxpool_tiled_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ b, const float* __restrict__ mean,
                                                                    const float* __restrict__ var, float eps, int variant, int C, int H,
                                                                    int W, int PH, int PW, int k, int stride, int pad,
                                                                    float* __restrict__ y) {
  extern __shared__ float tile[];                       // [rows][W + 2 * pad]
  const int plane = blockIdx.y;
  const int c = plane % C;
  const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
  const int ph0 = blockIdx.x * kPoolRows;
  const int n_out = min(kPoolRows, PH - ph0);
  const int rows = (n_out - 1) * stride + k;
  const int h_first = ph0 * stride - pad;               // input row of tile row 0 (may be negative)
  const int TWp = W + 2 * pad;
  const float* src = x + static_cast<int64_t>(plane) * H * W;
  // 8 loads in flight per lane before the first LDS store (a store between two loads serialises them on the HBM latency)
  for (int base = threadIdx.x; base < rows * TWp; base += 256 * 8) {
    float v[8];
    bool in[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      const int r = i / TWp, cx = i - r * TWp;
      const int h = h_first + r, ww = cx - pad;
      in[u] = i < rows * TWp && h >= 0 && h < H && ww >= 0 && ww < W;
      v[u] = in[u] ? src[h * W + ww] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      if (i < rows * TWp) tile[i] = in[u] ? fmaxf(bn_value(v[u], m, is, wc, bc, variant), 0.f) : -INFINITY;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n_out * PW; q += 256) {
    const int pr = q / PW, pw = q - pr * PW;
    const float* t = tile + (pr * stride) * TWp + pw * stride;
    float best = -INFINITY;
    for (int a = 0; a < k; ++a)
      for (int bb = 0; bb < k; ++bb) {
        const float v = t[a * TWp + bb];
        if (v > best || v != v) best = v;
      }
    y[(static_cast<int64_t>(plane) * PH + ph0 + pr) * PW + pw] = best;
  }
}

// kernel 3, stride 2, pad 1 (every shipped classifier's stem) has its geometry at compile time: bn_relu_maxpool_fwd_kernel_fixed
// below, shared with the autograd stem; code == nullptr: this forward-only form (fmaxf, no code written)
void launch_stem_fwd_321(const float* x, const float* weight, const float* bias, const float* mean, const float* var, float eps, int variant,
                         int N, int C, int H, int W, int PH, int PW, size_t lds, float* y, uint8_t* code, hipStream_t st);

}  // namespace

XAI_EXPORT int xai_bn_relu_maxpool_fwd_f32(const float* x, const float* weight, const float* bias, const float* mean, const float* var,
                                           float eps, int variant, int N, int C, int H, int W, int PH, int PW, int kernel, int stride,
                                           int pad, float* y, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(bias); XAI_REQUIRE_PTR(mean); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(y);
  XAI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0 && kernel > 0 && stride > 0 && pad >= 0 && variant >= 0 && variant < 16,
              XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(N) * C <= 65535 && static_cast<int64_t>(H) * W <= INT32_MAX, XAI_E_UNSUPPORTED);
  const size_t lds = static_cast<size_t>((kPoolRows - 1) * stride + kernel) * (W + 2 * pad) * sizeof(float);
  if (lds <= 48 * 1024 && kernel == 3 && stride == 2 && pad == 1 && PH == (H - 1) / 2 + 1 && PW == (W - 1) / 2 + 1) {
    launch_stem_fwd_321(x, weight, bias, mean, var, eps, variant, N, C, H, W, PH, PW, lds, y, nullptr, static_cast<hipStream_t>(stream));
  } else if (lds <= 48 * 1024) {
    dim3 grid(static_cast<unsigned>(xai_ceil_div(PH, kPoolRows)), N * C);
    hipLaunchKernelGGL(bn_relu_maxpool_tiled_kernel, grid, dim3(256), lds, static_cast<hipStream_t>(stream), x, weight, bias, mean, var, eps,
                       variant, C, H, W, PH, PW, kernel, stride, pad, y);
  } else {
    dim3 grid(static_cast<unsigned>(xai_ceil_div(static_cast<int64_t>(PH) * PW, 256)), N * C);
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, weight, bias, mean, var, eps, variant,
                       C, H, W, PH, PW, kernel, stride, pad, y);
  }
  return xai_launch_status();
}

// ---- the stem with autograd: max_pool( relu( bn(x) ) ) forward and its whole backward, one kernel each -----------------
// Forward: the tiled kernel above, which also writes one uint8 code per pooled output -- the position a * k + b of the
// arg-max inside its k x k window (a, b counted from the window's padded origin) under PyTorch's rule (scan h then w
// ascending, update on val > max || isnan(val)), or kStemClosed when the pooled value is <= 0, i.e. when PyTorch's
// threshold_backward passes no gradient at the selected position.  A NaN goes through the ReLU as in PyTorch's clamp_min,
// wins every window it is in and keeps its gate open.  The un-pooled activation is never stored.
// Backward: per input position the gradients gy[q] (+ gy2[q]) of the windows q that selected it are added in (ph, pw)
// ascending order from +0 -- the order of maxpool_bwd_tiled_kernel and of PyTorch's max_pool_backward_nchw -- and the sum
// goes through (g * w) * invstd.  Gating per window is PyTorch's gate per position: every window that selects position p
// has the pooled value y[p], so either all of p's contributions pass or none does, and a position that nothing selected
// gets +0 both ways.
namespace {

constexpr int kStemClosed = 255;

__device__ __forceinline__ float relu_keep_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

__global__ __launch_bounds__(256) void bn_relu_maxpool_code_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ b, const float* __restrict__ mean,
                                                                   const float* __restrict__ var, float eps, int variant, int C, int H,
                                                                   int W, int PH, int PW, int k, int stride, int pad,
                                                                   float* __restrict__ y, uint8_t* __restrict__ code) {
  extern __shared__ float tile[];                       // [rows][W + 2 * pad]
  const int plane = blockIdx.y;
  const int c = plane % C;
  const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
  const int ph0 = blockIdx.x * kPoolRows;
  const int n_out = min(kPoolRows, PH - ph0);
  const int rows = (n_out - 1) * stride + k;
  const int h_first = ph0 * stride - pad;               // input row of tile row 0 (may be negative)
  const int TWp = W + 2 * pad;
  const float* src = x + static_cast<int64_t>(plane) * H * W;
  for (int base = threadIdx.x; base < rows * TWp; base += 256 * 8) {
    float v[8];
    bool in[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      const int r = i / TWp, cx = i - r * TWp;
      const int h = h_first + r, ww = cx - pad;
      in[u] = i < rows * TWp && h >= 0 && h < H && ww >= 0 && ww < W;
      v[u] = in[u] ? src[h * W + ww] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      if (i < rows * TWp) tile[i] = in[u] ? relu_keep_nan(bn_value(v[u], m, is, wc, bc, variant)) : -INFINITY;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n_out * PW; q += 256) {
    const int pr = q / PW, pw = q - pr * PW;
    const float* t = tile + (pr * stride) * TWp + pw * stride;
    float best = -INFINITY;
    int arg = 0;
    for (int a = 0; a < k; ++a)
      for (int bb = 0; bb < k; ++bb) {
        const float v = t[a * TWp + bb];
        if (v > best || v != v) { best = v; arg = a * k + bb; }
      }
    const int64_t o = (static_cast<int64_t>(plane) * PH + ph0 + pr) * PW + pw;
    y[o] = best;
    code[o] = static_cast<uint8_t>(best <= 0.f ? kStemClosed : arg);
  }
}

// The same kernel with the pool geometry at compile time and a 2-D lane mapping: no integer division is left (the form above
// spends most of its instructions on i / TWp per staged input and q / PW per output).  Staging: lane (ty, tx) of a TX-wide,
// 256 / TX-high arrangement takes tile rows ty, ty + TY, .. of columns tx, tx + TX, ..; all of a lane's loads of one column are
// in flight before its first LDS store.  Output: lanes TX / 2 wide over the pooled row (TX >= W + 2 P makes that one trip at
// stride 2).  Grid (row tiles, C, N): the channel is blockIdx.y.  Same tile values, same scan, same y and code.
// CODE = false is the forward-only bn_relu_maxpool_tiled_kernel in the same way: fmaxf in place of relu_keep_nan, no code.
template <int K, int S, int P, int TX, bool CODE>
__global__ __launch_bounds__(256) void bn_relu_maxpool_fwd_kernel_fixed(const float* __restrict__ x, const float* __restrict__ w,
                                                                         const float* __restrict__ b, const float* __restrict__ mean,
                                                                         const float* __restrict__ var, float eps, int variant, int H,
                                                                         int W, int PH, int PW, float* __restrict__ y,
                                                                         uint8_t* __restrict__ code) {
  extern __shared__ float tile[];                       // [rows][W + 2 * P]
  constexpr int TY = 256 / TX, TXO = TX / 2, TYO = 256 / TXO;
  constexpr int kRows = (kPoolRows - 1) * S + K, U = (kRows + TY - 1) / TY;
  const int c = blockIdx.y;
  const int64_t plane = static_cast<int64_t>(blockIdx.z) * gridDim.y + c;
  const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
  const int ph0 = blockIdx.x * kPoolRows;
  const int n_out = min(kPoolRows, PH - ph0);
  const int rows = (n_out - 1) * S + K;
  const int h_first = ph0 * S - P;                      // input row of tile row 0 (may be negative)
  const int TWp = W + 2 * P;
  const float* src = x + plane * H * W;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
  for (int cx = tx; cx < TWp; cx += TX) {
    const int ww = cx - P;
    const bool col_in = ww >= 0 && ww < W;
    float v[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = ty + u * TY, h = h_first + r;
      in[u] = col_in && r < rows && h >= 0 && h < H;
      v[u] = in[u] ? src[h * W + ww] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = ty + u * TY;
      if (r < rows) {
        const float t = bn_value(v[u], m, is, wc, bc, variant);
        tile[r * TWp + cx] = in[u] ? (CODE ? relu_keep_nan(t) : fmaxf(t, 0.f)) : -INFINITY;
      }
    }
  }
  __syncthreads();
  const int txo = threadIdx.x & (TXO - 1), tyo = threadIdx.x / TXO;
  for (int pr = tyo; pr < n_out; pr += TYO)
    for (int pw = txo; pw < PW; pw += TXO) {
      const float* t = tile + (pr * S) * TWp + pw * S;
      float best = -INFINITY;
      int arg = 0;
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int bb = 0; bb < K; ++bb) {
          const float v = t[a * TWp + bb];
          if (v > best || v != v) { best = v; arg = a * K + bb; }
        }
      const int64_t o = (plane * PH + ph0 + pr) * PW + pw;
      y[o] = best;
      if (CODE) code[o] = static_cast<uint8_t>(best <= 0.f ? kStemClosed : arg);
    }
}

// GUIDED: guided_clamp on the position's SUM over the windows that selected it (the complete gradient of the ReLU's output, as the
// pool's backward scatters it), not per window: overlapping windows can bring gradients of both signs to one position.
template <int NW, bool GUIDED>
__global__ __launch_bounds__(256) void bn_relu_maxpool_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ gy2,
                                                                  const uint8_t* __restrict__ code, const float* __restrict__ w,
                                                                  const float* __restrict__ var, float eps, int variant, int C, int H,
                                                                  int W, int PH, int PW, int k, int stride, int pad,
                                                                  float* __restrict__ gx) {
  extern __shared__ int lds_i[];                         // [rows][PW] codes, then [rows][PW] gradients
  const int c = blockIdx.y % C;
  const float is = inv_std(var[c], eps, variant), wc = w[c];
  const int h0 = blockIdx.x * kBwdRows;
  const int h_last = min(h0 + kBwdRows, H) - 1;
  const int pr0 = (h0 + pad < k) ? 0 : (h0 + pad - k) / stride + 1;           // first pooled row that can cover row h0
  const int pr1 = min((h_last + pad) / stride + 1, PH);                         // one past the last that can cover h_last
  const int rows = max(pr1 - pr0, 0);
  float* lds_g = reinterpret_cast<float*>(lds_i + rows * PW);
  const int64_t off = static_cast<int64_t>(blockIdx.y) * PH * PW + static_cast<int64_t>(pr0) * PW;
  const int total = rows * PW;
  for (int base = threadIdx.x; base < total; base += 256 * 8) {
    int iv[8];
    float gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      iv[u] = i < total ? static_cast<int>(code[off + i]) : kStemClosed;
      gv[u] = i < total ? gy[off + i] : 0.f;
      if (gy2 != nullptr && i < total) gv[u] += gy2[off + i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * 256;
      if (i < total) { lds_i[i] = iv[u]; lds_g[i] = gv[u]; }
    }
  }
  __syncthreads();
  const int n_rows = h_last - h0 + 1;
  for (int q = threadIdx.x; q < n_rows * W; q += 256) {
    const int r = q / W, ww = q - r * W;
    const int h = h0 + r;
    const int ph0 = (h + pad < k) ? 0 : (h + pad - k) / stride + 1;
    const int ph1 = min((h + pad) / stride + 1, PH);
    const int pw0 = (ww + pad < k) ? 0 : (ww + pad - k) / stride + 1;
    const int pw1 = min((ww + pad) / stride + 1, PW);
    float g = 0.f;
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
      for (int bb = 0; bb < NW; ++bb) {
        const int ph = ph0 + a, pw = pw0 + bb;
        if (ph < ph1 && pw < pw1) {
          const int t = (ph - pr0) * PW + pw;
          const int mine = (h + pad - ph * stride) * k + (ww + pad - pw * stride);   // this position inside window (ph, pw)
          if (lds_i[t] == mine) g += lds_g[t];
        }
      }
    if (GUIDED) g = guided_clamp(g);
    gx[static_cast<int64_t>(blockIdx.y) * H * W + h * W + ww] = bn_grad(g, is, wc, variant);
  }
}

// The same backward for kernel 3, stride 2, pad 1 at compile time, without LDS and without an integer division.  A lane owns
// input rows 2m, 2m + 1 and columns 4j .. 4j + 3: every window that can select one of those eight positions lies in pooled
// rows m, m + 1 and pooled columns 2j .. 2j + 2, so the lane loads those six codes and gradients (gy + gy2 formed at once),
// all loads in flight together, and then adds per position, from +0, the windows that selected it in (ph, pw) ascending order:
// the loops below are the ones of the form above with their bounds known, so the sums are the same sums.  Lanes are TX wide
// over the columns and 256 / TX row pairs high; `vec`: W % 4 == 0 and gx 16-byte aligned, one float4 store per row.
// Grid (row-pair tiles, C, N).
template <int K, int S, int P, int TX, bool GUIDED>
__global__ __launch_bounds__(256) void bn_relu_maxpool_bwd_kernel_fixed(const float* __restrict__ gy, const float* __restrict__ gy2,
                                                                        const uint8_t* __restrict__ code, const float* __restrict__ w,
                                                                        const float* __restrict__ var, float eps, int variant, int H,
                                                                        int W, int PH, int PW, int vec, float* __restrict__ gx) {
  static_assert(K == 3 && S == 2 && P == 1, "row pairs and column quads below cover exactly the windows of 3/2/1");
  constexpr int TY = 256 / TX;
  const int c = blockIdx.y;
  const int64_t plane = static_cast<int64_t>(blockIdx.z) * gridDim.y + c;
  const float is = inv_std(var[c], eps, variant), wc = w[c];
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
  const int m = blockIdx.x * TY + ty;
  if (2 * m >= H) return;
  const uint8_t* cp = code + plane * PH * PW;
  const float* gp = gy + plane * PH * PW;
  const float* gp2 = gy2 != nullptr ? gy2 + plane * PH * PW : nullptr;
  float* dst = gx + plane * H * W;
  for (int j = tx; 4 * j < W; j += TX) {
    int cd[2][3];
    float gv[2][3];
#pragma unroll
    for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
      for (int b2 = 0; b2 < 3; ++b2) {
        const int ph = m + a2, pw = 2 * j + b2;
        const bool ok = ph < PH && pw < PW;               // outside: no such window; its slot never matches
        const int q = ok ? ph * PW + pw : 0;
        const int raw = cp[q];
        cd[a2][b2] = ok ? raw : kStemClosed;
        gv[a2][b2] = gp[q];
        if (gp2 != nullptr) gv[a2][b2] += gp2[q];
      }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int h = 2 * m + rr;
      if (h < H) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float g = 0.f;
#pragma unroll
          for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
            for (int b2 = 0; b2 < 3; ++b2) {
              const int a = rr + P - S * a2, bb = e + P - S * b2;   // this position inside window (m + a2, 2j + b2)
              if (a >= 0 && a < K && bb >= 0 && bb < K)
                if (cd[a2][b2] == a * K + bb) g += gv[a2][b2];
            }
          if (GUIDED) g = guided_clamp(g);
          o[e] = bn_grad(g, is, wc, variant);
        }
        float* row = dst + h * W + 4 * j;
        if (vec) {
          st4(row, make_float4(o[0], o[1], o[2], o[3]));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * j + e < W) row[e] = o[e];
        }
      }
    }
  }
}

// lanes across the staged row: the smallest of 64, 128, 256 that covers W + 2 columns in one trip (256 loops beyond that)
void launch_stem_fwd_321(const float* x, const float* weight, const float* bias, const float* mean, const float* var, float eps, int variant,
                         int N, int C, int H, int W, int PH, int PW, size_t lds, float* y, uint8_t* code, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(xai_ceil_div(PH, kPoolRows)), C, N);
  xai_dispatch(code != nullptr, [&](auto coded) {
#define XAI_STEM_FWD(TX) \
  hipLaunchKernelGGL((bn_relu_maxpool_fwd_kernel_fixed<3, 2, 1, TX, decltype(coded)::value>), grid, dim3(256), lds, st, x, weight, bias, mean, var, eps, variant, H, W, PH, PW, y, code)
    if (W + 2 <= 64) XAI_STEM_FWD(64);
    else if (W + 2 <= 128) XAI_STEM_FWD(128);
    else XAI_STEM_FWD(256);
#undef XAI_STEM_FWD
  });
}

// what both stem entry points accept: a plain square pool whose windows all hold an input element, codes that fit a byte
// next to kStemClosed, consistent pooled extents (the kernels index by them), planes on grid.y
static int stem_geometry_status(int N, int C, int H, int W, int PH, int PW, int kernel, int stride, int pad, int variant) {
  XAI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0 && kernel > 0 && stride > 0 && pad >= 0 && variant >= 0 && variant < 16,
              XAI_E_SHAPE);
  XAI_REQUIRE(2 * pad <= kernel && H + 2 * pad >= kernel && W + 2 * pad >= kernel, XAI_E_SHAPE);
  XAI_REQUIRE(PH == (H + 2 * pad - kernel) / stride + 1 && PW == (W + 2 * pad - kernel) / stride + 1, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(N) * C <= 65535 && static_cast<int64_t>(H) * W <= INT32_MAX && kernel * kernel <= kStemClosed &&
                  (kernel + stride - 1) / stride <= 2,
              XAI_E_UNSUPPORTED);
  return XAI_OK;
}

}  // namespace

XAI_EXPORT int xai_bn_relu_maxpool_fwd_code_f32(const float* x, const float* weight, const float* bias, const float* mean,
                                                const float* var, float eps, int variant, int N, int C, int H, int W, int PH, int PW,
                                                int kernel, int stride, int pad, float* y, uint8_t* code, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(bias); XAI_REQUIRE_PTR(mean); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(y);
  XAI_REQUIRE_PTR(code);
  const int rc = stem_geometry_status(N, C, H, W, PH, PW, kernel, stride, pad, variant);
  if (rc != XAI_OK) return rc;
  const size_t lds = static_cast<size_t>((kPoolRows - 1) * stride + kernel) * (W + 2 * pad) * sizeof(float);
  XAI_REQUIRE(lds <= 48 * 1024, XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (kernel == 3 && stride == 2 && pad == 1) {         // every shipped classifier's stem: geometry at compile time
    launch_stem_fwd_321(x, weight, bias, mean, var, eps, variant, N, C, H, W, PH, PW, lds, y, code, st);
    return xai_launch_status();
  }
  dim3 grid(static_cast<unsigned>(xai_ceil_div(PH, kPoolRows)), N * C);
  hipLaunchKernelGGL(bn_relu_maxpool_code_kernel, grid, dim3(256), lds, st, x, weight, bias, mean, var, eps, variant, C, H, W, PH, PW, kernel,
                     stride, pad, y, code);
  return xai_launch_status();
}

template <bool GUIDED>
static int bn_relu_maxpool_bwd_launch(const float* gy, const float* gy2, const uint8_t* code, const float* weight, const float* var, float eps,
                                      int variant, int N, int C, int H, int W, int PH, int PW, int kernel, int stride, int pad, float* gx,
                                      xai_stream_t stream) {
  XAI_REQUIRE_PTR(gy); XAI_REQUIRE_PTR(code); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(gx);
  const int rc = stem_geometry_status(N, C, H, W, PH, PW, kernel, stride, pad, variant);
  if (rc != XAI_OK) return rc;
  const int pooled_rows = (kBwdRows + kernel - 2) / stride + 2;                   // upper bound of the pooled rows one tile needs
  const size_t lds = static_cast<size_t>(pooled_rows) * PW * 8;
  XAI_REQUIRE(lds <= 48 * 1024, XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (kernel == 3 && stride == 2 && pad == 1) {         // every shipped classifier's stem: geometry at compile time, no LDS
    const int vec = xai_can_vec4(W, {gx});
    const int pairs = (H + 1) / 2;
#define XAI_STEM_BWD(TX) \
  hipLaunchKernelGGL((bn_relu_maxpool_bwd_kernel_fixed<3, 2, 1, TX, GUIDED>), dim3(static_cast<unsigned>(xai_ceil_div(pairs, 256 / TX)), C, N), \
                     dim3(256), 0, st, gy, gy2, code, weight, var, eps, variant, H, W, PH, PW, vec, gx)
    if (W <= 64) XAI_STEM_BWD(16);
    else if (W <= 128) XAI_STEM_BWD(32);
    else XAI_STEM_BWD(64);
#undef XAI_STEM_BWD
    return xai_launch_status();
  }
  dim3 grid(static_cast<unsigned>(xai_ceil_div(H, kBwdRows)), N * C);
  if ((kernel + stride - 1) / stride == 1)
    hipLaunchKernelGGL((bn_relu_maxpool_bwd_kernel<1, GUIDED>), grid, dim3(256), lds, st, gy, gy2, code, weight, var, eps, variant, C, H, W, PH, PW,
                       kernel, stride, pad, gx);
  else
    hipLaunchKernelGGL((bn_relu_maxpool_bwd_kernel<2, GUIDED>), grid, dim3(256), lds, st, gy, gy2, code, weight, var, eps, variant, C, H, W, PH, PW,
                       kernel, stride, pad, gx);
  return xai_launch_status();
}

XAI_EXPORT int xai_bn_relu_maxpool_bwd_f32(const float* gy, const float* gy2, const uint8_t* code, const float* weight, const float* var,
                                           float eps, int variant, int N, int C, int H, int W, int PH, int PW, int kernel, int stride,
                                           int pad, float* gx, xai_stream_t stream) {
  return bn_relu_maxpool_bwd_launch<false>(gy, gy2, code, weight, var, eps, variant, N, C, H, W, PH, PW, kernel, stride, pad, gx, stream);
}

XAI_EXPORT int xai_bn_relu_maxpool_bwd_guided_f32(const float* gy, const float* gy2, const uint8_t* code, const float* weight,
                                                  const float* var, float eps, int variant, int N, int C, int H, int W, int PH, int PW,
                                                  int kernel, int stride, int pad, float* gx, xai_stream_t stream) {
  return bn_relu_maxpool_bwd_launch<true>(gy, gy2, code, weight, var, eps, variant, N, C, H, W, PH, PW, kernel, stride, pad, gx, stream);
}
