// K62-K64: the fused BN/ReLU kernels of bnrelu_kernels.hip around a strided 1x1 shortcut convolution that runs on COMPACT,
// channel-major tensors (CNHW), and behind a pool + Linear head.  Part of libxai_compact.so (include/xai_hip_compact.h).
//
// A stride-s 1x1 convolution reads one input position in s*s and, run by MIOpen on NCHW tensors, is wrapped in layout kernels: a
// strided NCHW->CNHW gather and a CNHW->NCHW transpose forward; a zero-fill of the full-resolution input gradient, a transpose and a
// strided scatter backward.  Only the fused kernels touch the tensors on either side, so they take over the layouts:
//   K62 gather    Xc[c][n][ho][wo] = side[n][c][ho*s][wo*s]: the one strided pass that remains.  The convolution then runs at
//                 stride 1 on the (1, C, N*Ho, Wo) view of Xc, where NCHW and CNHW coincide and MIOpen moves nothing.
//   K63 forward   relu(bn(x) + bn2(identity)) with the identity operand read in CNHW order, what that convolution wrote; y and the
//                 gate mask as xai_bn_relu_fwd_mask_f32 writes them.
//   K64 backward  xai_bn_relu_bwd_mask_f32 (guided or not) with any of
//                   g_identity written in CNHW order, what that convolution's backward reads;
//                   gy2 given compact, [C][N][Ho][Wo]: the shortcut's input gradient, added at (h, w) = (ho*s, wo*s) and +0 added
//                     everywhere else -- the dense tensor MIOpen zero-fills and scatters into, never stored;
//                   gy given as a broadcast operand: (grad_out[n] * fc_weight[target[n]][c]) * (1 / HW), what gather + Linear +
//                     mean hand back for score[n] = logits[n][target[n]], never stored either.
// Per element the expressions, their order and the mask layout are those of bnrelu_kernels.hip (xai_bn_device.h holds them once).
// A lane owns flat NCHW elements 4t .. 4t+3 as there.  VEC (HW % 4 == 0): they share image and channel, and every tensor, CNHW ones
// included, moves 16 bytes at a time.  Otherwise (image, channel, position) are stepped per element; NCHW tensors still move 16
// bytes at a time where n % 4 == 0 and they are aligned (`wide`), CNHW and compact operands 4 bytes at a time.
#include "xai_bn_device.h"
#include "xai_hip_compact.h"

// the version pair of libxai_compact.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_compact_version, XAI_COMPACT_VERSION, XAI_COMPACT_MINOR)

namespace {

// where a flat NCHW element sits
struct Pos {
  XaiBnLane s;          // r = position inside the plane, c = channel
  int image;
};

__device__ __forceinline__ Pos pos_first(int64_t i, int64_t n, int HW, int C) {
  return Pos{xai_bn_lane_first(i, n, HW, C), xai_bn_image_first(i, n, HW, C)};
}

__device__ __forceinline__ Pos pos_step(Pos p, int HW, int C) {
  p.s = xai_bn_lane_step(p.s, HW, C);
  p.image = xai_bn_image_step(p.image, p.s);
  return p;
}

__device__ __forceinline__ int64_t cnhw_index(Pos p, int N, int HW) { return xai_bn_cnhw_index(p.image, p.s.c, p.s.r, N, HW); }

// ---- K62 ----------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kBlock) void stride_gather_cnhw_kernel(const float* __restrict__ side, int N, int C, int H, int W, int s,
                                                                    int Ho, int Wo, int64_t total, float* __restrict__ out) {
  const int64_t o = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (o >= total) return;
  // o = ((c * N + n) * Ho + ho) * Wo + wo
  int64_t q = o / Wo;
  int wo = static_cast<int>(o - q * Wo);
  int ho = static_cast<int>(q % Ho);
  q /= Ho;
  int n = static_cast<int>(q % N), c = static_cast<int>(q / N);
  float v[VEC ? 4 : 1];
#pragma unroll
  for (int k = 0; k < (VEC ? 4 : 1); ++k) {
    v[k] = side[xai_bn_strided_index(n, c, ho, wo, C, H, W, s)];
    if (++wo == Wo) {
      wo = 0;
      if (++ho == Ho) {
        ho = 0;
        if (++n == N) { n = 0; ++c; }
      }
    }
  }
  if (VEC) st4(out + o, make_float4(v[0], v[VEC ? 1 : 0], v[VEC ? 2 : 0], v[VEC ? 3 : 0]));
  else out[o] = v[0];
}

// ---- K63 ----------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kBlock) void bn_relu_fwd_cnhw_kernel(const float* __restrict__ x, const float* __restrict__ idt,
                                                                  const float* __restrict__ w, const float* __restrict__ b,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  float eps, BnParams bn2, int variant, int N, int C, int HW,
                                                                  int64_t n, int wide, float* __restrict__ y,
                                                                  uint64_t* __restrict__ mask) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t group = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (group * kGateGroup >= n) return;                  // wave-uniform: this wavefront owns no element and no mask word
  const int64_t i = group * kGateGroup + lane * 4;
  const bool second = bn2.w != nullptr;
  float o[4] = {0.f, 0.f, 0.f, 0.f};                    // elements >= n keep +0: gate bit 0
  if (i < n) {
    Pos p = pos_first(i, n, HW, C);
    if (VEC) {                                          // HW % 4 == 0: one image, one channel, one aligned float4 per tensor
      const int c = p.s.c;
      const float m = mean[c], is = inv_std(var[c], eps, variant), wc = w[c], bc = b[c];
      const float4 v = ld4_nt(x + i);
      o[0] = bn_value(v.x, m, is, wc, bc, variant); o[1] = bn_value(v.y, m, is, wc, bc, variant);
      o[2] = bn_value(v.z, m, is, wc, bc, variant); o[3] = bn_value(v.w, m, is, wc, bc, variant);
      float4 a = ld4_nt(idt + cnhw_index(p, N, HW));
      if (second) {
        const float m2 = bn2.mean[c], is2 = inv_std(bn2.var[c], bn2.eps, variant), w2 = bn2.w[c], b2 = bn2.b[c];
        a = make_float4(bn_value(a.x, m2, is2, w2, b2, variant), bn_value(a.y, m2, is2, w2, b2, variant),
                        bn_value(a.z, m2, is2, w2, b2, variant), bn_value(a.w, m2, is2, w2, b2, variant));
      }
      o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
      st4(y + i, make_float4(o[0], o[1], o[2], o[3]));
    } else {
      float xv[4] = {0.f, 0.f, 0.f, 0.f};
      if (wide) {
        const float4 v = ld4_nt(x + i);
        xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i + k < n) {
          const int c = p.s.c;
          float v = bn_value(wide ? xv[k] : x[i + k], mean[c], inv_std(var[c], eps, variant), w[c], b[c], variant);
          const float a = idt[cnhw_index(p, N, HW)];
          v += second ? bn_value(a, bn2.mean[c], inv_std(bn2.var[c], bn2.eps, variant), bn2.w[c], bn2.b[c], variant) : a;
          v = fmaxf(v, 0.f);
          if (!wide) y[i + k] = v;
          o[k] = v;
        }
        p = pos_step(p, HW, C);
      }
      if (wide) st4(y + i, make_float4(o[0], o[1], o[2], o[3]));
    }
  }
  if (mask != nullptr) store_gate_words(mask, group, lane, o[0] > 0.f, o[1] > 0.f, o[2] > 0.f, o[3] > 0.f);
}

// ---- K64 ----------------------------------------------------------------------------------------------------------------
struct BwdExt {
  // gy as a broadcast operand (out != nullptr; gy is then null)
  const float* out;            // grad_out [N]
  const float* fc;             // fc_weight [classes][C]
  const int64_t* target;       // [N]
  int classes;
  float scale, divisor;
  // gy2 compact (gy2c != nullptr; the dense gy2 is then null): [C][N][Ho][Wo], stride s, W the width of a plane
  const float* gy2c;
  int W, s, Ho, Wo;
  int gid_cnhw;                // g_identity in CNHW order
  int N;
};

// two roundings, never contracted with the add of gy2 that may follow; a target outside [0, classes) is clamped (the
// forward's gather has trapped on it already)
__device__ __forceinline__ float bcast_gy(const BwdExt& e, int image, int c, int C) {
  int64_t t = e.target[image];
  t = t < 0 ? 0 : t >= e.classes ? e.classes - 1 : t;
  const float v = __fmul_rn(e.out[image], e.fc[t * C + c]);
  return e.divisor != 0.f ? __fdiv_rn(v, e.divisor) : __fmul_rn(v, e.scale);
}

// the value the dense, zero-filled and scattered gradient would hold at (h, w): the compact one where both are multiples of s,
// +0 elsewhere (still added by the caller: -0 + +0 = +0, as the dense path gives)
__device__ __forceinline__ float compact_gy2(const BwdExt& e, int image, int c, int h, int w) {
  int ho, wo;
  bool covered;
  if (e.s == 2) {
    covered = ((h | w) & 1) == 0;
    ho = h >> 1; wo = w >> 1;
  } else {
    ho = h / e.s; wo = w / e.s;
    covered = ho * e.s == h && wo * e.s == w;
  }
  return covered ? e.gy2c[xai_bn_cnhw_index(image, c, ho * e.Wo + wo, e.N, e.Ho * e.Wo)] : 0.f;
}

template <bool VEC, bool GUIDED>
__global__ __launch_bounds__(kBlock) void bn_relu_bwd_ext_kernel(const float* __restrict__ gy, const float* __restrict__ gy2,
                                                                 const uint64_t* __restrict__ mask, const float* __restrict__ w,
                                                                 const float* __restrict__ var, float eps, BnParams bn2, int variant,
                                                                 int C, int HW, int64_t n, int wide, BwdExt e,
                                                                 float* __restrict__ gx, float* __restrict__ gid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t group = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (group * kGateGroup >= n) return;
  const int64_t i = group * kGateGroup + lane * 4;
  if (i >= n) return;
  const uint64_t* mw = mask + group * 4;                // wave-uniform address: four words shared by the whole wavefront
  const bool open[4] = {((mw[0] >> lane) & 1) != 0, ((mw[1] >> lane) & 1) != 0, ((mw[2] >> lane) & 1) != 0, ((mw[3] >> lane) & 1) != 0};
  const bool add = gid != nullptr;
  const bool second = add && bn2.w != nullptr;          // g_identity then goes through the identity operand's own BatchNorm
  Pos p = pos_first(i, n, HW, C);
  if (VEC) {
    const int c = p.s.c;
    const float is = inv_std(var[c], eps, variant), wc = w[c];
    float is2 = 1.f, w2 = 1.f;
    if (second) { is2 = inv_std(bn2.var[c], bn2.eps, variant); w2 = bn2.w[c]; }
    float g[4];
    if (e.out != nullptr) {
      g[0] = g[1] = g[2] = g[3] = bcast_gy(e, p.image, c, C);
    } else {
      const float4 t = ld4_nt(gy + i);
      g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
    }
    if (gy2 != nullptr) {
      const float4 t = ld4_nt(gy2 + i);
      g[0] += t.x; g[1] += t.y; g[2] += t.z; g[3] += t.w;
    } else if (e.gy2c != nullptr) {
      int h = p.s.r / e.W, x0 = p.s.r - h * e.W;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[k] += compact_gy2(e, p.image, c, h, x0);
        if (++x0 == e.W) { x0 = 0; ++h; }
      }
    }
    float g1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (GUIDED) g[k] = guided_clamp(g[k]);
      g1[k] = open[k] ? g[k] : 0.f;
    }
    st4(gx + i, make_float4(bn_grad(g1[0], is, wc, variant), bn_grad(g1[1], is, wc, variant), bn_grad(g1[2], is, wc, variant),
                            bn_grad(g1[3], is, wc, variant)));
    if (add) {
      if (second) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g1[k] = bn_grad(g1[k], is2, w2, variant);
      }
      st4(gid + (e.gid_cnhw ? cnhw_index(p, e.N, HW) : i), make_float4(g1[0], g1[1], g1[2], g1[3]));
    }
  } else {
    float a[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f}, ox[4] = {0.f, 0.f, 0.f, 0.f}, oi[4] = {0.f, 0.f, 0.f, 0.f};
    if (wide) {                                         // n % 4 == 0: the lane is inside as a whole
      if (gy != nullptr) { const float4 t = ld4_nt(gy + i); a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w; }
      if (gy2 != nullptr) { const float4 t = ld4_nt(gy2 + i); a2[0] = t.x; a2[1] = t.y; a2[2] = t.z; a2[3] = t.w; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k < n) {
        const int c = p.s.c;
        float g = e.out != nullptr ? bcast_gy(e, p.image, c, C) : wide ? a[k] : gy[i + k];
        if (gy2 != nullptr) {
          g += wide ? a2[k] : gy2[i + k];
        } else if (e.gy2c != nullptr) {
          const int h = p.s.r / e.W;
          g += compact_gy2(e, p.image, c, h, p.s.r - h * e.W);
        }
        if (GUIDED) g = guided_clamp(g);
        const float g1 = open[k] ? g : 0.f;
        ox[k] = bn_grad(g1, inv_std(var[c], eps, variant), w[c], variant);
        if (!wide) gx[i + k] = ox[k];
        if (add) {
          oi[k] = second ? bn_grad(g1, inv_std(bn2.var[c], bn2.eps, variant), bn2.w[c], variant) : g1;
          if (e.gid_cnhw) gid[cnhw_index(p, e.N, HW)] = oi[k];
          else if (!wide) gid[i + k] = oi[k];
        }
      }
      p = pos_step(p, HW, C);
    }
    if (wide) {
      st4(gx + i, make_float4(ox[0], ox[1], ox[2], ox[3]));
      if (add && !e.gid_cnhw) st4(gid + i, make_float4(oi[0], oi[1], oi[2], oi[3]));
    }
  }
}

// the checks the entry points share
static int bn_extents_status(int N, int C, int HW, int variant) {
  XAI_REQUIRE(N > 0 && C > 0 && HW > 0 && variant >= 0 && variant < 16, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(N) * C <= INT32_MAX, XAI_E_UNSUPPORTED);
  return XAI_OK;
}

static int bwd_ext_launch(const float* gy, const float* gy2, const void* mask, const float* weight, const float* var, float eps,
                          const float* weight2, const float* var2, float eps2, int variant, int guided, int N, int C, int HW,
                          BwdExt e, float* gx, float* g_identity, xai_stream_t stream) {
  XAI_REQUIRE_PTR(mask); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(gx);
  if (const int rc = bn_extents_status(N, C, HW, variant)) return rc;
  XAI_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 7u) == 0, XAI_E_SHAPE);
  if (weight2 != nullptr) {
    XAI_REQUIRE_PTR(g_identity); XAI_REQUIRE_PTR(var2);
  }
  XAI_REQUIRE(!e.gid_cnhw || g_identity != nullptr, XAI_E_NULL);
  XAI_REQUIRE(gy2 == nullptr || e.gy2c == nullptr, XAI_E_SHAPE);
  e.N = N;
  const BnParams bn2{weight2, nullptr, nullptr, var2, eps2};
  const int64_t n = static_cast<int64_t>(N) * C * HW;
  // g_identity in CNHW order is a 16-byte access on the vector path only (where HW % 4 == 0 keeps it aligned)
  const bool vec_gid = g_identity != nullptr && (!e.gid_cnhw || (HW & 3) == 0);
  const XaiBnPath path = xai_bn_path(n, HW, bn_low_bits({gy, gx, gy2, vec_gid ? g_identity : nullptr}));
  const bool vec = path == XAI_BN_VEC4;
  const int wide = path == XAI_BN_FLAT4;
  const unsigned grid = static_cast<unsigned>(xai_ceil_div(n, static_cast<int64_t>(kBlock) * 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint64_t* mk = static_cast<const uint64_t*>(mask);
  xai_dispatch(vec, [&](auto V) {
    xai_dispatch(guided != 0, [&](auto G) {
      hipLaunchKernelGGL((bn_relu_bwd_ext_kernel<decltype(V)::value, decltype(G)::value>), dim3(grid), dim3(kBlock), 0, st, gy, gy2, mk, weight,
                         var, eps, bn2, variant, C, HW, n, wide, e, gx, g_identity);
    });
  });
  return xai_launch_status();
}

}  // namespace

XAI_EXPORT int xai_stride_gather_cnhw_f32(const float* side, int N, int C, int H, int W, int stride, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(side); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && stride > 0, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(N) * C <= INT32_MAX, XAI_E_UNSUPPORTED);
  const int Ho = xai_bn_strided_extent(H, stride), Wo = xai_bn_strided_extent(W, stride);
  const int64_t total = static_cast<int64_t>(N) * C * Ho * Wo;
  const bool vec = xai_can_vec4(total, {out});
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(xai_ceil_div(total, vec ? 4 : 1), kBlock, &blocks), XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V) {
    hipLaunchKernelGGL((stride_gather_cnhw_kernel<decltype(V)::value>), dim3(blocks), dim3(kBlock), 0, st, side, N, C, H, W, stride, Ho, Wo,
                       total, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_bn_relu_fwd_cnhw_f32(const float* x, const float* identity_cnhw, const float* weight, const float* bias,
                                        const float* mean, const float* var, float eps, const float* weight2, const float* bias2,
                                        const float* mean2, const float* var2, float eps2, int variant, int N, int C, int HW, float* y,
                                        void* mask, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(identity_cnhw); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(bias); XAI_REQUIRE_PTR(mean);
  XAI_REQUIRE_PTR(var); XAI_REQUIRE_PTR(y);
  if (const int rc = bn_extents_status(N, C, HW, variant)) return rc;
  XAI_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 7u) == 0, XAI_E_SHAPE);
  if (weight2 != nullptr) {
    XAI_REQUIRE_PTR(bias2); XAI_REQUIRE_PTR(mean2); XAI_REQUIRE_PTR(var2);
  }
  const BnParams bn2{weight2, bias2, mean2, var2, eps2};
  const int64_t n = static_cast<int64_t>(N) * C * HW;
  const XaiBnPath path = xai_bn_path(n, HW, bn_low_bits({x, y, (HW & 3) == 0 ? identity_cnhw : nullptr}));
  const bool vec = path == XAI_BN_VEC4;
  const int wide = path == XAI_BN_FLAT4;
  const unsigned grid = static_cast<unsigned>(xai_ceil_div(n, static_cast<int64_t>(kBlock) * 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V) {
    hipLaunchKernelGGL((bn_relu_fwd_cnhw_kernel<decltype(V)::value>), dim3(grid), dim3(kBlock), 0, st, x, identity_cnhw, weight, bias, mean,
                       var, eps, bn2, variant, N, C, HW, n, wide, y, static_cast<uint64_t*>(mask));
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_bn_relu_bwd_compact_f32(const float* gy, const float* gy2, const float* gy2_compact, int W, int stride,
                                           const void* mask, const float* weight, const float* var, float eps, const float* weight2,
                                           const float* var2, float eps2, int variant, int guided, int N, int C, int HW, float* gx,
                                           float* g_identity, int g_identity_cnhw, xai_stream_t stream) {
  XAI_REQUIRE_PTR(gy);
  BwdExt e{};
  if (gy2_compact != nullptr) {
    XAI_REQUIRE(W > 0 && stride > 0 && HW > 0 && HW % W == 0, XAI_E_SHAPE);
    e.gy2c = gy2_compact; e.W = W; e.s = stride;
    e.Ho = xai_bn_strided_extent(HW / W, stride); e.Wo = xai_bn_strided_extent(W, stride);
  }
  e.gid_cnhw = g_identity_cnhw != 0;
  return bwd_ext_launch(gy, gy2, mask, weight, var, eps, weight2, var2, eps2, variant, guided, N, C, HW, e, gx, g_identity, stream);
}

XAI_EXPORT int xai_bn_relu_bwd_bcast_f32(const float* grad_out, const float* fc_weight, const int64_t* targets, int classes, float scale,
                                         float divisor, const float* gy2, const void* mask, const float* weight, const float* var,
                                         float eps, const float* weight2, const float* var2, float eps2, int variant, int guided, int N,
                                         int C, int HW, float* gx, float* g_identity, xai_stream_t stream) {
  XAI_REQUIRE_PTR(grad_out); XAI_REQUIRE_PTR(fc_weight); XAI_REQUIRE_PTR(targets);
  XAI_REQUIRE(classes > 0, XAI_E_SHAPE);
  BwdExt e{};
  e.out = grad_out; e.fc = fc_weight; e.target = targets; e.classes = classes; e.scale = scale; e.divisor = divisor;
  return bwd_ext_launch(nullptr, gy2, mask, weight, var, eps, weight2, var2, eps2, variant, guided, N, C, HW, e, gx, g_identity, stream);
}
