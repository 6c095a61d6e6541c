// Device parts shared by the two files of fused BN/ReLU kernels, bnrelu_kernels.hip (libxai_hip.so) and bnrelu_compact_kernels.hip
// (libxai_compact.so): the BatchNorm expressions in their `variant` orderings, the per-channel parameter fetch of the flat 16-byte
// path, the guided clamp and the gate-mask words.  One definition of each, so both files round alike and share one mask layout.
#pragma once
#include "xai_common.h"
#include "xai_bn_index.h"

constexpr int kBlock = 256;

// all tensors a launch would access 16 bytes at a time -> their addresses OR-ed, for xai_bn_path
static inline uintptr_t bn_low_bits(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return bits;
}

// every activation / gradient tensor here is read exactly once by these kernels: non-temporal loads keep them from pushing
// the just-written outputs (which the next convolution reads at once) out of L2 / Infinity Cache (ld4_nt, xai_common.h)

__device__ __forceinline__ float inv_std(float var, float eps, int variant) {
  return (variant & 1) ? rsqrtf(var + eps) : 1.f / sqrtf(var + eps);
}

__device__ __forceinline__ float bn_value(float x, float mean, float invstd, float w, float b, int variant) {
  const int grouping = (variant >> 1) & 3;
  const bool fma = (variant >> 3) & 1;
  if (grouping == 0) {                       // ((x - mean) * invstd) * w + b
    const float h = (x - mean) * invstd;
    return fma ? __builtin_fmaf(h, w, b) : h * w + b;
  }
  if (grouping == 1) {                       // (x - mean) * (w * invstd) + b
    const float s = w * invstd;
    return fma ? __builtin_fmaf(x - mean, s, b) : (x - mean) * s + b;
  }
  const float s = w * invstd;                // x * s + (b - mean * s)
  const float t = b - mean * s;
  return fma ? __builtin_fmaf(x, s, t) : x * s + t;
}

__device__ __forceinline__ float bn_grad(float g, float invstd, float w, int variant) {
  const int grouping = (variant >> 1) & 3;
  if (grouping == 0) return (g * w) * invstd;
  if (grouping == 1) return g * (w * invstd);
  return (g * invstd) * w;
}

// second BN (bn2.*, nullable as a set): the identity operand is itself a raw convolution output that still needs its own
// eval-mode BatchNorm -- the down-sample branch of a residual block: y = relu(bn(x) + bn2(identity)).
struct BnParams {
  const float* w;
  const float* b;
  const float* mean;
  const float* var;
  float eps;
};

// ---- the flat 16-byte path (XAI_BN_FLAT4, xai_bn_index.h): n % 4 == 0 and every tensor 16-byte aligned, but HW % 4 != 0
// (layer4: HW = 49).  A lane owns flat elements 4t .. 4t+3 exactly as on the vector path and moves them with one 16-byte
// access per tensor; only the channel differs per element.  It comes from i / HW and % C once per lane (32-bit where n < 2^31) and stepping, and the
// BN parameters are fetched per distinct channel, not per element.  Same expressions per element in the same order as the
// other two paths.  The VEC = false instantiations take it on a wave-uniform kernel argument (`flat`).
struct BnChannel {
  float m, is, w, b;                        // mean, inv_std, weight, bias of one channel (the backward uses is and w only)
};

// p[k] = load(channel of element k) for the four flat elements from s on.  HW >= 4: at most two channels, both fetched
// unconditionally and selected per element.  Below that up to four: fetched again wherever r wraps.
template <typename Load>
__device__ __forceinline__ void lane_channels(BnChannel (&p)[4], XaiBnLane s, int HW, int C, Load load) {
  if (HW >= 4) {
    const int split = xai_bn_lane_split(s, HW);
    const BnChannel a = load(s.c), b = load(xai_bn_next_channel(s.c, C));
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = k < split ? a : b;
  } else {
    p[0] = load(s.c);
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      s = xai_bn_lane_step(s, HW, C);
      p[k] = s.r != 0 ? p[k - 1] : load(s.c);
    }
  }
}

// Guided Backprop's rule at a ReLU (captum 0.7.0 GuidedBackprop, evaluatePerturbation.py:154-158): the COMPLETE gradient of the
// ReLU's output -- all consumers summed -- is clamped with relu() before the gate.  g <= 0 ? +0 : g keeps a NaN like F.relu and
// hands exactly +0 on, the value a closed gate hands on.
__device__ __forceinline__ float guided_clamp(float g) { return g <= 0.f ? 0.f : g; }

// ---- the 1-bit ReLU gate mask (layout: bnrelu_kernels.hip, "Mask layout")
constexpr int kGateGroup = 256;                 // elements per mask group = 4 per lane * 64 lanes

__device__ __forceinline__ void store_gate_words(uint64_t* __restrict__ mask, int64_t group, int lane, bool p0, bool p1, bool p2, bool p3) {
  const uint64_t b0 = __ballot(p0), b1 = __ballot(p1), b2 = __ballot(p2), b3 = __ballot(p3);
  if (lane < 4) mask[group * 4 + lane] = lane == 0 ? b0 : lane == 1 ? b1 : lane == 2 ? b2 : b3;
}
