// Index arithmetic of the fused BN/ReLU kernels (bnrelu_kernels.hip): which of the three element paths a launch takes, and
// the channels of the four consecutive flat elements a lane owns in a [N][C][HW] tensor.  Plain C++17 with nothing of HIP in
// it, usable from device code, so a host compiler builds it alone (tests/bn_index_main.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XAI_HD __host__ __device__
#else
#define XAI_HD
#endif

// XAI_BN_VEC4:   HW % 4 == 0, a lane's four elements share a channel; one 16-byte access per tensor.
// XAI_BN_FLAT4:  n % 4 == 0 but HW % 4 != 0 (layer4: HW = 49): still one 16-byte access per tensor, the channel is taken per
//                element by stepping (below).
// XAI_BN_SCALAR: everything else, one 4-byte access per element.
enum XaiBnPath { XAI_BN_SCALAR = 0, XAI_BN_VEC4 = 1, XAI_BN_FLAT4 = 2 };

// low_bits: the addresses of all tensors the kernel would access 16 bytes at a time, OR-ed together (a null one adds nothing)
XAI_HD inline XaiBnPath xai_bn_path(int64_t n, int HW, uintptr_t low_bits) {
  if ((n & 3) != 0 || (low_bits & 15u) != 0) return XAI_BN_SCALAR;
  return (HW & 3) == 0 ? XAI_BN_VEC4 : XAI_BN_FLAT4;
}

// 32-bit index arithmetic is exact when every flat index fits: n < 2^31
XAI_HD inline bool xai_bn_index32(int64_t n) { return n < (int64_t{1} << 31); }

// Where flat element i sits: r = i % HW inside its plane, c = (i / HW) % C its channel.
struct XaiBnLane {
  int r, c;
};

// Two unsigned 32-bit divisions where n < 2^31 (i < n), the 64-bit form otherwise.
XAI_HD inline XaiBnLane xai_bn_lane_first(int64_t i, int64_t n, int HW, int C) {
  XaiBnLane s;
  if (xai_bn_index32(n)) {
    const uint32_t ii = static_cast<uint32_t>(i), q = ii / static_cast<uint32_t>(HW);
    s.r = static_cast<int>(ii - q * static_cast<uint32_t>(HW));
    s.c = static_cast<int>(q % static_cast<uint32_t>(C));
  } else {
    const int64_t q = i / HW;
    s.r = static_cast<int>(i - q * HW);
    s.c = static_cast<int>(q % C);
  }
  return s;
}

XAI_HD inline int xai_bn_next_channel(int c, int C) { return c + 1 == C ? 0 : c + 1; }

// The element after s: r wraps to 0 and carries into c, c wraps to 0 at C (the next image).
XAI_HD inline XaiBnLane xai_bn_lane_step(XaiBnLane s, int HW, int C) {
  if (++s.r == HW) {
    s.r = 0;
    s.c = xai_bn_next_channel(s.c, C);
  }
  return s;
}

// The image of flat element i: (i / HW) / C, the n of [N][C][HW] (the broadcast-gradient backward reads per-image operands).
XAI_HD inline int xai_bn_image_first(int64_t i, int64_t n, int HW, int C) {
  if (xai_bn_index32(n)) return static_cast<int>(static_cast<uint32_t>(i) / static_cast<uint32_t>(HW) / static_cast<uint32_t>(C));
  return static_cast<int>(i / HW / C);
}

// The image of the element after one of image `image`, where `after` = xai_bn_lane_step(its position): a step that lands on
// (r, c) = (0, 0) has entered the next image.
XAI_HD inline int xai_bn_image_step(int image, XaiBnLane after) { return image + (after.r == 0 && after.c == 0 ? 1 : 0); }

// ---- channel-major (CNHW) and strided operands of bnrelu_compact_kernels.hip
// Where element (image, c, r) of an [N][C][HW] tensor sits in its [C][N][HW] (CNHW) twin.  N * C fits an int (the wrappers check).
XAI_HD inline int64_t xai_bn_cnhw_index(int image, int c, int r, int N, int HW) {
  return (static_cast<int64_t>(c) * N + image) * HW + r;
}

// Output extent of a kernel-1, pad-0 window at stride s over H positions: the positions 0, s, 2s, ... below H.
XAI_HD inline int xai_bn_strided_extent(int H, int s) { return (H - 1) / s + 1; }

// Flat index of side[n][c][ho * s][wo * s] in an [N][C][H][W] tensor: what output (ho, wo) of that window reads.
XAI_HD inline int64_t xai_bn_strided_index(int n, int c, int ho, int wo, int C, int H, int W, int s) {
  return ((static_cast<int64_t>(n) * C + c) * H + static_cast<int64_t>(ho) * s) * W + static_cast<int64_t>(wo) * s;
}

// HW >= 4: a lane's four elements touch at most two channels, s.c and the next one; elements k < xai_bn_lane_split(s, HW) are
// in the first.
XAI_HD inline int xai_bn_lane_split(XaiBnLane s, int HW) { return HW - s.r; }
