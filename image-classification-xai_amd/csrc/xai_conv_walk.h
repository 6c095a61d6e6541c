// The K-walk of the 1x1 backward-data GEMM (conv1x1_bwd_kernels.hip): which 16-wide K-blocks go to which partial sum, in which
// order the partial sums are added, and how the 16 k of a block are spread over four v_mfma_f32_16x16x4_f32.  It is data, not
// code: the kernels walk whatever plan they are handed, so one kernel restates every split-K summation order of this family.
// Plain C++17 with nothing of HIP in it, usable from device code, so a host compiler builds it alone (tests/conv_walk_main.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XAI_WALK_HD __host__ __device__
#else
#define XAI_WALK_HD
#endif

constexpr int kWalkBlock = 16;      // k per K-block: one LDS slab, four MFMAs of four k
constexpr int kWalkMaxSplits = 32;

// Split membership: which K-blocks belong to partial sum s of S, nb = K / 16 blocks in all, q = nb / S, r = nb % S.  Either way
// partial s owns q + (s < r) blocks, the remainder in front.
//   XAI_WALK_CONTIGUOUS:  blocks s*q + min(s, r) ... in one run
//   XAI_WALK_ROUND_ROBIN: blocks s, s + S, s + 2S, ...
enum XaiWalkMembership { XAI_WALK_CONTIGUOUS = 0, XAI_WALK_ROUND_ROBIN = 1 };
// k grouping: the k (inside its block) that MFMA m = 0..3 takes in slot q = 0..3; an MFMA is the fmaf chain over its slots in order.
//   XAI_WALK_K_CONSECUTIVE: 4m + q        XAI_WALK_K_STRIDE4: m + 4q
enum XaiWalkGrouping { XAI_WALK_K_CONSECUTIVE = 0, XAI_WALK_K_STRIDE4 = 1 };
// Partial-sum order: the partial sums are added one after the other, ascending (0, 1, ...) or descending (S-1, ...), starting from
// the first of them or (from_zero) from +0.
enum XaiWalkOrder { XAI_WALK_ASCENDING = 0, XAI_WALK_DESCENDING = 1 };

struct XaiWalkPart {
  int first, step, count;      // K-blocks first, first + step, ..., `count` of them (0: an empty partial sum, +0)
};

struct XaiWalk {
  int splits;                  // S
  int grouping;                // XaiWalkGrouping
  int from_zero;               // the sum of the partial sums starts from +0, not from the first of them
  XaiWalkPart part[kWalkMaxSplits];      // in the order in which they are added
};

// -> false (and *w untouched) for K < 16, K % 16 != 0, S outside 1 .. kWalkMaxSplits or an unknown enum value
XAI_WALK_HD inline bool xai_walk_plan(int K, int splits, int membership, int grouping, int order, int from_zero, XaiWalk* w) {
  if (K < kWalkBlock || K % kWalkBlock != 0 || splits < 1 || splits > kWalkMaxSplits) return false;
  if ((membership != XAI_WALK_CONTIGUOUS && membership != XAI_WALK_ROUND_ROBIN) ||
      (grouping != XAI_WALK_K_CONSECUTIVE && grouping != XAI_WALK_K_STRIDE4) ||
      (order != XAI_WALK_ASCENDING && order != XAI_WALK_DESCENDING))
    return false;
  const int nb = K / kWalkBlock, q = nb / splits, r = nb % splits;
  XaiWalk out{};
  out.splits = splits;
  out.grouping = grouping;
  out.from_zero = from_zero != 0;
  for (int i = 0; i < splits; ++i) {
    const int s = order == XAI_WALK_ASCENDING ? i : splits - 1 - i;
    XaiWalkPart& p = out.part[i];
    p.count = q + (s < r ? 1 : 0);
    if (membership == XAI_WALK_CONTIGUOUS) {
      p.first = s * q + (s < r ? s : r);
      p.step = 1;
    } else {
      p.first = s;
      p.step = splits;
    }
  }
  *w = out;
  return true;
}

// K-block t of part p
XAI_WALK_HD inline int xai_walk_block(const XaiWalk& w, int p, int t) { return w.part[p].first + t * w.part[p].step; }

// The k inside its block that MFMA m takes in slot q, and its inverse: the row (4m + q) at which k lies in a slab laid out for
// MFMA m to read rows 4m .. 4m+3.
XAI_WALK_HD inline int xai_walk_k(int grouping, int m, int q) { return grouping == XAI_WALK_K_STRIDE4 ? m + 4 * q : 4 * m + q; }
XAI_WALK_HD inline int xai_walk_row(int grouping, int k) { return grouping == XAI_WALK_K_STRIDE4 ? (k & 3) * 4 + (k >> 2) : k; }

#undef XAI_WALK_HD
