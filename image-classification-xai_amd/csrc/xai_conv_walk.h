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

// ---- the staggered start of a K loop -------------------------------------------------------------------------------------
// A GEMM library's kernel whose name says SU<n> and SUS<bytes> (n > 0) does not start every output tile's K loop at k = 0: the loop
// runs K / depth iterations of `depth` k each, and the workgroup whose output tile is number w along one axis starts at iteration
// s(w) = (w & mask) << shift, goes on to the last iteration, wraps and ends with iteration s(w) - 1.  shift makes a step of s `stride`
// bytes of a K-contiguous operand (log2(stride / (4 * depth)), 0 where that is below one iteration), and mask + 1 is the largest
// power of two <= n with (mask + 1) << shift <= K / depth (mask 0: every tile starts at 0).  One partial sum; what is a rotation of
// the K-blocks per tile.  profiles/wide_bwd_walk_probe.txt has the kernels whose bits this reproduces.
enum XaiStaggerAxis { XAI_STAGGER_COLUMNS = 0, XAI_STAGGER_ROWS = 1 };      // the tile number counts hw / tile, or c / tile

struct XaiStagger {
  int blocks;                  // K-blocks (of kWalkBlock) in K
  int per_iter;                // K-blocks per loop iteration: depth / kWalkBlock
  int tile;                    // outputs per tile along the axis
  int axis;                    // XaiStaggerAxis
  int mask, shift;
};

// -> false (and *st untouched) for K or depth no positive multiple of 16, K % depth != 0, tile no positive multiple of 16, an
// unknown axis, n negative or no power of two (0: no stagger), stride negative
XAI_WALK_HD inline bool xai_stagger_plan(int K, int depth, int tile, int axis, int n, int stride, XaiStagger* st) {
  if (K < kWalkBlock || depth < kWalkBlock || depth % kWalkBlock != 0 || K % depth != 0 || tile < 16 || tile % 16 != 0) return false;
  if ((axis != XAI_STAGGER_COLUMNS && axis != XAI_STAGGER_ROWS) || n < 0 || (n & (n - 1)) != 0 || stride < 0) return false;
  XaiStagger out{};
  out.blocks = K / kWalkBlock;
  out.per_iter = depth / kWalkBlock;
  out.tile = tile;
  out.axis = axis;
  const int iters = K / depth;
  int shift = 0;
  while ((static_cast<int64_t>(4) * depth << (shift + 1)) <= stride) ++shift;
  int su = n;
  while (su > 1 && iters < (static_cast<int64_t>(su) << shift)) su /= 2;
  out.mask = su >= 1 ? su - 1 : 0;
  out.shift = out.mask != 0 ? shift : 0;
  *st = out;
  return true;
}

// the K-block at which the output at `at` along the axis (hw inside its image, or c) starts, and the t-th K-block of its chain
XAI_WALK_HD inline int xai_stagger_first(const XaiStagger& st, int at) { return (((at / st.tile) & st.mask) << st.shift) * st.per_iter; }
XAI_WALK_HD inline int xai_stagger_block(const XaiStagger& st, int first, int t) { return (first + t) % st.blocks; }

#undef XAI_WALK_HD
