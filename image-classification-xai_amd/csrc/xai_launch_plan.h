// The row-chunk launch plan of the write-bound row builders (K1, K6, K26, K31): plain C++17 with nothing of HIP in it, so a host
// compiler builds it alone (tests/launch_plan_main.cpp).
#pragma once
#include <stdint.h>
#include <algorithm>

struct XaiRowPlan {
  int64_t tiles, chunks;  // gridDim.x: tiles of block * (4|1) floats along a row; gridDim.y: chunks of `per` rows
  int zdim, per;          // gridDim.z: C where every channel gets lanes of its own, else 1; rows a lane writes
  bool ok, hbm;           // chunks <= 65535 (a caller that bounds tiles too checks that itself); the HBM-sized branch was taken
};

// n rows of C * row_len floats for each of `images` images.  An output of `threshold` bytes or more is HBM-sized: it is written
// as many short streams, two rows per lane (and one channel, where the kernel can `split` its channels over gridDim.z and
// C <= 64).  A smaller one gets just enough row chunks for about 2048 workgroups.
static inline XaiRowPlan xai_row_chunk_plan(int64_t row_len, int block, bool vec, int n, int C, int64_t images, int64_t threshold,
                                            bool split) {
  XaiRowPlan p;
  p.tiles = (row_len + block * (vec ? 4 : 1) - 1) / (block * (vec ? 4 : 1));
  p.hbm = images * n * C * row_len * 4 >= threshold && (!split || C <= 64);
  p.zdim = p.hbm && split ? C : 1;
  if (p.hbm) {
    p.per = n >= 2 ? 2 : 1;
  } else {
    const int64_t wanted = (2048 + p.tiles * images - 1) / (p.tiles * images);
    const int c0 = static_cast<int>(std::min<int64_t>(n, std::max<int64_t>(1, wanted)));
    p.per = static_cast<int>((static_cast<int64_t>(n) + c0 - 1) / c0);
  }
  p.chunks = (static_cast<int64_t>(n) + p.per - 1) / p.per;
  p.ok = p.chunks <= 65535;
  return p;
}
