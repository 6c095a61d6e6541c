// K78-K79: the input gradient of a kernel-1, stride-1, pad-0 convolution, gx[n][c][hw] = sum_k gy[n][k][hw] * W[k][c], as an fp32
// MFMA GEMM whose order of summation is a launch argument (xai_conv_walk.h).  Part of libxai_conv.so (include/xai_conv.h).
//
// MIOpen hands this convolution to a GEMM library as N GEMMs of HW x C x K.  At layer4 of ResNet-50 (HW = 49, C = 512, K = 2048)
// that library cuts K into 19 partial sums, writes them to a workspace of its handle and adds them in a second kernel, on tiles
// of 192 x 48 that are mostly padding because 49 = 48 + 1.  Here the batch is folded into the columns (N * HW of them, padding only in the
// last tile), and the partial sums stay in registers and are added there in the library's order, so the result is the same bits.
//   K78  a workgroup owns TM x 64 outputs (rows c, columns the folded (n, hw)), TM / 32 x 2 waves of 32 x 32 each; slabs of 16 k go
//        from global memory through registers into one of two LDS buffers while the other is multiplied: one barrier per slab.
//   K79  one wave per 16 x 16 outputs, operands straight from global memory: the plain restatement K78 is held to.
// Per output element both do the same thing: for every partial sum of the walk, in its order, an accumulator starts at +0 and takes
// the partial sum's K-blocks in ascending order, four v_mfma_f32_16x16x4_f32 per block; a 16x16x4 MFMA is the fmaf chain over its
// four k slots in order, and which k sits in which slot of which MFMA is the walk's grouping.  Then total = first partial (or
// +0 + it), total += the next, ...
#include "xai_common.h"
#include "xai_conv_walk.h"
#include "xai_conv.h"

// the version pair of libxai_conv.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_conv_version, XAI_CONV_VERSION, XAI_CONV_MINOR)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileCols = 64;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// total (op) partial, the first time and every later time
__device__ __forceinline__ f32x4 fold(f32x4 total, f32x4 part, bool first, bool from_zero) {
  if (!first) return total + part;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  return from_zero ? zero + part : part;
}

// Where the folded column `col` = n * HW + hw starts in gy ([N][K][HW], + k * HW per k) and in gx ([N][C][HW], + c * HW per c)
struct Column {
  int64_t gy, gx;
};
__device__ __forceinline__ Column column_of(int col, int K, int C, int HW) {
  const int n = col / HW, hw = col - n * HW;
  return Column{static_cast<int64_t>(n) * K * HW + hw, static_cast<int64_t>(n) * C * HW + hw};
}

// ---- K79 ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void conv1x1_bwd_simple_kernel(const float* __restrict__ gy, const float* __restrict__ W, int K,
                                                                   int C, int HW, int cols, XaiWalk walk, float* __restrict__ gx) {
  const int lane = threadIdx.x, slot = lane >> 4, l16 = lane & 15;
  const int row = blockIdx.y * 16 + l16;             // the A operand's c
  const int col = blockIdx.x * 16 + l16;             // the B operand's (n, hw); also the column this lane stores
  const bool row_ok = row < C, col_ok = col < cols;
  const Column cl = column_of(col_ok ? col : 0, K, C, HW);
  f32x4 total = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < walk.splits; ++p) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < walk.part[p].count; ++t) {
      const int k0 = xai_walk_block(walk, p, t) * kWalkBlock;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int k = k0 + xai_walk_k(walk.grouping, m, slot);
        const float a = row_ok ? W[static_cast<int64_t>(k) * C + row] : 0.f;
        const float b = col_ok ? gy[cl.gy + static_cast<int64_t>(k) * HW] : 0.f;
        acc = mfma4(a, b, acc);
      }
    }
    total = fold(total, acc, p == 0, walk.from_zero != 0);
  }
  if (!col_ok) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {                       // D[i = 4 * slot + r][j = l16]
    const int c = blockIdx.y * 16 + 4 * slot + r;
    if (c < C) gx[cl.gx + static_cast<int64_t>(c) * HW] = total[r];
  }
}

// ---- K78 ----------------------------------------------------------------------------------------------------------------
// The K-blocks of the walk, one after the other across the partial sums; empty partial sums are stepped over
struct WalkCursor {
  int p, t;
};
__device__ __forceinline__ void cursor_settle(const XaiWalk& w, WalkCursor& c) {
  while (c.p < w.splits && c.t >= w.part[c.p].count) {
    ++c.p;
    c.t = 0;
  }
}

template <int TM>
__global__ __launch_bounds__(TM * 4) void conv1x1_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ W, int K, int C,
                                                             int HW, int cols, XaiWalk walk, float* __restrict__ gx) {
  constexpr int NT = TM * 4, TN = kTileCols;
  // + 16: the four k rows an MFMA operand read touches fall into four different quarters of the banks
  constexpr int LDA = TM + 16, LDB = TN + 16;
  constexpr int RA = kWalkBlock * TM / NT, RB = kWalkBlock * TN / NT;      // loads per lane and slab
  constexpr int KA = NT / TM, KB = NT / TN;                                // k rows one pass of the workgroup covers
  __shared__ float As[2][kWalkBlock * LDA];
  __shared__ float Bs[2][kWalkBlock * LDB];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int slot = lane >> 4, l16 = lane & 15;
  const int row0 = blockIdx.y * TM, col0 = blockIdx.x * TN;

  // what this lane carries from global memory to LDS: one row (c) of A and one column of B, at k rows ak + r * KA / bk + r * KB
  const int ai = tid % TM, ak = tid / TM;
  const bool a_ok = row0 + ai < C;
  const float* ap = W + (a_ok ? row0 + ai : 0);
  const int bj = tid % TN, bk = tid / TN;
  const bool b_ok = col0 + bj < cols;
  const float* bp = gy + column_of(b_ok ? col0 + bj : 0, K, C, HW).gy;
  float ra[RA], rb[RB];
  auto load = [&](int block) {
    const int k0 = block * kWalkBlock;
#pragma unroll
    for (int r = 0; r < RA; ++r) ra[r] = a_ok ? ap[static_cast<int64_t>(k0 + ak + r * KA) * C] : 0.f;
#pragma unroll
    for (int r = 0; r < RB; ++r) rb[r] = b_ok ? bp[static_cast<int64_t>(k0 + bk + r * KB) * HW] : 0.f;
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int r = 0; r < RA; ++r) As[buf][xai_walk_row(walk.grouping, ak + r * KA) * LDA + ai] = ra[r];
#pragma unroll
    for (int r = 0; r < RB; ++r) Bs[buf][xai_walk_row(walk.grouping, bk + r * KB) * LDB + bj] = rb[r];
  };

  // this wave's 32 x 32 outputs: 2 x 2 MFMA tiles
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  f32x4 total[2][2], acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) total[i][j] = acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  WalkCursor next{0, 0};                              // the block being fetched, one ahead of the one being multiplied
  cursor_settle(walk, next);
  if (next.p < walk.splits) {
    load(xai_walk_block(walk, next.p, next.t));
    ++next.t;
    cursor_settle(walk, next);
  }
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int p = 0; p < walk.splits; ++p) {
    for (int t = 0; t < walk.part[p].count; ++t) {
      const bool more = next.p < walk.splits;
      if (more) {
        load(xai_walk_block(walk, next.p, next.t));
        ++next.t;
        cursor_settle(walk, next);
      }
      const float* A = As[buf];
      const float* B = Bs[buf];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int krow = 4 * m + slot;
        const float a0 = A[krow * LDA + wr + l16], a1 = A[krow * LDA + wr + 16 + l16];
        const float b0 = B[krow * LDB + wc + l16], b1 = B[krow * LDB + wc + 16 + l16];
        acc[0][0] = mfma4(a0, b0, acc[0][0]);
        acc[0][1] = mfma4(a0, b1, acc[0][1]);
        acc[1][0] = mfma4(a1, b0, acc[1][0]);
        acc[1][1] = mfma4(a1, b1, acc[1][1]);
      }
      if (more) stage(buf ^ 1);                       // last read before the barrier that ended the block before this one
      __syncthreads();
      buf ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        total[i][j] = fold(total[i][j], acc[i][j], p == 0, walk.from_zero != 0);
        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = col0 + wc + 16 * j + l16;
    if (col >= cols) continue;
    const int64_t at = column_of(col, K, C, HW).gx;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {                   // D[4 * slot + r][l16] of MFMA tile (i, j)
        const int c = row0 + wr + 16 * i + 4 * slot + r;
        if (c < C) gx[at + static_cast<int64_t>(c) * HW] = total[i][j][r];
      }
  }
}

// the checks the two entry points share -> the plan and the folded column count
static int conv_args_status(const float* gy, const float* weight, int N, int K, int C, int HW, int splits, int membership, int grouping,
                            int order, int from_zero, const float* gx, XaiWalk* walk, int* cols) {
  XAI_REQUIRE_PTR(gy); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(gx);
  XAI_REQUIRE(N > 0 && K > 0 && C > 0 && HW > 0, XAI_E_SHAPE);
  XAI_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(gx)) & 3u) == 0,
              XAI_E_SHAPE);
  XAI_REQUIRE(xai_walk_plan(K, splits, membership, grouping, order, from_zero, walk), XAI_E_SHAPE);
  const int64_t n_cols = static_cast<int64_t>(N) * HW;
  XAI_REQUIRE(n_cols <= INT32_MAX && n_cols * K <= INT32_MAX && n_cols * C <= INT32_MAX, XAI_E_UNSUPPORTED);
  *cols = static_cast<int>(n_cols);
  return XAI_OK;
}

}  // namespace

XAI_EXPORT int xai_conv1x1_bwd_data_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int splits, int membership,
                                        int grouping, int order, int from_zero, int tile_rows, float* gx, xai_stream_t stream) {
  XaiWalk walk;
  int cols;
  if (const int rc = conv_args_status(gy, weight, N, K, C, HW, splits, membership, grouping, order, from_zero, gx, &walk, &cols)) return rc;
  XAI_REQUIRE(tile_rows == 0 || tile_rows == 32 || tile_rows == 64, XAI_E_SHAPE);
  const int tm = tile_rows != 0 ? tile_rows : 64;
  const dim3 grid(static_cast<unsigned>(xai_ceil_div(cols, kTileCols)), static_cast<unsigned>(xai_ceil_div(C, tm)));
  XAI_REQUIRE(grid.y <= 65535u, XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(tm == 64, [&](auto big) {
    constexpr int TM = decltype(big)::value ? 64 : 32;
    hipLaunchKernelGGL((conv1x1_bwd_kernel<TM>), grid, dim3(TM * 4), 0, st, gy, weight, K, C, HW, cols, walk, gx);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_conv1x1_bwd_data_simple_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int splits,
                                               int membership, int grouping, int order, int from_zero, float* gx, xai_stream_t stream) {
  XaiWalk walk;
  int cols;
  if (const int rc = conv_args_status(gy, weight, N, K, C, HW, splits, membership, grouping, order, from_zero, gx, &walk, &cols)) return rc;
  const dim3 grid(static_cast<unsigned>(xai_ceil_div(cols, 16)), static_cast<unsigned>(xai_ceil_div(C, 16)));
  XAI_REQUIRE(grid.y <= 65535u, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(conv1x1_bwd_simple_kernel, grid, dim3(kWave), 0, static_cast<hipStream_t>(stream), gy, weight, K, C, HW, cols, walk, gx);
  return xai_launch_status();
}
