// K80-K81: the input gradient of a kernel-1, stride-1, pad-0 convolution on large planes, gx[n][c][hw] = sum_k gy[n][k][hw] * W[k][c],
// as an fp32 MFMA GEMM that reads every element of gy from global memory once and writes every element of gx once, in an order of
// summation that is a launch argument.  Part of libxai_convw.so (include/xai_convw.h).
//
// MIOpen hands this convolution to a GEMM library as one GEMM per image, HW x C x K.  For some shapes (in ResNet-50 at batch 50: 512 ->
// 128 on 28 x 28, and the 14 x 14 planes) that library picks kernels with output tiles 32 wide (MT32x32x64, MT32x64x64), which fetch gy
// C / 32 or C / 64 times, and which start each tile's K loop at an iteration of its own (xai_conv_walk.h: the staggered start).
// Here a workgroup of four waves owns TM rows (c) of TN columns (hw) of one image, TN being at most the library's tile so that one
// start holds for the workgroup, and walks the K-blocks of 16 from that start round to it: a slab of gy (16 x TN) and one of W
// (16 x TM) go from global memory through registers into LDS while the slab before is multiplied, one barrier per slab.  C > TM is cut into chunks of TM rows: with K small enough the workgroup keeps all
// its gy slabs in LDS and loops over the chunks (gy read once), else a chunk is a workgroup of its own (blockIdx.z).
//   K80  the kernel above.  Loads are 16 bytes wide where HW % 4 == 0, C % 4 == 0 and the pointers allow it, else dwords.
//   K81  one wave per 16 x 16 outputs of one image, operands straight from global memory: the plain restatement K80 is held to; with
//        no stagger it is K79's sum of one partial sum.
// Per output element both do the same thing: an accumulator starts at +0 and takes the K-blocks in the chain's order, four
// v_mfma_f32_16x16x4_f32 per block; a 16x16x4 MFMA is the fmaf chain over its four k slots in order (xai_walk_k has which k sits where).
#include "xai_common.h"
#include "xai_conv_walk.h"
#include "xai_convw.h"

XAI_VERSION_ENTRIES(xai_convw_version, XAI_CONVW_VERSION, XAI_CONVW_MINOR)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- K81 ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void conv1x1_bwd_wide_simple_kernel(const float* __restrict__ gy, const float* __restrict__ W, int K,
                                                                        int C, int HW, int grouping, int from_zero, XaiStagger st,
                                                                        float* __restrict__ gx) {
  const int lane = threadIdx.x, slot = lane >> 4, l16 = lane & 15;
  const int row = blockIdx.y * 16 + l16;             // the A operand's c
  const int col = blockIdx.x * 16 + l16;             // the B operand's hw; also the column this lane stores
  const bool row_ok = row < C, col_ok = col < HW;
  const float* gyn = gy + static_cast<int64_t>(blockIdx.z) * K * HW + (col_ok ? col : 0);
  float* gxn = gx + static_cast<int64_t>(blockIdx.z) * C * HW + (col_ok ? col : 0);
  // 16 | tile: the 16 rows and the 16 columns of this wave lie in one tile, so they start at the same K-block
  const int first = xai_stagger_first(st, 16 * (st.axis == XAI_STAGGER_ROWS ? blockIdx.y : blockIdx.x));
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < st.blocks; ++t) {
    const int k0 = xai_stagger_block(st, first, t) * kWalkBlock;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = k0 + xai_walk_k(grouping, m, slot);
      const float a = row_ok ? W[static_cast<int64_t>(k) * C + row] : 0.f;
      const float b = col_ok ? gyn[static_cast<int64_t>(k) * HW] : 0.f;
      acc = mfma4(a, b, acc);
    }
  }
  if (from_zero) acc = f32x4{0.f, 0.f, 0.f, 0.f} + acc;
  if (!col_ok) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {                       // D[i = 4 * slot + r][j = l16]
    const int c = blockIdx.y * 16 + 4 * slot + r;
    if (c < C) gxn[static_cast<int64_t>(c) * HW] = acc[r];
  }
}

// ---- K80 ----------------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kPad = 16;       // floats: the two k rows the 32 lanes of an operand read touch fall into the two halves of the banks

// four values that lie side by side in memory, as one 16-byte load or as dwords of which only the first `valid` exist
__device__ __forceinline__ f32x4 load4(const float* p, int valid, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid <= 0) return v;
  if (vec) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < valid) v[j] = p[j];
  return v;
}

// TM x TN outputs per workgroup and chunk; the waves lie TM / 32 down the rows and the rest across the columns, 32 x (16 NJ) each
template <int TM, int TN>
__global__ __launch_bounds__(kThreads) void conv1x1_bwd_wide_kernel(const float* __restrict__ gy, const float* __restrict__ W, int K, int C,
                                                                    int HW, int grouping, int from_zero, XaiStagger st, int hold, int vec,
                                                                    float* __restrict__ gx) {
  constexpr int LDA = TM + kPad, LDB = TN + kPad;
  constexpr int WROWS = TM / 32, WCOLS = 4 / WROWS, NJ = TN / (16 * WCOLS);
  constexpr int UA = TM / 4, UB = TN / 4;                                  // 4-wide units per k row
  constexpr int RA = kWalkBlock * UA / kThreads;                           // units of A per lane and slab: 1 or 2
  static_assert(RA >= 1 && kWalkBlock * UB <= kThreads && NJ >= 1, "tile sizes");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* As = lds;                                                         // [2][16 * LDA]
  float* Bs = lds + 2 * kWalkBlock * LDA;                                  // [hold ? K / 16 : 2][16 * LDB]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int slot = lane >> 4, l16 = lane & 15;
  const int col0 = blockIdx.x * TN, n = blockIdx.y;
  const int nb = st.blocks;
  const int chunks = hold ? (C + TM - 1) / TM : 1, chunk0 = hold ? 0 : blockIdx.z;
  const int first = xai_stagger_first(st, col0);                           // TN <= tile and tile % TN == 0: one start for all columns

  // what this lane carries from global memory to LDS per slab: RA units of A (rows ai .. ai + 3 at k row ak) and one of B
  const int bk = tid / UB, bj = (tid % UB) * 4;
  const bool b_lane = tid < kWalkBlock * UB;
  const int b_valid = b_lane ? min(4, HW - (col0 + bj)) : 0;
  const float* bp = gy + static_cast<int64_t>(n) * K * HW + (b_valid > 0 ? col0 + bj : 0);
  f32x4 ra[RA], rb;
  auto load = [&](int g) {                           // g: the slab's number, chunk after chunk
    const int chunk = chunk0 + g / nb, block = xai_stagger_block(st, first, g % nb);
    const int k0 = block * kWalkBlock;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      const int u = tid + r * kThreads, ak = u / UA, ai = chunk * TM + (u % UA) * 4;
      ra[r] = load4(W + static_cast<int64_t>(k0 + ak) * C + (ai < C ? ai : 0), C - ai, vec != 0);
    }
    if (g < nb || !hold) rb = load4(bp + static_cast<int64_t>(k0 + bk) * HW, b_valid, vec != 0);
  };
  auto stage = [&](int g) {
    float* A = As + (g & 1) * kWalkBlock * LDA;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      const int u = tid + r * kThreads, ak = u / UA, ai = (u % UA) * 4;
      *reinterpret_cast<f32x4*>(A + xai_walk_row(grouping, ak) * LDA + ai) = ra[r];
    }
    if (b_lane && (g < nb || !hold)) {
      float* B = Bs + (hold ? xai_stagger_block(st, first, g % nb) : (g & 1)) * kWalkBlock * LDB;
      *reinterpret_cast<f32x4*>(B + xai_walk_row(grouping, bk) * LDB + bj) = rb;
    }
  };

  const int wr = (wave / WCOLS) * 32, wc = (wave % WCOLS) * (16 * NJ);
  f32x4 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int slabs = chunks * nb;
  load(0);
  stage(0);
  __syncthreads();
  int t = 0;                                          // g % nb
  for (int g = 0; g < slabs; ++g) {
    const bool more = g + 1 < slabs;
    if (more) load(g + 1);
    const float* A = As + (g & 1) * kWalkBlock * LDA;
    const float* B = Bs + (hold ? xai_stagger_block(st, first, t) : (g & 1)) * kWalkBlock * LDB;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int krow = 4 * m + slot;
      const float a0 = A[krow * LDA + wr + l16], a1 = A[krow * LDA + wr + 16 + l16];
      float b[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[j] = B[krow * LDB + wc + 16 * j + l16];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        acc[0][j] = mfma4(a0, b[j], acc[0][j]);
        acc[1][j] = mfma4(a1, b[j], acc[1][j]);
      }
    }
    if (more) stage(g + 1);                           // last read before the barrier that ended the slab before this one
    __syncthreads();
    if (++t < nb) continue;
    t = 0;
    const int row0 = (chunk0 + g / nb) * TM;          // the chunk is complete: its rows leave, the accumulators start again
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = col0 + wc + 16 * j + l16;
      float* out = gx + static_cast<int64_t>(n) * C * HW + col;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (from_zero) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f} + acc[i][j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                 // D[4 * slot + r][l16] of MFMA tile (i, j)
          const int c = row0 + wr + 16 * i + 4 * slot + r;
          if (col < HW && c < C) out[static_cast<int64_t>(c) * HW] = acc[i][j][r];
        }
        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
}

constexpr int kHoldBytes = 40 * 1024;      // all of a workgroup's gy slabs stay in LDS up to this size (K = 128 at 64 columns): with the
                                           // two slabs of W under 64 KiB of dynamic LDS, two workgroups per CU

// the checks the two entry points share -> the stagger plan
static int wide_args_status(const float* gy, const float* weight, int N, int K, int C, int HW, int grouping, int depth, int tile, int axis,
                            int stagger, int stride, const float* gx, XaiStagger* st) {
  XAI_REQUIRE_PTR(gy); XAI_REQUIRE_PTR(weight); XAI_REQUIRE_PTR(gx);
  XAI_REQUIRE(N > 0 && K > 0 && C > 0 && HW > 0, XAI_E_SHAPE);
  XAI_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(gx)) & 3u) == 0,
              XAI_E_SHAPE);
  XAI_REQUIRE(grouping == XAI_WALK_K_CONSECUTIVE || grouping == XAI_WALK_K_STRIDE4, XAI_E_SHAPE);
  XAI_REQUIRE(xai_stagger_plan(K, depth, tile, axis, stagger, stride, st), XAI_E_SHAPE);
  XAI_REQUIRE(N <= 65535 && static_cast<int64_t>(K) * HW <= INT32_MAX && static_cast<int64_t>(C) * HW <= INT32_MAX, XAI_E_UNSUPPORTED);
  return XAI_OK;
}

}  // namespace

XAI_EXPORT int xai_convw_bwd_data_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int grouping, int from_zero,
                                      int depth, int tile, int axis, int stagger, int stride, float* gx, xai_stream_t stream) {
  XaiStagger st;
  if (const int rc = wide_args_status(gy, weight, N, K, C, HW, grouping, depth, tile, axis, stagger, stride, gx, &st)) return rc;
  // one start per workgroup: its columns lie in one tile of the stagger.  Tiles along the rows would cut a workgroup's rows.
  XAI_REQUIRE(st.mask == 0 || (axis == XAI_STAGGER_COLUMNS && tile % 32 == 0), XAI_E_UNSUPPORTED);
  const int tn = st.mask != 0 && tile % 64 != 0 ? 32 : 64, tm = C <= 64 ? 64 : 128;
  const int chunks = static_cast<int>(xai_ceil_div(C, tm));
  const size_t slab_b = sizeof(float) * kWalkBlock * (tn + kPad);
  const bool hold = chunks > 1 && slab_b * st.blocks <= static_cast<size_t>(kHoldBytes);
  XAI_REQUIRE(chunks <= 65535, XAI_E_UNSUPPORTED);
  const bool vec = HW % 4 == 0 && C % 4 == 0 && xai_aligned16(gy) && xai_aligned16(weight);
  const size_t lds = sizeof(float) * 2 * kWalkBlock * (tm + kPad) + slab_b * (hold ? st.blocks : 2);
  const dim3 grid(static_cast<unsigned>(xai_ceil_div(HW, tn)), static_cast<unsigned>(N), static_cast<unsigned>(hold ? 1 : chunks));
  hipStream_t s = static_cast<hipStream_t>(stream);
  xai_dispatch(tm == 128, [&](auto tall) {
    xai_dispatch(tn == 64, [&](auto broad) {
      constexpr int TM = decltype(tall)::value ? 128 : 64, TN = decltype(broad)::value ? 64 : 32;
      hipLaunchKernelGGL((conv1x1_bwd_wide_kernel<TM, TN>), grid, dim3(kThreads), lds, s, gy, weight, K, C, HW, grouping, from_zero != 0, st,
                         hold ? 1 : 0, vec ? 1 : 0, gx);
    });
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_convw_bwd_data_simple_f32(const float* gy, const float* weight, int N, int K, int C, int HW, int grouping, int from_zero,
                                             int depth, int tile, int axis, int stagger, int stride, float* gx, xai_stream_t stream) {
  XaiStagger st;
  if (const int rc = wide_args_status(gy, weight, N, K, C, HW, grouping, depth, tile, axis, stagger, stride, gx, &st)) return rc;
  const dim3 grid(static_cast<unsigned>(xai_ceil_div(HW, 16)), static_cast<unsigned>(xai_ceil_div(C, 16)), static_cast<unsigned>(N));
  XAI_REQUIRE(grid.y <= 65535u, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(conv1x1_bwd_wide_simple_kernel, grid, dim3(kWave), 0, static_cast<hipStream_t>(stream), gy, weight, K, C, HW, grouping,
                     from_zero != 0, st, gx);
  return xai_launch_status();
}
