// K56-K57: complete-linkage agglomerative clustering of a precomputed distance matrix as scipy's nearest-neighbour chain computes it
// (scipy/cluster/_hierarchy.pyx `nn_chain`, then linkage's stable sort and `label`), for gfx950.  Part of libxai_ext6.so
// (include/xai_hip_ext6.h, which states the algorithm, the tie rules, the bounds and the cap).
//
// The algorithm is sequential: about 2n-3n row scans and n - 1 Lance-Williams updates, each depending on the one before.  So
//   K56 copy      W[i][j] = W[j][i] = distance[min][max], one lane per element of W, one flag per workgroup for the finite check
//   K56 chain     ONE workgroup walks the chain.  A scan is one pass over row x of W (global memory, L2-resident) and one
//                 lexicographic (value, index) minimum over the workgroup; `size` and the chain live in LDS, the chain's state in
//                 registers, the same in every lane.  An update reads rows x and y and writes row y and column y.
//   K57           one workgroup: a bitonic sort of (height, position) keys, which is the stable sort, then one lane's union-find
// The only operations on distances are compare and select.  Every output word has one owner: no atomics, the same bytes on every run.
#include "xai_common.h"
#include "xai_hip_ext6.h"

#include <limits.h>
#include <math.h>

// the version pair of libxai_ext6.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext6_version, XAI_EXT6_VERSION, XAI_EXT6_MINOR)

namespace {

constexpr int kLkMaxN = XAI_LINKAGE_MAX_N;
constexpr int kLkCopyThreads = 256;
constexpr int kLkSortThreads = 1024;
constexpr int kLkDefaultLanes = 256;
constexpr int kLkBatch = 4;             // row entries a lane loads before it compares the first of them

// The words of `ws` (the header's layout).
struct LkWs {
  float* W;
  int32_t* flags;
  int32_t* merges;
  int copy_blocks_x, nflags;
};

__host__ __device__ inline bool lk_nonfinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u; }

// ------------------------------------------------------------------------------------------------ K56, the working copy
__global__ __launch_bounds__(kLkCopyThreads) void linkage_copy_kernel(const float* __restrict__ distance, int n, float* __restrict__ W,
                                                                      int32_t* __restrict__ flags) {
  const int i = blockIdx.y, j = blockIdx.x * kLkCopyThreads + threadIdx.x;
  int bad = 0;
  if (j < n) {
    float v = 0.f;
    if (i != j) {
      const int a = min(i, j), b = max(i, j);          // only the entry above the diagonal is read
      v = distance[static_cast<int64_t>(a) * n + b];
      bad = lk_nonfinite(v);
    }
    W[static_cast<int64_t>(i) * n + j] = v;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) flags[blockIdx.y * gridDim.x + blockIdx.x] = bad ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ K56, the chain
// (v, i) before (bv, bi) in the scan's order: the smaller value, on equal values the smaller rank
__device__ __forceinline__ bool lk_before(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

// One exchange of the minimum inside a row of 16 lanes as a DPP move instead of a trip through the LDS crossbar.  Every lane keeps
// the lesser of its own pair and its partner's; the order is total, so partners agree.  After lane ^ 1 and lane ^ 2 a quad holds one
// pair, so the mirrored lane of the other quad (then of the other eight) serves as well as the xor partner.
template <int CTRL>
__device__ __forceinline__ void lk_min_dpp(float& bv, int& bi) {
  const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(bv), CTRL, 0xf, 0xf, false));
  const int oi = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xf, 0xf, false);
  const bool take = lk_before(ov, oi, bv, bi);
  bv = take ? ov : bv;
  bi = take ? oi : bi;
}

template <int T>
__global__ __launch_bounds__(T) void linkage_chain_kernel(float* W, const int32_t* __restrict__ flags, int nflags, int n, int32_t* __restrict__ merges,
                                                          int32_t* __restrict__ info) {
  constexpr int WAVES = T / kWave;
  __shared__ int size[kLkMaxN];
  __shared__ int chain[kLkMaxN];
  __shared__ float red_v[2][WAVES];
  __shared__ int red_i[2][WAVES];
  const int t = threadIdx.x;

  int bad = 0;
  for (int f = t; f < nflags; f += T) bad |= flags[f];
  bad = __syncthreads_or(bad);
  if (bad) {
    if (t == 0) {
      info[0] = XAI_LINKAGE_NONFINITE;
      info[1] = info[2] = info[3] = 0;
    }
    return;
  }
  for (int i = t; i < n; i += T) size[i] = 1;
  __syncthreads();

  // the chain's state, the same in every lane: its length, its tip x, the entry below the tip (-1: none), the lowest index that
  // may still be live (a cluster only ever dies, so it never moves back)
  int len = 0, x = -1, below = -1, first = 0;
  int scans = 0, pushes = 0, status = XAI_LINKAGE_OK, k = 0, par = 0;
  for (; k < n - 1 && status == XAI_LINKAGE_OK; ++k) {
    if (len == 0) {
      while (first < n && size[first] == 0) ++first;
      if (first >= n) {
        status = XAI_LINKAGE_BOUND;
        break;
      }
      x = first;
      below = -1;
      if (t == 0) chain[0] = x;
      len = 1;
      ++pushes;
    }
    float cur = INFINITY;
    int y = -1;
    for (;;) {
      // One scan of row x.  The entry below the tip has rank -1, every other live i its index: the least (value, rank) is the first
      // index of the strict minimum unless the entry below the tip has that value too, which is scipy's scan started from W[x][below].
      float bv = INFINITY;
      int bi = INT_MAX;
      const float* row = W + static_cast<int64_t>(x) * n;
      for (int base = t; base < n; base += kLkBatch * T) {
        float v[kLkBatch];
        int live[kLkBatch];
#pragma unroll
        for (int u = 0; u < kLkBatch; ++u) {     // every load of the batch is in flight before the first compare waits for one
          const int i = base + u * T;
          v[u] = i < n ? row[i] : INFINITY;
          live[u] = i < n ? size[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kLkBatch; ++u) {
          const int i = base + u * T;
          const int rank = i == below ? -1 : i;
          if (live[u] > 0 && i != x && lk_before(v[u], rank, bv, bi)) {
            bv = v[u];
            bi = rank;
          }
        }
      }
      lk_min_dpp<0xB1>(bv, bi);        // quad_perm [1, 0, 3, 2]: lane ^ 1
      lk_min_dpp<0x4E>(bv, bi);        // quad_perm [2, 3, 0, 1]: lane ^ 2
      lk_min_dpp<0x141>(bv, bi);       // row_half_mirror: the other quad of the eight
      lk_min_dpp<0x140>(bv, bi);       // row_mirror: the other eight of the row
#pragma unroll
      for (int off = 16; off < kWave; off <<= 1) {
        const float ov = __shfl_xor(bv, off, kWave);
        const int oi = __shfl_xor(bi, off, kWave);
        const bool take = lk_before(ov, oi, bv, bi);
        bv = take ? ov : bv;
        bi = take ? oi : bi;
      }
      if constexpr (WAVES > 1) {
        // two slots in turn: a lane overwrites a slot only after the barrier of the scan in between, which every reader has passed
        if ((t & (kWave - 1)) == 0) {
          red_v[par][t / kWave] = bv;
          red_i[par][t / kWave] = bi;
        }
        __syncthreads();
        bv = red_v[par][0];
        bi = red_i[par][0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
          const float ov = red_v[par][w];
          const int oi = red_i[par][w];
          if (lk_before(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
          }
        }
        par ^= 1;
      }
      ++scans;
      if (bi == INT_MAX) {            // nothing live beside x: cannot happen while two clusters are left
        status = XAI_LINKAGE_BOUND;
        break;
      }
      cur = bv;
      y = bi < 0 ? below : bi;
      if (bi < 0) break;              // mutual nearest neighbours: x and the entry below it
      if (pushes >= 4 * n || len >= n) {
        status = XAI_LINKAGE_BOUND;
        break;
      }
      if (t == 0) chain[len] = y;
      ++len;
      ++pushes;
      below = x;
      x = y;
    }
    if (status != XAI_LINKAGE_OK) break;
    len -= 2;
    const int a = min(x, y), b = max(x, y);     // a is dropped, b becomes the merged cluster
    if (t == 0) {
      merges[3 * k] = a;
      merges[3 * k + 1] = b;
      merges[3 * k + 2] = __float_as_int(cur);
      size[b] += size[a];
      size[a] = 0;
    }
    float* ra = W + static_cast<int64_t>(a) * n;
    float* rb = W + static_cast<int64_t>(b) * n;
    for (int base = t; base < n; base += kLkBatch * T) {
      float va[kLkBatch], vb[kLkBatch];
      int live[kLkBatch];
#pragma unroll
      for (int u = 0; u < kLkBatch; ++u) {
        const int i = base + u * T;
        va[u] = i < n ? ra[i] : 0.f;
        vb[u] = i < n ? rb[i] : 0.f;
        live[u] = i < n ? size[i] : 0;
      }
#pragma unroll
      for (int u = 0; u < kLkBatch; ++u) {
        const int i = base + u * T;
        if (i != a && i != b && live[u] > 0) {  // size[a] and size[b] are not looked at: lane 0 may have changed them already
          const float m = vb[u] > va[u] ? vb[u] : va[u];
          rb[i] = m;
          W[static_cast<int64_t>(i) * n + b] = m;
        }
      }
    }
    __syncthreads();                            // W, size and the chain as every lane left them
    if (len >= 1) {
      x = chain[len - 1];
      below = len >= 2 ? chain[len - 2] : -1;
    }
  }
  if (t == 0) {
    info[0] = status;
    info[1] = scans;
    info[2] = pushes;
    info[3] = k;
  }
}

// ------------------------------------------------------------------------------------------------ K57
__device__ __forceinline__ int lk_find(int* parent, int i, int n) {
  for (int step = 0; step < n; ++step) {        // path halving; a path has fewer than n links
    const int p = parent[i];
    if (p == i) break;
    const int g = parent[p];
    parent[i] = g;
    i = g;
  }
  return i;
}

__global__ __launch_bounds__(kLkSortThreads) void linkage_sort_relabel_kernel(const int32_t* __restrict__ merges, int n, int32_t* __restrict__ children,
                                                                              float* __restrict__ heights, int32_t* info) {
  __shared__ uint64_t keys[kLkMaxN];
  __shared__ uint32_t pairs[kLkMaxN];
  __shared__ int parent[kLkMaxN];
  __shared__ int ident[kLkMaxN];
  const int t = threadIdx.x, m = n - 1;
  const int failed = info[0];
  int P = 1;
  while (P < m) P <<= 1;
  int bad = 0;
  if (failed == XAI_LINKAGE_OK) {
    for (int j = t; j < P; j += kLkSortThreads) {
      uint64_t key = ~uint64_t(0);                       // the padding sorts behind every merge
      if (j < m) {
        const int x = merges[3 * j], y = merges[3 * j + 1];
        bad |= !(0 <= x && x < y && y < n);
        float h = __int_as_float(merges[3 * j + 2]);
        h = h == 0.f ? 0.f : h;                           // -0 and +0 are one height
        uint32_t u = __float_as_uint(h);
        u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;       // finite floats in their order as unsigned integers
        key = (uint64_t(u) << 32) | uint32_t(j);          // the position breaks ties: stable
      }
      keys[j] = key;
    }
  }
  bad = __syncthreads_or(bad);                            // also: every lane has read info[0]
  if (failed != XAI_LINKAGE_OK) return;
  if (bad) {
    if (t == 0) info[0] = XAI_LINKAGE_BOUND;
    return;
  }
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int i = t; i < P; i += kLkSortThreads) {
        const int l = i ^ j2;
        if (l > i) {
          const uint64_t a = keys[i], b = keys[l];
          if ((a > b) == ((i & k2) == 0)) {
            keys[i] = b;
            keys[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int j = t; j < n; j += kLkSortThreads) {
    parent[j] = j;
    ident[j] = j;
    if (j < m) {
      const int o = static_cast<int>(keys[j] & 0xffffffffu);
      heights[j] = __int_as_float(merges[3 * o + 2]);
      pairs[j] = (uint32_t(merges[3 * o]) << 16) | uint32_t(merges[3 * o + 1]);     // both below 2048
    }
  }
  __syncthreads();
  if (t != 0) return;
  for (int k = 0; k < m; ++k) {
    const int rx = lk_find(parent, static_cast<int>(pairs[k] >> 16), n), ry = lk_find(parent, static_cast<int>(pairs[k] & 0xffffu), n);
    if (rx == ry) {                                        // the pair is inside one cluster already: no dendrogram
      info[0] = XAI_LINKAGE_BOUND;
      return;
    }
    const int a = ident[rx], b = ident[ry];
    children[2 * k] = min(a, b);
    children[2 * k + 1] = max(a, b);
    parent[rx] = ry;
    ident[ry] = n + k;
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The checks both entries share, in the header's order -> XAI_OK and the layout, or the refusal.
int lk_check(int n, const void* ws, size_t ws_bytes, LkWs* lay) {
  XAI_REQUIRE(n >= 2, XAI_E_SHAPE);
  XAI_REQUIRE(n <= kLkMaxN, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= xai_linkage_workspace_bytes(n) && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, XAI_E_SHAPE);
  lay->copy_blocks_x = static_cast<int>(xai_ceil_div(n, kLkCopyThreads));
  lay->nflags = n * lay->copy_blocks_x;
  lay->W = static_cast<float*>(const_cast<void*>(ws));
  lay->flags = reinterpret_cast<int32_t*>(lay->W + static_cast<size_t>(n) * n);
  lay->merges = lay->flags + lay->nflags;
  return XAI_OK;
}

}  // namespace

XAI_EXPORT int xai_linkage_max_n(void) { return kLkMaxN; }

XAI_EXPORT size_t xai_linkage_workspace_bytes(int n) {
  if (n < 2 || n > kLkMaxN) return 0;
  const size_t N = static_cast<size_t>(n);
  return (N * N + N * static_cast<size_t>(xai_ceil_div(n, kLkCopyThreads)) + 3 * (N - 1)) * sizeof(int32_t);
}

XAI_EXPORT int xai_linkage_complete_f32(const float* distance, int n, void* ws, size_t ws_bytes, int32_t* info, int lanes,
                                        xai_stream_t stream) {
  XAI_REQUIRE_PTR(distance);
  XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE_PTR(info);
  LkWs lay;
  const int rc = lk_check(n, ws, ws_bytes, &lay);
  if (rc != XAI_OK) return rc;
  if (lanes == 0) lanes = kLkDefaultLanes;
  XAI_REQUIRE(lanes == 64 || lanes == 256 || lanes == 1024, XAI_E_SHAPE);
  hipStream_t s = static_cast<hipStream_t>(stream);
  linkage_copy_kernel<<<dim3(unsigned(lay.copy_blocks_x), unsigned(n)), kLkCopyThreads, 0, s>>>(distance, n, lay.W, lay.flags);
  const int st = xai_launch_status();
  if (st != XAI_OK) return st;
  if (lanes == 64) linkage_chain_kernel<64><<<1, 64, 0, s>>>(lay.W, lay.flags, lay.nflags, n, lay.merges, info);
  else if (lanes == 256) linkage_chain_kernel<256><<<1, 256, 0, s>>>(lay.W, lay.flags, lay.nflags, n, lay.merges, info);
  else linkage_chain_kernel<1024><<<1, 1024, 0, s>>>(lay.W, lay.flags, lay.nflags, n, lay.merges, info);
  return xai_launch_status();
}

XAI_EXPORT int xai_linkage_sort_relabel_i32(int n, const void* ws, size_t ws_bytes, int32_t* children, float* heights, int32_t* info,
                                            xai_stream_t stream) {
  XAI_REQUIRE_PTR(ws);
  XAI_REQUIRE_PTR(children);
  XAI_REQUIRE_PTR(heights);
  XAI_REQUIRE_PTR(info);
  LkWs lay;
  const int rc = lk_check(n, ws, ws_bytes, &lay);
  if (rc != XAI_OK) return rc;
  linkage_sort_relabel_kernel<<<1, kLkSortThreads, 0, static_cast<hipStream_t>(stream)>>>(lay.merges, n, children, heights, info);
  return xai_launch_status();
}
