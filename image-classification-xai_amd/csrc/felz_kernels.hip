// K69-K74: Felzenszwalb-Huttenlocher segmentation as scikit-image 0.18.3 computes it (_felzenszwalb_cy.pyx, with
// scipy.ndimage.gaussian_filter), for gfx950.  libxai_felz.so; include/xai_hip_felz.h states the contract (fp64, every operation
// rounded once, the stable order among equal costs).
//
//   K69 smooth   one lane per sample of one axis: the symmetric correlate1d with reflected indices
//   K70 costs    one lane per edge: the two pixels from the edge's index, the key = the bits of sqrt(sum d * d)
//   K71 count    one wave per chunk of 1024 edges: the lanes of equal digit found by eight ballots, their number added by one of them
//   (scan)       one workgroup per image: the exclusive prefix of the counters in (digit, chunk) order
//   K72 place    the same chunks: offset of the digit + rank among the equal digits before the edge, in the wave's own LDS
//   K73 merge    one wave per (image, scale): 64 edges at a time, roots found by every lane, differing ones kept by a ballot with
//                the rule evaluated on them, committed by lane 0 in ascending order (an edge whose roots an earlier commit of the 64
//                joined is looked at again); then the minimum-size walk; then every pixel's root
//   K74 labels   one workgroup per map: flags, an integer prefix scan, the ranks
// Nothing waits on another workgroup and every loop has a bound fixed at launch.  The only atomics are integer ones whose
// result does not depend on their order (an OR into the status word, an AND that clears K73's touched bits).
#include "xai_common.h"
#include "xai_hip_felz.h"

#include <math.h>

XAI_VERSION_ENTRIES(xai_felz_version, XAI_FELZ_VERSION, XAI_FELZ_MINOR)

namespace {

constexpr int kFelzBlock = 256;
constexpr int kFelzChunk = 1024;                    // K71 / K72: consecutive edges of one wave
constexpr int kFelzDigits = 256;                    // eight bits a pass
constexpr int kFelzScan = 1024;                     // lanes of the one workgroup the scan and K74 give an image / a map
constexpr int kFelzMaxChains = 1 << 20;

__host__ __device__ inline int felz_edges(int H, int W) { return H * (W - 1) + (H - 1) * W + 2 * (H - 1) * (W - 1); }

// ------------------------------------------------------------------------------------------------ K69
__device__ __forceinline__ int felz_reflect(int idx, int n) {
  const int period = 2 * n;
  int m = idx % period;
  if (m < 0) m += period;
  return m >= n ? period - 1 - m : m;
}

__global__ __launch_bounds__(kFelzBlock) void felz_smooth_kernel(const double* __restrict__ src, const double* __restrict__ w, int r, int axis,
                                                                 int64_t total, int H, int W, int C, double* __restrict__ dst) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kFelzBlock + threadIdx.x;
  if (i >= total) return;
  const int wc = W * C;
  const int64_t image = i / (static_cast<int64_t>(H) * wc);
  const int in = static_cast<int>(i - image * H * wc);
  const int y = in / wc, xc = in - y * wc, x = xc / C, c = xc - x * C;
  const int n = axis == 0 ? H : W, l = axis == 0 ? y : x, stride = axis == 0 ? wc : C;
  const double* line = src + image * H * wc + (axis == 0 ? xc : y * wc + c);        // sample j of the line is line[j * stride]
  double t = line[static_cast<int64_t>(l) * stride] * w[r];
  for (int ll = -r; ll < 0; ++ll) {
    const double a = line[static_cast<int64_t>(felz_reflect(l + ll, n)) * stride];
    const double b = line[static_cast<int64_t>(felz_reflect(l - ll, n)) * stride];
    t = t + (a + b) * w[ll + r];
  }
  dst[i] = t;
}

// ------------------------------------------------------------------------------------------------ K70
// the two pixels (flat indices) of edge e; false for an index outside the four families
__device__ __forceinline__ bool felz_edge_pixels(int e, int H, int W, int& pa, int& pb) {
  if (e < 0) return false;
  const int n_right = H * (W - 1), n_down = (H - 1) * W, n_diag = (H - 1) * (W - 1);
  if (e < n_right) {
    const int y = e / (W - 1), x = e - y * (W - 1);
    pa = y * W + x;
    pb = pa + 1;
    return true;
  }
  e -= n_right;
  if (e < n_down) {
    pa = e;
    pb = e + W;
    return true;
  }
  e -= n_down;
  if (e < n_diag) {
    const int y = e / (W - 1), x = e - y * (W - 1);
    pa = y * W + x;
    pb = pa + W + 1;
    return true;
  }
  e -= n_diag;
  if (e < n_diag) {
    const int y = e / (W - 1), x = e - y * (W - 1);
    pa = y * W + x + 1;
    pb = pa + W - 1;
    return true;
  }
  return false;
}

__global__ __launch_bounds__(kFelzBlock) void felz_costs_kernel(const double* __restrict__ image, int H, int W, int C, int E,
                                                                uint64_t* __restrict__ keys, int32_t* __restrict__ index,
                                                                int32_t* __restrict__ status) {
  const int e = blockIdx.x * kFelzBlock + threadIdx.x, b = blockIdx.y;
  if (e >= E) return;
  int pa = 0, pb = 0;
  felz_edge_pixels(e, H, W, pa, pb);
  const double* base = image + static_cast<size_t>(b) * H * W * C;
  const double* qa = base + static_cast<size_t>(pa) * C;
  const double* qb = base + static_cast<size_t>(pb) * C;
  double sum = 0.0;
  for (int c = 0; c < C; ++c) {
    const double d = qb[c] - qa[c];
    sum = sum + d * d;
  }
  const double cost = __dsqrt_rn(sum);
  if (!(cost <= 1.7976931348623157e308)) atomicOr(status, XAI_FELZ_NONFINITE);       // NaN or +inf
  keys[static_cast<size_t>(b) * E + e] = static_cast<uint64_t>(__double_as_longlong(cost));
  index[static_cast<size_t>(b) * E + e] = e;
}

// ------------------------------------------------------------------------------------------------ K71, scan, K72
// the lanes of the wave that hold digit d, among those with `valid`
__device__ __forceinline__ uint64_t felz_same_digit(uint32_t d, bool valid) {
  uint64_t mask = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool set = (d >> bit) & 1u;
    const uint64_t with = __ballot(set);
    mask &= set ? with : ~with;
  }
  return mask;
}

__global__ __launch_bounds__(kFelzBlock) void felz_count_kernel(const uint64_t* __restrict__ keys, int E, int nchunks, int shift,
                                                                uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist_all[kFelzBlock / kWave][kFelzDigits];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, b = blockIdx.y;
  const int chunk = blockIdx.x * (kFelzBlock / kWave) + wave;
  volatile uint32_t* hist = hist_all[wave];           // this wave's alone
  for (int d = lane; d < kFelzDigits; d += kWave) hist[d] = 0u;
  if (chunk >= nchunks) return;
  const uint64_t* k = keys + static_cast<size_t>(b) * E;
  for (int i = 0; i < kFelzChunk; i += kWave) {
    const int e = chunk * kFelzChunk + i + lane;
    const bool valid = e < E;
    const uint32_t d = valid ? static_cast<uint32_t>(k[e] >> shift) & 255u : 0u;
    const uint64_t same = felz_same_digit(d, valid);
    if (valid && (same & ((uint64_t(1) << lane) - 1)) == 0) hist[d] = hist[d] + __popcll(same);      // the first lane of its digit
  }
  uint32_t* out = counts + static_cast<size_t>(b) * kFelzDigits * nchunks;
  for (int d = lane; d < kFelzDigits; d += kWave) out[static_cast<size_t>(d) * nchunks + chunk] = hist[d];
}

__global__ __launch_bounds__(kFelzScan) void felz_scan_kernel(uint32_t* __restrict__ counts, int total) {
  __shared__ uint32_t wsum[kFelzScan / kWave];
  const int t = threadIdx.x;
  uint32_t* c = counts + static_cast<size_t>(blockIdx.x) * total;
  uint32_t run = 0;
  for (int base = 0; base < total; base += kFelzScan) {
    const int i = base + t;
    const uint32_t below = block_scan_excl<kFelzScan>(i < total ? c[i] : 0u, run, wsum);
    if (i < total) c[i] = below;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFelzBlock) void felz_place_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ index, int E,
                                                                int nchunks, int shift, const uint32_t* __restrict__ counts,
                                                                uint64_t* __restrict__ keys_out, int32_t* __restrict__ index_out) {
  __shared__ uint32_t off_all[kFelzBlock / kWave][kFelzDigits];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, b = blockIdx.y;
  const int chunk = blockIdx.x * (kFelzBlock / kWave) + wave;
  if (chunk >= nchunks) return;
  volatile uint32_t* off = off_all[wave];
  const uint32_t* in = counts + static_cast<size_t>(b) * kFelzDigits * nchunks;
  for (int d = lane; d < kFelzDigits; d += kWave) off[d] = in[static_cast<size_t>(d) * nchunks + chunk];
  const size_t image = static_cast<size_t>(b) * E;
  for (int i = 0; i < kFelzChunk; i += kWave) {
    const int e = chunk * kFelzChunk + i + lane;
    const bool valid = e < E;
    const uint64_t key = valid ? keys[image + e] : 0u;
    const uint32_t d = static_cast<uint32_t>(key >> shift) & 255u;
    const uint64_t same = felz_same_digit(d, valid);
    const uint64_t below = same & ((uint64_t(1) << lane) - 1);
    const uint32_t start = valid ? off[d] : 0u;
    const uint32_t pos = start + __popcll(below);
    if (valid && below == 0) off[d] = start + __popcll(same);      // after every lane of the digit has read it: one instruction earlier
    if (valid && pos < static_cast<uint32_t>(E)) {
      keys_out[image + pos] = key;
      index_out[image + pos] = index[image + e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ K73
// The forest: a pixel's parent, never above the pixel, a 16-bit word in LDS (include/xai_hip_felz.h, THE LIMITS).  Lanes read and
// write it side by side while no root changes (every value a lane can meet is an ancestor), so the accesses are volatile: none is
// kept in a register across another lane's store.
struct FelzForest {
  volatile uint16_t* p;
  __device__ __forceinline__ int get(int i) const { return p[i]; }
  __device__ __forceinline__ void set(int i, int v) const { p[i] = static_cast<uint16_t>(v); }
};

// the root of x, or -1 where the forest is not one (a parent above its child or outside it, more than n hops)
__device__ __forceinline__ int felz_find(const FelzForest& f, int x, int n) {
  for (int hop = 0; hop <= n; ++hop) {
    const int q = f.get(x);
    if (q == x) return x;
    if (q < 0 || q > x) return -1;
    x = q;
  }
  return -1;
}

// ... and every pixel passed now points at the root
__device__ __forceinline__ int felz_find_compress(const FelzForest& f, int x, int n) {
  const int root = felz_find(f, x, n);
  if (root < 0) return -1;
  for (int hop = 0; hop <= n && x != root; ++hop) {
    const int q = f.get(x);
    if (q < root || q > x) return -1;
    f.set(x, root);
    x = q;
  }
  return root;
}

// does `cost` pass the rule of the walk for two roots of sizes sa, sc and internal differences ca, cc?
__device__ __forceinline__ bool felz_rule(int walk, double cost, double scale, int min_size, int sa, int sc, double ca, double cc) {
  if (walk != 0) return sa < min_size || sc < min_size;
  const double ia = ca + scale / static_cast<double>(sa);
  const double ic = cc + scale / static_cast<double>(sc);
  return cost < (ia < ic ? ia : ic);
}

__global__ __launch_bounds__(kWave) void felz_merge_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ order,
                                                           const double* __restrict__ scales, int S, int H, int W, int E, int min_size,
                                                           int32_t* __restrict__ roots, int32_t* __restrict__ stats,
                                                           int32_t* __restrict__ status, double* cint_all, int32_t* size_all) {
  extern __shared__ uint32_t felz_lds[];             // the forest, n 16-bit words; then a bit per pixel, `touched`
  __shared__ int s_a[kWave], s_b[kWave], s_sa[kWave], s_sb[kWave];
  __shared__ uint64_t s_key[kWave];
  __shared__ int s_yes[kWave];
  __shared__ int s_fail;
  const int lane = threadIdx.x, chain = blockIdx.x, b = chain / S, n = H * W;
  const double scale = scales[chain - b * S];
  volatile double* cint = cint_all + static_cast<size_t>(chain) * n;
  volatile int32_t* size = size_all + static_cast<size_t>(chain) * n;
  FelzForest f;
  f.p = reinterpret_cast<volatile uint16_t*>(felz_lds);
  // touched: the roots a commit of the current 64 edges joined.  Every other root still has the size and cint its lane read.
  uint32_t* touched = felz_lds + (n + 1) / 2;
  for (int p = lane; p < n; p += kWave) {
    f.set(p, p);
    size[p] = 1;
    cint[p] = 0.0;
  }
  for (int w = lane; w < (n + 31) / 32; w += kWave) touched[w] = 0u;
  if (lane == 0) s_fail = 0;
  __threadfence_block();
  __syncthreads();
  const uint64_t* k = keys + static_cast<size_t>(b) * E;
  const int32_t* ord = order + static_cast<size_t>(b) * E;
  int tested = 0, merged = 0;
  bool failed = false;
  for (int walk = 0; walk < 2 && !failed; ++walk) {                // 0: the thresholds; 1: the minimum size
    if (walk == 1 && min_size <= 1) break;                        // no root is smaller than 1
    for (int base = 0; base < E; base += kWave) {
      const int e = base + lane;
      int ra = 0, rb = 0;
      uint64_t key = 0;
      bool bad = false;
      if (e < E) {
        int pa = 0, pb = 0;
        key = k[e];
        bad = !felz_edge_pixels(ord[e], H, W, pa, pb);
        if (!bad) {
          ra = felz_find_compress(f, pa, n);
          rb = felz_find_compress(f, pb, n);
          bad = ra < 0 || rb < 0;
        }
      }
      if (bad) s_fail = 1;
      const bool keep = e < E && !bad && ra != rb;
      const uint64_t bits = __ballot(keep);
      if (keep) {                                                  // the rule on the roots as they are now: lane 0 takes it where both stay untouched
        const int slot = __popcll(bits & ((uint64_t(1) << lane) - 1));
        const int sa = size[ra], sb = size[rb];
        s_a[slot] = ra;
        s_b[slot] = rb;
        s_sa[slot] = sa;
        s_sb[slot] = sb;
        s_key[slot] = key;
        s_yes[slot] = felz_rule(walk, __longlong_as_double(static_cast<long long>(key)), scale, min_size, sa, sb,
                                walk == 0 ? cint[ra] : 0.0, walk == 0 ? cint[rb] : 0.0);
      }
      __threadfence_block();
      __syncthreads();
      if (lane == 0 && !s_fail) {
        const int kept = __popcll(bits);
        for (int i = 0; i < kept; ++i) {                           // ascending lane = ascending position in the order
          int a = s_a[i], c = s_b[i], sa = s_sa[i], sc = s_sb[i];
          bool yes = s_yes[i] != 0;
          const double cost = __longlong_as_double(static_cast<long long>(s_key[i]));
          if (((touched[a >> 5] >> (a & 31)) | (touched[c >> 5] >> (c & 31))) & 1u) {       // joined since: look again
            const int a0 = a, c0 = c;
            a = felz_find(f, a0, n);
            c = felz_find(f, c0, n);
            if (a < 0 || c < 0) {
              s_fail = 1;
              break;
            }
            if (a == c) continue;
            if (a0 != a) f.set(a0, a);                             // a root of the batch's start: point it at its root
            if (c0 != c) f.set(c0, c);
            sa = size[a];
            sc = size[c];
            yes = felz_rule(walk, cost, scale, min_size, sa, sc, walk == 0 ? cint[a] : 0.0, walk == 0 ? cint[c] : 0.0);
          }
          if (walk == 0) ++tested;
          if (!yes) continue;
          const int lo = a < c ? a : c, hi = a < c ? c : a;
          f.set(hi, lo);
          size[lo] = sa + sc;
          if (walk == 0) {
            ++merged;
            cint[lo] = cost;
          }
          touched[a >> 5] |= 1u << (a & 31);
          touched[c >> 5] |= 1u << (c & 31);
        }
      }
      __threadfence_block();
      __syncthreads();
      if (s_fail) {
        failed = true;
        break;
      }
      // Every root a commit touched is a root some lane staged (a join only joins such roots), so this clears all of `touched`.
      // An integer AND: its result does not depend on the lanes' order.  The next commit is behind the next barrier.
      if (keep) {
        atomicAnd(&touched[ra >> 5], ~(1u << (ra & 31)));
        atomicAnd(&touched[rb >> 5], ~(1u << (rb & 31)));
      }
    }
  }
  if (failed) {
    if (lane == 0) atomicOr(status, XAI_FELZ_INVARIANT);
    for (int p = lane; p < n; p += kWave) roots[static_cast<size_t>(chain) * n + p] = -1;
    return;
  }
  bool bad = false;
  for (int p = lane; p < n; p += kWave) {
    const int r = felz_find(f, p, n);
    bad |= r < 0;
    roots[static_cast<size_t>(chain) * n + p] = r;
  }
  if (bad) atomicOr(status, XAI_FELZ_INVARIANT);
  if (lane == 0) {
    stats[2 * chain] = tested;
    stats[2 * chain + 1] = merged;
  }
}

// ------------------------------------------------------------------------------------------------ K74
__global__ __launch_bounds__(kFelzScan) void felz_labels_kernel(const int32_t* __restrict__ roots, int n, int32_t* __restrict__ labels,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ uint32_t wsum[kFelzScan / kWave];
  const int m = blockIdx.x, t = threadIdx.x;
  const int32_t* rt = roots + static_cast<size_t>(m) * n;
  int32_t* lab = labels + static_cast<size_t>(m) * n;
  uint32_t run = 0;                                  // the roots below this pass
  for (int base = 0; base < n; base += kFelzScan) {
    const int p = base + t;
    const uint32_t flag = (p < n && rt[p] == p) ? 1u : 0u;
    const uint32_t below = block_scan_excl<kFelzScan>(flag, run, wsum);
    if (flag) lab[p] = static_cast<int32_t>(below);
    __syncthreads();
  }
  if (t == 0) counts[m] = static_cast<int32_t>(run);
  __threadfence_block();
  __syncthreads();
  bool bad = false;
  for (int p = t; p < n; p += kFelzScan) {
    const int r = rt[p];
    if (r == p) continue;                            // a root has its rank already, and no other lane writes it
    if (r < 0 || r >= n || rt[r] != r) {
      lab[p] = -1;
      bad = true;
    } else {
      lab[p] = lab[r];
    }
  }
  if (bad) atomicOr(status, XAI_FELZ_INVARIANT);
}

// ------------------------------------------------------------------------------------------------ host side
int felz_check(int B, int H, int W) {
  XAI_REQUIRE(B >= 1 && H >= 1 && W >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && static_cast<int64_t>(H) * W <= XAI_FELZ_MAX_PIXELS, XAI_E_UNSUPPORTED);
  return XAI_OK;
}

int felz_chunks(int E) { return static_cast<int>(xai_ceil_div(E, kFelzChunk)); }

size_t felz_sort_bytes(int B, int E) {
  return xai_align_up(static_cast<size_t>(B) * E * 8, 8) + xai_align_up(static_cast<size_t>(B) * E * 4, 8) +
         static_cast<size_t>(B) * kFelzDigits * felz_chunks(E) * 4;
}

size_t felz_merge_bytes(int B, int S, int n) { return static_cast<size_t>(B) * S * n * 12; }

}  // namespace

XAI_EXPORT int xai_felz_max_pixels(void) { return XAI_FELZ_MAX_PIXELS; }
XAI_EXPORT int xai_felz_max_channels(void) { return XAI_FELZ_MAX_CHANNELS; }
XAI_EXPORT int xai_felz_max_scales(void) { return XAI_FELZ_MAX_SCALES; }
XAI_EXPORT int xai_felz_max_radius(void) { return XAI_FELZ_MAX_RADIUS; }

XAI_EXPORT int xai_felz_edges(int H, int W) {
  if (felz_check(1, H, W) != XAI_OK) return 0;
  return felz_edges(H, W);
}

XAI_EXPORT size_t xai_felz_workspace_bytes(int B, int H, int W, int S) {
  if (felz_check(B, H, W) != XAI_OK || S < 1 || S > XAI_FELZ_MAX_SCALES || static_cast<int64_t>(B) * S > kFelzMaxChains) return 0;
  const size_t sort = felz_sort_bytes(B, felz_edges(H, W)), merge = felz_merge_bytes(B, S, H * W);
  return sort > merge ? sort : merge;
}

XAI_EXPORT int xai_felz_clear_i32(int32_t* status, int n, xai_stream_t stream) {
  XAI_REQUIRE_PTR(status);
  XAI_REQUIRE(n >= 1, XAI_E_SHAPE);
  return xai_clear_i32(status, n, static_cast<hipStream_t>(stream));
}

XAI_EXPORT int xai_felz_smooth_f64(const double* src, const double* weights, int radius, int axis, int B, int H, int W, int C, double* dst,
                                   xai_stream_t stream) {
  XAI_REQUIRE_PTR(src);
  XAI_REQUIRE_PTR(weights);
  XAI_REQUIRE_PTR(dst);
  const int rc = felz_check(B, H, W);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(C >= 1 && radius >= 0 && (axis == 0 || axis == 1) && src != dst, XAI_E_SHAPE);
  XAI_REQUIRE(C <= XAI_FELZ_MAX_CHANNELS && radius <= XAI_FELZ_MAX_RADIUS, XAI_E_UNSUPPORTED);
  const int64_t total = static_cast<int64_t>(B) * H * W * C;
  unsigned blocks = 0;
  XAI_REQUIRE(xai_blocks_checked(total, kFelzBlock, &blocks), XAI_E_UNSUPPORTED);
  felz_smooth_kernel<<<blocks, kFelzBlock, 0, static_cast<hipStream_t>(stream)>>>(src, weights, radius, axis, total, H, W, C, dst);
  return xai_launch_status();
}

XAI_EXPORT int xai_felz_costs_u64(const double* image, int B, int H, int W, int C, uint64_t* keys, int32_t* index, int32_t* status,
                                  xai_stream_t stream) {
  XAI_REQUIRE_PTR(image);
  XAI_REQUIRE_PTR(keys);
  XAI_REQUIRE_PTR(index);
  XAI_REQUIRE_PTR(status);
  const int rc = felz_check(B, H, W);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(C >= 1, XAI_E_SHAPE);
  XAI_REQUIRE(C <= XAI_FELZ_MAX_CHANNELS, XAI_E_UNSUPPORTED);
  const int E = felz_edges(H, W);
  if (E == 0) return XAI_OK;
  const dim3 grid(unsigned(xai_ceil_div(E, kFelzBlock)), unsigned(B));
  felz_costs_kernel<<<grid, kFelzBlock, 0, static_cast<hipStream_t>(stream)>>>(image, H, W, C, E, keys, index, status);
  return xai_launch_status();
}

XAI_EXPORT int xai_felz_sort_u64(uint64_t* keys, int32_t* index, int B, int H, int W, int S, void* ws, size_t ws_bytes,
                                 xai_stream_t stream) {
  XAI_REQUIRE_PTR(keys);
  XAI_REQUIRE_PTR(index);
  XAI_REQUIRE_PTR(ws);
  const int rc = felz_check(B, H, W);
  if (rc != XAI_OK) return rc;
  const size_t need = xai_felz_workspace_bytes(B, H, W, S);
  XAI_REQUIRE(need != 0, S < 1 ? XAI_E_SHAPE : XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, XAI_E_SHAPE);
  const int E = felz_edges(H, W);
  if (E == 0) return XAI_OK;
  const int nchunks = felz_chunks(E);
  char* w = static_cast<char*>(ws);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(w);
  int32_t* index_b = reinterpret_cast<int32_t*>(w + xai_align_up(static_cast<size_t>(B) * E * 8, 8));
  uint32_t* counts = reinterpret_cast<uint32_t*>(w + xai_align_up(static_cast<size_t>(B) * E * 8, 8) + xai_align_up(static_cast<size_t>(B) * E * 4, 8));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(xai_ceil_div(nchunks, kFelzBlock / kWave)), unsigned(B));
  uint64_t* kin = keys;
  int32_t* iin = index;
  uint64_t* kout = keys_b;
  int32_t* iout = index_b;
  for (int pass = 0; pass < 8; ++pass) {                           // an even number: the sorted pairs end in keys / index
    felz_count_kernel<<<grid, kFelzBlock, 0, s>>>(kin, E, nchunks, 8 * pass, counts);
    felz_scan_kernel<<<unsigned(B), kFelzScan, 0, s>>>(counts, kFelzDigits * nchunks);
    felz_place_kernel<<<grid, kFelzBlock, 0, s>>>(kin, iin, E, nchunks, 8 * pass, counts, kout, iout);
    const int st = xai_launch_status();
    if (st != XAI_OK) return st;
    uint64_t* const tk = kin;
    kin = kout;
    kout = tk;
    int32_t* const ti = iin;
    iin = iout;
    iout = ti;
  }
  return XAI_OK;
}

XAI_EXPORT int xai_felz_merge_f64(const uint64_t* keys, const int32_t* order, const double* scales, int B, int S, int H, int W, int min_size,
                                  int32_t* roots, int32_t* stats, int32_t* status, void* ws, size_t ws_bytes,
                                  xai_stream_t stream) {
  XAI_REQUIRE_PTR(keys);
  XAI_REQUIRE_PTR(order);
  XAI_REQUIRE_PTR(scales);
  XAI_REQUIRE_PTR(roots);
  XAI_REQUIRE_PTR(stats);
  XAI_REQUIRE_PTR(status);
  XAI_REQUIRE_PTR(ws);
  const int rc = felz_check(B, H, W);
  if (rc != XAI_OK) return rc;
  XAI_REQUIRE(S >= 1 && min_size >= 0, XAI_E_SHAPE);
  const size_t need = xai_felz_workspace_bytes(B, H, W, S);
  XAI_REQUIRE(need != 0, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, XAI_E_SHAPE);
  const int n = H * W, E = felz_edges(H, W);
  const size_t cells = static_cast<size_t>(B) * S * n;
  double* cint = static_cast<double*>(ws);
  int32_t* size = reinterpret_cast<int32_t*>(cint + cells);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned chains = unsigned(B) * unsigned(S);
  const size_t lds = (static_cast<size_t>(n + 1) / 2 + static_cast<size_t>(n + 31) / 32) * sizeof(uint32_t);      // forest, touched
  if (lds > 48 * 1024) {                                           // over the default cap of a launch's dynamic LDS
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&felz_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    if (e != hipSuccess) return static_cast<int>(e);
  }
  felz_merge_kernel<<<chains, kWave, lds, s>>>(keys, order, scales, S, H, W, E, min_size, roots, stats, status, cint, size);
  return xai_launch_status();
}

XAI_EXPORT int xai_felz_labels_i32(const int32_t* roots, int M, int n, int32_t* labels, int32_t* counts, int32_t* status,
                                   xai_stream_t stream) {
  XAI_REQUIRE_PTR(roots);
  XAI_REQUIRE_PTR(labels);
  XAI_REQUIRE_PTR(counts);
  XAI_REQUIRE_PTR(status);
  XAI_REQUIRE(M >= 1 && n >= 1 && labels != roots, XAI_E_SHAPE);
  XAI_REQUIRE(n <= XAI_FELZ_MAX_PIXELS && M <= kFelzMaxChains, XAI_E_UNSUPPORTED);
  felz_labels_kernel<<<unsigned(M), kFelzScan, 0, static_cast<hipStream_t>(stream)>>>(roots, n, labels, counts, status);
  return xai_launch_status();
}
