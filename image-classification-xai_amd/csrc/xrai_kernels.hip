// XRAI (reference util/attribution_methods/XRAIBuilder.py) for gfx950: K29 turns label maps or boolean masks into dilated bit
// planes, K30 runs the greedy region ranking of XRAI._xrai / _xrai_fast on them.
//
// Bit planes: mask m is n_words = ceil(H*W / 64) 64-bit words, pixel p = y*W + x is bit p % 64 of word p / 64, the bits at
// positions >= H*W are zero.  The reference walks every remaining boolean mask over all H*W pixels in every greedy iteration
// (_get_diff_cnt, _gain_density, :266-284); here a candidate costs one popcount per word of its span, and its fp64 sum is taken
// again only when its remainder has changed.
//
// K29 scatters: a source pixel (y, x) of mask m sets, for every dy with |dy| <= r, the run [x - hw(dy), x + hw(dy)] of row y + dy
// clipped to the image (hw(dy) = the largest dx with dx*dx + dy*dy <= r*r: skimage's disk(r)), which is one contiguous bit range
// of the plane.  Integer atomicOr only, so the result does not depend on the order.  A second kernel finds each mask's first and
// last non-empty word.
//
// K30: one workgroup per image runs the whole loop (the K22 shape, gig_kernels.hip); `current` lives in LDS, a wave takes one
// candidate at a time, no workgroup waits for another.  Counts are integers; sums are fp64 in one fixed order (a lane adds its
// words in ascending order, bits ascending inside a word, then the xor butterfly over the 64 lanes), no floating-point atomics:
// two runs give the same bits.
#include "xai_common.h"

namespace {

constexpr int kPackBlock = 256;
constexpr int kMaxRadius = 64;
constexpr int kRankBlock = 1024;
constexpr int kRankWaves = kRankBlock / kWave;
constexpr int kMaxWords = 4096;                      // 32 KiB of LDS for `current`: H*W <= 262144 (512 x 512)

typedef unsigned long long u64;

// bits [lo, hi] (inclusive, flat pixel indices of one row) of plane `dst`
__device__ __forceinline__ void or_run(u64* dst, int64_t lo, int64_t hi) {
  for (int64_t w = lo >> 6; w <= (hi >> 6); ++w) {
    const int b0 = w == (lo >> 6) ? static_cast<int>(lo & 63) : 0;
    const int b1 = w == (hi >> 6) ? static_cast<int>(hi & 63) : 63;
    const u64 m = (b1 == 63 ? ~u64(0) : ((u64(1) << (b1 + 1)) - 1)) & ~((u64(1) << b0) - 1);
    atomicOr(dst + w, m);
  }
}

// grid = (pixel tiles, planes in strides of gridDim.y); a plane is a label map (labels != NULL) or one uint8 mask
__global__ __launch_bounds__(kPackBlock) void pack_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ label_min,
                                                          const int32_t* __restrict__ label_max, const uint8_t* __restrict__ masks,
                                                          int64_t planes, int64_t M, int H, int W, int radius, int64_t n_words,
                                                          u64* __restrict__ bits) {
  __shared__ int half[2 * kMaxRadius + 1];
  for (int t = threadIdx.x; t <= 2 * radius; t += kPackBlock) {
    const int dy = t - radius;
    int dx = 0;
    while ((dx + 1) * (dx + 1) + dy * dy <= radius * radius) ++dx;
    half[t] = dx;
  }
  __syncthreads();
  const int64_t hw = static_cast<int64_t>(H) * W;
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kPackBlock + threadIdx.x;
  if (p >= hw) return;
  const int y = static_cast<int>(p / W), x = static_cast<int>(p - static_cast<int64_t>(y) * W);
  for (int64_t s = blockIdx.y; s < planes; s += gridDim.y) {
    int64_t m;
    if (labels != nullptr) {
      const int l = labels[s * hw + p], lo = label_min[s];
      if (l < lo || l > label_max[s]) continue;                     // outside the stated range: no mask holds it
      m = static_cast<int64_t>(l) - lo;
      for (int64_t q = 0; q < s; ++q) m += static_cast<int64_t>(label_max[q]) - label_min[q] + 1;      // _unpack_segs_to_masks order
      if (m < 0 || m >= M) continue;                              // a stated range that does not fit the M planes
    } else {
      if (masks[s * hw + p] == 0) continue;
      m = s;
    }
    u64* dst = bits + m * n_words;
    for (int dy = -radius; dy <= radius; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;                               // out-of-image neighbours count as false
      const int h = half[dy + radius];
      const int x0 = max(x - h, 0), x1 = min(x + h, W - 1);
      or_run(dst, static_cast<int64_t>(yy) * W + x0, static_cast<int64_t>(yy) * W + x1);
    }
  }
}

// one wave per mask: span[m] = (first, last) non-empty word, (n_words, -1) for an empty mask
__global__ __launch_bounds__(kPackBlock) void span_kernel(const u64* __restrict__ bits, int64_t M, int64_t n_words,
                                                          int32_t* __restrict__ span) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t m = static_cast<int64_t>(blockIdx.x) * (kPackBlock / kWave) + threadIdx.x / kWave;
  if (m >= M) return;
  const u64* b = bits + m * n_words;
  int lo = static_cast<int>(n_words), hi = -1;
  for (int w = lane; w < n_words; w += kWave)
    if (b[w] != 0) {
      lo = min(lo, w);
      hi = max(hi, w);
    }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) {
    span[2 * m] = lo;
    span[2 * m + 1] = hi;
  }
}

// ------------------------------------------------------------------------------------------------ K30

// what a plane may hold in word w: the bits at positions >= H*W never count, whatever the caller's buffer holds there
struct Plane {
  int nw;
  u64 last;                    // the valid bits of word nw - 1
  __device__ __forceinline__ u64 word(const u64* __restrict__ mask, int w) const { return w == nw - 1 ? mask[w] & last : mask[w]; }
};

// popcount of mask & ~current over the words [w0, w1] (one wave; every lane returns the total)
__device__ __forceinline__ int diff_count(const Plane& pl, const u64* __restrict__ mask, const u64* cur, int w0, int w1, int lane) {
  int c = 0;
  for (int w = w0 + lane; w <= w1; w += kWave) c += __popcll(pl.word(mask, w) & ~cur[w]);
  return wave_sum(c);
}

// fp64 sum of attr over mask & ~current, in the fixed order (one wave; every lane returns the total)
__device__ __forceinline__ double diff_sum(const Plane& pl, const u64* __restrict__ mask, const u64* cur, int w0, int w1, int lane,
                                           const float* __restrict__ attr) {
  double s = 0.0;
  for (int w = w0 + lane; w <= w1; w += kWave) {
    u64 d = pl.word(mask, w) & ~cur[w];
    const float* a = attr + static_cast<int64_t>(w) * 64;
    while (d) {
      s += static_cast<double>(a[__ffsll(d) - 1]);
      d &= d - 1;
    }
  }
  return wave_sum(s);
}

struct RankArgs {
  const float* attr;           // [n_img][H*W]
  const u64* bits;             // [M_total][n_words]
  const int32_t* span;         // [M_total][2]
  const int32_t* mask_first;   // [n_img + 1]
  int64_t M_total, hw;
  int n_words, min_pixel_diff, fast;
  double area_threshold;
  float* out;                  // [n_img][H*W]
  int32_t* pixel_iter;         // [n_img][H*W]
  int32_t* sel_key;            // [M_total]
  float* sel_gain;             // [M_total]
  int32_t* state;              // [n_img][4]: selections, uncomputed pixels, status, covered pixels
  int32_t* ws_cnt;             // [M_total]  cached remainder count; -1 = dropped or used, -2 = not yet evaluated
  float* ws_gain;              // [M_total]  cached gain
  int32_t* ws_order;           // [M_total]  fast mode: masks by descending full-mask gain, stable
};

constexpr int kGone = -1, kUnknown = -2;

__global__ __launch_bounds__(kRankBlock) void rank_kernel(RankArgs a) {
  __shared__ u64 cur[kMaxWords];
  __shared__ float w_gain[kRankWaves];
  __shared__ int w_key[kRankWaves], w_cnt[kRankWaves], w_alive[kRankWaves];
  __shared__ double w_sum[kRankWaves];

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int nw = a.n_words;
  const int64_t hw = a.hw;
  const float* attr = a.attr + img * hw;
  float* out = a.out + img * hw;
  int32_t* piter = a.pixel_iter + img * hw;
  // this image's masks, clamped to the table (the offsets are read from device memory)
  int64_t m_lo = a.mask_first[img], m_hi = a.mask_first[img + 1];
  m_lo = m_lo < 0 ? 0 : (m_lo > a.M_total ? a.M_total : m_lo);
  m_hi = m_hi < m_lo ? m_lo : (m_hi > a.M_total ? a.M_total : m_hi);
  const int tail = static_cast<int>(hw & 63);
  const Plane pl{nw, tail ? (u64(1) << tail) - 1 : ~u64(0)};
  const int n_masks = static_cast<int>(m_hi - m_lo);
  const u64* bits = a.bits + m_lo * nw;
  const int32_t* span = a.span + 2 * m_lo;
  int32_t* ws_cnt = a.ws_cnt + m_lo;
  float* ws_gain = a.ws_gain + m_lo;
  int32_t* ws_order = a.ws_order + m_lo;
  int32_t* sel_key = a.sel_key + m_lo;
  float* sel_gain = a.sel_gain + m_lo;

  for (int w = tid; w < nw; w += kRankBlock) cur[w] = 0;
  for (int64_t p = tid; p < hw; p += kRankBlock) piter[p] = -1;
  for (int m = tid; m < n_masks; m += kRankBlock) ws_cnt[m] = kUnknown;
  __syncthreads();

  int n_sel = 0, status = 0;
  int64_t covered = 0;

  // the selected mask's remainder gets the gain, then current |= mask   (XRAIBuilder.py:683-689, :766-769)
  auto apply = [&](int m, float gain) {
    const u64* mk = bits + static_cast<int64_t>(m) * nw;
    const int w0 = max(span[2 * m], 0), w1 = min(span[2 * m + 1], nw - 1);
    for (int w = w0 + tid; w <= w1; w += kRankBlock) {
      const u64 mw = pl.word(mk, w);
      u64 d = mw & ~cur[w];
      while (d) {
        const int64_t p = static_cast<int64_t>(w) * 64 + (__ffsll(d) - 1);
        out[p] = gain;
        piter[p] = n_sel;
        d &= d - 1;
      }
      cur[w] |= mw;
    }
    if (tid == 0) {
      sel_key[n_sel] = m;
      sel_gain[n_sel] = gain;
      ws_cnt[m] = kGone;
    }
  };

  if (!a.fast) {
    // XRAI._xrai (:649-697): while the covered share is <= the threshold (fp64, np.mean of the boolean mask)
    while (static_cast<double>(covered) / static_cast<double>(hw) <= a.area_threshold) {
      float best = -INFINITY;
      int best_m = -1, best_c = 0, alive = 0;
      for (int m = wave; m < n_masks; m += kRankWaves) {             // ascending keys within a wave
        const int cached = ws_cnt[m];
        if (cached == kGone) continue;
        const u64* mk = bits + static_cast<int64_t>(m) * nw;
        const int w0 = max(span[2 * m], 0), w1 = min(span[2 * m + 1], nw - 1);
        const int c = diff_count(pl, mk, cur, w0, w1, lane);
        if (c < a.min_pixel_diff) {                                  // :667-673: dropped for good
          if (lane == 0) ws_cnt[m] = kGone;
          continue;
        }
        ++alive;
        float g;
        if (c != cached) {                                           // the remainder shrank (or first visit): sum again
          g = static_cast<float>(diff_sum(pl, mk, cur, w0, w1, lane, attr) / static_cast<double>(c));
          if (lane == 0) {
            ws_cnt[m] = c;
            ws_gain[m] = g;
          }
        } else {
          g = ws_gain[m];
        }
        if (g > best) {                                              // :675, `>` from -inf: NaN and -inf never win
          best = g;
          best_m = m;
          best_c = c;
        }
      }
      if (lane == 0) {
        w_gain[wave] = best;
        w_key[wave] = best_m;
        w_cnt[wave] = best_c;
        w_alive[wave] = alive;
      }
      __syncthreads();
      best = -INFINITY; best_m = -1; best_c = 0; alive = 0;
      for (int v = 0; v < kRankWaves; ++v) {                         // the first mask with the strictly greatest gain
        alive += w_alive[v];
        const int k = w_key[v];
        if (k >= 0 && (w_gain[v] > best || (w_gain[v] == best && k < best_m))) {
          best = w_gain[v];
          best_m = k;
          best_c = w_cnt[v];
        }
      }
      if (alive == 0) break;                                         // :680
      if (best_m < 0) {                                              // the reference dies here: remaining_masks[None], :682
        status = 1;
        break;
      }
      apply(best_m, best);
      covered += best_c;
      ++n_sel;
      __syncthreads();
    }
  } else {
    // XRAI._xrai_fast (:745-776): full-mask gains once, a stable sort by descending gain, then one sequential pass
    int bad = 0;
    for (int m = wave; m < n_masks; m += kRankWaves) {
      const u64* mk = bits + static_cast<int64_t>(m) * nw;
      const int w0 = max(span[2 * m], 0), w1 = min(span[2 * m + 1], nw - 1);
      const int c = diff_count(pl, mk, cur, w0, w1, lane);               // current is empty: the whole mask
      const float g = c > 0 ? static_cast<float>(diff_sum(pl, mk, cur, w0, w1, lane, attr) / static_cast<double>(c)) : -INFINITY;
      if (g != g) bad = 1;
      if (lane == 0) ws_gain[m] = g;
    }
    if (lane == 0) w_alive[wave] = bad;
    __syncthreads();
    for (int v = 0; v < kRankWaves; ++v) bad |= w_alive[v];
    if (bad) {
      status = 2;                                                    // a NaN key: the order of Python's sort is not defined
    } else {
      for (int m = tid; m < n_masks; m += kRankBlock) {
        const float g = ws_gain[m];
        int r = 0;
        for (int j = 0; j < n_masks; ++j) {
          const float gj = ws_gain[j];
          r += (gj > g || (gj == g && j < m)) ? 1 : 0;
        }
        ws_order[r] = m;
      }
      __syncthreads();
      for (int i = 0; i < n_masks; ++i) {
        const int m = ws_order[i];
        const u64* mk = bits + static_cast<int64_t>(m) * nw;
        const int w0 = max(span[2 * m], 0), w1 = min(span[2 * m + 1], nw - 1);
        if (wave == 0) {
          const int c = diff_count(pl, mk, cur, w0, w1, lane);
          float g = 0.f;
          if (c >= a.min_pixel_diff) g = static_cast<float>(diff_sum(pl, mk, cur, w0, w1, lane, attr) / static_cast<double>(c));
          if (lane == 0) {
            w_cnt[0] = c;
            w_gain[0] = g;
          }
        }
        __syncthreads();
        const int c = w_cnt[0];
        const float g = w_gain[0];
        if (c >= a.min_pixel_diff) {                                 // :761-765: otherwise skipped
          apply(m, g);
          covered += c;
          ++n_sel;
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();

  // :699-701: the uncomputed pixels get the mean of attr over them
  const int64_t n_unc = hw - covered;
  if (n_unc > 0) {
    double s = 0.0;
    for (int w = tid; w < nw; w += kRankBlock) {
      u64 u = pl.word(cur, w) ^ (w == nw - 1 ? pl.last : ~u64(0));
      const float* ap = attr + static_cast<int64_t>(w) * 64;
      while (u) {
        s += static_cast<double>(ap[__ffsll(u) - 1]);
        u &= u - 1;
      }
    }
    s = wave_sum(s);
    if (lane == 0) w_sum[wave] = s;
    __syncthreads();
    double total = 0.0;
    for (int v = 0; v < kRankWaves; ++v) total += w_sum[v];
    const float fill = static_cast<float>(total / static_cast<double>(n_unc));
    for (int w = tid; w < nw; w += kRankBlock) {
      u64 u = pl.word(cur, w) ^ (w == nw - 1 ? pl.last : ~u64(0));
      while (u) {
        out[static_cast<int64_t>(w) * 64 + (__ffsll(u) - 1)] = fill;
        u &= u - 1;
      }
    }
  }
  if (tid == 0) {
    int32_t* st = a.state + 4 * img;
    st[0] = n_sel;
    st[1] = static_cast<int32_t>(n_unc);
    st[2] = status;
    st[3] = static_cast<int32_t>(covered);
  }
}

}  // namespace

XAI_EXPORT size_t xai_xrai_workspace_bytes(int n_img, int H, int W, int64_t M_total) {
  if (n_img < 1 || H < 1 || W < 1 || M_total < 0) return 0;
  return 3 * xai_align_up(static_cast<size_t>(M_total > 0 ? M_total : 1) * 4, 16);       // cached counts, cached gains, the fast order
}

XAI_EXPORT int xai_xrai_pack_u64(const int32_t* labels, const int32_t* label_min, const int32_t* label_max, int S,
                                 const uint8_t* masks, int64_t M, int H, int W, int radius, uint64_t* bits, int32_t* span,
                                 xai_stream_t stream) {
  XAI_REQUIRE_PTR(bits); XAI_REQUIRE_PTR(span);
  XAI_REQUIRE((labels != nullptr) != (masks != nullptr), XAI_E_NULL);           // exactly one of the two inputs
  if (labels != nullptr) {
    XAI_REQUIRE_PTR(label_min); XAI_REQUIRE_PTR(label_max);
    XAI_REQUIRE(S > 0, XAI_E_SHAPE);
  }
  XAI_REQUIRE(H > 0 && W > 0 && M > 0 && radius >= 0, XAI_E_SHAPE);
  XAI_REQUIRE(radius <= kMaxRadius, XAI_E_UNSUPPORTED);
  const int64_t hw = static_cast<int64_t>(H) * W;
  XAI_REQUIRE(hw <= INT32_MAX - 64 && M <= INT32_MAX, XAI_E_UNSUPPORTED);
  const int64_t n_words = xai_ceil_div(hw, 64);
  const int64_t planes = labels != nullptr ? S : M;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(bits, 0, static_cast<size_t>(M) * n_words * 8, st);
  if (e != hipSuccess) return static_cast<int>(e);
  const dim3 grid(static_cast<unsigned>(xai_ceil_div(hw, kPackBlock)), static_cast<unsigned>(std::min<int64_t>(planes, 65535)));
  hipLaunchKernelGGL(pack_kernel, grid, dim3(kPackBlock), 0, st, labels, label_min, label_max, masks, planes, M, H, W, radius, n_words,
                     reinterpret_cast<u64*>(bits));
  int rc = xai_launch_status();
  if (rc != XAI_OK) return rc;
  hipLaunchKernelGGL(span_kernel, dim3(static_cast<unsigned>(xai_ceil_div(M, kPackBlock / kWave))), dim3(kPackBlock), 0, st,
                     reinterpret_cast<const u64*>(bits), M, n_words, span);
  return xai_launch_status();
}

XAI_EXPORT int xai_xrai_rank_f32(const float* attr, const uint64_t* bits, const int32_t* span, const int32_t* mask_first, int n_img,
                                 int64_t M_total, int H, int W, int min_pixel_diff, double area_threshold, int fast, float* out,
                                 int32_t* pixel_iter, int32_t* sel_key, float* sel_gain, int32_t* state, void* workspace,
                                 size_t workspace_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(attr); XAI_REQUIRE_PTR(mask_first); XAI_REQUIRE_PTR(out); XAI_REQUIRE_PTR(pixel_iter); XAI_REQUIRE_PTR(state);
  XAI_REQUIRE_PTR(workspace);
  XAI_REQUIRE(n_img > 0 && H > 0 && W > 0 && M_total >= 0, XAI_E_SHAPE);
  if (M_total > 0) {
    XAI_REQUIRE_PTR(bits); XAI_REQUIRE_PTR(span); XAI_REQUIRE_PTR(sel_key); XAI_REQUIRE_PTR(sel_gain);
  }
  XAI_REQUIRE(area_threshold == area_threshold, XAI_E_SHAPE);                   // NaN
  XAI_REQUIRE(min_pixel_diff >= 1, XAI_E_UNSUPPORTED);                          // the reference loops over empty masks, then crashes
  const int64_t hw = static_cast<int64_t>(H) * W;
  XAI_REQUIRE(hw <= static_cast<int64_t>(kMaxWords) * 64 && M_total <= INT32_MAX && n_img <= 65535 * 32, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(workspace_bytes >= xai_xrai_workspace_bytes(n_img, H, W, M_total) && xai_aligned16(workspace), XAI_E_SHAPE);
  const size_t part = xai_align_up(static_cast<size_t>(M_total > 0 ? M_total : 1) * 4, 16);
  char* ws = static_cast<char*>(workspace);
  RankArgs a;
  a.attr = attr;
  a.bits = reinterpret_cast<const u64*>(bits);
  a.span = span;
  a.mask_first = mask_first;
  a.M_total = M_total;
  a.hw = hw;
  a.n_words = static_cast<int>(xai_ceil_div(hw, 64));
  a.min_pixel_diff = min_pixel_diff;
  a.fast = fast != 0;
  a.area_threshold = area_threshold;
  a.out = out;
  a.pixel_iter = pixel_iter;
  a.sel_key = sel_key;
  a.sel_gain = sel_gain;
  a.state = state;
  a.ws_cnt = reinterpret_cast<int32_t*>(ws);
  a.ws_gain = reinterpret_cast<float*>(ws + part);
  a.ws_order = reinterpret_cast<int32_t*>(ws + 2 * part);
  hipLaunchKernelGGL(rank_kernel, dim3(static_cast<unsigned>(n_img)), dim3(kRankBlock), 0, static_cast<hipStream_t>(stream), a);
  return xai_launch_status();
}
