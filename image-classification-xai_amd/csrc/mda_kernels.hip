// K36-K38: the greedy patch search of MDA (MDAFunctions.py:39-311 find_insertion_patches, :313-597 find_deletion_patches) for
// gfx950.  Part of libxai_ext2.so (include/xai_hip_ext2.h).
//
// One search step of the reference is: pick the first n_cand segments of segment_order that are not in worst_segment_list yet
// (:129-139), build one image per candidate (start with the candidate's pixels taken from finish, :154-162), score them, take the
// argmax / argmin (:177-180), record it (:182-185), commit its pixels into start (:187-188) and, for insertion, test the stop
// (:190-192).  Here the loop state stays on the device and a step is three launches around the classifier pass:
//   K36 compose  out[img][r] = start[img] with the pixels of cand[img][r] taken from finish[img], for every row r < L.  A select,
//                not arithmetic: the bits of either source pass through.  A row whose candidate is a label no pixel carries (K37
//                writes -1 into the rows at and above the step's n_cand) is a plain copy of start, so one launch -- and one
//                captured graph -- of L rows serves the shrinking second phase.  Write-bound like K26: grid (pixel tiles, row
//                chunks, images x channel groups) from xai_row_chunk_plan, a lane keeps its pixels of both sources and their
//                labels in registers and emits one store per (row, channel).
//   K37 select   one workgroup per image: the step's (slot, n_cand, cutoff_slot) from the image's plan table at the step counter
//                in its state words, the first-index argmax / argmin with torch's NaN rule over one wave, the writes of
//                :182-185, the fp32 stop test of :190-191 / :260-261, the taken mark, and the next step's candidate list: the
//                first n_cand_next untaken entries of `order`, found with one block-wide prefix count.  An image that is done or
//                whose plan is exhausted returns before any write.
//   K38 commit   start[img] takes the pixels of the image's last winner (state word 2) from finish[img] (:187-188).  A launch of
//                its own behind K37: the next step's K36 then reads the committed image in every row.
// Capturable: no allocation, no memset, no atomics, no host value that changes between replays -- the step counter, the done
// word and the last winner live in the caller's state words.
#include "xai_common.h"
#include "xai_hip_ext2.h"

#include <math.h>

// the version pair of libxai_ext2.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext2_version, XAI_EXT2_VERSION, XAI_EXT2_MINOR)

namespace {

constexpr int kBlock = 256;
constexpr int kSelectThreads = 256;
constexpr int kSelectWaves = kSelectThreads / kWave;
constexpr int kMaxWidth = kWave;                 // the candidates of a step are reduced by one wave, one per lane
constexpr int kMaxSegments = 16384;              // 64 entries of `order` per lane of K37

// ------------------------------------------------------------------------------------------------ K36
template <int V>
struct Labels {
  int32_t v[V];
};

template <int V>
__device__ __forceinline__ Labels<V> ld_labels(const int32_t* p) {
  Labels<V> r;
  if constexpr (V == 4) {
    const int4 t = *reinterpret_cast<const int4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

// grid = (pixel tiles, row chunks, n_img * zdim): zdim == 1 -> a lane handles all channels, zdim == C -> one channel per lane
template <int V>
__global__ __launch_bounds__(kBlock) void mda_compose_kernel(const float* __restrict__ start, const float* __restrict__ finish,
                                                             const int32_t* __restrict__ seg, const int32_t* __restrict__ cand, int L,
                                                             int C, int64_t hw, int zdim, int per_chunk, float* __restrict__ out) {
  const int64_t p = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (p >= hw) return;
  const int img = blockIdx.z / zdim, zc = blockIdx.z - img * zdim;
  const int k0 = blockIdx.y * per_chunk;
  const int k1 = min(k0 + per_chunk, L);
  const int c_lo = zdim == 1 ? 0 : zc, c_hi = zdim == 1 ? C : zc + 1;
  const int64_t plane = static_cast<int64_t>(C) * hw;
  const Labels<V> lab = ld_labels<V>(seg + static_cast<int64_t>(img) * hw + p);
  const int32_t* cd = cand + static_cast<int64_t>(img) * L;
  for (int c = c_lo; c < c_hi; ++c) {
    const int64_t at = static_cast<int64_t>(img) * plane + c * hw + p;
    const Pack<V> s = ldp<V>(start + at), f = ldp<V>(finish + at);
    float* o = out + (static_cast<int64_t>(img) * L + k0) * plane + c * hw + p;
    for (int k = k0; k < k1; ++k, o += plane) {
      const int32_t want = cd[k];
      Pack<V> r;
#pragma unroll
      for (int i = 0; i < V; ++i) r.v[i] = lab.v[i] == want ? f.v[i] : s.v[i];
      stp<V>(o, r);
    }
  }
}

// ------------------------------------------------------------------------------------------------ K37
// argmin order of torch.min on the CPU: the first NaN if there is one, else the first minimal value.
__device__ __forceinline__ bool argmin_beats(float v, int i, float m, int mi) {
  const bool vn = v != v, mn = m != m;
  if (vn != mn) return vn;
  if (vn) return i < mi;
  return v < m || (v == m && i < mi);
}

// the winner of row[0..n), 1 <= n <= 64, over one wave: lane j holds row[j]; (-+inf, INT32_MAX) loses to every element
template <bool MAX>
__device__ __forceinline__ ArgMax wave_winner(const float* row, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  ArgMax b{MAX ? -INFINITY : INFINITY, INT32_MAX};
  if (lane < n) { b.v = row[lane]; b.i = lane; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(b.v, off, kWave);
    const int oi = __shfl_xor(b.i, off, kWave);
    if (MAX ? argmax_beats(ov, oi, b.v, b.i) : argmin_beats(ov, oi, b.v, b.i)) { b.v = ov; b.i = oi; }
  }
  return b;
}

// state words of an image: 0 = steps taken (the index into its plan), 1 = done (1: the stop test held, 2: a plan row or a
// candidate outside its range -- nothing is written through it), 2 = the last winner's segment (-1: none yet), 3 = plan rows
__global__ __launch_bounds__(kSelectThreads) void mda_select_kernel(const float* __restrict__ resp, const int32_t* __restrict__ order,
                                                                    const int32_t* __restrict__ plan, const float* __restrict__ stop_ref,
                                                                    int S, int L, int plan_stride, int mode, int stop_test, float cutoff,
                                                                    float* __restrict__ mr, int32_t* __restrict__ chosen,
                                                                    int32_t* __restrict__ taken, int32_t* __restrict__ cand,
                                                                    int32_t* __restrict__ state) {
  __shared__ int s_stop;
  __shared__ uint32_t s_wsum[kSelectWaves];
  const int img = blockIdx.x, t = threadIdx.x;
  int32_t* st = state + 4 * static_cast<int64_t>(img);
  const int32_t step = st[0], done = st[1], n_plan = st[3];
  if (done != 0 || step < 0 || step >= n_plan || n_plan > plan_stride) return;       // the whole workgroup: untouched
  const int32_t* pl = plan + (static_cast<int64_t>(img) * plan_stride + step) * 3;
  const int slot = pl[0], n_cand = pl[1], cutoff_slot = pl[2];
  int n_next = step + 1 < n_plan ? pl[4] : 0;
  float* mr_i = mr + static_cast<int64_t>(img) * S;
  int32_t* chosen_i = chosen + static_cast<int64_t>(img) * S;
  int32_t* taken_i = taken + static_cast<int64_t>(img) * S;
  int32_t* cand_i = cand + static_cast<int64_t>(img) * L;
  const int32_t* order_i = order + static_cast<int64_t>(img) * S;
  const bool plan_ok = slot >= 0 && slot < S && n_cand >= 1 && n_cand <= L && n_next >= 0 && n_next <= L;
  __syncthreads();                                       // every lane has read the state words before lane 0 writes them
  if (t < kWave) {
    ArgMax w{0.f, 0};
    if (plan_ok) w = mode == 1 ? wave_winner<true>(resp + static_cast<int64_t>(img) * L, n_cand)
                               : wave_winner<false>(resp + static_cast<int64_t>(img) * L, n_cand);
    if (t == 0) {
      const int32_t s = plan_ok ? cand_i[w.i] : -1;
      if (s < 0 || s >= S) {
        st[1] = 2;
        s_stop = 2;
      } else {
        mr_i[slot] = w.v;                                 // :182-185 / :252-255
        chosen_i[slot] = s;
        taken_i[s] = 1;
        int stop = 0;
        if (mode == 1 && stop_test) {                     // :190-191 / :260-261 in torch's fp32: two roundings, a true division
          const float num = w.v - stop_ref[2 * img];
          const float q = num / stop_ref[2 * img + 1];
          if (q >= cutoff) {
            if (cutoff_slot >= 0 && cutoff_slot < S) mr_i[cutoff_slot] = cutoff;
            stop = 1;
          }
        }
        st[0] = step + 1;
        st[1] = stop;
        st[2] = s;
        s_stop = stop;
      }
    }
  }
  __syncthreads();                                       // the taken mark and s_stop are visible to the workgroup
  if (s_stop == 2) return;
  if (s_stop) n_next = 0;
  // the next step's candidates: the first n_next entries of `order` whose segment is not taken (:129-139)
  const int per = (S + kSelectThreads - 1) / kSelectThreads;
  const int lo = min(t * per, S), hi = min(lo + per, S);
  uint32_t cnt = 0;
  for (int j = lo; j < hi; ++j) {
    const int32_t s = order_i[j];
    cnt += (s >= 0 && s < S && taken_i[s] == 0) ? 1u : 0u;
  }
  // one pass, and nothing writes s_wsum after it: no barrier behind the scan
  uint32_t total = 0;
  uint32_t rank = block_scan_excl<kSelectThreads>(cnt, total, s_wsum);
  for (int j = lo; j < hi && rank < static_cast<uint32_t>(n_next); ++j) {
    const int32_t s = order_i[j];
    if (s >= 0 && s < S && taken_i[s] == 0) cand_i[rank++] = s;
  }
  const int filled = static_cast<int>(min(total, static_cast<uint32_t>(n_next)));
  for (int r = filled + t; r < L; r += kSelectThreads) cand_i[r] = -1;      // rows without a candidate: a label no pixel carries
}

// ------------------------------------------------------------------------------------------------ K38
template <int V>
__global__ __launch_bounds__(kBlock) void mda_commit_kernel(const float* __restrict__ finish, const int32_t* __restrict__ seg,
                                                            const int32_t* __restrict__ state, int C, int64_t hw,
                                                            float* __restrict__ start) {
  const int64_t p = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (p >= hw) return;
  const int img = blockIdx.y;
  const int32_t winner = state[4 * static_cast<int64_t>(img) + 2];
  if (winner < 0) return;
  const Labels<V> lab = ld_labels<V>(seg + static_cast<int64_t>(img) * hw + p);
  bool any = false;
#pragma unroll
  for (int i = 0; i < V; ++i) any = any || lab.v[i] == winner;
  if (!any) return;
  for (int c = 0; c < C; ++c) {
    const int64_t at = (static_cast<int64_t>(img) * C + c) * hw + p;
    const Pack<V> f = ldp<V>(finish + at);
    Pack<V> s = ldp<V>(start + at);
#pragma unroll
    for (int i = 0; i < V; ++i) s.v[i] = lab.v[i] == winner ? f.v[i] : s.v[i];
    stp<V>(start + at, s);
  }
}

}  // namespace

XAI_EXPORT int xai_mda_max_segments(void) { return kMaxSegments; }
XAI_EXPORT int xai_mda_max_width(void) { return kMaxWidth; }

XAI_EXPORT int xai_mda_compose_f32(const float* start, const float* finish, const int32_t* seg, const int32_t* cand, int n_img, int L,
                                   int C, int64_t HW, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(start); XAI_REQUIRE_PTR(finish); XAI_REQUIRE_PTR(seg); XAI_REQUIRE_PTR(cand); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n_img > 0 && L > 0 && C > 0 && HW > 0, XAI_E_SHAPE);
  const bool vec = xai_can_vec4(HW, {start, finish, seg, out});
  // HBM-sized pass (64 MiB): one channel x two rows per lane, as K26
  const XaiRowPlan plan = xai_row_chunk_plan(HW, kBlock, vec, L, C, n_img, int64_t(64) << 20, true);
  XAI_REQUIRE(plan.ok && plan.tiles <= INT32_MAX && static_cast<int64_t>(n_img) * plan.zdim <= 65535, XAI_E_UNSUPPORTED);
  const dim3 grid(static_cast<unsigned>(plan.tiles), static_cast<unsigned>(plan.chunks), static_cast<unsigned>(n_img * plan.zdim));
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(mda_compose_kernel<V4 ? 4 : 1>, grid, dim3(kBlock), 0, st, start, finish, seg, cand, L, C, HW, plan.zdim,
                       plan.per, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_mda_select_f32(const float* resp, const int32_t* order, const int32_t* plan, const float* stop_ref, int n_img, int S,
                                  int L, int plan_stride, int mode, int stop_test, float cutoff, float* mr, int32_t* chosen,
                                  int32_t* taken, int32_t* cand, int32_t* state, xai_stream_t stream) {
  XAI_REQUIRE_PTR(resp); XAI_REQUIRE_PTR(order); XAI_REQUIRE_PTR(plan); XAI_REQUIRE_PTR(mr); XAI_REQUIRE_PTR(chosen);
  XAI_REQUIRE_PTR(taken); XAI_REQUIRE_PTR(cand); XAI_REQUIRE_PTR(state);
  XAI_REQUIRE(mode == 0 || mode == 1, XAI_E_SHAPE);
  XAI_REQUIRE(!(mode == 1 && stop_test) || stop_ref != nullptr, XAI_E_NULL);
  XAI_REQUIRE(n_img > 0 && S > 0 && L > 0 && plan_stride > 0, XAI_E_SHAPE);
  XAI_REQUIRE(S <= kMaxSegments && L <= kMaxWidth, XAI_E_UNSUPPORTED);
  hipLaunchKernelGGL(mda_select_kernel, dim3(static_cast<unsigned>(n_img)), dim3(kSelectThreads), 0, static_cast<hipStream_t>(stream),
                     resp, order, plan, stop_ref, S, L, plan_stride, mode, stop_test != 0 ? 1 : 0, cutoff, mr, chosen, taken, cand, state);
  return xai_launch_status();
}

XAI_EXPORT int xai_mda_commit_f32(const float* finish, const int32_t* seg, const int32_t* state, int n_img, int C, int64_t HW,
                                  float* start, xai_stream_t stream) {
  XAI_REQUIRE_PTR(finish); XAI_REQUIRE_PTR(seg); XAI_REQUIRE_PTR(state); XAI_REQUIRE_PTR(start);
  XAI_REQUIRE(n_img > 0 && C > 0 && HW > 0, XAI_E_SHAPE);
  XAI_REQUIRE(n_img <= 65535, XAI_E_UNSUPPORTED);
  const bool vec = xai_can_vec4(HW, {finish, seg, start});
  const int64_t tiles = xai_ceil_div(HW, int64_t(kBlock) * (vec ? 4 : 1));
  XAI_REQUIRE(tiles <= INT32_MAX, XAI_E_UNSUPPORTED);
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(n_img));
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(mda_commit_kernel<V4 ? 4 : 1>, grid, dim3(kBlock), 0, st, finish, seg, state, C, HW, start);
  });
  return xai_launch_status();
}
