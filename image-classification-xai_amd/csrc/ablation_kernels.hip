// Perturbation attributions of the captum family (FeatureAblation, Occlusion) for gfx950: the builder of the altered images
// (K26) and the finish that turns the target scores into the attribution and the harness's nearest-exact samples (K27).
//
// The altered images of a call form one flat list, row g = image * n_total + j (j = feature id - id_min, or window index);
// a classifier pass is a run [first, first + n) of that list and may cross from one image into the next.
//
// K26 is write-bound like K6 (perturb_kernels.hip: n * C * hw * 4 B out, the image, ids and baseline read once per lane): a
// lane keeps its 4 pixels, their ids (or coordinates) and baseline values in registers and emits one 16-byte store per
// (row, channel); the grid shape is K6's.  The value stored is captum's float expression x * (1 - m) + baseline * m, not a
// select: -0 becomes +0 next to a baseline >= +0, an infinite x inside the ablated region gives NaN, exactly as there.
#include "xai_common.h"

namespace {

constexpr int kBlock = 256;

// occlusion geometry over (H, W) for windows spanning all channels: window j starts at row (j % ch) * sh, column (j / ch) * sw
// (captum enumerates the shifts with the first non-batch dimension fastest; the channel dimension has one shift)
struct Windows {
  int W, wh, ww, sh, sw, ch, cw;
};

__device__ __forceinline__ bool in_window(const Windows& g, int j, int r, int c) {
  const int r0 = (j % g.ch) * g.sh, c0 = (j / g.ch) * g.sw;          // an overhanging window is clipped by r < H, c < W
  return r >= r0 && r < r0 + g.wh && c >= c0 && c < c0 + g.ww;
}

__device__ __forceinline__ float ablate1(float x, float base, bool hit) {
  const float m = hit ? 1.f : 0.f;
  return x * (1.f - m) + base * m;
}

// grid = (pixel tiles, row chunks, channel groups) as perturb_kernel: gridDim.z == 1 -> a lane handles all channels,
// gridDim.z == C -> one channel per lane
template <int V, bool WIN>
__global__ __launch_bounds__(kBlock) void ablate_kernel(const float* __restrict__ x, const int32_t* __restrict__ ids,
                                                        int64_t id_cstride, int id_min, Windows g, const float* __restrict__ base,
                                                        float base_scalar, int C, int64_t hw, int n_total, int first, int n,
                                                        int per_chunk, float* __restrict__ out) {
  const int64_t p = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (p >= hw) return;
  const int k0 = blockIdx.y * per_chunk;
  const int k1 = min(k0 + per_chunk, n);
  const int64_t img = static_cast<int64_t>(C) * hw;
  const int c_lo = gridDim.z == 1 ? 0 : blockIdx.z, c_hi = gridDim.z == 1 ? C : blockIdx.z + 1;
  int row[V], col[V];
  if constexpr (WIN) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      row[i] = static_cast<int>((p + i) / g.W);
      col[i] = static_cast<int>((p + i) - static_cast<int64_t>(row[i]) * g.W);
    }
  }
  for (int c = c_lo; c < c_hi; ++c) {
    int idv[V];
    float bv[V], xv[V], o4[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      idv[i] = WIN ? 0 : ids[c * id_cstride + p + i] - id_min;
      bv[i] = base ? base[c * hw + p + i] : base_scalar;
    }
    int cur_b = -1;
    float* o = out + k0 * img + c * hw + p;
    for (int k = k0; k < k1; ++k, o += img) {
      const int row_g = first + k, b = row_g / n_total, j = row_g - b * n_total;
      if (b != cur_b) {                          // the next image of the flat list: at most once per image and chunk
        const float* xs = x + b * img + c * hw + p;
        if constexpr (V == 4) {
          const float4 t = ld4(xs);
          xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
        } else {
          xv[0] = xs[0];
        }
        cur_b = b;
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if constexpr (WIN) o4[i] = ablate1(xv[i], bv[i], in_window(g, j, row[i], col[i]));
        else o4[i] = ablate1(xv[i], bv[i], idv[i] == j);
      }
      if constexpr (V == 4) st4(o, make_float4(o4[0], o4[1], o4[2], o4[3]));
      else *o = o4[0];
    }
  }
}

// captum's attribution of one element, gather form.  Every term d * m of its loop with m == 0 is a signed zero, and the running
// sum starts at +0, so those terms never change it: what is left is +0 + d over the covering ids / windows in ascending order.
template <bool WIN>
__device__ __forceinline__ float attr_at(const float* __restrict__ s0, const float* __restrict__ scores, const int32_t* __restrict__ ids,
                                         int64_t id_cstride, int id_min, const Windows& g, int n_total, int b, int c, int r, int col) {
  const float base = s0[b];
  const float* s = scores + static_cast<int64_t>(b) * n_total;
  if constexpr (!WIN) {
    const int j = ids[c * id_cstride + static_cast<int64_t>(r) * g.W + col] - id_min;
    return (j >= 0 && j < n_total) ? 0.f + (base - s[j]) : 0.f;
  } else {
    const int ri_lo = r < g.wh ? 0 : (r - g.wh) / g.sh + 1, ri_hi = min(r / g.sh, g.ch - 1);
    const int ci_lo = col < g.ww ? 0 : (col - g.ww) / g.sw + 1, ci_hi = min(col / g.sw, g.cw - 1);
    float acc = 0.f;
    int cover = 0;
    for (int ci = ci_lo; ci <= ci_hi; ++ci)          // ascending k = ri + ch * ci
      for (int ri = ri_lo; ri <= ri_hi; ++ri, ++cover) acc += base - s[ri + g.ch * ci];
    return acc / static_cast<float>(cover);           // captum's weights: the float count of covering windows (>= 1: stride <= window)
  }
}

// blocks [0, attr_blocks): one element of attr (B, C, H, W) per lane; the blocks behind them: one nearest-exact sample per lane,
// computed from the scores like an attr element (not read back from attr, so the two halves do not depend on each other)
template <bool WIN>
__global__ __launch_bounds__(kBlock) void finish_kernel(const float* __restrict__ s0, const float* __restrict__ scores,
                                                        const int32_t* __restrict__ ids, int64_t id_cstride, int id_min, Windows g,
                                                        int n_total, int B, int C, int H, int gs, float scale_h, float scale_w,
                                                        unsigned attr_blocks, float* __restrict__ attr, float* __restrict__ samples) {
  const int W = g.W;
  if (blockIdx.x < attr_blocks) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t hw = static_cast<int64_t>(H) * W;
    if (e >= static_cast<int64_t>(B) * C * hw) return;
    const int64_t plane = e / hw, p = e - plane * hw;
    const int b = static_cast<int>(plane / C), c = static_cast<int>(plane - static_cast<int64_t>(b) * C);
    const int r = static_cast<int>(p / W);
    attr[e] = attr_at<WIN>(s0, scores, ids, id_cstride, id_min, g, n_total, b, c, r, static_cast<int>(p - static_cast<int64_t>(r) * W));
    return;
  }
  const int64_t e = static_cast<int64_t>(blockIdx.x - attr_blocks) * kBlock + threadIdx.x;
  const int gg = gs * gs;
  if (e >= static_cast<int64_t>(B) * C * gg) return;
  const int plane = static_cast<int>(e / gg), q = static_cast<int>(e - static_cast<int64_t>(plane) * gg);
  const int b = plane / C, c = plane - b * C, i = q / gs, j = q - i * gs;
  // F.interpolate(mode="nearest-exact"): source index floor((i + 0.5) * scale), scale = float(in) / out, clamped to the last one
  const int r = min(static_cast<int>(floorf((i + 0.5f) * scale_h)), H - 1);
  const int col = min(static_cast<int>(floorf((j + 0.5f) * scale_w)), W - 1);
  samples[e] = attr_at<WIN>(s0, scores, ids, id_cstride, id_min, g, n_total, b, c, r, col);
}

// checks shared by the window entries; fills the geometry
int window_geometry(int H, int W, int win_h, int win_w, int stride_h, int stride_w, Windows* g) {
  XAI_REQUIRE(H > 0 && W > 0, XAI_E_SHAPE);
  XAI_REQUIRE(win_h >= 1 && win_h <= H && win_w >= 1 && win_w <= W, XAI_E_SHAPE);          // captum: window <= input
  // captum: stride <= window wherever the window can move at all (with window == dim there is one shift, whatever the stride)
  XAI_REQUIRE(stride_h >= 1 && (stride_h <= win_h || win_h == H) && stride_w >= 1 && (stride_w <= win_w || win_w == W), XAI_E_SHAPE);
  g->W = W; g->wh = win_h; g->ww = win_w; g->sh = stride_h; g->sw = stride_w;
  g->ch = static_cast<int>(xai_ceil_div(H - win_h, stride_h)) + 1;
  g->cw = static_cast<int>(xai_ceil_div(W - win_w, stride_w)) + 1;
  return XAI_OK;
}

template <bool WIN>
int launch_ablate(const float* x, const int32_t* ids, int ids_C, int id_min, const Windows& g, int n_total, const float* baseline,
                  float baseline_scalar, int B, int C, int H, int W, int64_t first, int n, float* out, xai_stream_t stream) {
  XAI_REQUIRE(B > 0 && C > 0 && n_total > 0 && n > 0 && first >= 0, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(B) * n_total <= INT32_MAX, XAI_E_UNSUPPORTED);
  XAI_REQUIRE(first + n <= static_cast<int64_t>(B) * n_total, XAI_E_SHAPE);
  const int64_t hw = static_cast<int64_t>(H) * W;
  const bool vec = xai_can_vec4(hw, {x, out, ids, baseline});
  // HBM-sized pass (64 MiB): one channel x two rows per lane
  const XaiRowPlan plan = xai_row_chunk_plan(hw, kBlock, vec, n, C, 1, int64_t(64) << 20, true);
  XAI_REQUIRE(plan.ok && plan.tiles <= INT32_MAX, XAI_E_UNSUPPORTED);
  const dim3 grid(static_cast<unsigned>(plan.tiles), static_cast<unsigned>(plan.chunks), plan.zdim);
  const int64_t id_cstride = ids_C > 1 ? hw : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL((ablate_kernel<V4 ? 4 : 1, WIN>), grid, dim3(kBlock), 0, st, x, ids, id_cstride, id_min, g, baseline,
                       baseline_scalar, C, hw, n_total, static_cast<int>(first), n, plan.per, out);
  });
  return xai_launch_status();
}

template <bool WIN>
int launch_finish(const float* s0, const float* scores, const int32_t* ids, int ids_C, int id_min, const Windows& g, int n_total,
                  int B, int C, int H, int W, int gs, float* attr, float* samples, xai_stream_t stream) {
  XAI_REQUIRE_PTR(s0); XAI_REQUIRE_PTR(scores);
  XAI_REQUIRE(attr != nullptr || samples != nullptr, XAI_E_NULL);
  XAI_REQUIRE(B > 0 && C > 0 && n_total > 0, XAI_E_SHAPE);
  XAI_REQUIRE(samples == nullptr || (gs >= 1 && gs <= 32768), XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(B) * n_total <= INT32_MAX, XAI_E_UNSUPPORTED);
  const int64_t hw = static_cast<int64_t>(H) * W;
  const int64_t a_blocks = attr ? xai_ceil_div(static_cast<int64_t>(B) * C * hw, kBlock) : 0;
  const int64_t s_blocks = samples ? xai_ceil_div(static_cast<int64_t>(B) * C * gs * gs, kBlock) : 0;
  XAI_REQUIRE(a_blocks + s_blocks <= INT32_MAX, XAI_E_UNSUPPORTED);
  const float scale_h = samples ? static_cast<float>(H) / static_cast<float>(gs) : 0.f;
  const float scale_w = samples ? static_cast<float>(W) / static_cast<float>(gs) : 0.f;
  hipLaunchKernelGGL(finish_kernel<WIN>, dim3(static_cast<unsigned>(a_blocks + s_blocks)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     s0, scores, ids, ids_C > 1 ? hw : int64_t(0), id_min, g, n_total, B, C, H, samples ? gs : 1, scale_h, scale_w,
                     static_cast<unsigned>(a_blocks), attr, samples);
  return xai_launch_status();
}

}  // namespace

XAI_EXPORT int xai_ablate_features_f32(const float* x, const int32_t* ids, int ids_C, int id_min, int n_total, const float* baseline,
                                       float baseline_scalar, int B, int C, int H, int W, int64_t first, int n, float* out,
                                       xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(ids); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(H > 0 && W > 0 && C > 0 && (ids_C == 1 || ids_C == C), XAI_E_SHAPE);
  Windows g{};
  g.W = W;
  return launch_ablate<false>(x, ids, ids_C, id_min, g, n_total, baseline, baseline_scalar, B, C, H, W, first, n, out, stream);
}

XAI_EXPORT int xai_ablate_windows_f32(const float* x, int win_h, int win_w, int stride_h, int stride_w, const float* baseline,
                                      float baseline_scalar, int B, int C, int H, int W, int64_t first, int n, float* out,
                                      xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(out);
  Windows g{};
  const int rc = window_geometry(H, W, win_h, win_w, stride_h, stride_w, &g);
  if (rc != XAI_OK) return rc;
  return launch_ablate<true>(x, nullptr, 1, 0, g, g.ch * g.cw, baseline, baseline_scalar, B, C, H, W, first, n, out, stream);
}

XAI_EXPORT int xai_ablation_finish_features_f32(const float* s0, const float* scores, const int32_t* ids, int ids_C, int id_min,
                                                int n_total, int B, int C, int H, int W, int g, float* attr, float* samples,
                                                xai_stream_t stream) {
  XAI_REQUIRE_PTR(ids);
  XAI_REQUIRE(H > 0 && W > 0 && C > 0 && (ids_C == 1 || ids_C == C), XAI_E_SHAPE);
  Windows geo{};
  geo.W = W;
  return launch_finish<false>(s0, scores, ids, ids_C, id_min, geo, n_total, B, C, H, W, g, attr, samples, stream);
}

XAI_EXPORT int xai_ablation_finish_windows_f32(const float* s0, const float* scores, int win_h, int win_w, int stride_h, int stride_w,
                                               int B, int C, int H, int W, int g, float* attr, float* samples, xai_stream_t stream) {
  Windows geo{};
  const int rc = window_geometry(H, W, win_h, win_w, stride_h, stride_w, &geo);
  if (rc != XAI_OK) return rc;
  return launch_finish<true>(s0, scores, nullptr, 1, 0, geo, geo.ch * geo.cw, B, C, H, W, g, attr, samples, stream);
}
