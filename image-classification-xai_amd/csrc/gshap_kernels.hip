// GradientShap (captum 0.7.0 as the reference's harness calls it, evaluatePerturbation.py:164-167): the interpolants in front of
// the classifier pass (K34) and everything behind its backward (K35).  Part of libxai_ext.so (include/xai_hip_ext.h).
#include "xai_common.h"
#include "xai_hip_ext.h"

// the version pair of libxai_ext.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext_version, XAI_EXT_VERSION, XAI_EXT_MINOR)

namespace {

// The baseline of row r.  The draw is the caller's (np.random.choice(n_base, ...)); a value outside [0, n_base) is clamped so
// that no read leaves the baselines whatever the array holds.
__device__ __forceinline__ int64_t base_of(const int64_t* __restrict__ idx, int64_t r, int n_base) {
  const int64_t i = idx[r];
  return i < 0 ? 0 : (i >= n_base ? n_base - 1 : i);
}

// V streamed-once floats (the gradients), past the caches' keep lists: Pack<V>'s flavour of ld4_nt / ld_nt
template <int V>
__device__ __forceinline__ Pack<V> ldp_nt(const float* p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const float4 t = ld4_nt(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = ld_nt(p);
  }
  return r;
}

// ---- K34: out[r] = alpha[r] * xr[r] + (1 - alpha[r]) * baselines[idx[r]] ------------------------------------------------
// A lane owns V consecutive elements of one IMAGE and writes them into the image's n_samples rows: with one input per image
// it is loaded once, and a baseline is loaded again only when a row's index differs from the row before (one baseline, the
// harness's case: once).  The store is plain, the classifier reads `out` next.
// Products and sum round separately (-ffp-contract=off): torch's a * x + (1 - a) * b, not K1's b + a * (x - b).
template <int V>
__global__ __launch_bounds__(256) void gshap_scale_kernel(const float* __restrict__ x, const float* __restrict__ baselines,
                                                          const float* __restrict__ alpha, const int64_t* __restrict__ idx, int n_samples,
                                                          int64_t n_elem, int n_base, int x_per_row, int64_t n_units,
                                                          float* __restrict__ out) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;     // unit = V elements of one image, all its rows
  if (u >= n_units) return;
  const int64_t per_img = n_elem / V;
  const int64_t b = u / per_img;
  const int64_t e = (u - b * per_img) * V;
  Pack<V> xv = {}, bv = {};
  int64_t have = -1;                                                           // the baseline `bv` holds
  for (int s = 0; s < n_samples; ++s) {
    const int64_t r = b * n_samples + s;
    if (x_per_row || s == 0) xv = ldp<V>(x + (x_per_row ? r : b) * n_elem + e);
    const int64_t bi = base_of(idx, r, n_base);
    if (bi != have) {
      bv = ldp<V>(baselines + bi * n_elem + e);
      have = bi;
    }
    const float a = alpha[r];
    const float one_minus_a = 1.0f - a;
    Pack<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float ax = a * xv.v[k];
      const float bb = one_minus_a * bv.v[k];
      o.v[k] = ax + bb;
    }
    stp<V>(out + r * n_elem + e, o);
  }
}

// ---- K35: attr = mean over the samples of (xr - baseline) * grad, map = |sum over channels| ------------------------------
// A lane owns V consecutive pixels of one image for all channels and all samples: one pass over the gradients (non-temporal
// loads, U rows in flight), coalesced per (row, channel) plane; the input is loaded once per channel when there is one per
// image, a baseline again only when the index changes.  The sample sum starts from +0 and runs ascending, the division is a
// true fp32 division, the channel sum runs left to right from the first channel -- the order the header states.
template <int V>
__global__ __launch_bounds__(256) void gshap_finish_kernel(const float* __restrict__ grads, const float* __restrict__ x,
                                                           const float* __restrict__ baselines, const int64_t* __restrict__ idx,
                                                           int n_samples, int C, int64_t HW, int n_base, int x_per_row, int64_t n_units,
                                                           float* __restrict__ attr, float* __restrict__ map) {
  constexpr int U = 2;      // rows in flight per lane; 4 and 8 cost occupancy and time
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;     // unit = V pixels of one image
  if (u >= n_units) return;
  const int64_t per_img = HW / V;
  const int64_t b = u / per_img;
  const int64_t p = (u - b * per_img) * V;
  const int64_t n_elem = static_cast<int64_t>(C) * HW;
  const float denom = static_cast<float>(n_samples);
  Pack<V> m = {};                                                              // overwritten at c == 0
  for (int c = 0; c < C; ++c) {
    const int64_t at = c * HW + p;
    Pack<V> acc = {}, xv = {}, bv = {};                                        // acc: +0
    if (!x_per_row) xv = ldp<V>(x + b * n_elem + at);
    int64_t have = -1;
    for (int s0 = 0; s0 < n_samples; s0 += U) {
      const int n_here = min(U, n_samples - s0);
      Pack<V> g[U];
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (k < n_here) g[k] = ldp_nt<V>(grads + (b * n_samples + s0 + k) * n_elem + at);
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (k < n_here) {
          const int64_t r = b * n_samples + s0 + k;
          if (x_per_row) xv = ldp<V>(x + r * n_elem + at);
          const int64_t bi = base_of(idx, r, n_base);
          if (bi != have) {
            bv = ldp<V>(baselines + bi * n_elem + at);
            have = bi;
          }
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float d = xv.v[j] - bv.v[j];
            const float t = d * g[k].v[j];
            acc.v[j] = acc.v[j] + t;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      acc.v[k] = acc.v[k] / denom;
      m.v[k] = c == 0 ? acc.v[k] : m.v[k] + acc.v[k];
    }
    if (attr != nullptr) stp<V>(attr + b * n_elem + at, acc);
  }
  if (map != nullptr) {
#pragma unroll
    for (int k = 0; k < V; ++k) m.v[k] = fabsf(m.v[k]);
    stp<V>(map + b * HW + p, m);
  }
}

}  // namespace

XAI_EXPORT int xai_gshap_scale_f32(const float* x, const float* baselines, const float* alpha, const int64_t* idx, int n_rows,
                                   int n_samples, int64_t n_elem, int n_base, int x_per_row, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x);
  XAI_REQUIRE_PTR(baselines);
  XAI_REQUIRE_PTR(alpha);
  XAI_REQUIRE_PTR(idx);
  XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n_rows > 0 && n_samples > 0 && n_elem > 0 && n_base > 0, XAI_E_SHAPE);
  XAI_REQUIRE(n_rows % n_samples == 0, XAI_E_SHAPE);
  const bool vec = xai_can_vec4(n_elem, {x, baselines, out});
  const int64_t n_units = static_cast<int64_t>(n_rows / n_samples) * (n_elem / (vec ? 4 : 1));
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(n_units, 256, &blocks), XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(gshap_scale_kernel<V4 ? 4 : 1>, dim3(blocks), dim3(256), 0, st, x, baselines, alpha, idx, n_samples, n_elem,
                       n_base, x_per_row, n_units, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_gshap_finish_f32(const float* grads, const float* x, const float* baselines, const int64_t* idx, int B, int n_samples,
                                    int C, int64_t HW, int n_base, int x_per_row, float* attr, float* map, xai_stream_t stream) {
  XAI_REQUIRE_PTR(grads);
  XAI_REQUIRE_PTR(x);
  XAI_REQUIRE_PTR(baselines);
  XAI_REQUIRE_PTR(idx);
  XAI_REQUIRE(attr != nullptr || map != nullptr, XAI_E_NULL);
  XAI_REQUIRE(B > 0 && n_samples > 0 && C > 0 && HW > 0 && n_base > 0, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(B) * n_samples <= INT32_MAX, XAI_E_UNSUPPORTED);
  const bool vec = xai_can_vec4(HW, {grads, x, baselines, attr, map});
  const int64_t n_units = static_cast<int64_t>(B) * (HW / (vec ? 4 : 1));
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(n_units, 256, &blocks), XAI_E_UNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  xai_dispatch(vec, [&](auto V4) {
    hipLaunchKernelGGL(gshap_finish_kernel<V4 ? 4 : 1>, dim3(blocks), dim3(256), 0, st, grads, x, baselines, idx, n_samples, C, HW,
                       n_base, x_per_row, n_units, attr, map);
  });
  return xai_launch_status();
}
