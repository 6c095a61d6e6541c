// K46-K52: the element-wise steps of the relevance pass of Transformer Attribution (the reference's LRP.generate_LRP with alpha = 1:
// util/attribution_methods/VIT_LRP/util/layers_ours.py and ViT_LRP_timm.py) for gfx950.  Part of libxai_ext4.so
// (include/xai_hip_ext4.h, which states every expression and every summation tree).
//
// The reference builds each relprop from a dozen small torch kernels and a torch.autograd.grad call; at ViT-B/16 no tensor on that
// path is larger than 2.4 MB, so the pass is a few hundred launches of microseconds each.  Here the GEMMs stay with rocBLAS and what
// lies between two GEMMs is one launch:
//   K46 split         x -> (clamp(x, min=0), clamp(x, max=0))
//   K47 ratio         safe_divide(r, z1 [+ z2])
//   K48 gather        clamp(x, min=0) * g1 + clamp(x, max=0) * g2
//   K49 half product  x * c / 2, plain or into one third of cam_qkv
//   K50 add           Add.relprop: products and per-chunk fp64 partial sums, then the scalar arithmetic and the rescale
//   K51 clone         x * (safe_divide(r1, x) + safe_divide(r2, x))
//   K52 matrices      head mean of clamp(grad * cam, min=0) of all blocks, optionally + I and row-normalised, or the CLS row only
// Every output element has one owner: no atomics, nothing to zero beforehand, the same bytes on every run.  Capturable: nothing is
// allocated.
#include "xai_common.h"
#include "xai_hip_ext4.h"

#include <math.h>

// the version pair of libxai_ext4.so; its error texts stay with xai_strerror in libxai_hip.so
XAI_VERSION_ENTRIES(xai_ext4_version, XAI_EXT4_VERSION, XAI_EXT4_MINOR)

namespace {

constexpr int kLrpThreads = 256;
constexpr int kLrpWaves = kLrpThreads / kWave;

// torch's clamp: a NaN stays, else fmaxf / fminf
__device__ __forceinline__ float cmin(float x, float c) { return x != x ? x : fmaxf(x, c); }
__device__ __forceinline__ float cmax(float x, float c) { return x != x ? x : fminf(x, c); }

// safe_divide (layers_ours.py:10-13), operation for operation
__device__ __forceinline__ float sd(float a, float b) {
  float den = cmin(b, 1e-9f) + cmax(b, 1e-9f);
  den = den + (den == 0.f ? 1.f : 0.f) * 1e-9f;
  return a / den * (b != 0.f ? 1.f : 0.f);
}

// ------------------------------------------------------------------------------------------------ K46, K47, K48, K51
// one lane per V consecutive floats of a flat array of `total` floats (total % V == 0)
template <int V>
__global__ __launch_bounds__(kLrpThreads) void split_kernel(const float* __restrict__ x, int64_t total, float* __restrict__ pos,
                                                           float* __restrict__ neg) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kLrpThreads + threadIdx.x) * V;
  if (i >= total) return;
  const Pack<V> v = ldp<V>(x + i);
  Pack<V> p, q;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    p.v[k] = cmin(v.v[k], 0.f);
    q.v[k] = cmax(v.v[k], 0.f);
  }
  stp<V>(pos + i, p);
  stp<V>(neg + i, q);
}

// s may alias an input: a lane reads exactly the elements it writes, before it writes them (no __restrict__ on these)
template <int V, bool TWO>
__global__ __launch_bounds__(kLrpThreads) void ratio_kernel(const float* r, const float* z1, const float* z2, int64_t total, float* s) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kLrpThreads + threadIdx.x) * V;
  if (i >= total) return;
  const Pack<V> a = ldp<V>(r + i), b = ldp<V>(z1 + i);
  Pack<V> c, o;
  if constexpr (TWO) c = ldp<V>(z2 + i);
#pragma unroll
  for (int k = 0; k < V; ++k) o.v[k] = sd(a.v[k], TWO ? b.v[k] + c.v[k] : b.v[k]);
  stp<V>(s + i, o);
}

template <int V>
__global__ __launch_bounds__(kLrpThreads) void gather_kernel(const float* x, const float* g1, const float* g2, int64_t total, float* out) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kLrpThreads + threadIdx.x) * V;
  if (i >= total) return;
  const Pack<V> v = ldp<V>(x + i), a = ldp<V>(g1 + i), b = ldp<V>(g2 + i);
  Pack<V> o;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float c1 = cmin(v.v[k], 0.f) * a.v[k];
    const float c2 = cmax(v.v[k], 0.f) * b.v[k];
    o.v[k] = c1 + c2;
  }
  stp<V>(out + i, o);
}

template <int V>
__global__ __launch_bounds__(kLrpThreads) void clone_kernel(const float* x, const float* r1, const float* r2, int64_t total, float* out) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kLrpThreads + threadIdx.x) * V;
  if (i >= total) return;
  const Pack<V> v = ldp<V>(x + i), a = ldp<V>(r1 + i), b = ldp<V>(r2 + i);
  Pack<V> o;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float s = sd(a.v[k], v.v[k]) + sd(b.v[k], v.v[k]);
    o.v[k] = v.v[k] * s;
  }
  stp<V>(out + i, o);
}

// ------------------------------------------------------------------------------------------------ K49
// one lane per V consecutive floats of x [B][h][N][d] (d % V == 0, so the V floats share b, hh and t); slots == 1 writes in place,
// slots == 3 writes to out[b][t][slot][hh][e .. e + V)
template <int V>
__global__ __launch_bounds__(kLrpThreads) void half_product_kernel(const float* __restrict__ x, const float* __restrict__ c, int64_t total,
                                                                  int h, int N, int d, int slots, int slot, float* __restrict__ out) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kLrpThreads + threadIdx.x) * V;
  if (i >= total) return;
  const Pack<V> a = ldp<V>(x + i), g = ldp<V>(c + i);
  Pack<V> o;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float p = a.v[k] * g.v[k];
    o.v[k] = p / 2.f;
  }
  int64_t dst = i;
  if (slots != 1) {
    const int e = static_cast<int>(i % d);
    const int64_t row = i / d;                       // (b * h + hh) * N + t
    const int t = static_cast<int>(row % N);
    const int64_t bh = row / N;
    const int hh = static_cast<int>(bh % h);
    const int64_t b = bh / h;
    dst = (((b * N + t) * slots + slot) * h + hh) * static_cast<int64_t>(d) + e;
  }
  stp<V>(out + dst, o);
}

// ------------------------------------------------------------------------------------------------ K50
constexpr int kAddChunk = 4096;                      // elements of one image one workgroup sums: 256 lanes x 4 quads of 4
constexpr int kAddQuads = kAddChunk / (kLrpThreads * 4);

// grid (P, B).  Lane t owns the quads q * 256 + t of its chunk, q = 0..3: the elements i of the chunk with (i / 4) % 256 == t, visited
// in ascending i -- the same elements in the same order for both widths.
template <bool VEC>
__global__ __launch_bounds__(kLrpThreads) void add_parts_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                               const float* __restrict__ r, int64_t n, float* __restrict__ a,
                                                               float* __restrict__ b, double* __restrict__ part) {
  __shared__ double red[kLrpWaves];
  const int64_t img = static_cast<int64_t>(blockIdx.y) * n;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kAddChunk;
  double sa = 0.0, sb = 0.0, sr = 0.0;
#pragma unroll
  for (int q = 0; q < kAddQuads; ++q) {
    const int64_t i = base + (static_cast<int64_t>(q) * kLrpThreads + threadIdx.x) * 4;
    if (i >= n) break;
    if constexpr (VEC) {
      const Pack<4> u = ldp<4>(x0 + img + i), v = ldp<4>(x1 + img + i), w = ldp<4>(r + img + i);
      Pack<4> oa, ob;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float s = sd(w.v[k], u.v[k] + v.v[k]);
        oa.v[k] = u.v[k] * s;
        ob.v[k] = v.v[k] * s;
        sa += static_cast<double>(oa.v[k]);
        sb += static_cast<double>(ob.v[k]);
        sr += static_cast<double>(w.v[k]);
      }
      stp<4>(a + img + i, oa);
      stp<4>(b + img + i, ob);
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) {
        const float u = x0[img + i + k], v = x1[img + i + k], w = r[img + i + k];
        const float s = sd(w, u + v);
        const float oa = u * s, ob = v * s;
        a[img + i + k] = oa;
        b[img + i + k] = ob;
        sa += static_cast<double>(oa);
        sb += static_cast<double>(ob);
        sr += static_cast<double>(w);
      }
    }
  }
  sa = block_sum<kLrpWaves>(sa, red);
  sb = block_sum<kLrpWaves>(sb, red);
  sr = block_sum<kLrpWaves>(sr, red);
  if (threadIdx.x == 0) {
    double* p = part + (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x) * 3;
    p[0] = sa; p[1] = sb; p[2] = sr;
  }
}

// grid (P, B): every workgroup folds its image's P parts in the same order (thread 0, broadcast through LDS) and scales its chunk
template <bool VEC>
__global__ __launch_bounds__(kLrpThreads) void add_scale_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n,
                                                               const double* __restrict__ part) {
  __shared__ float fac[2];
  if (threadIdx.x == 0) {
    const double* p = part + static_cast<int64_t>(blockIdx.y) * gridDim.x * 3;
    double A = 0.0, Bs = 0.0, R = 0.0;
    for (unsigned c = 0; c < gridDim.x; ++c) {
      A += p[3 * c];
      Bs += p[3 * c + 1];
      R += p[3 * c + 2];
    }
    const float a_sum = static_cast<float>(A), b_sum = static_cast<float>(Bs), r_sum = static_cast<float>(R);
    const float den = fabsf(a_sum) + fabsf(b_sum);
    const float a_fact = sd(fabsf(a_sum), den) * r_sum;
    const float b_fact = sd(fabsf(b_sum), den) * r_sum;
    fac[0] = sd(a_fact, a_sum);
    fac[1] = sd(b_fact, b_sum);
  }
  __syncthreads();
  const float fa = fac[0], fb = fac[1];
  const int64_t img = static_cast<int64_t>(blockIdx.y) * n;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kAddChunk;
#pragma unroll
  for (int q = 0; q < kAddQuads; ++q) {
    const int64_t i = base + (static_cast<int64_t>(q) * kLrpThreads + threadIdx.x) * 4;
    if (i >= n) break;
    if constexpr (VEC) {
      Pack<4> u = ldp<4>(a + img + i), v = ldp<4>(b + img + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        u.v[k] = u.v[k] * fa;
        v.v[k] = v.v[k] * fb;
      }
      stp<4>(a + img + i, u);
      stp<4>(b + img + i, v);
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) {
        a[img + i + k] = a[img + i + k] * fa;
        b[img + i + k] = b[img + i + k] * fb;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ K52
// grid (ceil(rows / 4), L, B), 4 waves: wave w owns row blockIdx.x * 4 + w of block l = blockIdx.y, image b = blockIdx.z
// (rows = S, mode 2: 1).  A lane holds its columns j = lane, lane + 64, ... one at a time; mode 1 visits them twice (the sum, then
// the quotients) and recomputes m, which costs less than keeping S / 64 values per lane for any S.
template <bool GRAD>
__device__ __forceinline__ float head_mean(const float* __restrict__ cam, const float* __restrict__ grad, int h, int64_t plane, int64_t at) {
  float s = 0.f;
  for (int hh = 0; hh < h; ++hh) {
    const float c = cam[hh * plane + at];
    float t = c;
    if constexpr (GRAD) t = grad[hh * plane + at] * c;
    s += cmin(t, 0.f);
  }
  return s / static_cast<float>(h);
}

template <bool GRAD>
__global__ __launch_bounds__(kLrpThreads) void attn_matrices_kernel(const float* __restrict__ cam, const float* __restrict__ grad, int B,
                                                                   int h, int S, int mode, float* __restrict__ out) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int i = blockIdx.x * kLrpWaves + wave;
  const int rows = mode == 2 ? 1 : S;
  if (i >= rows) return;                             // whole waves leave; no barrier follows
  const int l = blockIdx.y, b = blockIdx.z, L = gridDim.y;
  const int64_t plane = static_cast<int64_t>(S) * S;
  const int64_t in0 = (static_cast<int64_t>(l) * B + b) * h * plane + static_cast<int64_t>(i) * S;
  const float* c0 = cam + in0;
  const float* g0 = GRAD ? grad + in0 : nullptr;
  float* o = mode == 2 ? out + (static_cast<int64_t>(b) * L + l) * S : out + (static_cast<int64_t>(b) * L + l) * plane + static_cast<int64_t>(i) * S;
  if (mode != 1) {
    for (int j = lane; j < S; j += kWave) o[j] = head_mean<GRAD>(c0, g0, h, plane, j);
    return;
  }
  float sum = 0.f;
  for (int j = lane; j < S; j += kWave) {
    const float m = head_mean<GRAD>(c0, g0, h, plane, j) + (i == j ? 1.f : 0.f);
    sum += m;
  }
  sum = wave_sum(sum);
  for (int j = lane; j < S; j += kWave) {
    const float m = head_mean<GRAD>(c0, g0, h, plane, j) + (i == j ? 1.f : 0.f);
    o[j] = m / sum;
  }
}

// the checks every flat entry shares -> the element count, or a negative code
inline int64_t flat_total(int B, int64_t n) {
  if (B <= 0 || n <= 0) return XAI_E_SHAPE;
  if (n > INT64_MAX / B) return XAI_E_UNSUPPORTED;
  return static_cast<int64_t>(B) * n;
}

inline int64_t add_chunks(int64_t n) { return xai_ceil_div(n, kAddChunk); }

// B, n of a K50 call -> 0 or a negative code
inline int add_shape(int B, int64_t n) {
  XAI_REQUIRE(B > 0 && n > 0, XAI_E_SHAPE);
  XAI_REQUIRE(B <= 65535 && n <= INT32_MAX - kAddChunk, XAI_E_UNSUPPORTED);
  return XAI_OK;
}

}  // namespace

XAI_EXPORT int xai_lrp_split_f32(const float* x, int B, int64_t n, float* pos, float* neg, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(pos); XAI_REQUIRE_PTR(neg);
  const int64_t total = flat_total(B, n);
  XAI_REQUIRE(total > 0, static_cast<int>(total));
  const bool vec = xai_can_vec4(total, {x, pos, neg});
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(total / (vec ? 4 : 1), kLrpThreads, &blocks), XAI_E_UNSUPPORTED);
  xai_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((split_kernel<decltype(v)::value ? 4 : 1>), dim3(blocks), dim3(kLrpThreads), 0, static_cast<hipStream_t>(stream), x,
                       total, pos, neg);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_ratio_f32(const float* r, const float* z1, const float* z2, int B, int64_t n, float* s, xai_stream_t stream) {
  XAI_REQUIRE_PTR(r); XAI_REQUIRE_PTR(z1); XAI_REQUIRE_PTR(s);
  const int64_t total = flat_total(B, n);
  XAI_REQUIRE(total > 0, static_cast<int>(total));
  const bool vec = xai_can_vec4(total, {r, z1, z2, s});
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(total / (vec ? 4 : 1), kLrpThreads, &blocks), XAI_E_UNSUPPORTED);
  xai_dispatch(vec, [&](auto v) {
    xai_dispatch(z2 != nullptr, [&](auto two) {
      hipLaunchKernelGGL((ratio_kernel<decltype(v)::value ? 4 : 1, decltype(two)::value>), dim3(blocks), dim3(kLrpThreads), 0,
                         static_cast<hipStream_t>(stream), r, z1, z2, total, s);
    });
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_gather_f32(const float* x, const float* g1, const float* g2, int B, int64_t n, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(g1); XAI_REQUIRE_PTR(g2); XAI_REQUIRE_PTR(out);
  const int64_t total = flat_total(B, n);
  XAI_REQUIRE(total > 0, static_cast<int>(total));
  const bool vec = xai_can_vec4(total, {x, g1, g2, out});
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(total / (vec ? 4 : 1), kLrpThreads, &blocks), XAI_E_UNSUPPORTED);
  xai_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((gather_kernel<decltype(v)::value ? 4 : 1>), dim3(blocks), dim3(kLrpThreads), 0, static_cast<hipStream_t>(stream), x,
                       g1, g2, total, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_clone_f32(const float* x, const float* r1, const float* r2, int B, int64_t n, float* out, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(r1); XAI_REQUIRE_PTR(r2); XAI_REQUIRE_PTR(out);
  const int64_t total = flat_total(B, n);
  XAI_REQUIRE(total > 0, static_cast<int>(total));
  const bool vec = xai_can_vec4(total, {x, r1, r2, out});
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(total / (vec ? 4 : 1), kLrpThreads, &blocks), XAI_E_UNSUPPORTED);
  xai_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((clone_kernel<decltype(v)::value ? 4 : 1>), dim3(blocks), dim3(kLrpThreads), 0, static_cast<hipStream_t>(stream), x,
                       r1, r2, total, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_half_product_f32(const float* x, const float* c, int B, int h, int N, int d, int slots, int slot, float* out,
                                        xai_stream_t stream) {
  XAI_REQUIRE_PTR(x); XAI_REQUIRE_PTR(c); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(B > 0 && h > 0 && N > 0 && d > 0, XAI_E_SHAPE);
  XAI_REQUIRE((slots == 1 || slots == 3) && slot >= 0 && slot < slots, XAI_E_SHAPE);
  const int64_t per = static_cast<int64_t>(h) * N;
  XAI_REQUIRE(per <= INT64_MAX / d && per * d <= INT64_MAX / (3 * static_cast<int64_t>(B)), XAI_E_UNSUPPORTED);
  const int64_t total = per * d * B;
  // the V floats of a lane must share their row of d: the flat plain mode needs only total % 4 == 0, the strided one d % 4 == 0
  const bool vec = xai_can_vec4(slots == 1 ? total : d, {x, c, out});
  unsigned blocks;
  XAI_REQUIRE(xai_blocks_checked(total / (vec ? 4 : 1), kLrpThreads, &blocks), XAI_E_UNSUPPORTED);
  xai_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((half_product_kernel<decltype(v)::value ? 4 : 1>), dim3(blocks), dim3(kLrpThreads), 0, static_cast<hipStream_t>(stream),
                       x, c, total, h, N, d, slots, slot, out);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_add_chunk(void) { return kAddChunk; }

XAI_EXPORT size_t xai_lrp_add_workspace_bytes(int B, int64_t n) {
  if (add_shape(B, n) != XAI_OK) return 0;
  return static_cast<size_t>(B) * static_cast<size_t>(add_chunks(n)) * 3 * sizeof(double);
}

XAI_EXPORT int xai_lrp_add_parts_f32(const float* x0, const float* x1, const float* r, int B, int64_t n, float* a, float* b, void* ws,
                                     size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(x0); XAI_REQUIRE_PTR(x1); XAI_REQUIRE_PTR(r); XAI_REQUIRE_PTR(a); XAI_REQUIRE_PTR(b); XAI_REQUIRE_PTR(ws);
  const int shape = add_shape(B, n);
  XAI_REQUIRE(shape == XAI_OK, shape);
  XAI_REQUIRE(ws_bytes >= xai_lrp_add_workspace_bytes(B, n) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, XAI_E_SHAPE);
  const bool vec = xai_can_vec4(n, {x0, x1, r, a, b});
  xai_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((add_parts_kernel<decltype(v)::value>), dim3(unsigned(add_chunks(n)), unsigned(B)), dim3(kLrpThreads), 0,
                       static_cast<hipStream_t>(stream), x0, x1, r, n, a, b, static_cast<double*>(ws));
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_add_scale_f32(float* a, float* b, int B, int64_t n, const void* ws, size_t ws_bytes, xai_stream_t stream) {
  XAI_REQUIRE_PTR(a); XAI_REQUIRE_PTR(b); XAI_REQUIRE_PTR(ws);
  const int shape = add_shape(B, n);
  XAI_REQUIRE(shape == XAI_OK, shape);
  XAI_REQUIRE(ws_bytes >= xai_lrp_add_workspace_bytes(B, n) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, XAI_E_SHAPE);
  const bool vec = xai_can_vec4(n, {a, b});
  xai_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((add_scale_kernel<decltype(v)::value>), dim3(unsigned(add_chunks(n)), unsigned(B)), dim3(kLrpThreads), 0,
                       static_cast<hipStream_t>(stream), a, b, n, static_cast<const double*>(ws));
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_lrp_attn_matrices_f32(const float* cam, const float* grad, int L, int B, int h, int S, int mode, float* out,
                                         xai_stream_t stream) {
  XAI_REQUIRE_PTR(cam); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(L > 0 && B > 0 && h > 0 && S > 0 && mode >= 0 && mode <= 2, XAI_E_SHAPE);
  XAI_REQUIRE(L <= 65535 && B <= 65535, XAI_E_UNSUPPORTED);
  const int rows = mode == 2 ? 1 : S;
  const dim3 grid(unsigned(xai_ceil_div(rows, kLrpWaves)), unsigned(L), unsigned(B));
  xai_dispatch(grad != nullptr, [&](auto g) {
    hipLaunchKernelGGL((attn_matrices_kernel<decltype(g)::value>), grid, dim3(kLrpThreads), 0, static_cast<hipStream_t>(stream), cam, grad,
                       B, h, S, mode, out);
  });
  return xai_launch_status();
}
