// K23-K25: Adversarial Gradient Integration (AGI.py:39-115, evaluatePerturbation.py:119-139) for gfx950.
//
// A "pair" is one (image, false class) attack; pair p = image * n_cls + k attacks classes[k].  Pairs are independent and one
// classifier pass carries all of them, so each entry covers every pair of a pass in one launch.
//   K23 init     the initial prediction of every image (the first maximal logit, NaN counted as maximal, as torch.max on the
//                CPU), the pair state words and x_cur = data, c_delta = 0.  Grid (chunks, pairs); only the chunk-0 block of a
//                pair computes the argmax and writes that pair's state (and, for k = 0, init_pred): no block reads a state word.
//   K24 step     one iteration of pgd_step (:57-79) for every pair, as TWO launches:
//                  decide  one wave per pair: argmax of the pair's logits, then the pair's state: an active pair whose argmax is
//                          its class stops (the reference's break, :64-65) and is not updated; any other active pair is updated,
//                          and stops after its max_iter-th update.  Word 3 records whether this launch updates the pair.
//                  update  grid (chunks, pairs): x_cur = clamp(data + eps * sign(g_adv), 0, 1) and c_delta += -g_lab * (x_cur -
//                          data) (fgsm_step, :39-49) where word 3 says so.
//                Every block of a pair reads the decision the previous launch wrote, so all of them agree, and no block reads a
//                state word that another block of the same launch writes.  The decide launch is tiny (one wave per pair over
//                the logits, L2-resident), so splitting costs one launch, inside the captured graph, per iteration.
//   K25 heatmap  per image, one workgroup of 1024 lanes: step_grad = sum of the pairs' c_delta in class order (from +0, as the
//                reference's `step_grad = 0; step_grad += delta`), the channel mean ((c0 + c1) + c2) / 3, NumPy's two 'linear'
//                percentiles, the clip and the normalisation.  A 224^2 map (196 KB) does not fit in LDS: the map is written to
//                `out` by the first sweep, and the order statistics come from a three-pass radix select (11, 11, 10 key bits)
//                over it (L2-resident), one histogram per order statistic from the second pass on, so all four order statistics
//                (floor and floor + 1 of both percentiles) are found in the same three sweeps.  A NaN anywhere makes NumPy's
//                percentiles NaN and with them the whole map; the kernel writes NaN everywhere then.
// Bit-exactness: every element's arithmetic is the reference's fp32 expression in its order (-ffp-contract=off keeps a*b+c two
// roundings); nothing is summed across elements, so there are no float atomics and two runs give identical bytes.  The
// histograms count with LDS integer atomics (counts do not depend on arrival order).
// Capturable: no memset (K23 writes every word), no float atomics, no host value that changes between replays: the iteration
// count lives in the state words.
#include "xai_common.h"

#include <math.h>

namespace {

constexpr int kBlock = 256;                  // init / update
constexpr int kDecideBlock = 256;            // four waves, one pair each
constexpr int kMapThreads = 1024;            // K25
constexpr int kMapWaves = kMapThreads / kWave;
constexpr int kBins = 2048;
constexpr int kMaxChunks = 1024;             // grid-stride beyond this

enum : int32_t { kRunning = 0, kReached = 1, kSkipped = 2, kMaxIter = 3 };

// ------------------------------------------------------------------------------------------------ K23
template <int V>
__global__ __launch_bounds__(kBlock) void agi_init_kernel(const float* __restrict__ logits, const float* __restrict__ data,
                                                          const int32_t* __restrict__ classes, int n_cls, int n_out, int64_t N,
                                                          int64_t* __restrict__ init_pred, float* __restrict__ x_cur,
                                                          float* __restrict__ c_delta, int32_t* __restrict__ state) {
  const int p = blockIdx.y;
  const int b = p / n_cls, k = p - b * n_cls;
  const float* src = data + static_cast<int64_t>(b) * N;
  float* xc = x_cur + static_cast<int64_t>(p) * N;
  float* cd = c_delta + static_cast<int64_t>(p) * N;
  Pack<V> z;
#pragma unroll
  for (int u = 0; u < V; ++u) z.v[u] = 0.f;
  for (int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V; i < N;
       i += static_cast<int64_t>(gridDim.x) * kBlock * V) {
    stp<V>(xc + i, ldp<V>(src + i));
    stp<V>(cd + i, z);
  }
  if (blockIdx.x == 0 && threadIdx.x < kWave) {
    const int pred = wave_argmax(logits + static_cast<int64_t>(b) * n_out, n_out).i;
    if (threadIdx.x == 0) {
      const bool skip = classes[k] == pred;                       // AGI.py:97-98
      int32_t* st = state + 4 * static_cast<int64_t>(p);
      st[0] = skip ? 0 : 1;
      st[1] = 0;
      st[2] = skip ? kSkipped : kRunning;
      st[3] = 0;
      if (k == 0) init_pred[b] = pred;
    }
  }
}

// ------------------------------------------------------------------------------------------------ K24
__global__ __launch_bounds__(kDecideBlock) void agi_decide_kernel(const float* __restrict__ logits, const int32_t* __restrict__ classes,
                                                                  int n_pair, int n_cls, int n_out, int max_iter,
                                                                  int32_t* __restrict__ state) {
  const int p = blockIdx.x * (kDecideBlock / kWave) + threadIdx.x / kWave;
  if (p >= n_pair) return;                                        // whole waves leave together
  int32_t* st = state + 4 * static_cast<int64_t>(p);
  const int32_t active = st[0];
  const int pred = wave_argmax(logits + static_cast<int64_t>(p) * n_out, n_out).i;
  if ((threadIdx.x & (kWave - 1)) != 0) return;
  if (!active) {
    st[3] = 0;
    return;
  }
  if (pred == classes[p % n_cls]) {                               // the attack succeeded: break before any update (:64-65)
    st[0] = 0;
    st[2] = kReached;
    st[3] = 0;
    return;
  }
  const int32_t done = st[1] + 1;
  st[1] = done;
  st[3] = 1;
  if (done >= max_iter) {
    st[0] = 0;
    st[2] = kMaxIter;
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void agi_update_kernel(const float* __restrict__ g_adv, const float* __restrict__ g_lab,
                                                            const float* __restrict__ data, int n_cls, int64_t N, float eps,
                                                            const int32_t* __restrict__ state, float* __restrict__ x_cur,
                                                            float* __restrict__ c_delta) {
  const int p = blockIdx.y;
  if (state[4 * static_cast<int64_t>(p) + 3] == 0) return;
  const int64_t off = static_cast<int64_t>(p) * N;
  const float* x0 = data + static_cast<int64_t>(p / n_cls) * N;
  for (int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V; i < N;
       i += static_cast<int64_t>(gridDim.x) * kBlock * V) {
    const Pack<V> ga = ldp<V>(g_adv + off + i), gl = ldp<V>(g_lab + off + i), d = ldp<V>(x0 + i);
    Pack<V> c = ldp<V>(c_delta + off + i), xn;
#pragma unroll
    for (int u = 0; u < V; ++u) {
      const float g = ga.v[u];
      const float s = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);    // torch.sign: NaN and -0 give +0
      const float v = d.v[u] + eps * s;
      const float r = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);        // torch.clamp(., 0, 1): NaN and -0 pass through
      xn.v[u] = r;
      c.v[u] = c.v[u] + (-gl.v[u]) * (r - d.v[u]);
    }
    stp<V>(x_cur + off + i, xn);
    stp<V>(c_delta + off + i, c);
  }
}

// ------------------------------------------------------------------------------------------------ K25
// Order-preserving key of a non-NaN float (-0 keyed as +0: NumPy orders them as equal).
__device__ __forceinline__ uint32_t okey(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// NumPy's _lerp in float32 (numpy/lib/_function_base_impl.py): a + (b - a) * t, or b - (b - a) * (1 - t) where t >= 0.5
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
  const float d = b - a;
  return t >= 0.5f ? b - d * (1.f - t) : a + d * t;
}

struct Pct {
  uint32_t rank[4];            // floor and floor + 1 of the low percentile, then of the high one (NumPy's clipped indexes)
  float gamma[2];
};

__global__ __launch_bounds__(kMapThreads) void agi_heatmap_kernel(const float* __restrict__ c_delta, int n_cls, int C, int64_t HW,
                                                                  Pct pct, float* __restrict__ out, float* __restrict__ step_grad,
                                                                  float* __restrict__ qu) {
  __shared__ uint32_t hist[4][kBins];
  __shared__ uint32_t wsum[kMapWaves];
  __shared__ uint32_t pick[2];
  __shared__ uint32_t nan_seen;
  __shared__ uint32_t digit[4];
  __shared__ float bounds[2];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int64_t plane = static_cast<int64_t>(C) * HW;
  const float* cd = c_delta + static_cast<int64_t>(b) * n_cls * plane;
  float* m = out + static_cast<int64_t>(b) * HW;
  float* sg = step_grad != nullptr ? step_grad + static_cast<int64_t>(b) * plane : nullptr;
  for (int j = tid; j < 4 * kBins; j += kMapThreads) (&hist[0][0])[j] = 0u;
  if (tid == 0) nan_seen = 0u;
  __syncthreads();
  const float fc = static_cast<float>(C);
  // ---- sweep 1: step_grad, the channel mean (written to out), the top key digit
  for (int64_t i = tid; i < HW; i += kMapThreads) {
    float h = 0.f;
    for (int c = 0; c < C; ++c) {
      float s = 0.f;                                              // step_grad = 0; step_grad += delta (AGI.py:93,101)
      for (int k = 0; k < n_cls; ++k) s = s + cd[static_cast<int64_t>(k) * plane + c * HW + i];
      if (sg != nullptr) sg[c * HW + i] = s;
      h = c == 0 ? s : h + s;                                     // np.mean(axis=0): ((c0 + c1) + c2) ...
    }
    h = h / fc;                                                   // ... / C in float32
    m[i] = h;
    if (h != h) nan_seen = 1u;
    else atomicAdd(&hist[0][okey(h) >> 21], 1u);
  }
  __syncthreads();
  const bool any_nan = nan_seen != 0u;
  if (any_nan) {                                                  // NumPy: NaN percentiles, and (x - NaN) / NaN everywhere
    const float qn = __builtin_nanf("");
    for (int64_t i = tid; i < HW; i += kMapThreads) m[i] = qn;
    if (qu != nullptr && tid == 0) { qu[2 * b] = qn; qu[2 * b + 1] = qn; }
    return;
  }
  // ---- sweeps 2 and 3: the next 11 and the last 10 key bits of every order statistic
  uint32_t kr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kr[j] = pct.rank[j];
  uint32_t d1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) d1[j] = select_digit<kMapThreads>(hist[0], kr[j], wsum, pick);
  for (int j = tid; j < 4 * kBins; j += kMapThreads) (&hist[0][0])[j] = 0u;
  __syncthreads();
  for (int64_t i = tid; i < HW; i += kMapThreads) {
    const uint32_t key = okey(m[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((key >> 21) == d1[j]) atomicAdd(&hist[j][(key >> 10) & 0x7FFu], 1u);
  }
  __syncthreads();
  uint32_t hi[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) hi[j] = (d1[j] << 11) | select_digit<kMapThreads>(hist[j], kr[j], wsum, pick);
  for (int j = tid; j < 4 * kBins; j += kMapThreads) (&hist[0][0])[j] = 0u;
  __syncthreads();
  for (int64_t i = tid; i < HW; i += kMapThreads) {
    const uint32_t key = okey(m[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((key >> 10) == hi[j]) atomicAdd(&hist[j][key & 0x3FFu], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t d = select_digit<kMapThreads>(hist[j], kr[j], wsum, pick);
    if (tid == 0) digit[j] = (hi[j] << 10) | d;
  }
  if (tid == 0) {
    const float q = np_lerp(unkey(digit[0]), unkey(digit[1]), pct.gamma[0]);
    const float u = np_lerp(unkey(digit[2]), unkey(digit[3]), pct.gamma[1]);
    bounds[0] = q;
    bounds[1] = u;
    if (qu != nullptr) { qu[2 * b] = q; qu[2 * b + 1] = u; }
  }
  __syncthreads();
  // ---- sweep 4: hm[hm < q] = q; hm[hm > u] = u; hm = (hm - q) / (u - q)   (evaluatePerturbation.py:136-138)
  const float q = bounds[0], u = bounds[1];
  const float span = u - q;
  for (int64_t i = tid; i < HW; i += kMapThreads) {
    float h = m[i];
    if (h < q) h = q;
    if (h > u) h = u;
    m[i] = (h - q) / span;
  }
}

// NumPy 2 percentile of a float32 array, method 'linear' (numpy/lib/_function_base_impl.py: percentile, _quantile, _get_indexes,
// _get_gamma): q / float32(100) in float32, the virtual index (n - 1) * q in float32, the neighbours floor and floor + 1 clipped
// to the last element (index -1) at or above n - 1, and gamma = virtual - previous index, taken in float64 and rounded to float32.
void np_percentile_plan(double q, int64_t n, uint32_t* rank, float* gamma) {
  const float qf = static_cast<float>(q) / 100.0f;
  const float v = static_cast<float>(n - 1) * qf;
  double prev;
  if (v >= static_cast<float>(n - 1)) {
    rank[0] = rank[1] = static_cast<uint32_t>(n - 1);
    prev = -1.0;                                                  // the index -1 itself enters gamma
  } else {
    prev = floor(static_cast<double>(v));
    rank[0] = static_cast<uint32_t>(prev);
    rank[1] = rank[0] + 1;
  }
  *gamma = static_cast<float>(static_cast<double>(v) - prev);
}

unsigned chunks_for(int64_t N, int V) {
  const int64_t c = xai_ceil_div(N, static_cast<int64_t>(kBlock) * V);
  return static_cast<unsigned>(c < kMaxChunks ? c : kMaxChunks);
}

}  // namespace

XAI_EXPORT int xai_agi_init_f32(const float* logits, const float* data, const int32_t* classes, int n_img, int n_cls, int n_out,
                                int64_t n_elem, int64_t* init_pred, float* x_cur, float* c_delta, int32_t* state,
                                xai_stream_t stream) {
  XAI_REQUIRE_PTR(logits); XAI_REQUIRE_PTR(data); XAI_REQUIRE_PTR(classes); XAI_REQUIRE_PTR(init_pred); XAI_REQUIRE_PTR(x_cur);
  XAI_REQUIRE_PTR(c_delta); XAI_REQUIRE_PTR(state);
  XAI_REQUIRE(n_img > 0 && n_cls > 0 && n_out > 0 && n_elem > 0, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(n_img) * n_cls <= 65535 && n_elem < (int64_t{1} << 31), XAI_E_UNSUPPORTED);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int n_pair = n_img * n_cls;
  xai_dispatch(xai_can_vec4(n_elem, {data, x_cur, c_delta}), [&](auto V4) {
    constexpr int V = V4 ? 4 : 1;
    hipLaunchKernelGGL(agi_init_kernel<V>, dim3(chunks_for(n_elem, V), n_pair), dim3(kBlock), 0, st, logits, data, classes, n_cls, n_out,
                       n_elem, init_pred, x_cur, c_delta, state);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_agi_step_f32(const float* logits, const float* g_adv, const float* g_lab, const float* data, const int32_t* classes,
                                int n_img, int n_cls, int n_out, int64_t n_elem, float epsilon, int max_iter, float* x_cur,
                                float* c_delta, int32_t* state, xai_stream_t stream) {
  XAI_REQUIRE_PTR(logits); XAI_REQUIRE_PTR(g_adv); XAI_REQUIRE_PTR(g_lab); XAI_REQUIRE_PTR(data); XAI_REQUIRE_PTR(classes);
  XAI_REQUIRE_PTR(x_cur); XAI_REQUIRE_PTR(c_delta); XAI_REQUIRE_PTR(state);
  XAI_REQUIRE(n_img > 0 && n_cls > 0 && n_out > 0 && n_elem > 0 && max_iter > 0, XAI_E_SHAPE);
  XAI_REQUIRE(epsilon == epsilon, XAI_E_SHAPE);
  XAI_REQUIRE(static_cast<int64_t>(n_img) * n_cls <= 65535 && n_elem < (int64_t{1} << 31), XAI_E_UNSUPPORTED);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int n_pair = n_img * n_cls;
  const int per = kDecideBlock / kWave;
  hipLaunchKernelGGL(agi_decide_kernel, dim3((n_pair + per - 1) / per), dim3(kDecideBlock), 0, st, logits, classes, n_pair, n_cls,
                     n_out, max_iter, state);
  int rc = xai_launch_status();
  if (rc != XAI_OK) return rc;
  xai_dispatch(xai_can_vec4(n_elem, {g_adv, g_lab, data, x_cur, c_delta}), [&](auto V4) {
    constexpr int V = V4 ? 4 : 1;
    hipLaunchKernelGGL(agi_update_kernel<V>, dim3(chunks_for(n_elem, V), n_pair), dim3(kBlock), 0, st, g_adv, g_lab, data, n_cls, n_elem,
                       epsilon, state, x_cur, c_delta);
  });
  return xai_launch_status();
}

XAI_EXPORT int xai_agi_heatmap_f32(const float* c_delta, int n_img, int n_cls, int C, int64_t HW, double q_lo, double q_hi,
                                   float* out, float* step_grad, float* qu, xai_stream_t stream) {
  XAI_REQUIRE_PTR(c_delta); XAI_REQUIRE_PTR(out);
  XAI_REQUIRE(n_img > 0 && n_cls > 0 && C > 0 && HW > 0, XAI_E_SHAPE);
  XAI_REQUIRE(q_lo >= 0.0 && q_lo <= 100.0 && q_hi >= 0.0 && q_hi <= 100.0, XAI_E_SHAPE);
  XAI_REQUIRE(n_img <= 65535 && static_cast<int64_t>(n_cls) * C * HW < (int64_t{1} << 31) && HW < (int64_t{1} << 24),
              XAI_E_UNSUPPORTED);
  Pct pct;
  np_percentile_plan(q_lo, HW, pct.rank, &pct.gamma[0]);
  np_percentile_plan(q_hi, HW, pct.rank + 2, &pct.gamma[1]);
  hipLaunchKernelGGL(agi_heatmap_kernel, dim3(n_img), dim3(kMapThreads), 0, static_cast<hipStream_t>(stream), c_delta, n_cls, C, HW, pct,
                     out, step_grad, qu);
  return xai_launch_status();
}
