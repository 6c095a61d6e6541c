// Shared helpers for the gfx950 kernels of libxai_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <type_traits>
#include "xai_hip.h"
#include "xai_launch_plan.h"

#define XAI_EXPORT extern "C" __attribute__((visibility("default")))
// The two version entry points every library exports, `name` and `name`_minor, returning the two version defines of the library's
// header.  Said once per library, in the first source file of its SRCS_<key> line (csrc/Makefile).
#define XAI_VERSION_ENTRIES(name, version, minor) \
  XAI_EXPORT int name(void) { return version; }   \
  XAI_EXPORT int name##_minor(void) { return minor; }

#define XAI_REQUIRE_PTR(p) \
  do {                     \
    if ((p) == nullptr) return XAI_E_NULL; \
  } while (0)
#define XAI_REQUIRE(cond, code) \
  do {                          \
    if (!(cond)) return (code); \
  } while (0)

// hipGetLastError after a launch: >0 on failure, 0 on success.
static inline int xai_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? XAI_OK : static_cast<int>(e);
}

static inline bool xai_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// May a launch over n floats take the float4 flavour of its kernel: n is a multiple of 4 and every pointer the kernel reads or
// writes 16 bytes at a time is 16-byte aligned.  Optional pointers are passed as they are; a null one is skipped.
static inline bool xai_can_vec4(int64_t n, std::initializer_list<const void*> ptrs) {
  if (n & 3) return false;
  for (const void* p : ptrs)
    if (p && !xai_aligned16(p)) return false;
  return true;
}

static inline int64_t xai_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// n rounded up to a multiple of `to`, a power of two: the parts of a workspace
static inline size_t xai_align_up(size_t n, size_t to) { return (n + to - 1) & ~(to - 1); }

// ---- host launch blocks: DESIGN.md ("Host launch blocks") has the rule for what may be shared.
// f(std::true_type) or f(std::false_type): a launch written once in a generic lambda names its kernel from the constant,
// kernel<F ? 4 : 1> or kernel<F>; nested calls handle two flags.
template <typename Fn>
static inline void xai_dispatch(bool flag, Fn&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}
// gridDim.x of a launch over n floats, one lane per 4 (vec) or 1 of them
static inline unsigned xai_grid_x(int64_t n, int block, bool vec) { return unsigned(xai_ceil_div(n, int64_t(block) * (vec ? 4 : 1))); }
// blocks of a 1-D grid of one lane per unit -> false where they do not fit gridDim.x
static inline bool xai_blocks_checked(int64_t n_units, int block, unsigned* blocks) {
  *blocks = static_cast<unsigned>(xai_ceil_div(n_units, block));
  return xai_ceil_div(n_units, block) <= INT32_MAX;
}

// Compute units of the current device (256 on MI355X).  One definition for the whole library (abi.hip): the per-device
// value is queried once and published through a std::atomic, so concurrent first calls from several host threads race
// only on storing the same number.
int xai_cu_count();

constexpr int kWave = 64;  // gfx950 wavefront

// ---- device building blocks --------------------------------------------------------------------------------------------
// One definition of each; DESIGN.md ("Device building blocks") has the rule for what may be shared.

// Wave-wide reductions over 64 lanes (butterfly through DPP/bpermute shuffles); every lane gets the result.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, kWave));
  return v;
}

// Inclusive prefix sum over the 64 lanes of a wave.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t up = __shfl_up(v, off, kWave);
    if (lane >= off) v += up;
  }
  return v;
}

// Streamed exclusive prefix sum of one value per lane over a workgroup of THREADS lanes -> `run` (on entry) plus the sum of v over
// the lanes below this one; `run` grows by the sum over the workgroup, the same in every lane, so a loop that walks an array THREADS
// elements a pass calls this once per pass.  wave_scan_incl inside a wave, the waves' totals through `wsum`: THREADS / 64 words,
// whatever is in them.  All lanes of the workgroup must call.
// Of the scan's two barriers one is inside, between the waves' totals written to `wsum` and their reads.  The other is the
// caller's: `wsum` is being read until the workgroup's next barrier, so a loop ends its pass with __syncthreads() behind its own
// store (which that barrier also shows to the workgroup), and `wsum` is free again from there; one call whose `wsum` nothing
// writes afterwards needs none.  Inside, that barrier would stand between the ranks and their store and cost every pass the
// time of the sums (profiles/r22_scan_blocks.txt).
template <int THREADS>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t& run, uint32_t* wsum) {
  static_assert(THREADS % kWave == 0, "whole waves");
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint32_t incl = wave_scan_incl(v);
  if (lane == kWave - 1) wsum[wave] = incl;
  __syncthreads();
  uint32_t pre = run + incl - v, total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / kWave; ++w) {
    if (w < wave) pre += wsum[w];
    total += wsum[w];
  }
  run += total;
  return pre;
}

// ptr[0..n) = 0 on `stream`, n >= 1: the status words of the segmenters.  -> xai_launch_status()
// Templates, so that only the files that clear anything carry the kernel.
template <int BLOCK>
__global__ void clear_i32_kernel(int32_t* __restrict__ ptr, int n) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) ptr[i] = 0;
}
template <int BLOCK = 256>
static inline int xai_clear_i32(int32_t* ptr, int n, hipStream_t stream) {
  clear_i32_kernel<BLOCK><<<unsigned(xai_ceil_div(n, BLOCK)), BLOCK, 0, stream>>>(ptr, n);
  return xai_launch_status();
}

// argmax order of torch.max on the CPU: the first NaN if there is one, else the first maximal value.
// -> true if the candidate (v, i) beats the best so far (m, mi).
__device__ __forceinline__ bool argmax_beats(float v, int i, float m, int mi) {
  const bool vn = v != v, mn = m != m;
  if (vn != mn) return vn;
  if (vn) return i < mi;
  return v > m || (v == m && i < mi);
}

struct ArgMax {
  float v;
  int i;
};

// argmax of row[0..n), n >= 1, over one wave; every lane gets the result.  (-inf, INT32_MAX) loses to every element of a row,
// so a lane that holds none (n < 64) never wins the exchange.
__device__ __forceinline__ ArgMax wave_argmax(const float* row, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  ArgMax b{-INFINITY, INT32_MAX};
  for (int j = lane; j < n; j += kWave) {
    const float v = row[j];
    if (argmax_beats(v, j, b.v, b.i)) { b.v = v; b.i = j; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(b.v, off, kWave);
    const int oi = __shfl_xor(b.i, off, kWave);
    if (argmax_beats(ov, oi, b.v, b.i)) { b.v = ov; b.i = oi; }
  }
  return b;
}

// ---- workgroup reductions.  The value of a floating-point sum depends on its tree: each of these is ONE tree, for the users that
// have always had exactly it.  All lanes of the workgroup must call.

// Sum of one fp64 value per lane over a workgroup of WAVES waves: xor butterfly inside a wave (a+b on both partners, so all
// lanes agree), then the waves in ascending order from +0.  Every lane gets the same bits; `red` (WAVES doubles) is free again
// on return.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += red[w];
  __syncthreads();
  return s;
}

// Sum of one fp32 value per lane over a workgroup of WAVES <= 64 waves: butterfly inside a wave, the wave partials through
// `part` (WAVES floats), then a second butterfly over them in wave 0.  Only thread 0's return value is specified.
template <int WAVES>
__device__ __forceinline__ float block_sum_lane0(float v, float* part) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
  __syncthreads();
  if (threadIdx.x < kWave) {
    v = threadIdx.x < WAVES ? part[threadIdx.x] : 0.f;
    v = wave_sum(v);
  }
  return v;
}

// min / max over a workgroup of WAVES waves; every lane gets the result.  `red` holds 2 * WAVES floats; the barrier in front of
// the writes makes a second call with the same `red` safe.  fminf / fmaxf: a NaN is dropped, not propagated.
template <int WAVES>
__device__ __forceinline__ void block_min_max(float& lo, float& hi, float* red) {
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int wave = threadIdx.x / kWave;
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[wave] = lo;
    red[WAVES + wave] = hi;
  }
  __syncthreads();
  lo = red[0];
  hi = red[WAVES];
  for (int i = 1; i < WAVES; ++i) {
    lo = fminf(lo, red[i]);
    hi = fmaxf(hi, red[WAVES + i]);
  }
}

// ---- radix select over a 2 * THREADS-bin LDS histogram, one workgroup of THREADS lanes; lane t owns bins 2t and 2t + 1.

__device__ __forceinline__ void select_zero_hist(uint32_t* hist) {
  hist[2 * threadIdx.x] = 0u;
  hist[2 * threadIdx.x + 1] = 0u;
}

// Digit d of `hist` with count(< d) <= k < count(<= d); k becomes the rank inside that digit.  The histogram must be complete
// (a barrier after the last atomicAdd) and k below its total.  `wsum` holds THREADS / 64 words, `pick` 2; both are free again on
// return, so the calls of one kernel share them.
template <int THREADS>
__device__ __forceinline__ uint32_t select_digit(const uint32_t* hist, uint32_t& k, uint32_t* wsum, uint32_t* pick) {
  static_assert(THREADS % kWave == 0, "whole waves");
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const uint32_t c0 = hist[2 * t], c1 = hist[2 * t + 1], c = c0 + c1;
  const uint32_t incl = wave_scan_incl(c);             // not block_scan_excl: the `pick` exchange sits between the scan's two barriers
  if (lane == kWave - 1) wsum[wave] = incl;
  __syncthreads();
  uint32_t pre = incl - c;
  for (int w = 0; w < wave; ++w) pre += wsum[w];
  if (k >= pre && k < pre + c0) {
    pick[0] = 2 * t; pick[1] = k - pre;
  } else if (k >= pre + c0 && k < pre + c) {
    pick[0] = 2 * t + 1; pick[1] = k - pre - c0;
  }
  __syncthreads();
  const uint32_t d = pick[0];
  k = pick[1];
  __syncthreads();
  return d;
}

// ---- 16-byte and non-temporal accesses
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// Non-temporal (nt): for data that is streamed once, so that it does not displace lines that will be read again from L2 /
// Infinity Cache.  The builtins take clang's vector type, not HIP's float4.
typedef float xai_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4_nt(const float* p) {
  const xai_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const xai_f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4_nt(float* p, float4 v) {
  const xai_f32x4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<xai_f32x4*>(p));
}
__device__ __forceinline__ float ld_nt(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_nt(float* p, float v) { __builtin_nontemporal_store(v, p); }

// V floats of one lane, V = 4 (one 16-byte access) or 1: a kernel written once over Pack<V> exists in both flavours.
template <int V>
struct Pack {
  float v[V];
};

template <int V>
__device__ __forceinline__ Pack<V> ldp(const float* p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const float4 t = ld4(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void stp(float* p, const Pack<V>& a) {
  if constexpr (V == 4) {
    st4(p, make_float4(a.v[0], a.v[1], a.v[2], a.v[3]));
  } else {
    *p = a.v[0];
  }
}
