// What more than one CLIP kernel file needs of the operand dtype T (float or __half), once: the kernels compute in fp32 and the
// headers under include/ say where a value is rounded to T.
//   ld: an operand as fp32;  rT: the headers' rounding to T;  st: a result that already passed rT, or is rounded to T here, once
#pragma once
#include <hip/hip_fp16.h>

#include <type_traits>

__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const __half* p) { return __half2float(*p); }
template <typename T>
__device__ __forceinline__ float rT(float x) {
  if constexpr (std::is_same<T, __half>::value) return __half2float(__float2half_rn(x));
  else return x;
}
__device__ __forceinline__ void st(float* p, float x) { *p = x; }
__device__ __forceinline__ void st(__half* p, float x) { *p = __float2half_rn(x); }
