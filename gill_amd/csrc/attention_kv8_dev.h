// The e4m3 KV-cache format the two kv8 attention kernels share (attention_decode_kv8.hip, attention_extend_kv8.hip; AttnDecodeKv8Args in ops.h).
// A key row and a value row of one token and one head (dp elements) are dp OCP e4m3 bytes and one power-of-two scale 2^e, e an int8 per
// (row, head, slot).  The rule is linear_w8.hip's: e = ceil(log2(amax / 448)) from the maximum's mantissa and exponent (amax = f 2^p, f in
// [0.5, 1): e = p - 9 for f <= 0.875 = 448 / 512 and p - 8 above), kept >= -100; a zero (or non-finite) row has e = 0.  x / 2^e is exact in
// fp32, the rounding is the conversion instruction's round-to-nearest-even, and every code times 2^e is a bf16 number.
#pragma once
#include "ops.h"

namespace kv8 {

typedef __attribute__((ext_vector_type(2))) float f32x2;

// the row's exponent from its maximum magnitude
__device__ __forceinline__ int row_exp(float amax) {
  int e = 0;
  if (amax > 0.f && amax < __builtin_inff()) {
    int pw;
    const float f = frexpf(amax, &pw);
    e = f <= 0.875f ? pw - 9 : pw - 8;
    if (e < -100) e = -100;
  }
  return e;
}

// 2^e as fp32 for a STORED exponent: a slot that holds data has e in [-100, 120]; whatever a stale slot holds is kept inside the normal
// numbers, so that a product with it is finite and the selection that follows discards a number, not a NaN
__device__ __forceinline__ float pow2(int e) {
  e = e < -126 ? -126 : (e > 127 ? 127 : e);
  return __uint_as_float((uint32_t)(e + 127) << 23);
}

// two bf16 of a word -> their e4m3 codes (low 16 bits), inv = 2^-e
__device__ __forceinline__ uint32_t quant2(uint32_t u, float inv) {
  const float v0 = clamp_fp8_keep_nan(__uint_as_float(u << 16) * inv), v1 = clamp_fp8_keep_nan(__uint_as_float(u & 0xffff0000u) * inv);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false) & 0xffffu;
}
// four bf16 of two words -> four codes
__device__ __forceinline__ uint32_t quant4(uint32_t u0, uint32_t u1, float inv) {
  const float v0 = clamp_fp8_keep_nan(__uint_as_float(u0 << 16) * inv), v1 = clamp_fp8_keep_nan(__uint_as_float(u0 & 0xffff0000u) * inv);
  const float v2 = clamp_fp8_keep_nan(__uint_as_float(u1 << 16) * inv), v3 = clamp_fp8_keep_nan(__uint_as_float(u1 & 0xffff0000u) * inv);
  int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false);
  pk = __builtin_amdgcn_cvt_pk_fp8_f32(v2, v3, pk, true);
  return (uint32_t)pk;
}
__device__ __forceinline__ float amax2(uint32_t u) { return fmaxf(fabsf(__uint_as_float(u << 16)), fabsf(__uint_as_float(u & 0xffff0000u))); }

// four codes -> fp32 (exact)
__device__ __forceinline__ void cvt4f(uint32_t x, float* f) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
}
// four codes -> four bf16 in two words (exact: a code has four significant bits), as w8_cvt4 of linear_w8.hip
__device__ __forceinline__ void cvt4bf(uint32_t x, uint32_t& lo, uint32_t& hi) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x, true);
  lo = (__float_as_uint(a[0]) >> 16) | (__float_as_uint(a[1]) & 0xffff0000u);
  hi = (__float_as_uint(b[0]) >> 16) | (__float_as_uint(b[1]) & 0xffff0000u);
}

}  // namespace kv8
