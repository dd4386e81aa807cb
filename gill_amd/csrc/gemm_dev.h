// Device helpers shared by the GEMM / convolution kernels (gemm.hip) and the split-K reducers (gemm_reduce.hip).
#pragma once
#include "ops.h"

#define LN_MAX_PLANES 20   // row-sum planes a folded-LayerNorm consumer can add: 2 per N tile of the producer, or one per 64 columns of a split-K reducer (C <= 1280)

__device__ __noinline__ float gelu_erf_call(float v) { return gelu_erf(v); }  // keeps erff out of the unrolled epilogue

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == ACT_RELU) return fmaxf(v, 0.f);
  if (act == ACT_SILU) return silu_f(v);
  if (act == ACT_GELU) return gelu_erf_call(v);
  if (act == ACT_QUICK_GELU) return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * v));
  return v;
}

// folded LayerNorm: rstd and mean*rstd of A's row m from the producer's {sum, sum of squares}
__device__ __forceinline__ void ln_row_factors(const GemmArgs& p, int m, float& rr, float& rm) {
  // the producer's per-plane partial sums of this row, added in plane order (fixed order: bit-reproducible); the loads go out four
  // planes at a time (predicated), not one L2 round trip per plane — and not LN_MAX_PLANES predicated loads per row: a level-0
  // consumer reads 4 planes (the prologue of the GEGLU / QKV kernels was 80 load slots per lane for them)
  const int R = p.ln_rows ? p.ln_rows : p.M;
  if (m >= R) m -= R;
  const float* base = p.ln_stats + (size_t)m * 2;
  const size_t pstride = (size_t)R * 2;
  float2 st = make_float2(0.f, 0.f);
  for (int pl = 0; pl < p.ln_planes; pl += 4) {      // (wave-uniform trip count)
    float2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      v[u] = (pl + u < p.ln_planes) ? *reinterpret_cast<const float2*>(base + (size_t)(pl + u) * pstride) : make_float2(0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) { st.x += v[u].x; st.y += v[u].y; }
  }
  const float invk = 1.f / (float)p.K;
  const float mean = st.x * invk;
  const float var = fmaxf(st.y * invk - mean * mean, 0.f);
  rr = rsqrtf(var + p.ln_eps);
  rm = mean * rr;
}

// block geometry of the plain split-K reducer (gemm_reduce.hip); gemm_row_planes() / gemm_gn_slab_rows() report it to the consumers
int reduce_width(const GemmArgs& a);
int reduce_rows(const GemmArgs& a);
