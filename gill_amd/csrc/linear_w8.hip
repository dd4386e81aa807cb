// Weight-only fp8 linear for the decode step: bf16 activations of at most W8_MAX_ROWS rows against OCP e4m3 weights with one power-of-two
// scale per output row ("w8", include/gill_amd.h gill_opt_create_ex).
//
//   y[m][n] = act(s[n] * sum_k A[m][k] * bf16(w8[n][k]) + b[n]) (+ resid_f32[m][n])
//
// A decode step is weight-bandwidth-bound: every weight byte is read once and used for at most 16 rows.  Halving the bytes is the lever; the
// arithmetic stays that of the bf16 GEMM (bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation) because every e4m3 code converts to
// bf16 exactly and the power-of-two scale is applied to the fp32 sum, exactly.
//
// Storage ("the kernel's order"): [N / 16][K / 64][64 lanes][16 bytes].  Lane l of a 1-KiB chunk holds row n = 16 g + (l & 15), columns
// k = 64 kb + 16 (l >> 4) + 0 .. 15: its one 16-byte load is its own fragment of two MFMAs (bytes 0 .. 7, bytes 8 .. 15), and the wave's load
// instruction covers one contiguous KiB.  The weights are the MFMA's first operand (16 output columns), the activation rows, padded to 16 with
// zeros, the second: a lane ends up with four consecutive columns of one row.
//
// A workgroup of four waves owns 64 columns (four 16-column groups: one activation fragment feeds four MFMAs) and one K range; its waves
// take the 64-wide K steps of the range in turn (wave w: steps w, w + 4, ...), stream their weights from global memory straight to VGPRs
// with the non-temporal policy, W8_U steps (16 loads of 16 bytes per lane) at a time and the next block issued before the current one is
// converted, and add up through LDS in wave order.  The activation slice of the range is staged in LDS once, in fragment order (at most
// W8_STAGE_K columns at a time: 64 KiB).  Grid, K split and summation order depend on (N, K) and the split factor only: row m's bits depend
// neither on M nor on the other rows.  K may be split across workgroups (blockIdx.y): they store fp32 partials [sk][M][N], scale applied,
// which opt_reduce_ln_launch (the engine: residual + the next LayerNorm) or w8_finish_kernel adds in split order.  Vector stores only, no
// flags, no waiting on another workgroup.
#include "ops.h"

#define W8_THREADS 256
#define W8_G 4                    // 16-column groups per workgroup
#define W8_U 4                    // K steps per block of loads
#define W8_STAGE_K 2048           // activation columns staged at a time
#define W8_STAGE_KB (W8_STAGE_K / 64)
#define W8_SMEM (16 * W8_STAGE_K * 2)
static_assert(W8_STAGE_K / 8 == W8_THREADS, "staging: one 16-byte piece of every activation row per thread");

typedef __attribute__((ext_vector_type(2))) float w8_f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int w8_u32x4;

struct W8Dev {
  W8Args a;
  int nkb, sk;
};

// four e4m3 bytes -> four bf16 (exact: 3 mantissa bits, exponents inside bf16's), two per dword in byte order
__device__ __forceinline__ void w8_cvt4(uint32_t x, uint32_t& lo, uint32_t& hi) {
  const w8_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x, true);
  lo = (__float_as_uint(a[0]) >> 16) | (__float_as_uint(a[1]) & 0xffff0000u);
  hi = (__float_as_uint(b[0]) >> 16) | (__float_as_uint(b[1]) & 0xffff0000u);
}

__global__ __launch_bounds__(W8_THREADS) void linear_w8_kernel(const W8Dev d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const W8Args& p = d.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, z = blockIdx.y;
  const int kb0 = (int)(((int64_t)z * d.nkb) / d.sk), kb1 = (int)(((int64_t)(z + 1) * d.nkb) / d.sk);
  const unsigned char* wg[W8_G];
#pragma unroll
  for (int g = 0; g < W8_G; ++g) wg[g] = p.W8 + ((size_t)(tile * W8_G + g) * d.nkb) * 1024 + lane * 16;

  f32x4 acc[W8_G];
#pragma unroll
  for (int g = 0; g < W8_G; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int s0 = kb0; s0 < kb1; s0 += W8_STAGE_KB) {
    const int s1 = s0 + W8_STAGE_KB < kb1 ? s0 + W8_STAGE_KB : kb1;
    const int cnt = (s1 - s0 - w + 3) >> 2;        // this wave's K steps of the stage: s0 + w + 4 i, i < cnt
    const int nblk = (cnt + W8_U - 1) / W8_U;
    w8_u32x4 bufa[W8_U][W8_G], bufb[W8_U][W8_G];
    auto load = [&](w8_u32x4 (&buf)[W8_U][W8_G], int blk) {
#pragma unroll
      for (int u = 0; u < W8_U; ++u) {
        const int i = blk * W8_U + u;
        if (i < cnt) {
          const size_t off = (size_t)(s0 + w + 4 * i) * 1024;
#pragma unroll
          for (int g = 0; g < W8_G; ++g) buf[u][g] = __builtin_nontemporal_load(reinterpret_cast<const w8_u32x4*>(wg[g] + off));
        }
      }
    };
    auto compute = [&](const w8_u32x4 (&buf)[W8_U][W8_G], int blk) {
#pragma unroll
      for (int u = 0; u < W8_U; ++u) {
        const int i = blk * W8_U + u;
        if (i < cnt) {
          const unsigned char* ap = smem + ((size_t)(w + 4 * i) * 64 + lane) * 32;
          const uint4 a0 = *reinterpret_cast<const uint4*>(ap), a1 = *reinterpret_cast<const uint4*>(ap + 16);
          const bf16x8 af0 = __builtin_bit_cast(bf16x8, a0), af1 = __builtin_bit_cast(bf16x8, a1);
#pragma unroll
          for (int g = 0; g < W8_G; ++g) {
            uint4 f0, f1;
            w8_cvt4(buf[u][g][0], f0.x, f0.y);
            w8_cvt4(buf[u][g][1], f0.z, f0.w);
            w8_cvt4(buf[u][g][2], f1.x, f1.y);
            w8_cvt4(buf[u][g][3], f1.z, f1.w);
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f0), af0, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f1), af1, acc[g], 0, 0, 0);
          }
        }
      }
    };
    if (nblk > 0) load(bufa, 0);      // the weights do not wait for the activations
    __syncthreads();                  // (a later stage: the fragment reads of the one before are done)
    // the stage's activation slice in fragment order: (m, k) at ((k / 64) * 64 + (k % 64) / 16 * 16 + m) * 32 + (k % 16) * 2; rows M .. 15 zero
    // (a stage has at most W8_STAGE_K / 8 = W8_THREADS 16-byte pieces per row: one per thread; all rows' loads go out before the first
    // LDS write, one memory round trip for the slice, not one per row)
    const int ks8 = (s1 - s0) * 8;
    if (tid < ks8) {
      const int kl = tid * 8;
      const bf16_t* acol = p.A + (size_t)s0 * 64 + kl;
      uint4 v[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        v[m] = make_uint4(0u, 0u, 0u, 0u);
        if (m < p.M) v[m] = *reinterpret_cast<const uint4*>(acol + (size_t)m * p.K);
      }
      unsigned char* dst = smem + ((size_t)((kl >> 6) * 64 + ((kl & 63) >> 4) * 16)) * 32 + (kl & 15) * 2;
#pragma unroll
      for (int m = 0; m < 16; ++m) *reinterpret_cast<uint4*>(dst + m * 32) = v[m];
    }
    __syncthreads();
    for (int b = 0; b < nblk; b += 2) {
      if (b + 1 < nblk) load(bufb, b + 1);
      compute(bufa, b);
      if (b + 1 < nblk) {
        if (b + 2 < nblk) load(bufa, b + 2);
        compute(bufb, b + 1);
      }
    }
  }

  // the four waves' sums in wave order; wave w finishes column group w
  __syncthreads();
  float4* red = reinterpret_cast<float4*>(smem);       // [wave][group][lane]
#pragma unroll
  for (int g = 0; g < W8_G; ++g) red[(w * W8_G + g) * 64 + lane] = make_float4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
  __syncthreads();
  float4 v = red[(0 * W8_G + w) * 64 + lane];
#pragma unroll
  for (int o = 1; o < 4; ++o) {
    const float4 e = red[(o * W8_G + w) * 64 + lane];
    v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
  }
  const int m = lane & 15;
  const int n = tile * (16 * W8_G) + w * 16 + (lane >> 4) * 4;
  if (m >= p.M) return;
  const float4 sc = *reinterpret_cast<const float4*>(p.scale + n);
  v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;      // powers of two: exact
  if (d.sk > 1 || p.partials_only) {
    *reinterpret_cast<float4*>(p.ws + ((size_t)z * p.M + m) * p.N + n) = v;
    return;
  }
  if (p.bias) {
    const float4 bb = *reinterpret_cast<const float4*>(p.bias + n);
    v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
  }
  if (p.act == ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  const size_t o = (size_t)m * p.N + n;
  if (p.resid) {
    const float4 r = *reinterpret_cast<const float4*>(p.resid + o);
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
  }
  if (p.out_f32) {
    *reinterpret_cast<float4*>((float*)p.C + o) = v;
  } else {
    uint2 q;
    q.x = pack_bf2(v.x, v.y); q.y = pack_bf2(v.z, v.w);
    *reinterpret_cast<uint2*>((bf16_t*)p.C + o) = q;
  }
}

// the epilogue above on the sum of sk partial slices (slice order), for a split launch that does not end in opt_reduce_ln_launch
__global__ __launch_bounds__(256) void w8_finish_kernel(const float* __restrict__ ws, int sk, int M, int N, const float* __restrict__ bias,
                                                        const float* resid, int act, int out_f32, void* C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M * (N / 4)) return;
  const size_t o = (size_t)i * 4, slice = (size_t)M * N;
  const int n = (int)(o % N);
  float4 v = *reinterpret_cast<const float4*>(ws + o);
  for (int zz = 1; zz < sk; ++zz) {
    const float4 e = *reinterpret_cast<const float4*>(ws + zz * slice + o);
    v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
  }
  if (bias) {
    const float4 bb = *reinterpret_cast<const float4*>(bias + n);
    v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
  }
  if (act == ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  if (resid) {
    const float4 r = *reinterpret_cast<const float4*>(resid + o);
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
  }
  if (out_f32) {
    *reinterpret_cast<float4*>((float*)C + o) = v;
  } else {
    uint2 q;
    q.x = pack_bf2(v.x, v.y); q.y = pack_bf2(v.z, v.w);
    *reinterpret_cast<uint2*>((bf16_t*)C + o) = q;
  }
}

// The launcher's own K split, a function of (N, K) only: about one workgroup per CU of the MI355X for the narrow matrices, at least 8 K steps
// per workgroup, at most 4 slices (what opt_reduce_ln_kernel adds in one round trip).
int w8_pick_splitk(int N, int K) {
  const int tiles = N / (16 * W8_G), nkb = K / 64;
  int sk = cdiv(256, tiles);
  if (sk > nkb / 8) sk = nkb / 8;
  if (sk > 4) sk = 4;
  return sk < 1 ? 1 : sk;
}

int linear_w8_splitk(const W8Args& a) { return a.splitk > 0 ? a.splitk : w8_pick_splitk(a.N, a.K); }

int linear_w8_launch(const W8Args& a, hipStream_t s) {
  GILL_REQUIRE(a.A && a.W8 && a.scale, "linear w8: null operand");
  GILL_REQUIRE(a.M >= 1 && a.M <= W8_MAX_ROWS, "linear w8: 1 .. W8_MAX_ROWS activation rows");
  GILL_REQUIRE(a.N > 0 && a.K > 0 && a.N % 64 == 0 && a.K % 64 == 0, "linear w8: N and K must be multiples of 64");
  GILL_REQUIRE(a.act == ACT_NONE || a.act == ACT_RELU, "linear w8: act is none or ReLU");
  W8Dev d;
  d.a = a;
  d.nkb = a.K / 64;
  d.sk = linear_w8_splitk(a);
  GILL_REQUIRE(d.sk >= 1 && d.sk <= d.nkb, "linear w8: more K slices than 64-wide K steps");
  const bool partials = d.sk > 1 || a.partials_only;
  if (partials) GILL_REQUIRE(a.ws && (size_t)d.sk * a.M * a.N <= a.ws_floats, "linear w8: the partials do not fit the workspace");
  if (!a.partials_only) GILL_REQUIRE(a.C, "linear w8: null output");
  static bool attr_set = false;
  if (!attr_set) {
    GILL_CHECK_HIP(hipFuncSetAttribute((const void*)linear_w8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, W8_SMEM));
    attr_set = true;
  }
  hipLaunchKernelGGL(linear_w8_kernel, dim3(a.N / (16 * W8_G), d.sk), dim3(W8_THREADS), W8_SMEM, s, d);
  GILL_CHECK_HIP(hipGetLastError());
  if (partials && !a.partials_only) {
    hipLaunchKernelGGL(w8_finish_kernel, dim3(cdiv(a.M * (a.N / 4), 256)), dim3(256), 0, s, a.ws, d.sk, a.M, a.N, a.bias, a.resid, a.act, a.out_f32,
                       a.C);
    GILL_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------- load-time kernels
// element (n, k) of a bf16 matrix stored row-major or 64 x 64-blocked (convert_to_bf16_blk64_launch)
__device__ __forceinline__ size_t w8_src_index(int n, int k, int K, int blk) {
  return blk ? ((size_t)(n >> 6) * (K >> 6) + (k >> 6)) * 4096 + (size_t)(n & 63) * 64 + (k & 63) : (size_t)n * K + k;
}
// byte (n, k) of the kernel's order, k a multiple of 16
__device__ __forceinline__ size_t w8_dst_index(int n, int k, int K) {
  return ((size_t)(n >> 4) * (K >> 6) + (k >> 6)) * 1024 + (size_t)((((k & 63) >> 4) * 16) + (n & 15)) * 16;
}

// Quantiser: one workgroup per output row.  s = 2^e, e = ceil(log2(max|w| / 448)) from the exponent and mantissa of the maximum (no
// logarithm: max = f 2^p with f in [0.5, 1) gives e = p - 9 for f <= 0.875 = 448 / 512 and p - 8 above), so max|w / s| lies in (224, 448];
// an all-zero (or non-finite) row gets s = 1, and e is kept >= -100 so that s and 1 / s are normal fp32 numbers.  w / s is exact in fp32; the
// e4m3 rounding is the conversion instruction's round-to-nearest-even.  A maximum is the same in any order: deterministic.
__global__ __launch_bounds__(256) void w8_quant_kernel(const bf16_t* __restrict__ wsrc, int blk, int K, unsigned char* __restrict__ w8,
                                                       float* __restrict__ scale) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  float mx = 0.f;
  for (int k = tid * 8; k < K; k += 256 * 8) {
    const uint4 u = *reinterpret_cast<const uint4*>(wsrc + w8_src_index(n, k, K, blk));
    const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmaxf(mx, fmaxf(fabsf(bf2f((bf16_t)(uu[i] & 0xffff))), fabsf(bf2f((bf16_t)(uu[i] >> 16)))));
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  const float amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = 0;
  if (amax > 0.f && amax < __builtin_inff()) {
    int pw;
    const float f = frexpf(amax, &pw);
    e = f <= 0.875f ? pw - 9 : pw - 8;
    if (e < -100) e = -100;
  }
  const float inv = ldexpf(1.f, -e);
  if (tid == 0) scale[n] = ldexpf(1.f, e);
  for (int k = tid * 16; k < K; k += 256 * 16) {
    const bf16_t* src = wsrc + w8_src_index(n, k, K, blk);
    const uint4 u0 = *reinterpret_cast<const uint4*>(src), u1 = *reinterpret_cast<const uint4*>(src + 8);
    const uint32_t uu[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v0 = clamp_fp8_keep_nan(bf2f((bf16_t)(uu[2 * i] & 0xffff)) * inv), v1 = clamp_fp8_keep_nan(bf2f((bf16_t)(uu[2 * i] >> 16)) * inv);
      const float v2 = clamp_fp8_keep_nan(bf2f((bf16_t)(uu[2 * i + 1] & 0xffff)) * inv);
      const float v3 = clamp_fp8_keep_nan(bf2f((bf16_t)(uu[2 * i + 1] >> 16)) * inv);
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(v2, v3, pk, true);
      o[i] = (uint32_t)pk;
    }
    *reinterpret_cast<uint4*>(w8 + w8_dst_index(n, k, K)) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
int w8_quant_launch(const bf16_t* w, int blk, int N, int K, unsigned char* w8, float* scale, hipStream_t s) {
  GILL_REQUIRE(w && w8 && scale, "w8 quantiser: null operand");
  GILL_REQUIRE(N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, "w8 quantiser: N and K must be multiples of 64");
  hipLaunchKernelGGL(w8_quant_kernel, dim3(N), dim3(256), 0, s, w, blk, K, w8, scale);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

// Dequantiser: the same bytes -> bf16 [N][K], row-major or 64 x 64-blocked; every value w8 * s, exact in bf16.  One 16-byte piece per thread.
__global__ __launch_bounds__(256) void w8_dequant_kernel(const unsigned char* __restrict__ w8, const float* __restrict__ scale, int N, int K, int blk,
                                                         bf16_t* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)N * K / 16) return;
  const int nkb = K >> 6;
  const int lane = (int)(idx & 63);
  const int64_t chunk = idx >> 6;
  const int n = (int)(chunk / nkb) * 16 + (lane & 15), k = (int)(chunk % nkb) * 64 + (lane >> 4) * 16;
  const uint4 u = *reinterpret_cast<const uint4*>(w8 + idx * 16);
  const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
  const float sc = scale[n];
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const w8_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)uu[i], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)uu[i], true);
    o[2 * i] = pack_bf2(a[0] * sc, a[1] * sc);
    o[2 * i + 1] = pack_bf2(b[0] * sc, b[1] * sc);
  }
  bf16_t* dst = out + w8_src_index(n, k, K, blk);
  *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<uint4*>(dst + 8) = make_uint4(o[4], o[5], o[6], o[7]);
}
int w8_dequant_launch(const unsigned char* w8, const float* scale, int N, int K, int blk, bf16_t* out, hipStream_t s) {
  GILL_REQUIRE(w8 && scale && out, "w8 dequantiser: null operand");
  GILL_REQUIRE(N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, "w8 dequantiser: N and K must be multiples of 64");
  hipLaunchKernelGGL(w8_dequant_kernel, dim3((unsigned)cdiv64((int64_t)N * K / 16, 256)), dim3(256), 0, s, w8, scale, N, K, blk, out);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
