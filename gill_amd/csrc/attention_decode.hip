// Decode attention with append for gfx950: one new token per sequence, every sequence at its own cache length (AttnDecodeArgs in ops.h).
//
// The step is a read of the (b, h) pair's K and V^T up to its length and nothing else: ~2 flops per byte, memory-bound, so there is no MFMA and no LDS
// staging here.  One workgroup of four waves per (b, h):
//   1. scores.  K rows are dp contiguous bf16; LPK lanes share a key, each taking 16-byte chunks of the row straight into VGPRs (q is held scaled, in
//      fp32, in the same lanes), the four waves take interleaved blocks of 64 / LPK keys, UNROLL blocks in flight.  The new key comes from the input
//      row, never from the slot it is stored to.  Scores go to LDS (log2 domain).
//   2. softmax over the n + 1 scores in LDS: maximum, exp2, sum.
//   3. P V.  V^T rows are keys-contiguous: a lane takes 8 keys of a row with one 16-byte load, the wave covers 512 keys per pass, each wave owns
//      dp / 4 rows of the head.  The new value comes from the input row.
//   4. the appended K row, V^T column (and the ones-row entry the flash kernel expects where dpv > dp) are stored; O as bf16, token-major.
// Keys beyond the length are excluded by SELECTION: their scores are never formed, and the tail of the last 8-key chunk of V^T is selected out of
// the sum term by term, so whatever finite or non-finite bits a slot holds cannot reach the output.  Every 16-byte load lies inside the pitch
// (pitch % 32 == 0, chunk starts below the clamped length).
// Fixed function: every reduction has a fixed order (a lane's own terms in index order, xor trees over lanes, the four waves in index order), there
// are no atomics, and nothing depends on B, on another row's length or on the order workgroups run in: the same (b, h) data gives the same bits.
#include "ops.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / 64;

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

template <int DP, int LPK>
__global__ __launch_bounds__(kDecThreads) void attention_decode_kernel(const AttnDecodeArgs p) {
  constexpr int CH = DP / 8;            // 16-byte chunks of a key row
  constexpr int CPL = CH / LPK;         // chunks per lane
  constexpr int KPW = 64 / LPK;         // keys per wave pass
  constexpr int UNROLL = 4;
  constexpr int RPW = DP / kDecWaves;   // V^T rows per wave
  constexpr int RB = RPW % 8 == 0 ? 8 : RPW % 5 == 0 ? 5 : 4;     // rows whose loads are in flight together
  static_assert(CH % LPK == 0 && DP % kDecWaves == 0 && RPW % RB == 0, "decode attention geometry");
  extern __shared__ __attribute__((aligned(16))) float dec_sc[];     // [pitch + 8]: scores, then probabilities
  __shared__ float red[2 * kDecWaves];
  __shared__ float ob[DP];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  int n = p.lens[b];
  const bool clamped = n < 0 || n > p.pitch - 1;
  n = n < 0 ? 0 : (n > p.pitch - 1 ? p.pitch - 1 : n);
  if (clamped && p.flags && h == 0 && tid == 0) p.flags[b] = 1;

  const bf16_t* qrow = p.q + (size_t)b * p.ld + h * DP;
  const bf16_t* knew = p.k + (size_t)b * p.ld + h * DP;
  const bf16_t* vnew = p.v + (size_t)b * p.ld + h * DP;
  bf16_t* Kb = p.K + (size_t)(b * p.H + h) * p.pitch * DP;
  bf16_t* Vb = p.Vt + (size_t)(b * p.H + h) * p.dpv * p.pitch;

  // ---- 1. scores
  const int sub = lane % LPK, kl = lane / LPK;
  float qf[CPL][8];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(qrow + (i * LPK + sub) * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qf[i][2 * e] = bf_lo(u[e]) * p.qscale;
      qf[i][2 * e + 1] = bf_hi(u[e]) * p.qscale;
    }
  }
  for (int j0 = w * KPW; j0 <= n; j0 += kDecWaves * KPW * UNROLL) {
    u32x4 kr[UNROLL][CPL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = j0 + u * kDecWaves * KPW + kl;
      const bf16_t* src = j < n ? Kb + (size_t)j * DP : knew;       // j == n: the new key; j > n: loaded again, never used
#pragma unroll
      for (int i = 0; i < CPL; ++i) kr[u][i] = *reinterpret_cast<const u32x4*>(src + (i * LPK + sub) * 8);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = j0 + u * kDecWaves * KPW + kl;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s = fmaf(qf[i][2 * e], bf_lo(kr[u][i][e]), s);
          s = fmaf(qf[i][2 * e + 1], bf_hi(kr[u][i][e]), s);
        }
#pragma unroll
      for (int o = LPK / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (sub == 0 && j <= n) dec_sc[j] = s;
    }
  }
  __syncthreads();

  // ---- 2. softmax over scores 0 .. n
  float m = -INFINITY;
  for (int j = tid; j <= n; j += kDecThreads) m = fmaxf(m, dec_sc[j]);
  m = wave_max(m);
  if (lane == 0) red[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float l = 0.f;
  for (int j = tid; j <= n; j += kDecThreads) {
    const float e = __builtin_amdgcn_exp2f(dec_sc[j] - m);
    dec_sc[j] = e;
    l += e;
  }
  l = wave_sum(l);
  if (lane == 0) red[kDecWaves + w] = l;
  __syncthreads();
  l = (red[kDecWaves] + red[kDecWaves + 1]) + (red[kDecWaves + 2] + red[kDecWaves + 3]);
  const float pn = dec_sc[n];

  // ---- 3. P V over the cached keys 0 .. n - 1: wave w owns rows w, w + 4, ...
  float acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
  const int nch = (n + 7) >> 3;
  for (int c0 = 0; c0 < nch; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = c < nch;
    const int j8 = ok ? c * 8 : 0;      // chunk start: j8 < n <= pitch - 1 and pitch % 8 == 0, so j8 + 7 < pitch
    const float4 p0 = *reinterpret_cast<const float4*>(dec_sc + j8);
    const float4 p1 = *reinterpret_cast<const float4*>(dec_sc + j8 + 4);
    const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
    bool sel[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sel[e] = ok && j8 + e < n;
#pragma unroll
    for (int rb = 0; rb < RPW; rb += RB) {
      u32x4 vr[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) vr[r] = *reinterpret_cast<const u32x4*>(Vb + (size_t)(w + kDecWaves * (rb + r)) * p.pitch + j8);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        float a = acc[rb + r];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t0 = fmaf(pv[2 * e], bf_lo(vr[r][e]), a);
          a = sel[2 * e] ? t0 : a;
          const float t1 = fmaf(pv[2 * e + 1], bf_hi(vr[r][e]), a);
          a = sel[2 * e + 1] ? t1 : a;
        }
        acc[rb + r] = a;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const float a = wave_sum(acc[r]);
    if (lane == 0) ob[w + kDecWaves * r] = a;
  }
  __syncthreads();

  // ---- 4. output and append
  if (tid < DP / 2) {
    const uint32_t vv = *reinterpret_cast<const uint32_t*>(vnew + 2 * tid);
    const float o0 = fmaf(pn, bf_lo(vv), ob[2 * tid]) / l;
    const float o1 = fmaf(pn, bf_hi(vv), ob[2 * tid + 1]) / l;
    *reinterpret_cast<uint32_t*>(p.O + (size_t)b * p.ldo + h * DP + 2 * tid) = pack_bf2(o0, o1);
  }
  if (tid >= 64 && tid < 64 + CH)
    *reinterpret_cast<u32x4*>(Kb + (size_t)n * DP + (tid - 64) * 8) = *reinterpret_cast<const u32x4*>(knew + (tid - 64) * 8);
  if (tid >= 128 && tid < 128 + DP) Vb[(size_t)(tid - 128) * p.pitch + n] = vnew[tid - 128];
  if (tid == 0 && p.dpv > DP) Vb[(size_t)DP * p.pitch + n] = (bf16_t)0x3F80;
}

template <int DP, int LPK>
int launch_dp(const AttnDecodeArgs& a, hipStream_t s) {
  const size_t smem = sizeof(float) * (size_t)(a.pitch + 8);
  hipLaunchKernelGGL((attention_decode_kernel<DP, LPK>), dim3(a.B * a.H), dim3(kDecThreads), smem, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_decode_launch(const AttnDecodeArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K && a.Vt && a.lens && a.O, "decode attention: null argument");
  GILL_REQUIRE(a.B > 0 && a.H > 0, "decode attention: empty batch");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "decode attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "decode attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 2 == 0 && a.ldo >= a.H * a.dp, "decode attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K | (uintptr_t)a.Vt) % 16 == 0 && (uintptr_t)a.O % 4 == 0,
               "decode attention: operands must be 16-byte aligned");
  switch (a.dp) {
    case 64:  return launch_dp<64, 8>(a, s);
    case 80:  return launch_dp<80, 2>(a, s);
    case 128: return launch_dp<128, 8>(a, s);
    default:
      gill_set_error("decode attention: unsupported head dim (supported: 64, 80, 128)");
      return -2;
  }
}
