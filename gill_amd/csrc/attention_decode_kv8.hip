// Decode attention with append on an e4m3 KV cache for gfx950 (AttnDecodeKv8Args in ops.h; the format: attention_kv8_dev.h): the sibling of
// attention_decode.hip, one new token per sequence, every sequence at its own cache length.  The step is a read of the (b, h) pair's K8 and Vt8
// bytes and their exponents up to its length and nothing else; no MFMA, no LDS staging.  One workgroup of four waves per (b, h), the four steps
// of attn_dec::decode_token with one in front:
//   0. the new key and value rows are quantised in the workgroup (wave 0 the key, wave 1 the value: row maximum over the dp elements by an xor
//      tree, the exponent, the codes): bytes, exponents and the codes as fp32 go to LDS.  Everything after this uses the QUANTISED token.
//   1. scores.  K8 rows are dp contiguous bytes; LPK lanes share a key, a lane's 16-byte load covers 16 elements, converted to fp32 by
//      cvt_pk_f32_fp8 (exact); q is held scaled, in fp32, in the same lanes.  The key's scale 2^e multiplies the FINISHED score (exact).  The
//      four waves take interleaved blocks of 64 / LPK keys, UNROLL blocks in flight.  The new key's score comes from its codes in LDS (wave 0).
//   2. softmax over the n + 1 scores in LDS: maximum, exp2, sum; behind the sum each probability takes its value's scale 2^e (exact).
//   3. P V.  Vt8 rows are keys-contiguous: a lane takes 16 keys of a row with one 16-byte load, the wave covers 1024 keys per pass, each wave
//      owns dp / 4 rows of the head.
//   4. O as bf16, token-major (the new value's term from its codes); the appended K8 row, Vt8 column and the two exponents are stored.
// Keys beyond the length are excluded by SELECTION: their scores are never formed, their exponents never enter a kept number, and the tail of
// the last 16-key chunk of Vt8 is selected out of the sum term by term, so no byte pattern of a stale slot (the NaN codes included) and no
// stale exponent can reach the output.  Every load lies inside the pair's slab (pitch % 32 == 0, chunk starts below the clamped length; a key
// index beyond the length reads slot n of the slab, which is never used).
// Fixed function: every reduction has a fixed order (a lane's own terms in index order, xor trees over lanes, the four waves in index order),
// there are no atomics, and nothing depends on B, on another row's length or on the order workgroups run in: the same (b, h) data gives the
// same output and cache bits.
#include "attention_kv8_dev.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

template <int DP, int LPK>
__global__ __launch_bounds__(kThreads) void attention_decode_kv8_kernel(const AttnDecodeKv8Args p) {
  extern __shared__ __attribute__((aligned(16))) float dec_sc[];     // [pitch + 8]: scores, then probabilities (value scale folded in)
  __shared__ float red[2 * kWaves];
  __shared__ float ob[DP];
  __shared__ float kc[DP], vc[DP];                                    // the new key's and value's codes as fp32
  __shared__ __attribute__((aligned(16))) uint8_t kb8[DP];
  __shared__ __attribute__((aligned(16))) uint8_t vb8[DP];
  __shared__ int ex[2];                                               // their exponents
  constexpr int CH = DP / 16;           // 16-byte chunks of a key row
  constexpr int CPL = CH / LPK;         // chunks per lane
  constexpr int KPW = 64 / LPK;         // keys per wave pass
  constexpr int UNROLL = CPL > 2 ? 2 : 4;
  constexpr int RPW = DP / kWaves;      // Vt8 rows per wave
  constexpr int RB = RPW % 8 == 0 ? 8 : RPW % 5 == 0 ? 5 : 4;     // rows whose loads are in flight together
  static_assert(CH % LPK == 0 && DP % 16 == 0 && DP % kWaves == 0 && RPW % RB == 0 && DP / 2 <= 64, "kv8 decode attention geometry");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  int n = p.lens[b];
  const bool clamped = n < 0 || n > p.pitch - 1;
  n = n < 0 ? 0 : (n > p.pitch - 1 ? p.pitch - 1 : n);
  if (clamped && p.flags && h == 0 && tid == 0) p.flags[b] = 1;
  const int pitch = p.pitch;

  const size_t in = (size_t)b * p.ld + h * DP;
  const bf16_t* qrow = p.q + in;
  const bf16_t* knew = p.k + in;
  const bf16_t* vnew = p.v + in;
  const size_t pair = (size_t)(b * p.H + h);
  uint8_t* Kb = p.K8 + pair * pitch * DP;
  uint8_t* Vb = p.Vt8 + pair * p.dpv * pitch;
  int8_t* Ke = p.Kexp + pair * pitch;
  int8_t* Ve = p.Vexp + pair * pitch;
  bf16_t* orow = p.O + (size_t)b * p.ldo + h * DP;

  // ---- 0. the token's own rows -> codes
  if (w < 2) {
    const bf16_t* src = w == 0 ? knew : vnew;
    const uint32_t u = lane < DP / 2 ? *reinterpret_cast<const uint32_t*>(src + 2 * lane) : 0u;
    const int e = kv8::row_exp(wave_max(kv8::amax2(u)));
    if (lane < DP / 2) {
      const uint32_t c = kv8::quant2(u, kv8::pow2(-e));
      *reinterpret_cast<uint16_t*>((w == 0 ? kb8 : vb8) + 2 * lane) = (uint16_t)c;
      const kv8::f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, false);
      float* dst = w == 0 ? kc : vc;
      dst[2 * lane] = f[0];
      dst[2 * lane + 1] = f[1];
    }
    if (lane == 0) ex[w] = e;
  }
  __syncthreads();

  // ---- 1. scores of the cached keys 0 .. n - 1
  const int sub = lane % LPK, kl = lane / LPK;
  float qf[CPL][16];
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const u32x4 u = *reinterpret_cast<const u32x4*>(qrow + (i * LPK + sub) * 16 + hf * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[i][hf * 8 + 2 * e] = bf_lo(u[e]) * p.qscale;
        qf[i][hf * 8 + 2 * e + 1] = bf_hi(u[e]) * p.qscale;
      }
    }
  for (int j0 = w * KPW; j0 < n; j0 += kWaves * KPW * UNROLL) {
    u32x4 kr[UNROLL][CPL];
    int ke[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = j0 + u * kWaves * KPW + kl;
      const int jj = j < n ? j : n;                     // j >= n: slot n of the slab, loaded, never used
      const uint8_t* src = Kb + (size_t)jj * DP;
#pragma unroll
      for (int i = 0; i < CPL; ++i) kr[u][i] = *reinterpret_cast<const u32x4*>(src + (i * LPK + sub) * 16);
      ke[u] = Ke[jj];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = j0 + u * kWaves * KPW + kl;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
          float f[4];
          kv8::cvt4f(kr[u][i][wd], f);
#pragma unroll
          for (int t = 0; t < 4; ++t) s = fmaf(qf[i][4 * wd + t], f[t], s);
        }
#pragma unroll
      for (int o = LPK / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (sub == 0 && j < n) dec_sc[j] = s * kv8::pow2(ke[u]);
    }
  }
  if (w == 0) {      // the token's own score, from its codes
    float s = 0.f;
    if (lane < DP / 2) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(qrow + 2 * lane);
      s = (bf_lo(u) * p.qscale) * kc[2 * lane];
      s = fmaf(bf_hi(u) * p.qscale, kc[2 * lane + 1], s);
    }
    s = wave_sum(s);
    if (lane == 0) dec_sc[n] = s * kv8::pow2(ex[0]);
  }
  __syncthreads();

  // ---- 2. softmax over scores 0 .. n; the value scales go into the probabilities behind the sum
  float m = -INFINITY;
  for (int j = tid; j <= n; j += kThreads) m = fmaxf(m, dec_sc[j]);
  m = wave_max(m);
  if (lane == 0) red[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float l = 0.f;
  for (int j = tid; j <= n; j += kThreads) {
    const float e = __builtin_amdgcn_exp2f(dec_sc[j] - m);
    l += e;
    dec_sc[j] = e * kv8::pow2(j < n ? (int)Ve[j] : ex[1]);
  }
  l = wave_sum(l);
  if (lane == 0) red[kWaves + w] = l;
  __syncthreads();
  l = (red[kWaves] + red[kWaves + 1]) + (red[kWaves + 2] + red[kWaves + 3]);
  const float pn = dec_sc[n];

  // ---- 3. P V over the cached keys 0 .. n - 1: wave w owns rows w, w + 4, ...
  float acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
  const int nch = (n + 15) >> 4;
  for (int c0 = 0; c0 < nch; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = c < nch;
    const int j16 = ok ? c * 16 : 0;      // chunk start: j16 < n <= pitch - 1 and pitch % 16 == 0, so j16 + 15 < pitch
    float pv[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 p4 = *reinterpret_cast<const float4*>(dec_sc + j16 + 4 * g);
      pv[4 * g] = p4.x; pv[4 * g + 1] = p4.y; pv[4 * g + 2] = p4.z; pv[4 * g + 3] = p4.w;
    }
    bool sel[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) sel[e] = ok && j16 + e < n;
#pragma unroll
    for (int rb = 0; rb < RPW; rb += RB) {
      u32x4 vr[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) vr[r] = *reinterpret_cast<const u32x4*>(Vb + (size_t)(w + kWaves * (rb + r)) * pitch + j16);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        float a = acc[rb + r];
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
          float f[4];
          kv8::cvt4f(vr[r][wd], f);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float t0 = fmaf(pv[4 * wd + t], f[t], a);
            a = sel[4 * wd + t] ? t0 : a;
          }
        }
        acc[rb + r] = a;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const float a = wave_sum(acc[r]);
    if (lane == 0) ob[w + kWaves * r] = a;
  }
  __syncthreads();

  // ---- 4. output and append
  if (tid < DP / 2) {
    const float o0 = fmaf(pn, vc[2 * tid], ob[2 * tid]) / l;
    const float o1 = fmaf(pn, vc[2 * tid + 1], ob[2 * tid + 1]) / l;
    *reinterpret_cast<uint32_t*>(orow + 2 * tid) = pack_bf2(o0, o1);
  }
  if (tid >= 64 && tid < 64 + CH) *reinterpret_cast<u32x4*>(Kb + (size_t)n * DP + (tid - 64) * 16) = *reinterpret_cast<const u32x4*>(kb8 + (tid - 64) * 16);
  if (tid >= 128 && tid < 128 + DP) Vb[(size_t)(tid - 128) * pitch + n] = vb8[tid - 128];
  if (tid == 0) Ke[n] = (int8_t)ex[0];
  if (tid == 1) Ve[n] = (int8_t)ex[1];
}

template <int DP, int LPK>
int launch_dp(const AttnDecodeKv8Args& a, hipStream_t s) {
  const size_t smem = sizeof(float) * (size_t)(a.pitch + 8);
  hipLaunchKernelGGL((attention_decode_kv8_kernel<DP, LPK>), dim3(a.B * a.H), dim3(kThreads), smem, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_decode_kv8_launch(const AttnDecodeKv8Args& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K8 && a.Vt8 && a.Kexp && a.Vexp && a.lens && a.O, "kv8 decode attention: null argument");
  GILL_REQUIRE(a.B > 0 && a.H > 0, "kv8 decode attention: empty batch");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "kv8 decode attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "kv8 decode attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 2 == 0 && a.ldo >= a.H * a.dp, "kv8 decode attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K8 | (uintptr_t)a.Vt8) % 16 == 0 && (uintptr_t)a.O % 4 == 0,
               "kv8 decode attention: operands must be 16-byte aligned");
  switch (a.dp) {
    case 64:  return launch_dp<64, 4>(a, s);
    case 80:  return launch_dp<80, 1>(a, s);
    case 128: return launch_dp<128, 8>(a, s);
    default:
      gill_set_error("kv8 decode attention: unsupported head dim (supported: 64, 80, 128)");
      return -2;
  }
}
