// The body attention_decode.hip and attention_append.hip share: one query token of one (b, h) pair against that pair's cache, with append.
// One workgroup of four waves runs it; every reduction has a fixed order, so the same operands give the same bits from either kernel.
// BLOCK (the append kernel): the token is number n - n0 of a block of consecutive new tokens whose first one sits at slot n0.  The keys and values
// of the block's earlier tokens (slots n0 .. n - 1) are then taken from their INPUT rows (krow0 / vrow0 + t * ld for token t), not from the slots
// other workgroups are storing them to: the same bf16 values enter the same sums at the same places, so the bits are those of the single-token
// kernel run on a cache that already holds them, with no ordering between the tokens of a block.
#pragma once
#include "ops.h"

namespace attn_dec {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / 64;

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// qrow / knew / vnew: the token's head slices (DP bf16, 16-byte aligned); Kb [pitch][DP] and Vb [dpv][pitch]: the pair's cache; n: the token's
// slot, 0 <= n <= pitch - 1 (the caller has clamped it); orow: DP bf16 of output.  dec_sc [pitch + 8], red [2 * kDecWaves], ob [DP]: LDS.
// BLOCK only: n0 <= n, n - n0 <= kBlockMax - 1; krow0 / vrow0: the head slices of the block's first token, rows ld elements apart;
// vblk [kBlockMax * DP] bf16: LDS.
constexpr int kBlockMax = 16;
template <int DP, int LPK, bool BLOCK = false>
__device__ __forceinline__ void decode_token(const bf16_t* qrow, const bf16_t* knew, const bf16_t* vnew, bf16_t* Kb, bf16_t* Vb, bf16_t* orow,
                                             int n, int pitch, int dpv, float qscale, float* dec_sc, float* red, float* ob, int n0 = 0,
                                             const bf16_t* krow0 = nullptr, const bf16_t* vrow0 = nullptr, int ld = 0, bf16_t* vblk = nullptr) {
  constexpr int CH = DP / 8;            // 16-byte chunks of a key row
  constexpr int CPL = CH / LPK;         // chunks per lane
  constexpr int KPW = 64 / LPK;         // keys per wave pass
  constexpr int UNROLL = 4;
  constexpr int RPW = DP / kDecWaves;   // V^T rows per wave
  constexpr int RB = RPW % 8 == 0 ? 8 : RPW % 5 == 0 ? 5 : 4;     // rows whose loads are in flight together
  static_assert(CH % LPK == 0 && DP % kDecWaves == 0 && RPW % RB == 0, "decode attention geometry");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

  if constexpr (BLOCK) {      // the value rows of the block's earlier tokens -> LDS (visible behind the barrier that ends step 1)
    for (int c = tid; c < (n - n0) * CH; c += kDecThreads) {
      const int t = c / CH, cc = c - t * CH;
      *reinterpret_cast<u32x4*>(vblk + t * DP + cc * 8) = *reinterpret_cast<const u32x4*>(vrow0 + (size_t)t * ld + cc * 8);
    }
  }

  // ---- 1. scores
  const int sub = lane % LPK, kl = lane / LPK;
  float qf[CPL][8];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(qrow + (i * LPK + sub) * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qf[i][2 * e] = bf_lo(u[e]) * qscale;
      qf[i][2 * e + 1] = bf_hi(u[e]) * qscale;
    }
  }
  for (int j0 = w * KPW; j0 <= n; j0 += kDecWaves * KPW * UNROLL) {
    u32x4 kr[UNROLL][CPL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = j0 + u * kDecWaves * KPW + kl;
      const bf16_t* src = j < n ? Kb + (size_t)j * DP : knew;       // j == n: the new key; j > n: loaded again, never used
      if constexpr (BLOCK) {
        if (j >= n0 && j < n) src = krow0 + (size_t)(j - n0) * ld;    // an earlier token of the block: its input row
      }
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
      for (int r = 0; r < RB; ++r) vr[r] = *reinterpret_cast<const u32x4*>(Vb + (size_t)(w + kDecWaves * (rb + r)) * pitch + j8);
      if constexpr (BLOCK) {
        if (ok && j8 + 8 > n0) {      // the chunk reaches into the block: those keys' values from LDS in the place of what the slots hold
#pragma unroll
          for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int j = j8 + e;
              if (j >= n0 && j < n) {
                const uint32_t val = vblk[(j - n0) * DP + w + kDecWaves * (rb + r)];
                const uint32_t old = vr[r][e >> 1];
                vr[r][e >> 1] = (e & 1) ? ((old & 0xffffu) | (val << 16)) : ((old & 0xffff0000u) | val);
              }
            }
        }
      }
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
    *reinterpret_cast<uint32_t*>(orow + 2 * tid) = pack_bf2(o0, o1);
  }
  if (tid >= 64 && tid < 64 + CH)
    *reinterpret_cast<u32x4*>(Kb + (size_t)n * DP + (tid - 64) * 8) = *reinterpret_cast<const u32x4*>(knew + (tid - 64) * 8);
  if (tid >= 128 && tid < 128 + DP) Vb[(size_t)(tid - 128) * pitch + n] = vnew[tid - 128];
  if (tid == 0 && dpv > DP) Vb[(size_t)DP * pitch + n] = (bf16_t)0x3F80;
}

}  // namespace attn_dec
