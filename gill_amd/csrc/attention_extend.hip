// Ragged multi-token attention with append for gfx950 (AttnExtendArgs in ops.h): row b brings cnt = cu_new[b + 1] - cu_new[b] consecutive new tokens
// (any count, zero included) at its own cache length n = lens[b]; packed row cu_new[b] + i is token n + i of sequence b.  Token i's key / value go to
// slot n + i, and it attends to the slots 0 .. n + i.  With dozens to hundreds of query rows per (b, h) this is matmul-shaped work, so unlike
// attention_append.hip (one workgroup per token, no MFMA, at most 16 tokens) it is the flash pattern of attention.hip on the cache layout.
//
// Two launches on the stream:
//   1. attention_extend_store_kernel: one workgroup per (64-token tile, h, b) copies the tile's k rows into K[b][h][n + i][:] (16-byte chunks,
//      destination contiguous), its v rows into the columns n + i of Vt[b][h][:][.] (lanes along the tokens: consecutive slots) and, where
//      dpv > dp, the ones-row entry Vt[b][h][dp][n + i] = 1 that the flash kernel's row sum and the decode kernels' cache contract expect.
//   2. attention_extend_kernel: every key of a row, old or new, is then in the cache, and no slot is read in the kernel that stores it.
//      Grid (ceil(max_new / 128), H, B), four waves per workgroup, each wave 32 consecutive queries of one (b, h); a wave whose queries lie
//      beyond the row's count leaves at once.  The waves are independent: no LDS, no barrier.  Keys are walked in tiles of 32 (the pitch is a
//      multiple of 32, so a tile that starts inside the row's keys lies inside the pitch), in order from slot 0:
//        S^T[kv][q] = sum_d K[kv][d] q[q][d]        v_mfma_f32_32x32x16_bf16, A = a K fragment read straight from the cache row (16 bytes per lane),
//                                                   B = the q fragment held in registers (unscaled bf16, as projected)
//        s = S^T * log2(e) / sqrt(d) in fp32, keys beyond n + i SELECTED to -inf, online softmax (running max and sum in fp32, one xor-32
//        shuffle joins the two half waves that share a query)
//        O^T[d][q] += sum_kv Vt[d][kv] P[q][kv]     the S^T accumulator registers are, as they are, the k-slots of the B operand provided the
//                                                   Vt fragment is gathered with the permutation kv = 16 h4 + 8 (j >> 2) + 4 hi + (j & 3): two
//                                                   8-byte reads of the cache row per lane and MFMA
//      K and V^T are not staged: a (b, h) pair's cache is read by at most ceil(cnt / 32) waves and stays in L2 between them.  The kernel is bound by
//      those fragment reads (the V^T ones are 8 bytes per lane at a stride of the pitch), not by the matrix pipe; no throughput is claimed for it.
// Exclusion is by selection: a score of a slot beyond n + i is replaced by -inf whatever the MFMA made of the slot's bits, and in the tile that
// straddles n + cnt the V^T elements of slots at or beyond n + cnt are replaced by zeros before they meet their (zero) probabilities, so no
// finite or non-finite stale value can reach the output.  (Slots n + i + 1 .. n + cnt - 1 hold this launch's own finite values.)
// Fixed function: a query's tiles come in index order, its reductions are its own lanes' (a tile that only other queries of the wave can see
// contributes exact zeros and a rescale by exactly 1), there are no atomics, and query tiles are counted from the row's own first token: the same
// operands, length and count give the same output and cache bits at any B, anywhere in the pack, next to any other rows.
// Lengths and counts are read on the device and never trusted: n is clamped into [0, pitch - cnt] (flags[b] = 1), a count outside [0, max_new]
// or a row range outside [0, total_new) makes the row empty (flags[b] = 1); nothing outside the buffers is touched.
#include "ops.h"

namespace {

constexpr int kExtThreads = 256;
constexpr int kExtQB = 128;       // queries per workgroup: 32 per wave
constexpr int kExtStoreTok = 64;  // tokens per workgroup of the store kernel

struct ExtRow { int r0, cnt, n; bool flag; };

// the row's packed range, count and clamped length, the same in both kernels
__device__ __forceinline__ ExtRow ext_row(const AttnExtendArgs& p, int b) {
  ExtRow r;
  r.r0 = p.cu_new[b];
  r.cnt = p.cu_new[b + 1] - r.r0;
  r.flag = false;
  if (r.cnt < 0 || r.cnt > p.max_new || r.r0 < 0 || (int64_t)r.r0 + r.cnt > p.total_new) { r.cnt = 0; r.r0 = 0; r.flag = true; }
  const int top = p.pitch - r.cnt;      // >= 0: max_new <= pitch is checked by the launcher
  r.n = p.lens[b];
  if (r.n < 0 || r.n > top) { r.flag = true; r.n = r.n < 0 ? 0 : top; }
  return r;
}

template <int DP>
__global__ __launch_bounds__(kExtThreads) void attention_extend_store_kernel(const AttnExtendArgs p) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
  const int tid = threadIdx.x;
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * kExtStoreTok;
  const ExtRow r = ext_row(p, b);
  if (r.flag && p.flags && h == 0 && blockIdx.x == 0 && tid == 0) p.flags[b] = 1;
  if (i0 >= r.cnt) return;
  const int nt = r.cnt - i0 < kExtStoreTok ? r.cnt - i0 : kExtStoreTok;
  const size_t in0 = (size_t)(r.r0 + i0) * p.ld + h * DP;
  bf16_t* Kb = p.K + ((size_t)(b * p.H + h) * p.pitch + r.n + i0) * DP;
  bf16_t* Vb = p.Vt + (size_t)(b * p.H + h) * p.dpv * p.pitch + r.n + i0;
  constexpr int CH = DP / 8;
  for (int c = tid; c < nt * CH; c += kExtThreads) {
    const int t = c / CH, cc = c - t * CH;
    *reinterpret_cast<u32x4*>(Kb + (size_t)t * DP + cc * 8) = *reinterpret_cast<const u32x4*>(p.k + in0 + (size_t)t * p.ld + cc * 8);
  }
  const int t = tid & 63, g = tid >> 6;
  if (t < nt) {
    const bf16_t* vrow = p.v + in0 + (size_t)t * p.ld;
    for (int d = g; d < DP; d += kExtThreads / 64) Vb[(size_t)d * p.pitch + t] = vrow[d];
    if (g == 0 && p.dpv > DP) Vb[(size_t)DP * p.pitch + t] = (bf16_t)0x3F80;
  }
}

template <int DP>
__global__ __launch_bounds__(kExtThreads) void attention_extend_kernel(const AttnExtendArgs p) {
  constexpr int KS = DP / 16;             // QK^T k-steps
  constexpr int NDT = (DP + 31) / 32;     // 32-row tiles of O^T
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const ExtRow r = ext_row(p, b);
  const int q0 = blockIdx.x * kExtQB + w * 32;
  if (q0 >= r.cnt) return;
  const int lq = lane & 31, hi = lane >> 5;
  const bool qvalid = q0 + lq < r.cnt;
  const int qi = qvalid ? q0 + lq : r.cnt - 1;     // a lane beyond the count repeats the last query (never stored)
  const int qidx = r.n + qi;                       // the newest slot this query sees
  const int nkv = r.n + r.cnt;                     // slots that hold data: 1 <= nkv <= pitch
  const int wave_end = min(nkv, r.n + q0 + 32);    // keys this wave can see at all

  const bf16_t* qrow = p.q + (size_t)(r.r0 + qi) * p.ld + h * DP;
  const bf16_t* Kb = p.K + (size_t)(b * p.H + h) * p.pitch * DP;
  const bf16_t* Vb = p.Vt + (size_t)(b * p.H + h) * p.dpv * p.pitch;

  bf16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qrow + s * 16 + hi * 8);

  f32x16 oacc[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[t][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  for (int kv0 = 0; kv0 < wave_end; kv0 += 32) {     // kv0 < nkv <= pitch and pitch % 32 == 0: the tile lies inside the pitch
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
    const bf16_t* krow = Kb + (size_t)(kv0 + lq) * DP + hi * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(krow + ks * 16);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
    }
    // register e of a lane is key kv0 + (e & 3) + 8 (e >> 2) + 4 hi of query lq
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kv = kv0 + (e & 3) + 8 * (e >> 2) + 4 * hi;
      s[e] = kv > qidx ? -INFINITY : s[e] * p.qscale;
      mx = fmaxf(mx, s[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // tile 0 holds slot 0, which every query sees: m_new is finite from the first tile on
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float rs = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = __builtin_amdgcn_exp2f(s[e] - m_new);
      rs += s[e];
    }
    rs += __shfl_xor(rs, 32, 64);
    l_run = l_run * alpha + rs;
#pragma unroll
    for (int t = 0; t < NDT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[t][e] *= alpha;

    bf16x8 pa[2];
#pragma unroll
    for (int h4 = 0; h4 < 2; ++h4) {
      union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
      for (int j = 0; j < 4; ++j) pk.u[j] = pack_bf2(s[h4 * 8 + 2 * j], s[h4 * 8 + 2 * j + 1]);
      pa[h4] = pk.v;
    }
    const bool tail = kv0 + 32 > nkv;      // the tile reaches into slots that hold no data (wave-uniform)
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
      const bf16_t* vrow = Vb + (size_t)(t * 32 + lq) * p.pitch + kv0 + 4 * hi;
#pragma unroll
      for (int h4 = 0; h4 < 2; ++h4) {
        union { bf16x8 v; uint2 u[2]; uint16_t e[8]; } vf;
        vf.u[0] = *reinterpret_cast<const uint2*>(vrow + 16 * h4);
        vf.u[1] = *reinterpret_cast<const uint2*>(vrow + 16 * h4 + 8);
        if (tail) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int kv = kv0 + 16 * h4 + 8 * (j >> 2) + 4 * hi + (j & 3);
            vf.e[j] = kv >= nkv ? (uint16_t)0 : vf.e[j];
          }
        }
        oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf.v, pa[h4], oacc[t], 0, 0, 0);
      }
    }
  }

  if (!qvalid) return;
  const float inv = 1.f / l_run;
  bf16_t* orow = p.O + (size_t)(r.r0 + qi) * p.ldo + h * DP;
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = t * 32 + 8 * g + 4 * hi;
      if (d < DP) {
        uint2 o;
        o.x = pack_bf2(oacc[t][g * 4 + 0] * inv, oacc[t][g * 4 + 1] * inv);
        o.y = pack_bf2(oacc[t][g * 4 + 2] * inv, oacc[t][g * 4 + 3] * inv);
        *reinterpret_cast<uint2*>(orow + d) = o;
      }
    }
}

template <int DP>
int launch_dp(const AttnExtendArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((attention_extend_store_kernel<DP>), dim3(cdiv(a.max_new, kExtStoreTok), a.H, a.B), dim3(kExtThreads), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL((attention_extend_kernel<DP>), dim3(cdiv(a.max_new, kExtQB), a.H, a.B), dim3(kExtThreads), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_extend_launch(const AttnExtendArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K && a.Vt && a.lens && a.cu_new && a.O, "extend attention: null argument");
  GILL_REQUIRE(a.B > 0 && a.B <= 65535 && a.H > 0 && a.H <= 65535, "extend attention: empty batch");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "extend attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.max_new >= 1 && a.max_new <= a.pitch, "extend attention: max_new must be 1 .. pitch");
  GILL_REQUIRE(a.total_new >= 1, "extend attention: total_new must be at least 1");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "extend attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 4 == 0 && a.ldo >= a.H * a.dp, "extend attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K | (uintptr_t)a.Vt | (uintptr_t)a.O) % 16 == 0 &&
               ((uintptr_t)a.lens | (uintptr_t)a.cu_new | (uintptr_t)a.flags) % 4 == 0, "extend attention: operands must be 16-byte aligned");
  switch (a.dp) {
    case 64:  return launch_dp<64>(a, s);
    case 80:  return launch_dp<80>(a, s);
    case 128: return launch_dp<128>(a, s);
    default:
      gill_set_error("extend attention: unsupported head dim (supported: 64, 80, 128)");
      return -2;
  }
}
