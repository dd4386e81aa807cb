// Ragged multi-token attention with append on an e4m3 KV cache for gfx950 (AttnExtendKv8Args in ops.h; the format: attention_kv8_dev.h): the
// sibling of attention_extend.hip.  Row b brings cnt = cu_new[b + 1] - cu_new[b] consecutive new tokens (any count, zero included) at its own
// cache length n = lens[b]; packed row cu_new[b] + i is token n + i of sequence b, stored at slot n + i, attending to the slots 0 .. n + i.
//
// Two launches on the stream:
//   1. attention_extend_kv8_store_kernel: one workgroup per (64-token tile, h, b), four lanes per token.  A token's k row and v row are each
//      quantised: the row maximum over the dp elements (the lane's own 8-element chunks, then an xor tree over the four lanes), the exponent,
//      the codes.  K8 bytes go straight to K8[b][h][n + i][:] (8-byte pieces, destination contiguous); the value codes pass through LDS and
//      are written to the columns n + i of Vt8[b][h][:][.] with the lanes along the tokens (consecutive slots); one lane per token stores the
//      two exponents.  Rows dp .. dpv - 1 of Vt8 are not written: there is no ones-row.
//   2. attention_extend_kv8_kernel: every key of a row, old or new, is then in the cache AS CODES, the tokens' own included, and no slot is
//      read in the kernel that stores it.  Grid (ceil(max_new / 128), H, B), four waves per workgroup, each wave 32 consecutive queries of one
//      (b, h), no LDS, no barrier, keys in tiles of 32 in order from slot 0 — the walk of attention_extend_kernel, on the same
//      v_mfma_f32_32x32x16_bf16 sequence:
//        S^T[kv][q] = sum_d K[kv][d] q[q][d]     A = a K8 fragment (8 bytes per lane and k-step) converted to bf16 in registers, exactly
//                                                (cvt_pk_f32_fp8, the upper halves: a code has four significant bits), B = the q fragment
//        s = S^T * 2^Kexp[kv] * log2(e) / sqrt(d) in fp32: the KEY SCALE multiplies the fp32 score (exact), keys beyond n + i SELECTED to -inf,
//        online softmax as in the bf16 kernel (the running sum is that of the unscaled probabilities)
//        O^T[d][q] += sum_kv Vt[d][kv] P'[q][kv] the Vt8 fragment (two 4-byte reads per lane and MFMA) converted to bf16 exactly; the VALUE
//                                                SCALE is applied to P, in fp32, BEFORE it is packed to bf16: P' = bf16(p 2^Vexp[kv]).  A
//                                                power of two commutes with the rounding, so this is bf16(p) times the exact value
//                                                code 2^e, the product the bf16 kernel forms on the dequantised cache (short of a p below
//                                                2^-126 / 2^e, which the bf16 kernel keeps as a bf16 subnormal and this one may flush).
// Exclusion is by selection: a score of a slot beyond n + i is replaced by -inf whatever the MFMA and the slot's exponent made of it, its
// probability is then an exact zero and is SELECTED to zero again behind the value scale, and in the tile that straddles n + cnt the V^T
// elements of slots at or beyond n + cnt are replaced by zeros after the conversion, so no byte pattern (the two NaN codes included) and no
// exponent of a stale slot can reach the output.  A stored exponent is clamped into the normal fp32 exponents when it is turned into a factor.
// No fragment or exponent read leaves the (b, h) slab: a tile that starts inside the row's keys lies inside the pitch (pitch % 32 == 0).
// Fixed function: a query's tiles come in index order, its reductions are its own lanes', there are no atomics, a token's codes depend on its
// own row alone, and query tiles are counted from the row's own first token: the same operands, length and count give the same output and
// cache bits at any B, anywhere in the pack, next to any other rows.
// Lengths and counts are read on the device and never trusted: n is clamped into [0, pitch - cnt] (flags[b] = 1), a count outside [0, max_new]
// or a row range outside [0, total_new) makes the row empty (flags[b] = 1); nothing outside the buffers is touched.
#include "attention_kv8_dev.h"

namespace {

constexpr int kExtThreads = 256;
constexpr int kExtQB = 128;       // queries per workgroup: 32 per wave
constexpr int kExtStoreTok = 64;  // tokens per workgroup of the store kernel

struct ExtRow { int r0, cnt, n; bool flag; };

// the row's packed range, count and clamped length, the same in both kernels (ext_row of attention_extend.hip)
__device__ __forceinline__ ExtRow ext_row(const AttnExtendKv8Args& p, int b) {
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
__global__ __launch_bounds__(kExtThreads) void attention_extend_kv8_store_kernel(const AttnExtendKv8Args p) {
  constexpr int CH = DP / 8;              // 8-element chunks of a row
  constexpr int MAXC = (CH + 3) / 4;      // chunks per lane
  constexpr int LDV = DP + 4;             // LDS row stride of the value codes in bytes: the transposed read below walks all banks
  __shared__ __attribute__((aligned(4))) uint8_t vl[kExtStoreTok * LDV];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * kExtStoreTok;
  const ExtRow r = ext_row(p, b);
  if (r.flag && p.flags && h == 0 && blockIdx.x == 0 && tid == 0) p.flags[b] = 1;
  if (i0 >= r.cnt) return;
  const int nt = r.cnt - i0 < kExtStoreTok ? r.cnt - i0 : kExtStoreTok;
  const size_t in0 = (size_t)(r.r0 + i0) * p.ld + h * DP;
  const size_t pair = (size_t)(b * p.H + h);
  uint8_t* Kb = p.K8 + (pair * p.pitch + r.n + i0) * DP;
  uint8_t* Vb = p.Vt8 + pair * p.dpv * p.pitch + r.n + i0;
  int8_t* Ke = p.Kexp + pair * p.pitch + r.n + i0;
  int8_t* Ve = p.Vexp + pair * p.pitch + r.n + i0;

  const int tok = tid >> 2, sub = tid & 3;      // the four lanes of a token are neighbours in one wave
  const int tk = tok < nt ? tok : nt - 1;       // a lane beyond the tile repeats its last token (stores nothing)
#pragma unroll
  for (int kv = 0; kv < 2; ++kv) {
    const bf16_t* src = (kv == 0 ? p.k : p.v) + in0 + (size_t)tk * p.ld;
    uint4 u[MAXC];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = sub + 4 * i;
      u[i] = c < CH ? *reinterpret_cast<const uint4*>(src + c * 8) : make_uint4(0u, 0u, 0u, 0u);
      mx = fmaxf(mx, fmaxf(fmaxf(kv8::amax2(u[i].x), kv8::amax2(u[i].y)), fmaxf(kv8::amax2(u[i].z), kv8::amax2(u[i].w))));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    const int e = kv8::row_exp(mx);
    const float inv = kv8::pow2(-e);
    if (tok < nt) {
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = sub + 4 * i;
        if (c < CH) {
          const uint32_t lo = kv8::quant4(u[i].x, u[i].y, inv), hi = kv8::quant4(u[i].z, u[i].w, inv);
          if (kv == 0) {
            *reinterpret_cast<uint2*>(Kb + (size_t)tok * DP + c * 8) = make_uint2(lo, hi);
          } else {
            *reinterpret_cast<uint32_t*>(vl + tok * LDV + c * 8) = lo;
            *reinterpret_cast<uint32_t*>(vl + tok * LDV + c * 8 + 4) = hi;
          }
        }
      }
      if (sub == 0) (kv == 0 ? Ke : Ve)[tok] = (int8_t)e;
    }
  }
  __syncthreads();
  const int t = tid & 63, g = tid >> 6;
  if (t < nt)
    for (int d = g; d < DP; d += kExtThreads / 64) Vb[(size_t)d * p.pitch + t] = vl[t * LDV + d];
}

template <int DP>
__global__ __launch_bounds__(kExtThreads) void attention_extend_kv8_kernel(const AttnExtendKv8Args p) {
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

  const size_t pair = (size_t)(b * p.H + h);
  const bf16_t* qrow = p.q + (size_t)(r.r0 + qi) * p.ld + h * DP;
  const uint8_t* Kb = p.K8 + pair * p.pitch * DP;
  const uint8_t* Vb = p.Vt8 + pair * p.dpv * p.pitch;
  const int8_t* Ke = p.Kexp + pair * p.pitch;
  const int8_t* Ve = p.Vexp + pair * p.pitch;

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
    // register e of a lane is key kv0 + (e & 3) + 8 (e >> 2) + 4 hi of query lq: its exponents are four aligned words of the tile
    uint32_t kex[4], vex[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      kex[g] = *reinterpret_cast<const uint32_t*>(Ke + kv0 + 8 * g + 4 * hi);
      vex[g] = *reinterpret_cast<const uint32_t*>(Ve + kv0 + 8 * g + 4 * hi);
    }
    const uint8_t* krow = Kb + (size_t)(kv0 + lq) * DP + hi * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint2 kb = *reinterpret_cast<const uint2*>(krow + ks * 16);
      union { bf16x8 v; uint32_t u[4]; } kf;
      kv8::cvt4bf(kb.x, kf.u[0], kf.u[1]);
      kv8::cvt4bf(kb.y, kf.u[2], kf.u[3]);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.v, qf[ks], s, 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kv = kv0 + (e & 3) + 8 * (e >> 2) + 4 * hi;
      const float ksc = kv8::pow2((int)(int8_t)(kex[e >> 2] >> (8 * (e & 3))));
      s[e] = kv > qidx ? -INFINITY : (s[e] * ksc) * p.qscale;
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
    // the value scales, behind the row sum
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kv = kv0 + (e & 3) + 8 * (e >> 2) + 4 * hi;
      const float vsc = kv8::pow2((int)(int8_t)(vex[e >> 2] >> (8 * (e & 3))));
      s[e] = kv > qidx ? 0.f : s[e] * vsc;
    }

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
      const uint8_t* vrow = Vb + (size_t)(t * 32 + lq) * p.pitch + kv0 + 4 * hi;
#pragma unroll
      for (int h4 = 0; h4 < 2; ++h4) {
        union { bf16x8 v; uint32_t u[4]; uint16_t e[8]; } vf;
        kv8::cvt4bf(*reinterpret_cast<const uint32_t*>(vrow + 16 * h4), vf.u[0], vf.u[1]);
        kv8::cvt4bf(*reinterpret_cast<const uint32_t*>(vrow + 16 * h4 + 8), vf.u[2], vf.u[3]);
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
int launch_dp(const AttnExtendKv8Args& a, hipStream_t s) {
  hipLaunchKernelGGL((attention_extend_kv8_store_kernel<DP>), dim3(cdiv(a.max_new, kExtStoreTok), a.H, a.B), dim3(kExtThreads), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL((attention_extend_kv8_kernel<DP>), dim3(cdiv(a.max_new, kExtQB), a.H, a.B), dim3(kExtThreads), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_extend_kv8_launch(const AttnExtendKv8Args& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K8 && a.Vt8 && a.Kexp && a.Vexp && a.lens && a.cu_new && a.O, "kv8 extend attention: null argument");
  GILL_REQUIRE(a.B > 0 && a.B <= 65535 && a.H > 0 && a.H <= 65535, "kv8 extend attention: empty batch");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "kv8 extend attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.max_new >= 1 && a.max_new <= a.pitch, "kv8 extend attention: max_new must be 1 .. pitch");
  GILL_REQUIRE(a.total_new >= 1, "kv8 extend attention: total_new must be at least 1");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "kv8 extend attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 4 == 0 && a.ldo >= a.H * a.dp, "kv8 extend attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K8 | (uintptr_t)a.Vt8 | (uintptr_t)a.O) % 16 == 0 &&
               ((uintptr_t)a.lens | (uintptr_t)a.cu_new | (uintptr_t)a.flags | (uintptr_t)a.Kexp | (uintptr_t)a.Vexp) % 4 == 0,
               "kv8 extend attention: operands must be 16-byte aligned (exponents: 4-byte)");
  switch (a.dp) {
    case 64:  return launch_dp<64>(a, s);
    case 80:  return launch_dp<80>(a, s);
    case 128: return launch_dp<128>(a, s);
    default:
      gill_set_error("kv8 extend attention: unsupported head dim (supported: 64, 80, 128)");
      return -2;
  }
}
