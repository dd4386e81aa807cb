// Fork attention for gfx950 (AttnForkArgs in ops.h): many packed candidate continuations attend to ONE cache row's prefix, read-only and shared,
// and each causally to its own tokens.  Candidate c brings cnt = cu_new[c + 1] - cu_new[c] packed tokens (any count, zero included), names its
// cache row p = parent[c] and sees the slots 0 .. n - 1 of it, n = plen[c] (zero included).  Token i attends to [K[p][0 .. n - 1] ; k_0 .. k_i].
// Nothing is appended: K and Vt are const here, the candidate's own keys and values are read from the packed projection rows they arrive in.
//
// A sibling of attention_extend.hip (that file is not touched): the same wave tile (32 queries x 32 keys, v_mfma_f32_32x32x16_bf16, S^T
// accumulators handed to P.V as the B operand, online softmax in fp32, no LDS, no barrier, four independent waves per workgroup), grid
// (ceil(max_new / 128), H, C), ONE CANDIDATE PER WAVE TILE.  The key walk of a wave has two phases:
//   prefix   tiles of 32 slots of row p from slot 0, K fragments straight from the cache row, V^T fragments gathered from the cache's V^T with
//            the permutation of the extend kernel.  No causal mask; a slot at or beyond n is SELECTED to -inf, and in the tile that straddles n
//            the V^T elements of those slots are replaced by zeros before they meet their (zero) probabilities: whatever the row holds beyond
//            n, finite or not, cannot reach the output.
//   tail     tiles of 32 of the candidate's own tokens, counted from ITS token 0 (not from slot n: the tiles are aligned to the candidate,
//            which is why bit equality with the extend kernel is not claimed), causal.  K fragments are 16-byte reads of the packed k rows
//            (a key beyond the count re-reads the last row and is selected away); the V^T fragment of a lane is eight 2-byte reads of the
//            packed v rows (the 32 lanes of a half wave read 64 consecutive bytes of one row), zero for a token beyond the count and for the
//            padded head rows of d = 80.  This is "route B" without the LDS transpose: a candidate has ceil(cnt / 32) tail tiles against
//            n / 32 prefix tiles, the workspace is empty (attention_fork_ws_bytes returns 0) and there is one launch.
// Every query sees a key in the first tile it meets (slot 0 when n > 0, its candidate's token 0 otherwise), so the running maximum is finite
// from the first tile on and exp2(-inf - -inf) is never formed.  Tiles are never shared between candidates.
// Fixed function: a candidate's tiles come in index order, its reductions are its own lanes', there are no atomics, no flags between
// workgroups, no waiting; the output bits depend on the candidate's packed operands, K[p][0 .. n - 1] / V[p][0 .. n - 1] and n only: not on
// C, its place in the pack, its siblings or the index p.  All stores are vector stores.
// Device values are never trusted: n outside [0, pitch] is clamped (flags[c] = 1); a parent outside [0, Bc), a count outside [0, max_new] or a
// packed range outside [0, total_new) make the candidate empty (flags[c] = 1) with no read through it; nothing outside the buffers is touched.
// Not built: filling a wave's 32 query slots from several short candidates of one parent (a candidate of 8 tokens uses a quarter of the tile
// and re-reads the parent's K / V^T once per candidate, from L2 after the first).
#include "ops.h"

namespace {

constexpr int kForkThreads = 256;
constexpr int kForkQB = 128;       // queries per workgroup: 32 per wave

struct ForkRow { int r0, cnt, par, n; bool flag; };

__device__ __forceinline__ ForkRow fork_row(const AttnForkArgs& p, int c) {
  ForkRow r;
  const int64_t lo = p.cu_new[c], hi = p.cu_new[c + 1];
  const int64_t cnt = hi - lo;
  r.flag = false;
  r.r0 = (int)lo; r.cnt = (int)cnt;
  if (cnt < 0 || cnt > p.max_new || lo < 0 || hi > p.total_new) { r.cnt = 0; r.r0 = 0; r.flag = true; }
  r.par = p.parent[c];
  if (r.par < 0 || r.par >= p.Bc) { r.par = 0; r.cnt = 0; r.r0 = 0; r.flag = true; }
  r.n = p.plen[c];
  if (r.n < 0 || r.n > p.pitch) { r.flag = true; r.n = r.n < 0 ? 0 : p.pitch; }
  return r;
}

// one tile of the online softmax: s holds the tile's scaled, selected scores (register e of a lane: key (e & 3) + 8 (e >> 2) + 4 hi of query lq);
// -> the running maximum / sum, the accumulators rescaled, the probabilities packed to bf16 as the B operand of P.V
template <int NDT>
__device__ __forceinline__ void fork_softmax_tile(f32x16& s, float& m_run, float& l_run, f32x16 (&oacc)[NDT], bf16x8 (&pa)[2]) {
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[e]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // the first tile a query meets holds a key it sees (file header): m_new is finite from then on
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
#pragma unroll
  for (int h4 = 0; h4 < 2; ++h4) {
    union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk.u[j] = pack_bf2(s[h4 * 8 + 2 * j], s[h4 * 8 + 2 * j + 1]);
    pa[h4] = pk.v;
  }
}

template <int DP>
__global__ __launch_bounds__(kForkThreads) void attention_fork_kernel(const AttnForkArgs p) {
  constexpr int KS = DP / 16;             // QK^T k-steps
  constexpr int NDT = (DP + 31) / 32;     // 32-row tiles of O^T
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.z, h = blockIdx.y;
  const ForkRow r = fork_row(p, c);
  if (r.flag && p.flags && h == 0 && blockIdx.x == 0 && threadIdx.x == 0) p.flags[c] = 1;
  const int q0 = blockIdx.x * kForkQB + w * 32;
  if (q0 >= r.cnt) return;
  const int lq = lane & 31, hi = lane >> 5;
  const bool qvalid = q0 + lq < r.cnt;
  const int qi = qvalid ? q0 + lq : r.cnt - 1;     // a lane beyond the count repeats the last query (never stored)
  const int n = r.n;
  const int tail_end = min(r.cnt, q0 + 32);        // own tokens this wave can see at all

  const size_t col = (size_t)h * DP;
  const bf16_t* qrow = p.q + (size_t)(r.r0 + qi) * p.ld + col;
  const bf16_t* Kb = p.K + (size_t)(r.par * p.H + h) * p.pitch * DP;
  const bf16_t* Vb = p.Vt + (size_t)(r.par * p.H + h) * p.dpv * p.pitch;

  bf16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qrow + s * 16 + hi * 8);

  f32x16 oacc[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[t][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  bf16x8 pa[2];

  // ---- prefix: the slots 0 .. n - 1 of row par (kv0 < n <= pitch and pitch % 32 == 0: the tile lies inside the pitch) ----
  for (int kv0 = 0; kv0 < n; kv0 += 32) {
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
    const bf16_t* krow = Kb + (size_t)(kv0 + lq) * DP + hi * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(krow + ks * 16);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kv = kv0 + (e & 3) + 8 * (e >> 2) + 4 * hi;
      s[e] = kv >= n ? -INFINITY : s[e] * p.qscale;
    }
    fork_softmax_tile<NDT>(s, m_run, l_run, oacc, pa);
    const bool straddle = kv0 + 32 > n;      // the tile reaches into slots the candidate does not see (wave-uniform)
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
      const bf16_t* vrow = Vb + (size_t)(t * 32 + lq) * p.pitch + kv0 + 4 * hi;
#pragma unroll
      for (int h4 = 0; h4 < 2; ++h4) {
        union { bf16x8 v; uint2 u[2]; uint16_t e[8]; } vf;
        vf.u[0] = *reinterpret_cast<const uint2*>(vrow + 16 * h4);
        vf.u[1] = *reinterpret_cast<const uint2*>(vrow + 16 * h4 + 8);
        if (straddle) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int kv = kv0 + 16 * h4 + 8 * (j >> 2) + 4 * hi + (j & 3);
            vf.e[j] = kv >= n ? (uint16_t)0 : vf.e[j];
          }
        }
        oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf.v, pa[h4], oacc[t], 0, 0, 0);
      }
    }
  }

  // ---- tail: the candidate's own tokens 0 .. qi, from the packed rows ----
  const uint16_t* vpk = reinterpret_cast<const uint16_t*>(p.v) + col;
  for (int j0 = 0; j0 < tail_end; j0 += 32) {
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
    const int jr = min(j0 + lq, r.cnt - 1);       // a key beyond the count: the last row again, selected away below
    const bf16_t* krow = p.k + (size_t)(r.r0 + jr) * p.ld + col + hi * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(krow + ks * 16);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = j0 + (e & 3) + 8 * (e >> 2) + 4 * hi;
      s[e] = j > qi ? -INFINITY : s[e] * p.qscale;      // qi <= cnt - 1: a token beyond the count is beyond every query
    }
    fork_softmax_tile<NDT>(s, m_run, l_run, oacc, pa);
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
      const int d = t * 32 + lq;
      const bool dok = (t + 1) * 32 <= DP || d < DP;     // d = 80: the head rows 80 .. 95 of the last tile are zeros
#pragma unroll
      for (int h4 = 0; h4 < 2; ++h4) {
        union { bf16x8 v; uint16_t e[8]; } vf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int tok = j0 + 16 * h4 + 8 * (j >> 2) + 4 * hi + (j & 3);
          vf.e[j] = (dok && tok < r.cnt) ? vpk[(size_t)(r.r0 + tok) * p.ld + d] : (uint16_t)0;
        }
        oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf.v, pa[h4], oacc[t], 0, 0, 0);
      }
    }
  }

  if (!qvalid) return;
  const float inv = 1.f / l_run;
  bf16_t* orow = p.O + (size_t)(r.r0 + qi) * p.ldo + col;
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
int launch_dp(const AttnForkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((attention_fork_kernel<DP>), dim3(cdiv(a.max_new, kForkQB), a.H, a.C), dim3(kForkThreads), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

size_t attention_fork_ws_bytes(int C, int H, int d, int max_new) {
  (void)C; (void)H; (void)d; (void)max_new;     // the tail is read from the packed rows: no scratch slab
  return 0;
}

int attention_fork_launch(const AttnForkArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K && a.Vt && a.parent && a.plen && a.cu_new && a.O, "fork attention: null argument");
  GILL_REQUIRE(a.C > 0 && a.C <= 65535 && a.Bc > 0 && a.H > 0 && a.H <= 65535, "fork attention: empty batch");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "fork attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.max_new >= 1 && a.max_new <= (1 << 22), "fork attention: max_new must be at least 1");
  GILL_REQUIRE(a.total_new >= 1, "fork attention: total_new must be at least 1");
  GILL_REQUIRE(a.dp == 64 || a.dp == 80 || a.dp == 128, "fork attention: unsupported head dim (supported: 64, 80, 128)");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "fork attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 4 == 0 && a.ldo >= a.H * a.dp, "fork attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K | (uintptr_t)a.Vt | (uintptr_t)a.O) % 16 == 0 &&
               ((uintptr_t)a.parent | (uintptr_t)a.plen | (uintptr_t)a.cu_new | (uintptr_t)a.flags) % 4 == 0,
               "fork attention: operands must be 16-byte aligned");
  const size_t need = attention_fork_ws_bytes(a.C, a.H, a.dp, a.max_new);
  GILL_REQUIRE(a.ws_bytes >= need && (need == 0 || (a.ws && (uintptr_t)a.ws % 16 == 0)), "fork attention: workspace shorter than attention_fork_ws_bytes");
  switch (a.dp) {
    case 64:  return launch_dp<64>(a, s);
    case 80:  return launch_dp<80>(a, s);
    default:  return launch_dp<128>(a, s);
  }
}
