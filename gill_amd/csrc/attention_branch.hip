// Branch decode attention for gfx950 (AttnBranchArgs in ops.h): S sampled continuations ("branches") of cached dialogues decode ONE new token
// each.  The siblings of one dialogue share that dialogue's prefix in the main cache (K / Vt: const here, never written); every branch keeps its
// own few keys and values in a row of a small side cache (Kb / Vtb) and appends the new token there.  Branches are packed in groups of at most
// 32 siblings: group g holds the branches gstart[g] .. gstart[g + 1] - 1, all of which see the slots 0 .. n - 1, n = gplen[g], of main-cache row
// p = gparent[g]; branch s has m = lens[s] - gplen[g] own cached tokens in row s of the side cache and stores its new key at slot m of Kb[s], its
// new value at column m of Vtb[s] (no ones-row entry: kv_branch_adopt_launch writes that one where the tokens reach the main cache).
//   o[s] = softmax(qscale * q_s . [K[p][0 .. n - 1] ; Kb[s][0 .. m - 1] ; k_s]) . [V[p][0 .. n - 1] ; Vb[s][0 .. m - 1] ; v_s]
// with the scale applied in fp32 and the new key and value taken from their input rows, never from the slot they are stored to.
//
// Grid (G, H), four waves per workgroup, three phases:
//   shared   on bf16 MFMA, a sibling of attention_fork.hip's prefix loop (that file is not touched, the helpers are duplicated here).  The
//            group's up to 32 queries are the B operand of v_mfma_f32_32x32x16_bf16; a lane beyond the group's count repeats the last member
//            and is never stored.  The prefix tiles of 32 slots are dealt to the waves by tile index: wave w takes the tiles w, w + 4, ..: a
//            function of n alone.  K fragments come straight from the cache row, V^T fragments with the fork kernel's permutation; a slot at or
//            beyond n is SELECTED to -inf and in the tile that straddles n its V^T elements are replaced by zeros.  The first tile of a wave
//            starts below n, so its running maximum is finite from the first tile on and exp2(-inf - -inf) is never formed.  Each wave that
//            met a tile leaves its partial (O^T, running maximum, sum) for the 32 queries in LDS: 4 x 32 x (d + 2) floats.
//   own      one wave per branch (branch i of the group on wave i % 4), on the vector ALUs: lane j scores the branch's own slot j (slot m: the
//            new key from its input row; a slot beyond m is selected to -inf whatever it holds), the probabilities go through LDS, lane l owns
//            the head dims 2 l and 2 l + 1 of P.V, each a serial chain over the slots 0 .. m - 1 (selected per slot) and the new value.
//   merge    by the same wave: the maximum over the prefix partials and the own part (finite: the new token is always visible), then the sums
//            and outputs of the four partials IN WAVE ORDER, then the own part, then the normalisation.  A wave that met no tile (w * 32 >= n,
//            n = 0 included) is selected away by that condition: its LDS words are neither written nor read.
// The prefix of a group is therefore read once per (group, head), not once per branch.
// Fixed function: a branch's output bits and the bits it stores depend only on its own q / k / v, K[p][0 .. n - 1] / V[p][0 .. n - 1], n, its own
// branch row up to m, and m: every reduction is over the branch's own MFMA column or its own wave in a fixed order, so S, G, the group's size,
// the siblings, the branch's place in the pack and the index p do not enter.  No atomics, no flags between workgroups; all stores are vector
// stores or plain C++.
// Slots of row p at or beyond n and slots of the branch row at or beyond m are excluded by selection whatever bits they hold (NaN included).
// Device values are never trusted: n outside [0, pitch] is clamped (every branch of the group gets flags[s] = 1); m outside [0, bpitch - 1] is
// clamped (flags[s] = 1); a parent outside [0, Bc) empties the group and flags its branches; a group size outside [0, 32] or a range outside
// [0, S] empties the group with no read through the range and flags the one branch min(max(gstart[g], 0), S - 1).  Nothing outside the buffers
// is touched.  Errors reported before any launch: an unsupported d (supported: 64, 80, 128), a misaligned pointer, bpitch % 32 != 0 (or above
// 1024), S < 1, fewer branch rows than branches.  gill_attention_branch honours GILL_OP_REPEAT: a repeat stores the same bits at the same slot.
#include "ops.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
constexpr int kBrThreads = 256;
constexpr int kBrWaves = kBrThreads / 64;
constexpr int kBrGroup = 32;          // siblings per group: the query lanes of one MFMA tile
constexpr int kBrMaxBpitch = 1024;

__device__ __forceinline__ float br_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float br_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// orders a wave's LDS stores before its later LDS loads (DS operations of one wave complete in order; this keeps the compiler from moving them)
__device__ __forceinline__ void br_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// attention_fork.hip's fork_softmax_tile: one tile of the online softmax over the S^T accumulators
template <int NDT>
__device__ __forceinline__ void br_softmax_tile(f32x16& s, float& m_run, float& l_run, f32x16 (&oacc)[NDT], bf16x8 (&pa)[2]) {
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[e]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx);       // finite: the first slot of a wave's first tile is below n
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
__global__ __launch_bounds__(kBrThreads) void attention_branch_kernel(const AttnBranchArgs p) {
  constexpr int KS = DP / 16;             // QK^T k-steps
  constexpr int NDT = (DP + 31) / 32;     // 32-row tiles of O^T
  constexpr int PST = DP + 2;             // floats of one query's partial: O[0 .. DP - 1], running maximum, sum
  constexpr int CH = DP / 8;              // 16-byte chunks of a key row
  extern __shared__ __attribute__((aligned(16))) float br_smem[];
  float* part = br_smem;                                  // [kBrWaves][32][PST]
  float* ownp = br_smem + kBrWaves * 32 * PST;            // [kBrWaves][bpitch]: a wave's own-phase scores, then probabilities
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.x, h = blockIdx.y;
  const bool flagger = h == 0 && p.flags != nullptr;

  // ---- the group (every exit below is uniform over the workgroup and lies before the barrier)
  const int lo = p.gstart[g], hi_ = p.gstart[g + 1];
  const int64_t cnt64 = (int64_t)hi_ - (int64_t)lo;
  if (lo < 0 || hi_ > p.S || cnt64 < 0 || cnt64 > kBrGroup) {
    if (flagger && threadIdx.x == 0) p.flags[min(max(lo, 0), p.S - 1)] = 1;
    return;
  }
  const int cnt = (int)cnt64;
  if (cnt == 0) return;
  const int par = p.gparent[g];
  if (par < 0 || par >= p.Bc) {
    if (flagger && (int)threadIdx.x < cnt) p.flags[lo + threadIdx.x] = 1;
    return;
  }
  const int nraw = p.gplen[g];
  int n = nraw;
  if (n < 0 || n > p.pitch) {
    n = n < 0 ? 0 : p.pitch;
    if (flagger && (int)threadIdx.x < cnt) p.flags[lo + threadIdx.x] = 1;
  }

  const size_t col = (size_t)h * DP;
  const int lq = lane & 31, hi = lane >> 5;

  // ---- shared phase: the tiles w, w + 4, .. of the prefix against the group's queries (kv0 < n <= pitch, pitch % 32 == 0: inside the pitch)
  if (w * 32 < n) {
    const int qm = min(lq, cnt - 1);                   // a lane beyond the count repeats the last member (never stored)
    const bf16_t* qrow = p.q + (size_t)(lo + qm) * p.ld + col;
    const bf16_t* Kp = p.K + (size_t)(par * p.H + h) * p.pitch * DP;
    const bf16_t* Vp = p.Vt + (size_t)(par * p.H + h) * p.dpv * p.pitch;
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
    for (int kv0 = w * 32; kv0 < n; kv0 += kBrWaves * 32) {
      f32x16 s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.f;
      const bf16_t* krow = Kp + (size_t)(kv0 + lq) * DP + hi * 8;
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
      br_softmax_tile<NDT>(s, m_run, l_run, oacc, pa);
      const bool straddle = kv0 + 32 > n;      // the tile reaches into slots the group does not see (wave-uniform)
#pragma unroll
      for (int t = 0; t < NDT; ++t) {
        const bf16_t* vrow = Vp + (size_t)(t * 32 + lq) * p.pitch + kv0 + 4 * hi;
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
    // the wave's partial of query lq: register e of tile t is head dim t * 32 + 8 (e >> 2) + 4 hi + (e & 3)
    float* pw = part + (size_t)(w * 32 + lq) * PST;
#pragma unroll
    for (int t = 0; t < NDT; ++t)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = t * 32 + 8 * g4 + 4 * hi;
        if (d < DP) {
          *reinterpret_cast<float2*>(pw + d) = make_float2(oacc[t][g4 * 4 + 0], oacc[t][g4 * 4 + 1]);
          *reinterpret_cast<float2*>(pw + d + 2) = make_float2(oacc[t][g4 * 4 + 2], oacc[t][g4 * 4 + 3]);
        }
      }
    if (hi == 0) {
      pw[DP] = m_run;
      pw[DP + 1] = l_run;
    }
  }
  __syncthreads();

  // ---- own phase and merge: branch i of the group on wave i % 4
  float* pown = ownp + w * p.bpitch;
  const bool dlane = 2 * lane < DP;        // the lane owns the head dims 2 lane, 2 lane + 1
  for (int qi = w; qi < cnt; qi += kBrWaves) {
    const int s = lo + qi;
    const int64_t m64 = (int64_t)p.lens[s] - (int64_t)nraw;
    int m = (int)m64;
    if (m64 < 0 || m64 > p.bpitch - 1) {
      m = m64 < 0 ? 0 : p.bpitch - 1;
      if (flagger && lane == 0) p.flags[s] = 1;
    }
    const bf16_t* qrow = p.q + (size_t)s * p.ld + col;
    const bf16_t* knew = p.k + (size_t)s * p.ld + col;
    const bf16_t* vnew = p.v + (size_t)s * p.ld + col;
    bf16_t* Kr = p.Kb + ((size_t)s * p.H + h) * p.bpitch * DP;
    bf16_t* Vr = p.Vtb + ((size_t)s * p.H + h) * p.dpv * p.bpitch;

    // scores of the slots 0 .. m (slot m: the new key), lane j % 64 takes slot j
    float mx = -INFINITY;
    for (int j0 = 0; j0 <= m; j0 += 64) {
      const int j = j0 + lane;
      const bf16_t* src = j < m ? Kr + (size_t)j * DP : knew;     // j > m: the new key again, selected away
      float sc = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const u32x4 kk = *reinterpret_cast<const u32x4*>(src + c * 8);
        const u32x4 qq = *reinterpret_cast<const u32x4*>(qrow + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sc = fmaf(br_lo(qq[e]), br_lo(kk[e]), sc);
          sc = fmaf(br_hi(qq[e]), br_hi(kk[e]), sc);
        }
      }
      sc = j <= m ? sc * p.qscale : -INFINITY;
      if (j <= m) pown[j] = sc;            // j <= m <= bpitch - 1
      mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);                     // finite: slot m is visible
    br_wave_sync();
    float l = 0.f;
    for (int j = lane; j <= m; j += 64) {
      const float e = __builtin_amdgcn_exp2f(pown[j] - mx);
      pown[j] = e;
      l += e;
    }
    l = wave_sum(l);
    br_wave_sync();

    // P.V over the own slots 0 .. m - 1 (chunks of 8: m <= bpitch - 1 and bpitch % 32 == 0 keep a chunk inside the row), then the new value
    float o0 = 0.f, o1 = 0.f;
    if (dlane) {
      const bf16_t* v0 = Vr + (size_t)(2 * lane) * p.bpitch;
      const bf16_t* v1 = v0 + p.bpitch;
      for (int j8 = 0; j8 < m; j8 += 8) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(v0 + j8);
        const u32x4 b = *reinterpret_cast<const u32x4*>(v1 + j8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pl = pown[j8 + 2 * e], ph = pown[j8 + 2 * e + 1];     // beyond m: never written, selected away below
          const bool sl = j8 + 2 * e < m, sh = j8 + 2 * e + 1 < m;
          const float t0 = fmaf(pl, br_lo(a[e]), o0), t1 = fmaf(pl, br_lo(b[e]), o1);
          o0 = sl ? t0 : o0;
          o1 = sl ? t1 : o1;
          const float u0 = fmaf(ph, br_hi(a[e]), o0), u1 = fmaf(ph, br_hi(b[e]), o1);
          o0 = sh ? u0 : o0;
          o1 = sh ? u1 : o1;
        }
      }
      const uint32_t vv = *reinterpret_cast<const uint32_t*>(vnew + 2 * lane);
      const float pn = pown[m];
      o0 = fmaf(pn, br_lo(vv), o0);
      o1 = fmaf(pn, br_hi(vv), o1);
    }

    // merge: the prefix partials in wave order, then the own part
    float mw[kBrWaves];
    float M = mx;
#pragma unroll
    for (int ww = 0; ww < kBrWaves; ++ww) {
      mw[ww] = ww * 32 < n ? part[(size_t)(ww * 32 + qi) * PST + DP] : -INFINITY;
      M = fmaxf(M, mw[ww]);
    }
    float L = 0.f, r0 = 0.f, r1 = 0.f;
#pragma unroll
    for (int ww = 0; ww < kBrWaves; ++ww) {
      if (ww * 32 < n) {                   // a wave that met no tile is selected away here: its words were never written
        const float* pq = part + (size_t)(ww * 32 + qi) * PST;
        const float f = __builtin_amdgcn_exp2f(mw[ww] - M);
        L = fmaf(f, pq[DP + 1], L);
        if (dlane) {
          const float2 ov = *reinterpret_cast<const float2*>(pq + 2 * lane);
          r0 = fmaf(f, ov.x, r0);
          r1 = fmaf(f, ov.y, r1);
        }
      }
    }
    const float fo = __builtin_amdgcn_exp2f(mx - M);
    L = fmaf(fo, l, L);
    r0 = fmaf(fo, o0, r0);
    r1 = fmaf(fo, o1, r1);
    if (dlane) *reinterpret_cast<uint32_t*>(p.O + (size_t)s * p.ldo + col + 2 * lane) = pack_bf2(r0 / L, r1 / L);

    // append: slot m of the branch row (behind every read of this branch in program order)
    if (lane < CH) *reinterpret_cast<u32x4*>(Kr + (size_t)m * DP + lane * 8) = *reinterpret_cast<const u32x4*>(knew + lane * 8);
    if (dlane) {
      const uint32_t vv = *reinterpret_cast<const uint32_t*>(vnew + 2 * lane);
      Vr[(size_t)(2 * lane) * p.bpitch + m] = (bf16_t)(vv & 0xffffu);
      Vr[(size_t)(2 * lane + 1) * p.bpitch + m] = (bf16_t)(vv >> 16);
    }
    br_wave_sync();                        // the next branch reuses pown
  }
}

__global__ __launch_bounds__(256) void kv_branch_adopt_kernel(const KvBranchAdoptArgs p) {
  const int h = blockIdx.x, tid = threadIdx.x;
  const bf16_t* ks = p.Kb + ((size_t)p.s * p.H + h) * p.bpitch * p.dp;
  bf16_t* kd = p.K + ((size_t)p.r * p.H + h) * p.pitch * p.dp + (size_t)p.plen * p.dp;
  for (int c = tid; c < p.count * p.dp / 8; c += 256)       // dp % 8 == 0: both sides are 16-byte aligned
    *reinterpret_cast<u32x4*>(kd + (size_t)c * 8) = *reinterpret_cast<const u32x4*>(ks + (size_t)c * 8);
  const bf16_t* vs = p.Vtb + ((size_t)p.s * p.H + h) * p.dpv * p.bpitch;
  bf16_t* vd = p.Vt + ((size_t)p.r * p.H + h) * p.dpv * p.pitch + p.plen;
  for (int i = tid; i < p.count * p.dp; i += 256) {
    const int d = i / p.count, j = i - d * p.count;
    vd[(size_t)d * p.pitch + j] = vs[(size_t)d * p.bpitch + j];
  }
  if (p.dpv > p.dp)
    for (int j = tid; j < p.count; j += 256) vd[(size_t)p.dp * p.pitch + j] = (bf16_t)0x3F80;
}

template <int DP>
int launch_dp(const AttnBranchArgs& a, hipStream_t s) {
  static bool attr_set = false;
  constexpr int part_floats = kBrWaves * 32 * (DP + 2);
  if (!attr_set) {
    GILL_CHECK_HIP(hipFuncSetAttribute((const void*)attention_branch_kernel<DP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)sizeof(float) * (part_floats + kBrWaves * kBrMaxBpitch)));
    attr_set = true;
  }
  const size_t smem = sizeof(float) * (size_t)(part_floats + kBrWaves * a.bpitch);
  hipLaunchKernelGGL((attention_branch_kernel<DP>), dim3(a.G, a.H), dim3(kBrThreads), smem, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_branch_launch(const AttnBranchArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K && a.Vt && a.Kb && a.Vtb && a.gstart && a.gparent && a.gplen && a.lens && a.O, "branch attention: null argument");
  GILL_REQUIRE(a.S >= 1, "branch attention: S must be at least 1");
  GILL_REQUIRE(a.G >= 1 && a.Bc > 0 && a.H > 0 && a.H <= 65535 && a.Sb >= a.S, "branch attention: empty batch, or fewer branch rows than branches");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "branch attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.bpitch >= 32 && a.bpitch % 32 == 0 && a.bpitch <= kBrMaxBpitch, "branch attention: branch pitch must be a multiple of 32, at most 1024");
  GILL_REQUIRE(a.dp == 64 || a.dp == 80 || a.dp == 128, "branch attention: unsupported head dim (supported: 64, 80, 128)");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "branch attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 2 == 0 && a.ldo >= a.H * a.dp, "branch attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K | (uintptr_t)a.Vt | (uintptr_t)a.Kb | (uintptr_t)a.Vtb |
                (uintptr_t)a.O) % 16 == 0 &&
               ((uintptr_t)a.gstart | (uintptr_t)a.gparent | (uintptr_t)a.gplen | (uintptr_t)a.lens | (uintptr_t)a.flags) % 4 == 0,
               "branch attention: operands must be 16-byte aligned");
  switch (a.dp) {
    case 64:  return launch_dp<64>(a, s);
    case 80:  return launch_dp<80>(a, s);
    default:  return launch_dp<128>(a, s);
  }
}

int kv_branch_adopt_launch(const KvBranchAdoptArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.Kb && a.Vtb && a.K && a.Vt, "branch adopt: null argument");
  GILL_REQUIRE(a.H > 0 && a.H <= 65535 && a.dp > 0 && a.dp % 8 == 0 && a.dpv == round_up(a.dp, 32), "branch adopt: head geometry");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.bpitch >= 32 && a.bpitch % 32 == 0, "branch adopt: pitches must be multiples of 32");
  GILL_REQUIRE(((uintptr_t)a.Kb | (uintptr_t)a.Vtb | (uintptr_t)a.K | (uintptr_t)a.Vt) % 16 == 0, "branch adopt: operands must be 16-byte aligned");
  GILL_REQUIRE(a.s >= 0 && a.s < a.Sb, "branch adopt: branch row out of range");
  GILL_REQUIRE(a.r >= 0 && a.r < a.Bc, "branch adopt: cache row out of range");
  GILL_REQUIRE(a.plen >= 0 && a.count >= 0 && a.count <= a.bpitch, "branch adopt: count exceeds the branch pitch");
  GILL_REQUIRE((int64_t)a.plen + a.count <= a.pitch - 1, "branch adopt: plen + count exceeds pitch - 1");
  if (a.count == 0) return 0;
  hipLaunchKernelGGL(kv_branch_adopt_kernel, dim3(a.H), dim3(256), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
