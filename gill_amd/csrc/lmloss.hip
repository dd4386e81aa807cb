// LM-head loss without a logits tensor (include/gill_amd.h "LM-head loss"): for every row of X (M, D) bf16 against W (V, D) bf16 and a target
// column, log-sum-exp of the row's logits, the target's logit and the target's rank, from fp32 MFMA accumulators that are never stored.  Stands for
// HF's CrossEntropyLoss over lm_head(hidden_states[-1]) (gill/models.py:273-275, :363-365) and for utils.accuracy's topk (gill/validate.py:89).
//
// FIVE LAUNCHES, all on the caller's stream, none waiting on another workgroup:
//   1. compact   (one workgroup)  rows whose target is not -100 -> rowmap[j] (ascending), their count n_valid (device), their target column
//                                 clamped into [0, V); an ignored row gets its final answer here (rank -1, lse = tgt = 0).
//   2. pre-pass  (one wave per 16 valid rows)  the target's logit of every valid row, tref[j] = X[rowmap[j]] . W[tcol[j]], on the same matrix
//                                 instruction in the same K order as the main pass: 16 gathered rows of W are the B operand and the diagonal of the
//                                 16 x 16 result is kept.  An element of an MFMA result depends on its A row and its B column only, so tref is
//                                 bit for bit the logit the main pass forms for that column, and "larger than the target" means the same in both.
//   3. main      grid (row tiles of 128 valid rows) x (vocabulary slabs of 512 columns)
//                                 a 128 x 128 x 64 LDS-staged bf16 GEMM on v_mfma_f32_16x16x32_bf16 (2 x 2 waves, 64 x 64 each), restated here
//                                 (gemm.hip is not touched).  After each 128-column tile a lane folds its 16 rows x 4 accumulators into per-row
//                                 running (max, sum of exp(v - max), count of columns in front of the target); the target's column is never counted
//                                 and its accumulator is stored to tgt_main[j] by the one lane that holds it.  Columns >= V of the last tile enter
//                                 as -inf: nothing for max, sum or count.  At the slab's end the 16 lanes of a row and the two waves that share it
//                                 are merged in a fixed order and the slab's (max, sum, count) go to the workspace, [slab][j].
//   4. merge     (one thread per valid row)  the slabs in ascending order: m = max, s = sum s_k exp(m_k - m), lse = m + log s, rank = sum of
//                                 counts.  A slab without a valid column (max = -inf, sum = 0) merges as the identity: exp(-inf - -inf) is never
//                                 formed.
//   5. summary   (one workgroup, optional)  {mean of lse - tgt over valid rows (NaN when none, torch's answer), n_valid, #rank < 1, #rank < 5}:
//                                 per-thread strided sums, then a fixed tree.
// There are no float atomics and no workgroup waits for another one; every partial is written once by one known lane and every sum has a fixed
// order, so the result is a fixed function of the inputs: it does not depend on which workgroup finishes first, and two calls give equal bits.
// The partition depends on V alone (lm_loss_geometry), and a row's arithmetic on its own X row and W only — not on M, on the row's place in a
// tile, or on which rows are ignored: compaction changes no output, and a batch whose first rows are a smaller batch repeats that batch's bits.
//
// W is read as it lies, (V, D) row-major: rows are the B operand's columns, K contiguous, which is the layout the instruction wants.
#include "../../include/gill_amd.h"
#include "ops.h"
#include <math.h>

#define LML_BM 128            // rows of a tile
#define LML_BN 128            // columns of a tile
#define LML_BK 64             // K of a staged step (two MFMA k-steps)
#define LML_SLAB_TILES 4      // column tiles of a slab
#define LML_STAGE_BYTES ((LML_BM + LML_BN) * LML_BK * 2)
#define LML_SMEM (2 * LML_STAGE_BYTES + LML_BM * 8)
#define LML_LOG2E 1.4426950408889634f

void lm_loss_geometry(int M, int V, int D, int* row_tile, int* col_tile, int* n_slabs, int* cols_per_slab) {
  (void)M; (void)D;      // the partition is a function of V alone (file header)
  const int cps = LML_BN * LML_SLAB_TILES;
  if (row_tile) *row_tile = LML_BM;
  if (col_tile) *col_tile = LML_BN;
  if (cols_per_slab) *cols_per_slab = cps;
  if (n_slabs) *n_slabs = V > 0 ? cdiv(V, cps) : 0;
}

// the workspace, carved from one allocation (256-byte aligned pieces)
struct LmlWs {
  int* nvalid;        // [1]
  int* rowmap;        // [M]
  int* tcol;          // [M]
  float* tref;        // [M]
  float* tgt_main;    // [M]
  float* pm;          // [n_slabs][M]
  float* ps;          // [n_slabs][M]
  int* pc;            // [n_slabs][M]
};
static size_t lml_carve(void* base, int M, int n_slabs, LmlWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
  const size_t m = (size_t)(M > 0 ? M : 1), ns = (size_t)(n_slabs > 0 ? n_slabs : 1);
  LmlWs t;
  t.nvalid = (int*)take(256);
  t.rowmap = (int*)take(4 * m);
  t.tcol = (int*)take(4 * m);
  t.tref = (float*)take(4 * m);
  t.tgt_main = (float*)take(4 * m);
  t.pm = (float*)take(4 * m * ns);
  t.ps = (float*)take(4 * m * ns);
  t.pc = (int*)take(4 * m * ns);
  if (w) *w = t;
  return off;
}
size_t lm_loss_workspace_bytes(int M, int V) {
  int ns = 0;
  lm_loss_geometry(M, V, 0, nullptr, nullptr, &ns, nullptr);
  return lml_carve(nullptr, M, ns, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- 1. compact
// Thread t owns the rows [t * per, (t + 1) * per): counts, an exclusive scan of the 256 counts in LDS, then the rows go out in ascending order.
__global__ __launch_bounds__(256) void lml_compact_kernel(const int64_t* __restrict__ target, int M, int V, LmlWs w, float* __restrict__ lse,
                                                          float* __restrict__ tgt, int* __restrict__ rank) {
  __shared__ int cnt[256];
  const int t = threadIdx.x;
  const int per = (M + 255) / 256;
  const int r0 = t * per < M ? t * per : M, r1 = r0 + per < M ? r0 + per : M;
  int c = 0;
  for (int r = r0; r < r1; ++r) c += target[r] != -100 ? 1 : 0;
  cnt[t] = c;
  __syncthreads();
  int base = 0;
  for (int i = 0; i < t; ++i) base += cnt[i];
  for (int r = r0; r < r1; ++r) {
    const int64_t tg = target[r];
    if (tg != -100) {
      w.rowmap[base] = r;
      w.tcol[base] = tg < 0 ? 0 : (tg >= V ? V - 1 : (int)tg);      // out of range: clamped, as the embedding kernels do
      ++base;
    } else {
      lse[r] = 0.f; tgt[r] = 0.f; rank[r] = -1;
    }
  }
  if (t == 255) w.nvalid[0] = base;
}

// ---------------------------------------------------------------------------------------------------------------- 2. pre-pass
__global__ __launch_bounds__(256) void lml_target_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, int D, LmlWs w) {
  const int lane = threadIdx.x & 63;
  const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  const int nv = w.nvalid[0];
  if (j0 >= nv) return;
  const int fr = lane & 15, q = lane >> 4;
  const int j = j0 + fr < nv ? j0 + fr : nv - 1;      // rows past the end repeat the last one; their results are not kept
  const bf16_t* xa = X + (size_t)w.rowmap[j] * D + 8 * q;
  const bf16_t* wb = W + (size_t)w.tcol[j] * D + 8 * q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // 16 k-steps of loads in flight, then their MFMAs in ascending k (the main pass's order); a k-step past D multiplies zeros: the bits stay
  for (int k0 = 0; k0 < D; k0 += 32 * 16) {
    uint4 a[16], b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int k = k0 + 32 * u;
      a[u] = k < D ? *reinterpret_cast<const uint4*>(xa + k) : make_uint4(0, 0, 0, 0);
      b[u] = k < D ? *reinterpret_cast<const uint4*>(wb + k) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u]), __builtin_bit_cast(bf16x8, b[u]), acc, 0, 0, 0);
  }
  // result element (row 4 q + reg, column fr): the diagonal is at reg = fr - 4 q
  const int reg = fr - 4 * q;
  if (reg >= 0 && reg < 4 && j0 + fr < nv) {
    const float v = reg == 0 ? acc[0] : reg == 1 ? acc[1] : reg == 2 ? acc[2] : acc[3];
    w.tref[j0 + fr] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- 3. main
// LDS image of a 128 x 64 bf16 operand tile: 128-byte rows; the 16-byte chunk c of row r sits at chunk c ^ ((r >> 1) & 7), so that the 16 lanes
// of a fragment read (rows r .. r + 15, one chunk) and of a staging write (two rows, eight chunks) fall on 16 different 16-byte bank groups.
__device__ __forceinline__ int lml_lds_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

__device__ __forceinline__ float lml_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__global__ __launch_bounds__(256, 2) void lml_main_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, int V, int D, int M,
                                                          LmlWs w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lml_smem[];
  const int nv = w.nvalid[0];
  const int row0 = blockIdx.x * LML_BM;
  if (row0 >= nv) return;
  const int slab = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int fr = lane & 15, q = lane >> 4;
  int* s_tcol = reinterpret_cast<int*>(lml_smem + 2 * LML_STAGE_BYTES);
  float* s_tref = reinterpret_cast<float*>(lml_smem + 2 * LML_STAGE_BYTES + LML_BM * 4);
  if (tid < LML_BM) {
    const int j = row0 + tid;
    s_tcol[tid] = j < nv ? w.tcol[j] : -1;
    s_tref[tid] = j < nv ? w.tref[j] : 0.f;
  }

  // staging: thread t moves chunk t & 7 of the rows (t >> 3) + 32 i, i = 0..3, of both operands
  const int sc = tid & 7, sr = tid >> 3;
  const bf16_t* xrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = row0 + sr + 32 * i;
    xrow[i] = X + (size_t)w.rowmap[j < nv ? j : nv - 1] * D + 8 * sc;      // rows past the end repeat the last valid row; never written
  }
  const int col_begin = slab * (LML_BN * LML_SLAB_TILES);
  int ntiles = (V - col_begin + LML_BN - 1) / LML_BN;
  if (ntiles > LML_SLAB_TILES) ntiles = LML_SLAB_TILES;
  const int nk = (D + LML_BK - 1) / LML_BK;
  const int total = ntiles * nk;

  uint4 ra[4], rb[4];
  auto load_step = [&](int it) {
    const int ct = it / nk, ks = it - ct * nk;
    const int k = ks * LML_BK + 8 * sc;
    const bool kin = k < D;        // D % 64 == 32: the upper half of the last step is zero
    const int cb = col_begin + ct * LML_BN;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int col = cb + sr + 32 * i;
      if (col >= V) col = V - 1;    // columns past the end repeat the last one; masked in the fold
      ra[i] = kin ? *reinterpret_cast<const uint4*>(xrow[i] + ks * LML_BK) : make_uint4(0, 0, 0, 0);
      rb[i] = kin ? *reinterpret_cast<const uint4*>(W + (size_t)col * D + k) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_step = [&](int buf) {
    unsigned char* a = lml_smem + buf * LML_STAGE_BYTES;
    unsigned char* b = a + LML_BM * LML_BK * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint4*>(a + lml_lds_off(sr + 32 * i, sc)) = ra[i];
      *reinterpret_cast<uint4*>(b + lml_lds_off(sr + 32 * i, sc)) = rb[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  // per lane, for its 16 rows (mi, reg) over its own columns
  float rm[16], rs[16];
  int rc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { rm[i] = -INFINITY; rs[i] = 0.f; rc[i] = 0; }

  load_step(0);
  store_step(0);
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    if (it + 1 < total) load_step(it + 1);
    const unsigned char* a = lml_smem + cur * LML_STAGE_BYTES;
    const unsigned char* b = a + LML_BM * LML_BK * 2;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        fa[mi] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(a + lml_lds_off(wr * 64 + mi * 16 + fr, kk * 4 + q)));
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        fb[ni] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(b + lml_lds_off(wc * 64 + ni * 16 + fr, kk * 4 + q)));
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
    }
    if (it + 1 < total) store_step(cur ^ 1);
    __syncthreads();

    const int ct = it / nk;
    if (it - ct * nk == nk - 1) {
      // fold the finished 128-column tile into the running per-row state
      const int cbase = col_begin + ct * LML_BN + wc * 64 + fr;      // this lane's column of ni = 0
      const bool tail = col_begin + (ct + 1) * LML_BN > V;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = wr * 64 + mi * 16 + q * 4 + reg;
          const int tc = s_tcol[lr];
          const float tr = s_tref[lr];
          float v[4];
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            v[ni] = acc[mi][ni][reg];
            const int col = cbase + ni * 16;
            if (tail && col >= V) v[ni] = -INFINITY;
            if (col == tc) {
              if (row0 + lr < nv) w.tgt_main[row0 + lr] = v[ni];      // the one lane that holds the target's column of this row
            } else if (v[ni] > tr || (v[ni] == tr && col < tc)) {
              rc[mi * 4 + reg] += 1;
            }
          }
          const float vmax = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
          const float mo = rm[mi * 4 + reg];
          const float mn = fmaxf(mo, vmax);
          const float mref = mn == -INFINITY ? 0.f : mn;      // nothing valid so far: every term below is exp2(-inf) = 0
          float s = rs[mi * 4 + reg] * lml_exp2((mo - mref) * LML_LOG2E);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) s += lml_exp2((v[ni] - mref) * LML_LOG2E);
          rm[mi * 4 + reg] = mn;
          rs[mi * 4 + reg] = s;
        }
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  // the slab's end.  The 16 lanes of a row (a DPP row: same q): xor tree, fixed order; then wave wc = 1 hands its rows to wave wc = 0 through LDS
  // (the staging buffers are free: every wave is past the last barrier of the loop).
  float* x_m = reinterpret_cast<float*>(lml_smem);            // [128]
  float* x_s = x_m + LML_BM;
  int* x_c = reinterpret_cast<int*>(x_s + LML_BM);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float m = rm[i];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const float mref = m == -INFINITY ? 0.f : m;
    float s = rs[i] * lml_exp2((rm[i] - mref) * LML_LOG2E);
    int c = rc[i];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    rm[i] = m; rs[i] = s; rc[i] = c;
  }
  if (wc == 1 && fr == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int lr = wr * 64 + (i >> 2) * 16 + q * 4 + (i & 3);
      x_m[lr] = rm[i]; x_s[lr] = rs[i]; x_c[lr] = rc[i];
    }
  }
  __syncthreads();
  if (wc == 0 && fr == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int lr = wr * 64 + (i >> 2) * 16 + q * 4 + (i & 3);
      const int j = row0 + lr;
      if (j < nv) {
        const float m1 = x_m[lr];
        const float m = fmaxf(rm[i], m1);
        const float mref = m == -INFINITY ? 0.f : m;
        const float s = rs[i] * lml_exp2((rm[i] - mref) * LML_LOG2E) + x_s[lr] * lml_exp2((m1 - mref) * LML_LOG2E);
        const size_t o = (size_t)slab * M + j;
        w.pm[o] = m; w.ps[o] = s; w.pc[o] = rc[i] + x_c[lr];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- 4. merge
__global__ __launch_bounds__(256) void lml_merge_kernel(int M, int n_slabs, LmlWs w, float* __restrict__ lse, float* __restrict__ tgt,
                                                        int* __restrict__ rank) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= w.nvalid[0]) return;
  float m = -INFINITY;
  for (int k = 0; k < n_slabs; ++k) m = fmaxf(m, w.pm[(size_t)k * M + j]);
  float s = 0.f;
  int c = 0;
  for (int k = 0; k < n_slabs; ++k) {
    const float mk = w.pm[(size_t)k * M + j];
    if (mk != -INFINITY) s += w.ps[(size_t)k * M + j] * expf(mk - m);      // an empty slab is the identity
    c += w.pc[(size_t)k * M + j];
  }
  const int r = w.rowmap[j];
  lse[r] = m + logf(s);
  tgt[r] = w.tgt_main[j];
  rank[r] = c;
}

// ---------------------------------------------------------------------------------------------------------------- 5. summary
__global__ __launch_bounds__(256) void lml_summary_kernel(const float* __restrict__ lse, const float* __restrict__ tgt, const int* __restrict__ rank,
                                                          int M, float* __restrict__ summary) {
  __shared__ float s_l[256];
  __shared__ int s_n[256], s_1[256], s_5[256];
  const int t = threadIdx.x;
  float l = 0.f;
  int n = 0, a1 = 0, a5 = 0;
  for (int r = t; r < M; r += 256) {
    const int rk = rank[r];
    if (rk >= 0) { l += lse[r] - tgt[r]; n += 1; a1 += rk < 1 ? 1 : 0; a5 += rk < 5 ? 1 : 0; }
  }
  s_l[t] = l; s_n[t] = n; s_1[t] = a1; s_5[t] = a5;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { s_l[t] += s_l[t + o]; s_n[t] += s_n[t + o]; s_1[t] += s_1[t + o]; s_5[t] += s_5[t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    summary[0] = s_l[0] / (float)s_n[0];      // 0 / 0 = NaN: the mean over no target
    summary[1] = (float)s_n[0];
    summary[2] = (float)s_1[0];
    summary[3] = (float)s_5[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
int lm_loss_launch(const bf16_t* X, const bf16_t* W, const int64_t* target, int M, int V, int D, float* lse, float* tgt, int* rank, float* summary,
                   void* workspace, hipStream_t s) {
  GILL_REQUIRE(X && W && target && lse && tgt && rank && workspace, "lm_loss: null argument");
  GILL_REQUIRE(M >= 1 && V >= 1 && D >= 32 && D % 32 == 0, "lm_loss: M, V >= 1 and D a positive multiple of 32");
  GILL_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)W & 15) == 0, "lm_loss: X and W must be 16-byte aligned");
  int n_slabs = 0;
  lm_loss_geometry(M, V, D, nullptr, nullptr, &n_slabs, nullptr);
  GILL_REQUIRE(n_slabs <= 65535, "lm_loss: vocabulary too large for one launch");
  LmlWs w;
  lml_carve(workspace, M, n_slabs, &w);
  static bool attr_set = false;
  if (!attr_set) {
    GILL_CHECK_HIP(hipFuncSetAttribute((const void*)lml_main_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LML_SMEM));
    attr_set = true;
  }
  lml_compact_kernel<<<dim3(1), dim3(256), 0, s>>>(target, M, V, w, lse, tgt, rank);
  lml_target_kernel<<<dim3(cdiv(M, 64)), dim3(256), 0, s>>>(X, W, D, w);
  lml_main_kernel<<<dim3(cdiv(M, LML_BM), n_slabs), dim3(256), LML_SMEM, s>>>(X, W, V, D, M, w);
  lml_merge_kernel<<<dim3(cdiv(M, 256)), dim3(256), 0, s>>>(M, n_slabs, w, lse, tgt, rank);
  if (summary) lml_summary_kernel<<<dim3(1), dim3(256), 0, s>>>(lse, tgt, rank, M, summary);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
