// Split-K reducers of gemm.hip (and of conv_fp8.hip): sum the fp32 partial slices in slice order, apply the GEMM epilogue, file the fused
// statistics — and, where the output feeds a single-source GroupNorm, apply that norm too.
#include "gemm_dev.h"

// Generic epilogue for 4 consecutive columns n..n+3 of row m (n % 4 == 0, n + 3 < N): used by the split-K reducer.
// (Loading bias / row vector / residual up front, in flight with the partials, measured SLOWER: loop 518.3 -> 520.1 ms.)
__device__ __forceinline__ void store4(const GemmArgs& p, int m, int n, float v0, float v1, float v2, float v3,
                                       float* fin = nullptr) {
  float v[4] = {v0 * p.alpha, v1 * p.alpha, v2 * p.alpha, v3 * p.alpha};
  if (p.bias) {
    const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (p.rowvec) {
    const float4 b = *reinterpret_cast<const float4*>(p.rowvec + (size_t)(m / p.rows_per_batch) * p.rowvec_bstride + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (p.resid) {
    if (p.resid_f32) {
      const float4 r = *reinterpret_cast<const float4*>((const float*)p.resid + (size_t)m * p.ldr + n);
      v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
    } else {
      const uint2 r = *reinterpret_cast<const uint2*>((const bf16_t*)p.resid + (size_t)m * p.ldr + n);
      v[0] += bf2f((bf16_t)(r.x & 0xffff)); v[1] += bf2f((bf16_t)(r.x >> 16));
      v[2] += bf2f((bf16_t)(r.y & 0xffff)); v[3] += bf2f((bf16_t)(r.y >> 16));
    }
  }
  if (p.act != ACT_NONE) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = apply_act(v[i], p.act);
  }
  if (fin) { fin[0] = v[0]; fin[1] = v[1]; fin[2] = v[2]; fin[3] = v[3]; }
  if (p.out_mode == OUT_BF16) {
    uint2 o; o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]);
    *reinterpret_cast<uint2*>((bf16_t*)p.C + (size_t)m * p.ldc + n) = o;
  } else if (p.out_mode == OUT_F32) {
    *reinterpret_cast<float4*>((float*)p.C + (size_t)m * p.ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
  } else {  // OUT_QKV
    const int hd = p.heads * p.dp;
    const int seg = p.seg_base + n / hd;
    const int within = n % hd;
    const int h = within / p.dp, dd = within % p.dp;
    const int b = m / p.ntok, t = m % p.ntok;
    if (seg == 0) {
      uint2 o; o.x = pack_bf2(v[0] * p.qscale, v[1] * p.qscale); o.y = pack_bf2(v[2] * p.qscale, v[3] * p.qscale);
      *reinterpret_cast<uint2*>(p.Cq + ((size_t)(b * p.heads + h) * p.ntok_pad_q + t) * p.dp + dd) = o;
    } else if (seg == 1) {
      uint2 o; o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]);
      *reinterpret_cast<uint2*>(p.Ck + ((size_t)(b * p.heads + h) * p.ntok_pad_kv + t + p.kv_tok_offset) * p.dp + dd) = o;
    } else {
      bf16_t* base = p.Cvt + ((size_t)(b * p.heads + h) * p.dpv + dd) * p.ntok_pad_kv + t + p.kv_tok_offset;
#pragma unroll
      for (int i = 0; i < 4; ++i) base[(size_t)i * p.ntok_pad_kv] = f2bf(v[i]);
      if (dd + 4 == p.dp && p.dpv > p.dp) base[(size_t)4 * p.ntok_pad_kv] = (bf16_t)0x3F80;
    }
  }
}

// REDUCE + GROUPNORM.  Where a split-K GEMM's output feeds a single-source GroupNorm (every 3x3 convolution of UNet levels 2-3 at
// the 8-sample batch: conv1 -> norm2 inside a ResnetBlock2D, and a block's last GEMM -> the next block's first norm), the reducer is
// the first place that holds complete output values — and a unit that owns ALL rows of one sample for a run of whole groups holds
// complete GroupNorm statistics too.  Unit = (sample b, W output columns from col0 = whole groups of fn_cg channels): sums the split slices
// in slice order, applies the GEMM epilogue (bias, per-sample row vector, bf16 residual), optionally stores the raw tensor, totals
// {sum, sum of squares} per group in a fixed order (thread -> 16 row lanes -> the group's column quads), and writes the normalised
// (+ SiLU) tensor: the GroupNorm-apply launch of that norm (5.5-7.5 us each, 24 per forward) and its read of the raw tensor disappear.
// Also files the fused-statistics partials of the raw output (gn_stats: one slab = the whole sample) for a later two-source consumer.
// fn_Y == nullptr: the plain finish (raw tensor + partials only).
// RPT rows per thread: rows_per_batch = 16 * RPT (256 -> 16, 64 -> 4).  W columns (80 | 40): W / 4 column quads x 16 row lanes = the block's 4 W threads.
template <int RPT, int W>
__device__ __forceinline__ void splitk_finish_unit(const GemmArgs& p, const int b, const int col0, const int tidx, float2 (*part)[W / 4], float2* quad,
                                                   float2* mr) {
  constexpr int QW = W / 4, ROWS = 16 * RPT;
  const bool act = tidx < 4 * W;      // (always true: the block IS 4 W threads.  Kept: without the test the compiler schedules the body differently, profiles/gemm_prune_isa.md)
  const int tx = tidx % QW, ty = act ? tidx / QW : 0;
  const int n = col0 + tx * 4;
  const int mbase = b * ROWS;
  const bool norm = p.fn_Y != nullptr;
  // every global load of the unit goes out before the first use: the partials of the first slices, the epilogue's vectors, the
  // residual rows, the norm's parameters — one memory round trip in front of the reduction, not four
  float4 v[RPT];
  auto row_of = [&](int r) -> int { return mbase + ty + 16 * r; };     // row of the thread's r-th value
  float ps = 0.f, pq = 0.f;
  uint2 raw[RPT];
  float4 gam = make_float4(0, 0, 0, 0), bet = make_float4(0, 0, 0, 0);
  if (act) {
  float4 add = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0, 0, 0, 0);
  const float4 rv = p.rowvec ? *reinterpret_cast<const float4*>(p.rowvec + (size_t)b * p.rowvec_bstride + n) : make_float4(0, 0, 0, 0);
  if (norm) { gam = *reinterpret_cast<const float4*>(p.fn_gamma + n); bet = *reinterpret_cast<const float4*>(p.fn_beta + n); }
  uint2 rr[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
    rr[r] = p.resid ? *reinterpret_cast<const uint2*>((const bf16_t*)p.resid + (size_t)row_of(r) * p.ldr + n) : make_uint2(0u, 0u);
  const float* src = p.ws + (size_t)(mbase + ty) * p.N + n;
  const size_t zstride = (size_t)p.M * p.N, rstride = (size_t)16 * p.N;
  // slices are ADDED in slice order whatever the order their loads go out in.  Few rows per thread (RPT = 4: the 64-row samples of UNet level 3,
  // split up to eight ways): the first eight slices' loads all at once — 32 independent 16-B loads per thread, ONE memory round trip — where a loop
  // over the slices is one round trip per slice (clamped slice index + predicated add, so absent slices cost a redundant load and nothing else).
  constexpr int CH = (RPT <= 4) ? 8 : 2;
  {
    float4 t[CH][RPT];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int zz = (u < p.splitk) ? u : p.splitk - 1;
#pragma unroll
      for (int r = 0; r < RPT; ++r) t[u][r] = *reinterpret_cast<const float4*>(src + (size_t)zz * zstride + (size_t)r * rstride);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) v[r] = t[0][r];
#pragma unroll
    for (int u = 1; u < CH; ++u) {
      if (u < p.splitk) {      // (uniform; splitk >= 2)
#pragma unroll
        for (int r = 0; r < RPT; ++r) { v[r].x += t[u][r].x; v[r].y += t[u][r].y; v[r].z += t[u][r].z; v[r].w += t[u][r].w; }
      }
    }
  }
  for (int z = CH; z < p.splitk; ++z) {
    float4 t[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) t[r] = *reinterpret_cast<const float4*>(src + (size_t)z * zstride + (size_t)r * rstride);
#pragma unroll
    for (int r = 0; r < RPT; ++r) { v[r].x += t[r].x; v[r].y += t[r].y; v[r].z += t[r].z; v[r].w += t[r].w; }
  }
  add.x += rv.x; add.y += rv.y; add.z += rv.z; add.w += rv.w;
  // STATISTICS SOURCE.  The producers that file RAW partials for a later GroupNorm-apply launch — the in-kernel epilogue (gs / gq) and the plain reducer
  // (store4()'s `fin`) — sum the values AS STORED, i.e. after their rounding to bf16: their partials are the sums of the tensor the consumer reads
  // (tests/test_gn_stats_gpu.py holds them to that within fp32 summation error).  This unit, which normalises in the same breath, sums the fp32 values
  // BEFORE their rounding and normalises the ROUNDED tensor (below: raw[r], what a stand-alone apply pass would read); its one-slab
  // partials for a later two-source consumer are those same sums.  The fused and unfused forms of one layer differ by that rounding noise (~1e-4 of a
  // sum) and by the (fixed) order of the fp32 additions, which is why they are held to closeness, not equality.  Variance: E[x^2] - E[x]^2 in fp32 over a
  // (sample, group) slab of <= 256 x 80 values of O(1): cancellation costs ~1e-6 relative at |mean| ~ sigma, far below the bf16 output step.
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int m = row_of(r);
    v[r].x += add.x; v[r].y += add.y; v[r].z += add.z; v[r].w += add.w;
    v[r].x += bf2f((bf16_t)(rr[r].x & 0xffff)); v[r].y += bf2f((bf16_t)(rr[r].x >> 16));        // (zeros without a residual)
    v[r].z += bf2f((bf16_t)(rr[r].y & 0xffff)); v[r].w += bf2f((bf16_t)(rr[r].y >> 16));
    ps += (v[r].x + v[r].y) + (v[r].z + v[r].w);
    pq += (v[r].x * v[r].x + v[r].y * v[r].y) + (v[r].z * v[r].z + v[r].w * v[r].w);
    raw[r].x = pack_bf2(v[r].x, v[r].y); raw[r].y = pack_bf2(v[r].z, v[r].w);
    if (p.C) *reinterpret_cast<uint2*>((bf16_t*)p.C + (size_t)m * p.ldc + n) = raw[r];
  }
  part[ty][tx] = make_float2(ps, pq);
  }
  __syncthreads();
  if (tidx < QW) {
    float a = 0.f, q = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float2 t = part[r][tidx]; a += t.x; q += t.y; }
    quad[tidx] = make_float2(a, q);
  }
  __syncthreads();
  if (norm) {
    const int qpg = p.fn_cg / 4;             // column quads per group
    const int ngrp = W / p.fn_cg;
    if (tidx < ngrp) {
      float a = 0.f, q = 0.f;
      for (int t = 0; t < qpg; ++t) { const float2 u = quad[tidx * qpg + t]; a += u.x; q += u.y; }
      const float inv_n = 1.f / ((float)p.fn_cg * (float)ROWS);
      const float sm = a * inv_n, sq = q * inv_n;
      const float var = fmaxf(sq - sm * sm, 0.f);
      mr[tidx] = make_float2(sm, rsqrtf(var + p.fn_eps));
    }
  }
  if (p.gn_stats) {      // partials of the raw output for a later (two-source) GroupNorm: bins of gn_cg channels, one slab per sample
    const int qpb = p.gn_cg / 4, nbin = W / p.gn_cg;
    const int t2 = tidx - 32;
    if (t2 >= 0 && t2 < 2 * nbin) {
      const int which = t2 & 1, lb = t2 >> 1;
      float a = 0.f;
      for (int t = 0; t < qpb; ++t) { const float2 u = quad[lb * qpb + t]; a += which ? u.y : u.x; }
      p.gn_stats[((size_t)b * p.gn_groups + col0 / p.gn_cg + lb) * 2 + which] = a;
    }
  }
  __syncthreads();
  if (norm && act) {
    const float2 g = mr[(tx * 4) / p.fn_cg];
    const float s0 = g.y * gam.x, s1 = g.y * gam.y, s2 = g.y * gam.z, s3 = g.y * gam.w;
    const float h0 = bet.x - g.x * s0, h1 = bet.y - g.x * s1, h2 = bet.z - g.x * s2, h3 = bet.w - g.x * s3;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int m = row_of(r);
      // (the consumer of the unfused path reads the bf16 tensor: normalise the rounded values)
      float o0 = fmaf(bf2f((bf16_t)(raw[r].x & 0xffff)), s0, h0), o1 = fmaf(bf2f((bf16_t)(raw[r].x >> 16)), s1, h1);
      float o2 = fmaf(bf2f((bf16_t)(raw[r].y & 0xffff)), s2, h2), o3 = fmaf(bf2f((bf16_t)(raw[r].y >> 16)), s3, h3);
      if (p.fn_silu) { o0 = silu_f(o0); o1 = silu_f(o1); o2 = silu_f(o2); o3 = silu_f(o3); }
      uint2 o; o.x = pack_bf2(o0, o1); o.y = pack_bf2(o2, o3);
      *reinterpret_cast<uint2*>(p.fn_Y + (size_t)m * p.N + n) = o;
    }
  }
}

// split-K reduction + epilogue
// Block = 64 rows x W columns (W = 80 when the fused GroupNorm bins need it, else 64), 16 row lanes x W/4 column quads:
// thread = one float4 column quad of rows ty, ty+16, ty+32, ty+48.  The partials of every split are summed in split order.
// Fused statistics are fixed-order like the GEMM kernel's epilogue's: per-row / per-column cells in LDS written once each, then
// one thread per output sum adds them in index order (row sums -> plane blockIdx.x of row_stats, bins -> this slab's
// GroupNorm partial).
template <int W, int R>
__global__ __launch_bounds__(4 * W) void gemm_splitk_reduce_kernel(const GemmArgs p) {
  kernarg_warm<sizeof(GemmArgs)>();
  constexpr int QW = W / 4;                     // column quads per row
  constexpr int ROWS = 16 * R;                  // rows per block: 64 for large outputs, 16 when blocks would be too few
  __shared__ float2 rowp[ROWS][QW];               // per (row, quad) {sum, sum of squares} of the bf16-rounded outputs
  __shared__ float2 colp[16][W];                // per (row lane, column) {sum, sum of squares} over the lane's 4 rows
  const int tx = threadIdx.x % QW, ty = threadIdx.x / QW;
  const int n = blockIdx.x * W + tx * 4;
  const int mbase = blockIdx.y * ROWS;
  float gs[4] = {0.f, 0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
  float rsum[R], rsq[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { rsum[r] = 0.f; rsq[r] = 0.f; }
  // row of the thread's r-th value
  auto row_of = [&](int r) -> int { return mbase + ty + 16 * r; };
  if (n < p.N) {
    // all partial loads of the thread's 4 rows are issued before any epilogue store (a store in between would fence the
    // next row's loads): 4 rows x 4 splits = 16 independent 16-B loads in flight per pass
    float4 s[R];
    const float* src[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int m = mbase + ty + 16 * r;
      if (m > p.M - 1) m = p.M - 1;
      s[r] = make_float4(0, 0, 0, 0);
      src[r] = p.ws + (size_t)m * p.N + n;
    }
    const size_t zstride = (size_t)p.M * p.N;
    constexpr int U = 16 / R;        // slices per pass: 16 independent 16-B loads in flight per thread either way
    int z = 0;
    for (; z + U <= p.splitk; z += U) {
      float4 v[R][U];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = *reinterpret_cast<const float4*>(src[r] + (size_t)(z + u) * zstride);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) { s[r].x += v[r][u].x; s[r].y += v[r][u].y; s[r].z += v[r][u].z; s[r].w += v[r][u].w; }
    }
    for (; z < p.splitk; ++z) {
      float4 v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = *reinterpret_cast<const float4*>(src[r] + (size_t)z * zstride);
#pragma unroll
      for (int r = 0; r < R; ++r) { s[r].x += v[r].x; s[r].y += v[r].y; s[r].z += v[r].z; s[r].w += v[r].w; }
    }
    const float4 cs = p.ln_stats ? *reinterpret_cast<const float4*>(p.ln_colsum + n) : make_float4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int m = row_of(r);
      if (m >= p.M) continue;
      if (p.ln_stats) {
        float rr, rm;
        ln_row_factors(p, m, rr, rm);
        s[r].x = s[r].x * rr - rm * cs.x; s[r].y = s[r].y * rr - rm * cs.y;
        s[r].z = s[r].z * rr - rm * cs.z; s[r].w = s[r].w * rr - rm * cs.w;
      }
      float fin[4];
      store4(p, m, n, s[r].x, s[r].y, s[r].z, s[r].w, fin);
#pragma unroll
      for (int e = 0; e < 4; ++e) {      // both kinds of statistics are those of the STORED values (the fp32 output: as they are)
        const float q = bf2f(f2bf(fin[e])), g = (p.out_mode == OUT_F32) ? fin[e] : q;
        gs[e] += g; gq[e] += g * g;
        rsum[r] += q; rsq[r] += q * q;
      }
    }
  }
  if (p.row_stats) {
#pragma unroll
    for (int r = 0; r < R; ++r) rowp[ty + 16 * r][tx] = make_float2(rsum[r], rsq[r]);
    __syncthreads();
    if ((int)threadIdx.x < ROWS && mbase + (int)threadIdx.x < p.M) {
      int nq = (p.N - blockIdx.x * W + 3) / 4;
      if (nq > QW) nq = QW;
      float a = 0.f, q = 0.f;
      for (int t = 0; t < nq; ++t) { a += rowp[threadIdx.x][t].x; q += rowp[threadIdx.x][t].y; }
      *reinterpret_cast<float2*>(p.row_stats + ((size_t)blockIdx.x * p.M + mbase + threadIdx.x) * 2) = make_float2(a, q);
    }
  }
  if (p.gn_stats) {
#pragma unroll
    for (int e = 0; e < 4; ++e) colp[ty][tx * 4 + e] = make_float2(gs[e], gq[e]);
    __syncthreads();
    // two levels, each in index order: column totals over the 16 row lanes (one thread per column), then the bin's columns — a chain
    // of 16 + gn_cg additions instead of 16 x gn_cg on the 2 x bins threads that finish the block (640 at 40 channels per group)
    __shared__ float2 colt[W];
    if ((int)threadIdx.x < W) {
      float a = 0.f, q = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { const float2 v = colp[r][threadIdx.x]; a += v.x; q += v.y; }
      colt[threadIdx.x] = make_float2(a, q);
    }
    __syncthreads();
    const int bins_blk = W / p.gn_cg;            // gemm_fused_gn_ok(): W % gn_cg == 0
    if ((int)threadIdx.x < 2 * bins_blk && mbase < p.M) {
      const int which = threadIdx.x & 1, lb = threadIdx.x >> 1;
      const int bin = blockIdx.x * bins_blk + lb;
      if (bin < p.gn_groups) {
        float a = 0.f;
        for (int c = 0; c < p.gn_cg; ++c) { const float2 v = colt[lb * p.gn_cg + c]; a += which ? v.y : v.x; }
        const int b = mbase / p.rows_per_batch;
        const int slab = (mbase - b * p.rows_per_batch) / ROWS;
        const int nslab = p.rows_per_batch / ROWS;
        p.gn_stats[(((size_t)b * nslab + slab) * p.gn_groups + bin) * 2 + which] = a;
      }
    }
  }
}

template <int RPT, int W>
__global__ __launch_bounds__(4 * W) void gemm_splitk_reduce_gn_kernel(const GemmArgs p) {
  kernarg_warm<sizeof(GemmArgs)>();
  __shared__ float2 part[16][W / 4];     // per (row lane, column quad) {sum, sum of squares} over the thread's rows
  __shared__ float2 quad[W / 4];         // per column quad, over the 16 row lanes
  __shared__ float2 mr[W / 4];           // per group of the block: {mean, rstd}   (fn_cg >= 4)
  splitk_finish_unit<RPT, W>(p, blockIdx.y, blockIdx.x * W, threadIdx.x, part, quad, mr);
}
// blocks of 40 columns where 80-column blocks would leave half the CUs without one and the groups / bins allow it
static inline int reduce_gn_width(const GemmArgs& a) {
  const bool ok40 = 40 % a.fn_cg == 0 && (a.gn_stats == nullptr || 40 % a.gn_cg == 0) && a.N % 40 == 0;
  if (!ok40) return 80;
  return ((int64_t)(a.N / 80) * (a.M / a.rows_per_batch) < 256) ? 40 : 80;
}
// geometries the fused reducer takes: whole samples of 64 or 256 rows, 80-column blocks of whole groups, the plain bf16 epilogue
bool gemm_fused_norm_ok(const GemmArgs& a) {
  const int rows = a.rows_per_batch;
  const int M = (a.conv && a.ups == 2) ? 0 : a.M;      // (not the 4-tap upsample form: its partials are filed per parity class)
  return (rows == 64 || rows == 256) && M > 0 && M % rows == 0 && a.N % 80 == 0 && a.fn_cg >= 4 && a.fn_cg % 4 == 0 && 80 % a.fn_cg == 0 &&
         a.out_mode == OUT_BF16 && a.act == ACT_NONE && !a.resid_f32 && !a.row_stats && !a.ln_stats && a.alpha == 1.f && a.ldc == a.N &&
         (a.gn_stats == nullptr || (a.gn_cg >= 4 && a.gn_cg % 4 == 0 && 80 % a.gn_cg == 0));
}

// width of the split-K reducer's blocks: 80 when the fused GroupNorm bins do not divide 64 (UNet: 5 / 10 / 20 / 40 channels)
// (160 where N allows: a block row is then 640 B = five whole 128-B lines of a partial slice; 80-wide blocks read 320-B pieces, every
// other one straddling a line: loop 568.3 -> 562.5 ms, profiles/r02_big_tile.md)
int reduce_width(const GemmArgs& a) {
  if (a.gn_stats && 64 % a.gn_cg != 0) return (a.N % 160 == 0 && 160 % a.gn_cg == 0) ? 160 : 80;
  return 64;
}
// rows per block of the reducer: 64 for large outputs, 16 when there would be too few blocks to pull the partials
// (32-row blocks where they would still give every CU two blocks: measured equal, 536.2 vs 536.3 ms on the loop — not kept)
int reduce_rows(const GemmArgs& a) {
  return ((int64_t)cdiv(a.N, reduce_width(a)) * cdiv(a.M, 64) >= 1024) ? 64 : 16;
}

int gemm_splitk_reduce_launch(const GemmArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.splitk > 1 && a.ws != nullptr, "split-K reducer: no partials");
  if (a.fn_Y) {
    GILL_REQUIRE(gemm_fused_norm_ok(a) && a.fn_gamma && a.fn_beta, "split-K reducer: unsupported fused GroupNorm geometry");
    const int w = reduce_gn_width(a);
    const dim3 rg(a.N / w, a.M / a.rows_per_batch);
    if (a.rows_per_batch == 256 && w == 80) hipLaunchKernelGGL((gemm_splitk_reduce_gn_kernel<16, 80>), rg, dim3(320), 0, s, a);
    else if (a.rows_per_batch == 256) hipLaunchKernelGGL((gemm_splitk_reduce_gn_kernel<16, 40>), rg, dim3(160), 0, s, a);
    else if (w == 80) hipLaunchKernelGGL((gemm_splitk_reduce_gn_kernel<4, 80>), rg, dim3(320), 0, s, a);
    else hipLaunchKernelGGL((gemm_splitk_reduce_gn_kernel<4, 40>), rg, dim3(160), 0, s, a);
    GILL_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const int rw = reduce_width(a), rr = reduce_rows(a);
  const dim3 rg(cdiv(a.N, rw), cdiv(a.M, rr));
  if (rw == 160 && rr == 64) hipLaunchKernelGGL((gemm_splitk_reduce_kernel<160, 4>), rg, dim3(640), 0, s, a);
  else if (rw == 160) hipLaunchKernelGGL((gemm_splitk_reduce_kernel<160, 1>), rg, dim3(640), 0, s, a);
  else if (rw == 80 && rr == 64) hipLaunchKernelGGL((gemm_splitk_reduce_kernel<80, 4>), rg, dim3(320), 0, s, a);
  else if (rw == 80) hipLaunchKernelGGL((gemm_splitk_reduce_kernel<80, 1>), rg, dim3(320), 0, s, a);
  else if (rr == 64) hipLaunchKernelGGL((gemm_splitk_reduce_kernel<64, 4>), rg, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemm_splitk_reduce_kernel<64, 1>), rg, dim3(256), 0, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
