// The load-time kernels behind xf_weights.h and their launches.  Nothing here runs inside a forward.
#include "xf_weights.h"
#include <hip/hip_fp16.h>

__device__ __forceinline__ float ld_any(const void* p, int dtype, int64_t i) {
  if (dtype == 0) return bf2f(((const bf16_t*)p)[i]);
  if (dtype == 1) return ((const float*)p)[i];
  return (float)(((const __half*)p)[i]);
}
// dst[r][h*dp + dd] = src[r][h*d + dd] (dd < d), zero elsewhere.  dst pre-zeroed.
__global__ __launch_bounds__(256) void pad_head_cols_kernel(const void* src, int dtype, int rows, int H, int d, int dp,
                                                            bf16_t* dst) {
  const int64_t total = (int64_t)rows * H * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int dd = (int)(i % d);
    const int h = (int)((i / d) % H);
    const int64_t r = i / ((int64_t)d * H);
    dst[r * (int64_t)H * dp + h * dp + dd] = f2bf(ld_any(src, dtype, i));
  }
}
// dst[(h*dp + dd)][:] = src[(h*d + dd)][:]  (row padding of q/k/v projection weights).  dst pre-zeroed.
__global__ __launch_bounds__(256) void pad_head_rows_kernel(const void* src, int dtype, int H, int d, int dp, int cols,
                                                            bf16_t* dst) {
  const int64_t total = (int64_t)H * d * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cols);
    const int64_t r = i / cols;
    const int h = (int)(r / d), dd = (int)(r % d);
    dst[((int64_t)h * dp + dd) * cols + c] = f2bf(ld_any(src, dtype, i));
  }
}

// Feed-forward output and proj_out are two linear maps with only a residual add in between:
//   out = proj_out(ff2(h) + t) + x_in = h (Wp W2)^T + t Wp^T + (Wp b2 + bp) + x_in
// so they run as ONE two-source GEMM over K = [h (4C) | t (C)].  This builds its weight rows [Wp W2 | Wp] ([C][5C], products in
// fp32 from the checkpoint's own dtype, one rounding to bf16) and its bias Wp b2 + bp.  Load time only: plain loops.
__global__ __launch_bounds__(256) void ffo_fuse_kernel(const void* wp, int dt_p, const void* w2, int dt_2, const void* b2, int dt_b2,
                                                       const void* bp, int dt_bp, int C, bf16_t* w_out, float* b_out) {
  const int n = blockIdx.y;                       // output row
  const int k = blockIdx.x * 256 + threadIdx.x;   // column of [4C | C | 1 (bias)]
  const int K4 = 4 * C;
  if (k < K4) {
    float a = 0.f;
    for (int j = 0; j < C; ++j) a = fmaf(ld_any(wp, dt_p, (int64_t)n * C + j), ld_any(w2, dt_2, (int64_t)j * K4 + k), a);
    w_out[(size_t)n * 5 * C + k] = f2bf(a);
  } else if (k < 5 * C) {
    w_out[(size_t)n * 5 * C + k] = f2bf(ld_any(wp, dt_p, (int64_t)n * C + (k - K4)));
  } else if (k == 5 * C) {
    float a = ld_any(bp, dt_bp, n);
    for (int j = 0; j < C; ++j) a = fmaf(ld_any(wp, dt_p, (int64_t)n * C + j), ld_any(b2, dt_b2, j), a);
    b_out[n] = a;
  }
}

// CROSS-ATTENTION AS TWO GEMMs ("XALG": UNet levels 1-3, head dim >= 80).  The keys and values of attn2 are linear maps of the 77 prompt
// tokens, fixed for the whole denoising loop, so per sample b and head h
//   scores[m][j] = qs LN(t)[m] . Wq_h^T K_bh[j]            = LN(t)[m] . (ctx_b[j] G_h)^T,     G_h  = qs (g o Wq_h)^T Wk_h      [C][768]
//   out[m]       = sum_h softmax(scores)[m][h][:] V_bh Wo_h^T = sum_h P[m][h][:] (ctx_b G2_h)^T, G2_h = Wo_h Wv_h             [C][768]
// G / G2 depend on the weights only (built here at load, fp32 products of the bf16 weights, one rounding); once per prompt the
// context turns them into per-sample weight matrices (unet_ctx_cache) and every UNet call then runs attn2 as
//   P = softmax80(LN(t) Mq_b^T)  (GEMM, N = 80 H: GemmArgs::OUT_SOFTMAX80)   and   t += P Wo_b^T + bias  (GEMM, K = 80 H)
// instead of to_q + the attention kernel + to_out: at d = 160 (levels 2-3) both GEMMs are half the size of the projections they
// replace, and the attention launch is gone.  GILL_UNET_XALG = 0 keeps the three-kernel form.
// rows [0, H C): G[h][c][:]; rows [H C, 2 H C): G2[h][co][:].  8 rows per workgroup (one head), threads over the 768 context features.
__global__ __launch_bounds__(256) void xalg_fold_kernel(const bf16_t* __restrict__ wq, const bf16_t* __restrict__ wkv, const bf16_t* __restrict__ wo,
                                                        int H, int C, int dp, int E, float qs, bf16_t* __restrict__ G) {
  __shared__ float a[8][160];
  const int r0 = blockIdx.x * 8;                  // first of 8 rows (C % 8 == 0: one head, one half)
  const int half = r0 >= H * C;
  const int rr = r0 - half * H * C;
  const int h = rr / C, c0 = rr - h * C;
  const int hdp = H * dp;
  for (int i = threadIdx.x; i < 8 * dp; i += 256) {
    const int r = i / dp, n = i - r * dp;
    a[r][n] = half ? bf2f(wo[(size_t)(c0 + r) * hdp + h * dp + n]) : qs * bf2f(wq[(size_t)(h * dp + n) * C + c0 + r]);
  }
  __syncthreads();
  const bf16_t* wb = wkv + (size_t)(half * hdp + h * dp) * E;      // Wk_h | Wv_h: [dp][E]
  for (int e = threadIdx.x; e < E; e += 256) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int n = 0; n < dp; ++n) {
      const float b = bf2f(wb[(size_t)n * E + e]);
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = fmaf(a[r][n], b, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) G[(size_t)(r0 + r) * E + e] = f2bf(acc[r]);
  }
}
// gb[h][e] = qs sum_n c_q[h dp + n] Wk[h dp + n][e]   (c_q = beta . Wq^T: the constant part of the folded norm2 -> to_q)
__global__ __launch_bounds__(256) void xalg_fold_bias_kernel(const float* __restrict__ cq, const bf16_t* __restrict__ wk, int dp, int E, float qs,
                                                             float* __restrict__ gb) {
  const int h = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float acc = 0.f;
  for (int n = 0; n < dp; ++n) acc = fmaf(cq[h * dp + n], bf2f(wk[(size_t)(h * dp + n) * E + e]), acc);
  gb[(size_t)h * E + e] = qs * acc;
}
// Once per prompt: T [Bx ctx_len][2 H C] = ctx [G | G2]^T (one GEMM) is dealt into the per-sample operands of the two GEMMs.
// Scores operand: Mq[b][80 h + j][:] = T[b ctx_len + j][h C ..], its row sums (folded LayerNorm) and the constant term ctx_b[j] . gb[h];
// key slots j >= ctx_len: zero rows with constant -1e30 (softmax weight 0).  One workgroup per (b, h, j).
__global__ __launch_bounds__(256) void xalg_scores_operand_kernel(const bf16_t* __restrict__ T, const bf16_t* __restrict__ ctx, const float* __restrict__ gb,
                                                                  int H, int C, int E, int ctx_len, bf16_t* __restrict__ Mq, float* __restrict__ cs,
                                                                  float* __restrict__ cb) {
  __shared__ float red[2][4];
  const int j = blockIdx.x % 80, h = (blockIdx.x / 80) % H, b = blockIdx.x / (80 * H);
  bf16_t* dst = Mq + (size_t)blockIdx.x * C;
  float sum = 0.f, dot = 0.f;
  if (j < ctx_len) {
    const bf16_t* src = T + (size_t)(b * ctx_len + j) * (2 * H * C) + (size_t)h * C;
    for (int c = threadIdx.x * 8; c < C; c += 2048) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + c);
      *reinterpret_cast<uint4*>(dst + c) = v;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) sum += __uint_as_float(w[i] << 16) + __uint_as_float(w[i] & 0xffff0000u);
    }
    const bf16_t* cr = ctx + (size_t)(b * ctx_len + j) * E;
    for (int e = threadIdx.x; e < E; e += 256) dot = fmaf(bf2f(cr[e]), gb[(size_t)h * E + e], dot);
  } else {
    for (int c = threadIdx.x * 8; c < C; c += 2048) *reinterpret_cast<uint4*>(dst + c) = make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); dot += __shfl_xor(dot, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sum; red[1][threadIdx.x >> 6] = dot; }
  __syncthreads();
  if (threadIdx.x == 0) {
    cs[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    cb[blockIdx.x] = j < ctx_len ? red[1][0] + red[1][1] + red[1][2] + red[1][3] : -1e30f;
  }
}
// Values operand: Wo_b[co][80 h + j] = T[b ctx_len + j][H C + h C + co] (0 for j >= ctx_len): an 80 x 64 transpose per workgroup (b, h, co / 64).
__global__ __launch_bounds__(256) void xalg_values_operand_kernel(const bf16_t* __restrict__ T, int H, int C, int ctx_len, bf16_t* __restrict__ Wo) {
  __shared__ bf16_t tile[80][66];
  const int cb = blockIdx.x % (C / 64), h = (blockIdx.x / (C / 64)) % H, b = blockIdx.x / ((C / 64) * H);
  for (int i = threadIdx.x; i < 80 * 64; i += 256) {
    const int j = i >> 6, c = i & 63;
    tile[j][c] = j < ctx_len ? T[(size_t)(b * ctx_len + j) * (2 * H * C) + (size_t)H * C + (size_t)h * C + cb * 64 + c] : (bf16_t)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 80; i += 256) {
    const int c = i / 80, j = i - c * 80;
    Wo[((size_t)b * C + cb * 64 + c) * (80 * H) + h * 80 + j] = tile[j][c];
  }
}
// dst[h * dp + dd] = src[h * d + dd] (a projection bias padded like the weight rows).  dst pre-zeroed.
__global__ __launch_bounds__(256) void pad_head_vec_kernel(const float* __restrict__ src, int H, int d, int dp, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < H * d) dst[(i / d) * dp + i % d] = src[i];
}
// {sum, sum of squares} of every row of t [M][C]: one wave per row
__global__ __launch_bounds__(256) void ffn_op_rowsums_kernel(const bf16_t* __restrict__ t, int M, int C, float* __restrict__ stats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  float a = 0.f, q = 0.f;
  for (int k = lane; k < C; k += 64) { const float v = bf2f(t[(size_t)row * C + k]); a += v; q += v * v; }
  a = wave_sum(a); q = wave_sum(q);
  if (lane == 0) { stats[(size_t)row * 2] = a; stats[(size_t)row * 2 + 1] = q; }
}
static int launched() { GILL_CHECK_HIP(hipGetLastError()); return 0; }   // after a kernel launch
int pad_head_cols_launch(const void* src, int dtype, int rows, int H, int d, int dp, bf16_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(pad_head_cols_kernel, dim3(1024), dim3(256), 0, s, src, dtype, rows, H, d, dp, dst);
  return launched();
}
int row_sums_launch(const bf16_t* t, int M, int C, float* stats, hipStream_t s) {
  hipLaunchKernelGGL(ffn_op_rowsums_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, t, M, C, stats);
  return launched();
}
int xf_qkv_weights(const HeadRows* seg, int nseg, const float* bias, int H, int d, int dp, int cols, const float* ln_g, const float* ln_b,
                   bf16_t* w, float* colsum, float* cbias, bf16_t* wperm, hipStream_t s, int steps) {
  const int hdp = H * dp;
  for (int sg = 0; sg < nseg && (steps & XF_LAYOUT); ++sg) {
    hipLaunchKernelGGL(pad_head_rows_kernel, dim3(1024), dim3(256), 0, s, seg[sg].w, seg[sg].dtype, H, d, dp, cols, w + (size_t)sg * hdp * cols);
    if (bias) hipLaunchKernelGGL(pad_head_vec_kernel, dim3(cdiv(H * d, 256)), dim3(256), 0, s, bias + (size_t)sg * H * d, H, d, dp, cbias + (size_t)sg * hdp);
  }
  GILL_CHECK_HIP(hipGetLastError());
  if (ln_g && (steps & XF_FOLD)) GILL_TRY(ln_fold_rows_launch(w, nseg * hdp, cols, ln_g, ln_b, colsum, cbias, s));
  if (wperm && (steps & XF_KPERM)) GILL_TRY(lnproj_kperm_launch(w, nseg * hdp, wperm, s));
  return 0;
}
int xf_geglu_weights(const bf16_t* W, const float* b, int inner, int K, const float* ln_g, const float* ln_b, int32_t* idx, bf16_t* w,
                     float* bias, float* colsum, hipStream_t s, int steps) {
  if (steps & XF_LAYOUT) {
    const std::vector<int32_t> map = geglu_row_permutation(inner);
    GILL_CHECK_HIP(hipMemcpyAsync(idx, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice, s));
    GILL_CHECK_HIP(hipStreamSynchronize(s));      // `map` dies here: its copy must have completed
    GILL_TRY(scatter_rows_bf16_launch(W, 2 * inner, K, idx, w, K, s));
    if (b) GILL_TRY(permute_f32_launch(b, idx, 2 * inner, bias, s));
  }
  if (ln_g && (steps & XF_FOLD)) GILL_TRY(ln_fold_rows_launch(w, 2 * inner, K, ln_g, ln_b, colsum, bias, s));
  return 0;
}
int xf_ffo_weights(const void* wp, int dt_p, const void* w2, int dt_2, const void* b2, int dt_b2, const void* bp, int dt_bp, int C,
                   bf16_t* w_out, float* b_out, hipStream_t s) {
  hipLaunchKernelGGL(ffo_fuse_kernel, dim3(cdiv(5 * C + 1, 256), C), dim3(256), 0, s, wp, dt_p, w2, dt_2, b2, dt_b2, bp, dt_bp, C, w_out, b_out);
  return launched();
}
int xalg_fold_launch(const bf16_t* wq, const float* cq, const bf16_t* wkv, const bf16_t* wo, int H, int C, int d, int dp, int E, bf16_t* xg,
                     float* xgb, hipStream_t s) {
  const float qs = 1.4426950408889634f / sqrtf((float)d);
  hipLaunchKernelGGL(xalg_fold_kernel, dim3(2 * H * C / 8), dim3(256), 0, s, wq, wkv, wo, H, C, dp, E, qs, xg);
  hipLaunchKernelGGL(xalg_fold_bias_kernel, dim3(cdiv(E, 256), H), dim3(256), 0, s, cq, wkv, dp, E, qs, xgb);
  return launched();
}
int xalg_operands_launch(const bf16_t* ctx, const bf16_t* xg, const float* xgb, int B, int H, int C, int E, int ctx_len, bf16_t* T, bf16_t* Mq,
                         float* cs, float* cb, bf16_t* Wo, hipStream_t s) {
  GemmArgs g;
  g.M = B * ctx_len; g.N = 2 * H * C; g.K = E; g.K1 = E; g.A = ctx; g.lda = E; g.W = xg; g.C = T; g.ldc = g.N;
  GILL_TRY(gemm_launch(g, s));
  hipLaunchKernelGGL(xalg_scores_operand_kernel, dim3(B * H * 80), dim3(256), 0, s, T, ctx, xgb, H, C, E, ctx_len, Mq, cs, cb);
  hipLaunchKernelGGL(xalg_values_operand_kernel, dim3(B * H * (C / 64)), dim3(256), 0, s, T, H, C, ctx_len, Wo);
  return launched();
}
