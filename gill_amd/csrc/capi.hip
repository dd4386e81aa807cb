// extern "C" surface of libgill_amd (see include/gill_amd.h): error plumbing and the operator-level
// entry points.  The three stage engines export their own entry points from opt.hip / mapper.hip /
// unet.hip; the UNet's operator entries are in unet_ops.hip.
#include "../../include/gill_amd.h"
#include "ops.h"
#include "convnet.h"
#include "tfm.h"
#include "xf_weights.h"
#include "gemm_plan.h"
#include "attention_plan.h"
#include "xf_plan.h"
#include <vector>

static thread_local std::string g_last_error;
void gill_set_error(const std::string& msg) { g_last_error = msg; }

extern "C" const char* gill_last_error(void) { return g_last_error.c_str(); }
extern "C" int gill_version(void) { return 100; }

// One grow-only split-K workspace for the operator entry points (they synchronise before they return and the reference's threading model is one
// request at a time — SURVEY 8b — so one buffer serves them all): a per-call hipMalloc / hipFree of up to 100 MB sat inside every timed call
// (profiles/r05_opt_stream64.md: it poisoned a probe).  Freed at process exit with the context.
static float* op_splitk_ws(size_t floats) {
  static float* ws = nullptr;
  static size_t cap = 0;
  if (floats > cap) {
    if (ws) (void)hipFree(ws);
    ws = nullptr; cap = 0;
    const size_t want = floats + (floats >> 2);
    if (hipMalloc((void**)&ws, sizeof(float) * want) != hipSuccess) { ws = nullptr; return nullptr; }
    cap = want;
  }
  return ws;
}

// splitk: 0 = the launcher's heuristic, n > 1 = forced.  splitk < 0: FORCE THE GENERAL ROW-MAJOR TILES — never the 64 x 64-blocked
// blocked copy that weight-streaming shapes (N * K >= 4 Mi; the STREAM64 tile up to 256 rows, the general tiles on the blocked layout above) otherwise take — with the heuristic split (-1) or -splitk ways (< -1), so that
// the operator tests can pin both paths on the same shape (the UNet and CLIP engines run such shapes on the general tiles).
// out_f32: bit 0 = fp32 output, bit 1 = the residual is fp32 (GemmArgs::resid_f32, as the OPT / CLIP engines pass their residual stream).
extern "C" int gill_op_gemm(const void* A, const void* W, const float* bias, const void* resid_bf16, void* C, int M, int N,
                            int K, float alpha, int act, int out_f32, int splitk, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GemmArgs g;
  g.M = M; g.N = N; g.K = K; g.K1 = K;
  g.A = (const bf16_t*)A; g.lda = K;
  g.W = (const bf16_t*)W;
  g.alpha = alpha; g.bias = bias;
  g.resid = resid_bf16; g.ldr = N; g.resid_f32 = (out_f32 & 2) ? 1 : 0;
  g.act = act;
  g.out_mode = (out_f32 & 1) ? OUT_F32 : OUT_BF16;
  g.C = C; g.ldc = N;
  const bool row_major = splitk < 0;
  if (row_major) splitk = (splitk == -1) ? 0 : -splitk;
  // weight-streaming shapes run the way the OPT engine runs them: on a 64 x 64-blocked copy of W (gemm_launch picks the tile by M)
  DevBuf wblk;
  if (!row_major && act != ACT_GEGLU && gemm_stream64_weights(N, K)) {
    GILL_TRY(wblk.alloc(sizeof(bf16_t) * (size_t)N * K));
    GILL_TRY(convert_to_bf16_blk64_launch(W, 0, N, K, (bf16_t*)wblk.p, s));
    g.W = (const bf16_t*)wblk.p; g.w_blk64 = 1;
  }
  g.splitk = splitk > 0 ? splitk : (g.w_blk64 ? gemm_pick_splitk_blk64(M, N, K) : gemm_pick_splitk(M, N, K, act));
  if (g.splitk > 1) {
    g.ws = op_splitk_ws((size_t)g.splitk * M * N);
    GILL_REQUIRE(g.ws != nullptr, "split-K workspace allocation failed");
  }
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(gemm_launch(g, s));
  if (g.w_blk64) GILL_CHECK_HIP(hipStreamSynchronize(s));  // the blocked copy is freed on return
  return 0;
}

extern "C" int gill_op_geglu(const void* A, const void* W, const float* bias, void* C, int M, int inner, int K,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(inner % 64 == 0, "geglu: inner dim must be a multiple of 64");
  DevBuf wperm, bperm, idx;
  GILL_TRY(wperm.alloc(sizeof(bf16_t) * (size_t)2 * inner * K));
  GILL_TRY(bperm.alloc(sizeof(float) * (size_t)2 * inner));
  GILL_TRY(idx.alloc(sizeof(int32_t) * 2 * inner));
  GILL_TRY(xf_geglu_weights((const bf16_t*)W, bias, inner, K, nullptr, nullptr, (int32_t*)idx.p, (bf16_t*)wperm.p, (float*)bperm.p, nullptr, s));   // (no LayerNorm to fold)
  GemmArgs g;
  g.M = M; g.N = 2 * inner; g.K = K; g.K1 = K;
  g.A = (const bf16_t*)A; g.lda = K;
  g.W = (const bf16_t*)wperm.p;
  g.bias = bias ? (const float*)bperm.p : nullptr;
  g.act = ACT_GEGLU; g.out_mode = OUT_BF16;
  g.C = C; g.ldc = inner;
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(gemm_launch(g, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

static int op_conv3x3(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias, const float* rowvec,
                      const void* resid, void* y, int B, int IH, int IW, int Cout, int stride, int ups, int pad_shift, int splitk,
                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(pad_shift == 0 || (pad_shift == 1 && stride == 2 && !ups && IH % 2 == 0 && IW % 2 == 0),
               "conv3x3_ex: pad_shift is 0 or 1; 1 needs stride 2, no upsample and even IH and IW");
  const int Cin = C1 + C2;
  DevBuf wr, ws;
  GILL_TRY(wr.alloc(sizeof(bf16_t) * (size_t)Cout * 16 * Cin));     // 9 taps, or 4 classes x 4 taps
  // K order as the engines choose it
  int chunked = conv_k_chunked(IH * IW, Cin, Cout) ? 1 : 0;
  // ups = 1: the engines' form — four pre-summed 2x2-tap kernels on the source grid (GILL_CONV_UPS4 = 0, or a residual / row
  // vector, which that form does not take: the 9-tap gather over the upsampled grid)
  const char* u4 = getenv("GILL_CONV_UPS4");
  const bool ups4 = ups && stride == 1 && !rowvec && !resid && !(u4 && atoi(u4) == 0);
  if (ups4) { chunked = 0; GILL_TRY(conv_weight_relayout_ups4_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s)); }
  else if (chunked) GILL_TRY(conv_weight_relayout_chunked_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  else GILL_TRY(conv_weight_relayout_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  GemmArgs g;
  g.conv = 1;
  g.IH = IH; g.IW = IW; g.Cin = Cin; g.stride = stride; g.ups = ups4 ? 2 : ups; g.pad_shift = pad_shift;
  if (ups) { g.OH = 2 * IH; g.OW = 2 * IW; }
  else if (pad_shift) { g.OH = IH / 2; g.OW = IW / 2; }
  else { g.OH = (IH + 2 - 3) / stride + 1; g.OW = (IW + 2 - 3) / stride + 1; }
  g.M = B * g.OH * g.OW; g.N = Cout; g.K = (ups4 ? 4 : 9) * Cin;
  g.A = (const bf16_t*)x1; g.A2 = (const bf16_t*)x2; g.K1 = C1;
  g.W = (const bf16_t*)wr.p; g.k_chunked = chunked;
  g.bias = bias;
  g.rowvec = rowvec; g.rows_per_batch = g.OH * g.OW; g.rowvec_bstride = Cout;
  g.resid = resid; g.ldr = Cout;
  g.C = y; g.ldc = Cout;
  g.splitk = splitk > 0 ? splitk : gemm_pick_splitk(g.M, g.N, g.K, 0);
  if (g.splitk > 1) {
    GILL_TRY(ws.alloc(sizeof(float) * (size_t)g.splitk * g.M * g.N));
    g.ws = (float*)ws.p;
  }
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(gemm_launch(g, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
extern "C" int gill_op_conv3x3(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias,
                               const float* rowvec, const void* resid, void* y, int B, int IH, int IW, int Cout,
                               int stride, int ups, int splitk, void* stream) {
  return op_conv3x3(x1, C1, x2, C2, w_oihw, bias, rowvec, resid, y, B, IH, IW, Cout, stride, ups, 0, splitk, stream);
}
extern "C" int gill_op_conv3x3_ex(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias,
                                  const float* rowvec, const void* resid, void* y, int B, int IH, int IW, int Cout,
                                  int stride, int ups, int pad_shift, int splitk, void* stream) {
  return op_conv3x3(x1, C1, x2, C2, w_oihw, bias, rowvec, resid, y, B, IH, IW, Cout, stride, ups, pad_shift, splitk, stream);
}

// 3x3 convolution + the GroupNorm (+ SiLU) that consumes its output, without a GroupNorm launch of its own where the geometry allows:
// y_raw (optional) = conv(x) + bias + rowvec[b] + resid, y_norm = [silu](GroupNorm(y_raw; groups, gamma, beta, eps)).
//   splitk >= 2: the split-K reducer launch also normalises (gemm_reduce.hip "REDUCE + GROUPNORM": H * W in {64, 256}, Cout / groups a multiple of 4
//                dividing 80); coop is ignored;
//   splitk == 1: coop = 1: in the convolution's epilogue (COOP, EPI 6: H * W a multiple of the 128- / 256-row tile, <= 4096 pixels per sample,
//                grid <= CUs) — an error where the geometry does not allow it; coop = 0: the reference dataflow, conv with fused statistics +
//                groupnorm_apply_launch.
// ss_out (optional, splitk == 1 && coop == 1 only): the per-(sample, channel) scale | shift table [B][2][Cout] instead of / next to y_norm.
// For the operator tests.
extern "C" int gill_op_conv3x3_gn(const void* x, const float* w_oihw, const float* bias, const float* rowvec, const void* resid, const float* gamma,
                                  const float* beta, int groups, float eps, int silu, void* y_raw, void* y_norm, float* ss_out, int B, int H, int W,
                                  int Cin, int Cout, int splitk, int coop, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x && w_oihw && gamma && beta && (y_norm || ss_out) && groups > 0 && Cout % groups == 0 && splitk >= 1, "bad argument");
  GILL_REQUIRE(ss_out == nullptr || (splitk == 1 && coop), "conv3x3_gn: the scale | shift table comes from the in-kernel finish only");
  DevBuf wr, ws, ctr, st, raw_tmp;
  GILL_TRY(wr.alloc(sizeof(bf16_t) * (size_t)Cout * 9 * Cin));
  GILL_TRY(conv_weight_relayout_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  GemmArgs g;
  g.conv = 1; g.IH = H; g.IW = W; g.OH = H; g.OW = W; g.Cin = Cin; g.stride = 1;
  g.M = B * H * W; g.N = Cout; g.K = 9 * Cin;
  g.A = (const bf16_t*)x; g.K1 = Cin; g.W = (const bf16_t*)wr.p; g.bias = bias;
  g.rowvec = rowvec; g.rowvec_bstride = Cout;
  g.rows_per_batch = H * W; g.resid = resid; g.ldr = Cout; g.C = y_raw; g.ldc = Cout;
  g.splitk = splitk;
  if (splitk > 1) {
    GILL_TRY(ws.alloc(sizeof(float) * (size_t)splitk * g.M * g.N));
    g.ws = (float*)ws.p;
  }
  g.fn_Y = (bf16_t*)y_norm; g.fn_ss = ss_out; g.fn_gamma = gamma; g.fn_beta = beta; g.fn_eps = eps; g.fn_silu = silu; g.fn_cg = Cout / groups;
  const int ncnt = gemm_coop_counters(g);
  GILL_TRY(ctr.alloc(sizeof(unsigned) * (size_t)ncnt));
  // statistics bins as the engine's talloc() picks them (C / 64 channels, else one group), one partial per 16 rows at most
  const int sbin = (Cout % 64 == 0 && Cout / 64 >= 2) ? Cout / 64 : Cout / groups;
  if (splitk == 1) {
    GILL_REQUIRE(gemm_fused_gn_ok(Cout, sbin) && (H * W) % GN_SLAB_ROWS == 0, "conv3x3_gn: no fused statistics for this width / map size");
    GILL_TRY(st.alloc(sizeof(float) * (size_t)B * (H * W / GN_SLAB_ROWS_MIN) * (Cout / sbin) * 2));
    g.gn_stats = (float*)st.p; g.gn_groups = Cout / sbin; g.gn_cg = sbin;
  }
  if (coop && splitk == 1) g.coop_ctr = (unsigned*)ctr.p;
  if (splitk == 1 && !coop) {
    // reference dataflow: the convolution files its statistics, a GroupNorm-apply launch normalises the rounded tensor
    g.fn_Y = nullptr; g.fn_ss = nullptr;
    if (!g.C) { GILL_TRY(raw_tmp.alloc(sizeof(bf16_t) * (size_t)g.M * g.N)); g.C = raw_tmp.p; }
    for (int r = 0; r < op_repeat(); ++r) {
      GILL_TRY(gemm_launch(g, s));
      GILL_TRY(groupnorm_apply_launch((const bf16_t*)g.C, Cout, nullptr, 0, B, H * W, groups, gamma, beta, eps, silu, (bf16_t*)y_norm, g.gn_stats, sbin, Cout,
                                      H * W / gemm_gn_slab_rows(g), nullptr, 0, 0, s, 0.f, nullptr, nullptr));
    }
    GILL_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
  }
  if (splitk == 1) GILL_REQUIRE(gemm_coop_ok(g), "conv3x3_gn: splitk == 1 with coop needs the in-kernel finish's geometry (gemm_coop_ok)");
  else GILL_REQUIRE(gemm_fused_norm_ok(g), "conv3x3_gn: unsupported geometry (H * W in {64, 256}, Cout % 80 == 0, group width | 80)");
  for (int r = 0; r < op_repeat(); ++r) {
    GILL_CHECK_HIP(hipMemsetAsync(ctr.p, 0, sizeof(unsigned) * (size_t)ncnt, s));
    GILL_TRY(gemm_launch(g, s));
  }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ResnetBlock2D's conv2 with the 1x1 conv_shortcut fused as extra K channels: wf rows = [the 9 Cin conv taps of wr (its K order) | the CS shortcut channels
// of w_sc (fp32, rounded to bf16)], as the engines' fuse_shortcut_into_conv2() builds them.  Synchronises.
static int op_fuse_shortcut_rows(const bf16_t* wr, int k9, const float* w_sc, int CS, int Cout, DevBuf& wf, hipStream_t s) {
  const int kf = k9 + CS;
  DevBuf wsb, idx;
  GILL_TRY(wsb.alloc(sizeof(bf16_t) * (size_t)Cout * CS));
  GILL_TRY(wf.alloc(sizeof(bf16_t) * (size_t)Cout * kf));
  GILL_TRY(idx.alloc(sizeof(int32_t) * (size_t)Cout));
  GILL_TRY(convert_to_bf16_launch(w_sc, GILL_DTYPE_F32, (int64_t)Cout * CS, (bf16_t*)wsb.p, s));
  std::vector<int32_t> ident(Cout);
  for (int i = 0; i < Cout; ++i) ident[i] = i;
  GILL_CHECK_HIP(hipMemcpyAsync(idx.p, ident.data(), sizeof(int32_t) * Cout, hipMemcpyHostToDevice, s));
  GILL_TRY(scatter_rows_bf16_launch(wr, Cout, k9, (const int32_t*)idx.p, (bf16_t*)wf.p, kf, s));
  GILL_TRY(scatter_rows_bf16_launch((const bf16_t*)wsb.p, Cout, CS, (const int32_t*)idx.p, (bf16_t*)wf.p + k9, kf, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));     // (the staging buffers leave scope)
  return 0;
}

// ResnetBlock2D's conv2 with the 1x1 conv_shortcut of the raw block input fused as extra K channels (the engine's c2f weights):
// y = conv3x3(x1 ++ x2) + bias + conv1x1(xs1 ++ xs2), one implicit GEMM with K = 9 (C1 + C2) + CS1 + CS2.  For the operator tests.
extern "C" int gill_op_conv3x3_shortcut(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias,
                                        const void* xs1, int CS1, const void* xs2, int CS2, const float* w_sc, void* y, int B, int IH,
                                        int IW, int Cout, int splitk, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int Cin = C1 + C2, CS = CS1 + CS2, kf = 9 * Cin + CS;
  GILL_REQUIRE(x1 && w_oihw && xs1 && w_sc && y && CS % 64 == 0 && CS1 % 64 == 0, "bad argument");
  DevBuf wr, wf, ws;
  GILL_TRY(wr.alloc(sizeof(bf16_t) * (size_t)Cout * 9 * Cin));
  const int chunked = conv_k_chunked(IH * IW, Cin, Cout) ? 1 : 0;
  if (chunked) GILL_TRY(conv_weight_relayout_chunked_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  else GILL_TRY(conv_weight_relayout_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  GILL_TRY(op_fuse_shortcut_rows((const bf16_t*)wr.p, 9 * Cin, w_sc, CS, Cout, wf, s));
  GemmArgs g;
  g.conv = 1; g.IH = IH; g.IW = IW; g.OH = IH; g.OW = IW; g.Cin = Cin; g.stride = 1; g.ups = 0;
  g.M = B * IH * IW; g.N = Cout; g.K = kf;
  g.A = (const bf16_t*)x1; g.A2 = (const bf16_t*)x2; g.K1 = C1;
  g.X1 = (const bf16_t*)xs1; g.X2 = (const bf16_t*)xs2; g.KX = CS; g.KX1 = CS1;
  g.W = (const bf16_t*)wf.p; g.k_chunked = chunked; g.bias = bias;
  g.rows_per_batch = IH * IW;
  g.C = y; g.ldc = Cout;
  g.splitk = splitk > 0 ? splitk : gemm_pick_splitk(g.M, g.N, g.K, 0);
  if (g.splitk > 1) {
    GILL_TRY(ws.alloc(sizeof(float) * (size_t)g.splitk * g.M * g.N));
    g.ws = (float*)ws.p;
  }
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(gemm_launch(g, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_attention(const void* q, const void* k, const void* v, void* o, int B, int H, int nq, int nkv, int d,
                                 float scale, int causal, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int dp = attn_padded_dim(d);
  GILL_REQUIRE(dp > 0, "attention: head dim > 160 unsupported");
  const int dpv = round_up(dp, 32);
  const int nq_pad = round_up(nq, 32), nkv_pad = round_up(nkv, 32);
  DevBuf Q, K, Vt, O;
  GILL_TRY(Q.alloc_zero(sizeof(bf16_t) * (size_t)B * H * nq_pad * dp, s));
  GILL_TRY(K.alloc_zero(sizeof(bf16_t) * (size_t)B * H * nkv_pad * dp, s));
  GILL_TRY(Vt.alloc_zero(sizeof(bf16_t) * (size_t)B * H * dpv * nkv_pad, s));
  GILL_TRY(O.alloc_zero(sizeof(bf16_t) * (size_t)B * nq * H * dp, s));
  GILL_TRY(pack_heads_launch((const bf16_t*)q, B, nq, H, d, nq_pad, dp, dpv, 0, (bf16_t*)Q.p, s, scale * 1.4426950408889634f));
  GILL_TRY(pack_heads_launch((const bf16_t*)k, B, nkv, H, d, nkv_pad, dp, dpv, 0, (bf16_t*)K.p, s));
  GILL_TRY(pack_heads_launch((const bf16_t*)v, B, nkv, H, d, nkv_pad, dp, dpv, 1, (bf16_t*)Vt.p, s));
  AttnArgs a;
  a.Q = (const bf16_t*)Q.p; a.K = (const bf16_t*)K.p; a.Vt = (const bf16_t*)Vt.p; a.O = (bf16_t*)O.p;
  a.B = B; a.H = H; a.nq = nq; a.nkv = nkv; a.nq_pad = nq_pad; a.nkv_pad = nkv_pad; a.dp = dp; a.dpv = dpv;
  a.ldo = H * dp; a.scale = scale; a.causal = causal; a.d = d;
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_launch(a, s));
  GILL_TRY(unpad_heads_launch((const bf16_t*)O.p, (int64_t)B * nq, H, d, dp, (bf16_t*)o, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_attention_decode(const void* q, const void* k_new, const void* v_new, int ld, void* K, void* Vt, const int32_t* lens, void* o,
                                     int B, int H, int d, int pitch, int32_t* flags, void* stream) {
  AttnDecodeArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K = (bf16_t*)K; a.Vt = (bf16_t*)Vt; a.lens = lens; a.O = (bf16_t*)o; a.ldo = H * d; a.flags = flags;
  a.B = B; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_decode_launch(a, (hipStream_t)stream));
  return 0;
}

extern "C" int gill_attention_append(const void* q, const void* k_new, const void* v_new, int ld, void* K, void* Vt, const int32_t* lens, void* o,
                                     int B, int nq, int H, int d, int pitch, int32_t* flags, void* stream) {
  AttnAppendArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K = (bf16_t*)K; a.Vt = (bf16_t*)Vt; a.lens = lens; a.O = (bf16_t*)o; a.ldo = H * d; a.flags = flags;
  a.B = B; a.nq = nq; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  return attention_append_launch(a, (hipStream_t)stream);
}

extern "C" int gill_attention_extend(const void* q, const void* k_new, const void* v_new, int ld, void* K, void* Vt, const int32_t* lens,
                                     const int32_t* cu_new, void* o, int B, int total_new, int max_new, int H, int d, int pitch, int32_t* flags,
                                     void* stream) {
  AttnExtendArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K = (bf16_t*)K; a.Vt = (bf16_t*)Vt; a.lens = lens; a.cu_new = cu_new; a.O = (bf16_t*)o; a.ldo = H * d; a.flags = flags;
  a.B = B; a.total_new = total_new; a.max_new = max_new; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_extend_launch(a, (hipStream_t)stream));
  return 0;
}

extern "C" int64_t gill_attention_fork_ws_bytes(int C, int H, int d, int max_new) {
  return (int64_t)attention_fork_ws_bytes(C, H, d, max_new);
}

extern "C" int gill_attention_fork(const void* q, const void* k_new, const void* v_new, int ld, const void* K, const void* Vt, const int32_t* parent,
                                   const int32_t* plen, const int32_t* cu_new, void* o, int C, int Bc, int total_new, int max_new, int H, int d,
                                   int pitch, int32_t* flags, void* ws, int64_t ws_bytes, void* stream) {
  GILL_REQUIRE(ws_bytes >= 0, "fork attention: negative workspace size");
  AttnForkArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K = (const bf16_t*)K; a.Vt = (const bf16_t*)Vt; a.parent = parent; a.plen = plen; a.cu_new = cu_new; a.O = (bf16_t*)o; a.ldo = H * d;
  a.flags = flags; a.C = C; a.Bc = Bc; a.total_new = total_new; a.max_new = max_new; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  a.ws = ws; a.ws_bytes = (size_t)ws_bytes;
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_fork_launch(a, (hipStream_t)stream));
  return 0;
}

extern "C" int gill_attention_branch(const void* q, const void* k_new, const void* v_new, int ld, const void* K, const void* Vt, void* Kb, void* Vtb,
                                     const int32_t* gstart, const int32_t* gparent, const int32_t* gplen, const int32_t* lens, void* o, int S,
                                     int G, int Sb, int Bc, int H, int d, int pitch, int bpitch, int32_t* flags, void* stream) {
  AttnBranchArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K = (const bf16_t*)K; a.Vt = (const bf16_t*)Vt; a.Kb = (bf16_t*)Kb; a.Vtb = (bf16_t*)Vtb;
  a.gstart = gstart; a.gparent = gparent; a.gplen = gplen; a.lens = lens; a.O = (bf16_t*)o; a.ldo = H * d; a.flags = flags;
  a.S = S; a.G = G; a.Sb = Sb; a.Bc = Bc; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch; a.bpitch = bpitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  // a repeat stores the same new key and value at the same slot and reads only the slots below it: the same bits every time
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_branch_launch(a, (hipStream_t)stream));
  return 0;
}

extern "C" int gill_kv_branch_adopt(const void* Kb, const void* Vtb, void* K, void* Vt, int Sb, int Bc, int H, int d, int pitch, int bpitch, int s,
                                    int r, int plen, int count, void* stream) {
  KvBranchAdoptArgs a;
  a.Kb = (const bf16_t*)Kb; a.Vtb = (const bf16_t*)Vtb; a.K = (bf16_t*)K; a.Vt = (bf16_t*)Vt;
  a.Sb = Sb; a.Bc = Bc; a.H = H; a.dp = d; a.dpv = round_up(d > 0 ? d : 1, 32); a.pitch = pitch; a.bpitch = bpitch;
  a.s = s; a.r = r; a.plen = plen; a.count = count;
  return kv_branch_adopt_launch(a, (hipStream_t)stream);
}

extern "C" int gill_attention_decode_kv8(const void* q, const void* k_new, const void* v_new, int ld, void* K8, void* Vt8, void* Kexp, void* Vexp,
                                         const int32_t* lens, void* o, int B, int H, int d, int pitch, int32_t* flags, void* stream) {
  AttnDecodeKv8Args a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K8 = (uint8_t*)K8; a.Vt8 = (uint8_t*)Vt8; a.Kexp = (int8_t*)Kexp; a.Vexp = (int8_t*)Vexp;
  a.lens = lens; a.O = (bf16_t*)o; a.ldo = H * d; a.flags = flags;
  a.B = B; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_decode_kv8_launch(a, (hipStream_t)stream));
  return 0;
}

extern "C" int gill_attention_extend_kv8(const void* q, const void* k_new, const void* v_new, int ld, void* K8, void* Vt8, void* Kexp, void* Vexp,
                                         const int32_t* lens, const int32_t* cu_new, void* o, int B, int total_new, int max_new, int H, int d,
                                         int pitch, int32_t* flags, void* stream) {
  AttnExtendKv8Args a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.ld = ld;
  a.K8 = (uint8_t*)K8; a.Vt8 = (uint8_t*)Vt8; a.Kexp = (int8_t*)Kexp; a.Vexp = (int8_t*)Vexp;
  a.lens = lens; a.cu_new = cu_new; a.O = (bf16_t*)o; a.ldo = H * d; a.flags = flags;
  a.B = B; a.total_new = total_new; a.max_new = max_new; a.H = H; a.dp = d; a.dpv = round_up(d, 32); a.pitch = pitch;
  a.qscale = 1.4426950408889634f / sqrtf((float)d);
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(attention_extend_kv8_launch(a, (hipStream_t)stream));
  return 0;
}

extern "C" int gill_op_layernorm(const void* x, int x_f32, const float* gamma, const float* beta, void* y_bf16, int rows,
                                 int C, float eps, void* stream) {
  return layernorm_launch(x, x_f32, gamma, beta, (bf16_t*)y_bf16, rows, C, eps, (hipStream_t)stream);
}

extern "C" int gill_op_groupnorm(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups,
                                 const float* gamma, const float* beta, float eps, int silu, void* y, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DevBuf stats;
  GILL_TRY(stats.alloc(sizeof(float) * groupnorm_stats_floats(B, HW, groups)));
  GILL_TRY(groupnorm_launch((const bf16_t*)x1, C1, (const bf16_t*)x2, C2, B, HW, groups, gamma, beta, eps, silu,
                            (bf16_t*)y, (float*)stats.p, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// fp8 convolution (conv_fp8.hip) on bf16 NHWC input: quantises x (x F8_ACT_SCALE) and the fp32 OIHW weights (per output
// channel), runs the fp8 MFMA kernel (+ the split-K reducer), returns bf16 NHWC.  For tests/test_fp8_gpu.py and tools.
extern "C" int gill_op_conv3x3_fp8(const void* x_bf16, const float* w_oihw, const float* bias, const void* resid_bf16, void* y_bf16,
                                   int B, int H, int W, int Cin, int Cout, int splitk, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x_bf16 && w_oihw && y_bf16, "null argument");
  const int M = B * H * W, Kpad = conv_fp8_kpad(Cin);
  DevBuf x8, w8, sc, ws;
  GILL_TRY(x8.alloc((size_t)M * Cin));
  GILL_TRY(w8.alloc((size_t)Cout * Kpad));
  GILL_TRY(sc.alloc(sizeof(float) * (size_t)Cout));
  GILL_TRY(quant_bf16_fp8_launch((const bf16_t*)x_bf16, F8_ACT_SCALE, (int64_t)M * Cin, (unsigned char*)x8.p, s));
  GILL_TRY(conv_weight_quant_fp8_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, F8_ACT_SCALE, (unsigned char*)w8.p, (float*)sc.p, s));
  ConvF8Args a;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.M = M; a.N = Cout; a.Kpad = Kpad;
  a.A8 = (const unsigned char*)x8.p; a.W8 = (const unsigned char*)w8.p; a.colscale = (const float*)sc.p;
  a.C = (bf16_t*)y_bf16;
  a.splitk = splitk > 0 ? splitk : gemm_pick_splitk(M, Cout, 9 * Cin, 0);
  if (a.splitk > 1) {
    GILL_TRY(ws.alloc(sizeof(float) * (size_t)a.splitk * M * Cout));
    a.ws = (float*)ws.p;
    for (int r = 0; r < op_repeat(); ++r) {
      GILL_TRY(conv3x3_fp8_launch(a, s));
      GemmArgs g;     // finish the partials: + bias + residual -> bf16
      g.M = M; g.N = Cout; g.K = 9 * Cin; g.splitk = a.splitk; g.ws = a.ws; g.bias = bias;
      g.resid = resid_bf16; g.ldr = Cout; g.C = y_bf16; g.ldc = Cout;
      GILL_TRY(gemm_splitk_reduce_launch(g, s));
    }
  } else {
    a.bias = bias; a.resid = (const bf16_t*)resid_bf16;
    for (int r = 0; r < op_repeat(); ++r) GILL_TRY(conv3x3_fp8_launch(a, s));
  }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---- the fp8 path's launchers one by one, on QUANTISED operands in and out (tests/test_fp8_ops_gpu.py): each entry launches exactly the launcher
// the engine launches and synchronises; nothing is quantised behind the caller's back, so the bytes a test reads back are the bytes the next
// kernel multiplies.
extern "C" int gill_conv_fp8_kpad(int Cin) { return Cin > 0 && Cin % 64 == 0 ? conv_fp8_kpad(Cin) : -1; }

extern "C" int gill_op_quant_fp8(const void* x_bf16, float scale, int64_t n, void* y8, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x_bf16 && y8 && n > 0, "quant_fp8: null argument");
  GILL_TRY(quant_bf16_fp8_launch((const bf16_t*)x_bf16, scale, n, (unsigned char*)y8, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_conv_weight_quant_fp8(const void* w_oihw, int dtype, int Cout, int Cin, float act_scale, void* w8, float* colscale,
                                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(w_oihw && w8 && colscale && Cout > 0 && Cin > 0 && act_scale > 0.f, "conv_weight_quant_fp8: bad argument");
  GILL_TRY(conv_weight_quant_fp8_launch(w_oihw, dtype, Cout, Cin, act_scale, (unsigned char*)w8, colscale, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// UNetRun::conv8 on caller bytes: unsplit, bias / row vector / residual / GroupNorm partials (bins of stats_bin channels) in the kernel's own epilogue;
// split (ws [splitk][M][N] fp32 from the caller), the partials and — unless partials_only — the bf16 path's reducer with the same operands.
extern "C" int gill_op_conv3x3_fp8_q(const void* x8, const void* w8, const float* colscale, const float* bias, const float* rowvec,
                                     const void* resid_bf16, void* y_bf16, float* gn_stats, int stats_bin, float* ws, int partials_only, int B, int H,
                                     int W, int Cin, int Cout, int splitk, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x8 && w8 && colscale && B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 64 == 0 && Cout > 0, "conv3x3_fp8_q: bad argument");
  GILL_REQUIRE(splitk >= 1 && (splitk > 1) == (ws != nullptr), "conv3x3_fp8_q: the workspace comes with splitk > 1, and only then");
  GILL_REQUIRE(y_bf16 || (partials_only && splitk > 1), "conv3x3_fp8_q: output missing");
  GILL_REQUIRE((gn_stats != nullptr) == (stats_bin > 0) && (!gn_stats || (splitk == 1 && Cout % stats_bin == 0)),
               "conv3x3_fp8_q: statistics need a bin that divides Cout, and an unsplit launch");
  ConvF8Args a;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.M = B * H * W; a.N = Cout; a.Kpad = conv_fp8_kpad(Cin);
  a.A8 = (const unsigned char*)x8; a.W8 = (const unsigned char*)w8; a.colscale = colscale; a.C = (bf16_t*)y_bf16;
  a.rows_per_batch = H * W;
  a.splitk = splitk;
  if (splitk > 1) {
    a.ws = ws;
    GemmArgs g;
    g.M = a.M; g.N = a.N; g.K = 9 * Cin; g.splitk = splitk; g.ws = ws;
    g.bias = bias; g.rowvec = rowvec; g.rows_per_batch = a.rows_per_batch; g.rowvec_bstride = Cout;
    g.resid = resid_bf16; g.ldr = Cout; g.C = y_bf16; g.ldc = Cout;
    for (int r = 0; r < op_repeat(); ++r) {
      GILL_TRY(conv3x3_fp8_launch(a, s));
      if (!partials_only) GILL_TRY(gemm_splitk_reduce_launch(g, s));
    }
  } else {
    a.bias = bias; a.rowvec = rowvec; a.rowvec_bstride = Cout; a.resid = (const bf16_t*)resid_bf16;
    if (gn_stats) { a.gn_stats = gn_stats; a.gn_groups = Cout / stats_bin; a.gn_cg = stats_bin; }
    for (int r = 0; r < op_repeat(); ++r) GILL_TRY(conv3x3_fp8_launch(a, s));
  }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// groupnorm_launch(..., out8_scale): y8 [B][HW][C1 + C2] e4m3 = fp8(scale * [silu](GroupNorm(x1 ++ x2)))
extern "C" int gill_op_groupnorm_fp8(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups, const float* gamma,
                                     const float* beta, float eps, int silu, float scale, void* y8, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x1 && gamma && beta && y8 && scale > 0.f && B > 0 && HW > 0 && C1 > 0 && C2 >= 0 && groups > 0, "groupnorm_fp8: bad argument");
  DevBuf stats;
  GILL_TRY(stats.alloc(sizeof(float) * groupnorm_stats_floats(B, HW, groups)));
  GILL_TRY(groupnorm_launch((const bf16_t*)x1, C1, (const bf16_t*)x2, C2, B, HW, groups, gamma, beta, eps, silu, (bf16_t*)y8, (float*)stats.p, s,
                            scale));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---- fused GroupNorm statistics on their own (tests/test_gn_stats_gpu.py): the producers' raw partials, and the consumer on caller-made partials.
// Launches `g` with GemmArgs::gn_stats set the way ConvRun::fuse_stats() sets it (bins of `bin` channels, rows_per_batch = output rows per sample),
// forced `splitk` ways (<= 1: unsplit), and reports the slab geometry the launcher used.
static int op_gn_producer_launch(GemmArgs& g, int rows_per_batch, float* stats, int bin, int splitk, int* slab_rows, int* nslab, DevBuf& ws, hipStream_t s) {
  GILL_REQUIRE(stats && slab_rows && nslab && bin > 0 && g.N % bin == 0, "gn_stats producer: bad argument");
  GILL_REQUIRE(gemm_fused_gn_ok(g.N, bin) && rows_per_batch % GN_SLAB_ROWS == 0, "gn_stats producer: no fused statistics for this width / bin / map size");
  g.gn_stats = stats; g.gn_groups = g.N / bin; g.gn_cg = bin;
  g.rows_per_batch = rows_per_batch;
  g.splitk = splitk > 1 ? splitk : 1;
  if (g.splitk > 1) {
    GILL_TRY(ws.alloc(sizeof(float) * (size_t)g.splitk * g.M * g.N));
    g.ws = (float*)ws.p;
  }
  *slab_rows = gemm_gn_slab_rows(g);
  *nslab = rows_per_batch / *slab_rows;
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(gemm_launch(g, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_conv3x3_gn_stats(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias, const float* rowvec,
                                        const void* resid, const void* xs1, int CS1, const void* xs2, int CS2, const float* w_sc, void* y,
                                        float* gn_stats, int bin, int B, int IH, int IW, int Cout, int ups, int splitk, int* slab_rows, int* nslab,
                                        void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int Cin = C1 + C2, CS = xs1 ? CS1 + CS2 : 0, k9 = 9 * Cin, kf = k9 + CS;
  GILL_REQUIRE(x1 && w_oihw && y && Cin > 0, "bad argument");
  GILL_REQUIRE(!ups || (!rowvec && !resid && !xs1), "conv3x3_gn_stats: the four-tap upsample form takes no row vector, residual or shortcut segment");
  GILL_REQUIRE(!xs1 || (w_sc && CS % 64 == 0 && CS1 % 64 == 0 && !rowvec && !resid), "conv3x3_gn_stats: bad shortcut segment");
  DevBuf wr, wf, ws;
  GILL_TRY(wr.alloc(sizeof(bf16_t) * (size_t)Cout * 16 * Cin));     // 9 taps, or 4 classes x 4 taps
  const int chunked = (!ups && conv_k_chunked(IH * IW, Cin, Cout)) ? 1 : 0;
  if (ups) GILL_TRY(conv_weight_relayout_ups4_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  else if (chunked) GILL_TRY(conv_weight_relayout_chunked_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  else GILL_TRY(conv_weight_relayout_launch(w_oihw, GILL_DTYPE_F32, Cout, Cin, (bf16_t*)wr.p, s));
  const bf16_t* wk = (const bf16_t*)wr.p;
  if (CS) {
    GILL_TRY(op_fuse_shortcut_rows((const bf16_t*)wr.p, k9, w_sc, CS, Cout, wf, s));
    wk = (const bf16_t*)wf.p;
  }
  GemmArgs g;
  g.conv = 1; g.IH = IH; g.IW = IW; g.Cin = Cin; g.stride = 1; g.ups = ups ? 2 : 0;
  g.OH = ups ? 2 * IH : IH; g.OW = ups ? 2 * IW : IW;
  g.M = B * g.OH * g.OW; g.N = Cout; g.K = ups ? 4 * Cin : kf;
  g.A = (const bf16_t*)x1; g.A2 = (const bf16_t*)x2; g.K1 = C1;
  g.X1 = (const bf16_t*)xs1; g.X2 = (const bf16_t*)xs2; g.KX = CS; g.KX1 = CS ? CS1 : 0;
  g.W = wk; g.k_chunked = chunked; g.bias = bias;
  g.rowvec = rowvec; g.rowvec_bstride = Cout;
  g.resid = resid; g.ldr = Cout;
  g.C = y; g.ldc = Cout;
  return op_gn_producer_launch(g, g.OH * g.OW, gn_stats, bin, splitk, slab_rows, nslab, ws, s);
}

extern "C" int gill_op_gemm_gn_stats(const void* A, const void* W, const float* bias, const void* resid, void* C, float* gn_stats, int bin, int M, int N,
                                     int K, int rows_per_batch, int splitk, int act, int* slab_rows, int* nslab, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(A && W && C && rows_per_batch > 0 && M % rows_per_batch == 0 && act >= ACT_NONE && act <= ACT_SILU, "bad argument");
  DevBuf ws;
  GemmArgs g;
  g.M = M; g.N = N; g.K = K; g.K1 = K;
  g.A = (const bf16_t*)A; g.lda = K;
  g.W = (const bf16_t*)W; g.bias = bias;
  g.resid = resid; g.ldr = N; g.act = act;
  g.C = C; g.ldc = N;
  return op_gn_producer_launch(g, rows_per_batch, gn_stats, bin, splitk, slab_rows, nslab, ws, s);
}

extern "C" int gill_op_groupnorm_from_stats(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups, const float* gamma,
                                            const float* beta, float eps, int silu, const float* stats1, int bin1, int nslab1,
                                            const float* stats2, int bin2, int nslab2, void* y, float* ss_out, float out8_scale,
                                            void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x1 && gamma && beta && stats1 && (y || ss_out) && C1 > 0 && C2 >= 0 && bin1 > 0 && C1 % bin1 == 0, "bad argument");
  GILL_REQUIRE(out8_scale >= 0.f && (out8_scale == 0.f || (y && !ss_out)), "groupnorm_from_stats: the e4m3 output takes y and no table");
  GILL_REQUIRE((C2 == 0) == (stats2 == nullptr) && (C2 == 0 || (x2 && bin2 > 0 && C2 % bin2 == 0)), "groupnorm_from_stats: second source and its statistics come together");
  GILL_REQUIRE(ss_out == nullptr || C2 == 0, "groupnorm_from_stats: the scale | shift table is for single-source inputs");
  DevBuf tot;      // always passed, as ConvRun::gnorm() does
  GILL_TRY(tot.alloc(sizeof(float) * groupnorm_totals_floats(B, C1 / bin1, C2 ? C2 / bin2 : 0)));
  for (int r = 0; r < op_repeat(); ++r)
    GILL_TRY(groupnorm_apply_launch((const bf16_t*)x1, C1, (const bf16_t*)x2, C2, B, HW, groups, gamma, beta, eps, silu, (bf16_t*)y, stats1, bin1, C1,
                                    nslab1, stats2, C2 ? bin2 : 0, C2 ? nslab2 : 0, s, out8_scale, (float*)tot.p, ss_out));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---- the VAE's single-head attention chain (vae.hip vae_attention_chain(), what VRun::attention runs behind its GroupNorm) on caller tensors.
// The split-K workspace is held to the engine's 16 Mi floats, so every GEMM takes the split the engine gives that shape.
extern "C" int gill_op_vae_attention(const void* n_bf16, const void* resid_bf16, const void* wqkv_bf16, const float* bqkv, const void* wo_bf16,
                                     const float* bo, void* out_bf16, void* P_out_bf16, int B, int HW, int C, int* splits, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(n_bf16 && wqkv_bf16 && bqkv && wo_bf16 && bo && out_bf16 && splits, "vae_attention: null argument");
  GILL_REQUIRE(B >= 1 && HW > 0 && C > 0 && HW % 64 == 0 && C % 64 == 0, "vae_attention: HW and C must be multiples of 64");
  const size_t mc = (size_t)B * HW * C, ws_floats = (size_t)16 << 20;
  DevBuf q, k, vt, o, sc;
  GILL_TRY(q.alloc(sizeof(bf16_t) * mc));
  GILL_TRY(k.alloc(sizeof(bf16_t) * mc));
  GILL_TRY(vt.alloc(sizeof(bf16_t) * mc));
  GILL_TRY(o.alloc(sizeof(bf16_t) * mc));
  if (!P_out_bf16) GILL_TRY(sc.alloc(sizeof(bf16_t) * (size_t)HW * HW));
  VaeAttnArgs a;
  a.n = (const bf16_t*)n_bf16; a.wqkv = (const bf16_t*)wqkv_bf16; a.bqkv = bqkv; a.wo = (const bf16_t*)wo_bf16; a.bo = bo;
  a.q = (bf16_t*)q.p; a.k = (bf16_t*)k.p; a.vt = (bf16_t*)vt.p; a.o = (bf16_t*)o.p;
  a.sc = P_out_bf16 ? (bf16_t*)P_out_bf16 : (bf16_t*)sc.p;
  a.sc_bstride = P_out_bf16 ? (size_t)HW * HW : 0;
  a.ws = op_splitk_ws(ws_floats); a.ws_floats = ws_floats;
  GILL_REQUIRE(a.ws != nullptr, "split-K workspace allocation failed");
  a.B = B; a.HW = HW; a.C = C;
  a.out.resid = resid_bf16; a.out.ldr = C; a.out.C = out_bf16; a.out.ldc = C;
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(vae_attention_chain(a, s));
  for (int i = 0; i < 3; ++i) splits[i] = a.splits[i];
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_row_softmax(void* s_bf16, int rows, int n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(s_bf16 && rows > 0 && n > 0, "row_softmax: bad argument");
  GILL_TRY(vae_row_softmax_launch((bf16_t*)s_bf16, rows, n, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---- the kernels at the ends of the engines (tests/test_ends_gpu.py): conv_out, conv_in (im2col + the K = 64 GEMM), the timestep embedding,
// the transformer block's split-K reducer + LayerNorm, and the lm_head GEMV, each launched the way its engine launches it.
extern "C" int gill_op_conv_out(const void* x_bf16, const void* w_oihw, int w_dtype, const float* bias, float* y_f32, int B, int H, int W, int Cin,
                                int Cout, int force_general, int* path, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x_bf16 && w_oihw && y_f32 && path && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv_out: bad argument");
  DevBuf wr;      // load_conv_out's form: [Cout][9][Cin]
  GILL_TRY(wr.alloc(sizeof(bf16_t) * (size_t)Cout * 9 * Cin));
  GILL_TRY(conv_weight_relayout_launch(w_oihw, w_dtype, Cout, Cin, (bf16_t*)wr.p, s));
  for (int r = 0; r < op_repeat(); ++r)
    GILL_TRY(conv_out_launch((const bf16_t*)x_bf16, (const bf16_t*)wr.p, bias, B, Cin, H, W, Cout, y_f32, s, force_general, path));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// conv_in as the engines run it, K = conv_in_kpad(Cin): one 64-wide step up to 7 input channels, two up to 14 (the inpainting UNet's 9)
static int op_conv_in(const float* x_f32, const void* w_oihw, int w_dtype, const float* bias, void* y_bf16, int B, int Cin, int H, int W, int Cout,
                      uint32_t* counters, int ncounters, hipStream_t s) {
  const int M = B * H * W, kpad = conv_in_kpad(Cin);
  DevBuf tmp, wk, col;
  GILL_TRY(tmp.alloc(sizeof(bf16_t) * (size_t)Cout * 9 * Cin));
  GILL_TRY(wk.alloc_zero(sizeof(bf16_t) * (size_t)Cout * kpad, s));      // rows of kpad: what conv_in_im2col_weight writes
  GILL_TRY(col.alloc(sizeof(bf16_t) * (size_t)M * kpad));
  GILL_TRY(conv_in_im2col_weight(w_oihw, w_dtype, Cin, Cout, (bf16_t*)tmp.p, (bf16_t*)wk.p, s));
  GemmArgs g;      // the UNet's linear(col, kpad, ...)
  g.M = M; g.N = Cout; g.K = kpad; g.K1 = kpad; g.A = (const bf16_t*)col.p; g.lda = kpad; g.W = (const bf16_t*)wk.p; g.bias = bias;
  g.ldr = Cout; g.act = ACT_NONE; g.C = y_bf16; g.ldc = Cout;
  g.splitk = gemm_pick_splitk(M, Cout, kpad, ACT_NONE, true);
  GILL_REQUIRE(g.splitk == 1, "conv_in: one or two K steps cannot split");
  for (int r = 0; r < op_repeat(); ++r) {
    GILL_TRY(im2col_nchw_launch(x_f32, B, Cin, H, W, kpad, (bf16_t*)col.p, s, counters, ncounters));
    GILL_TRY(gemm_launch(g, s));
  }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
extern "C" int gill_op_conv_in(const float* x_f32, const void* w_oihw, int w_dtype, const float* bias, void* y_bf16, int B, int Cin, int H, int W,
                               int Cout, uint32_t* counters, int ncounters, void* stream) {
  GILL_REQUIRE(x_f32 && w_oihw && y_bf16 && B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0 && ncounters >= 0, "conv_in: bad argument");
  GILL_REQUIRE(Cin * 9 <= 64, "conv_in: in_channels * 9 must fit one 64-wide K step");      // (this entry stays the K = 64 form)
  return op_conv_in(x_f32, w_oihw, w_dtype, bias, y_bf16, B, Cin, H, W, Cout, counters, ncounters, (hipStream_t)stream);
}
extern "C" int gill_op_conv_in_wide(const float* x_f32, const void* w_oihw, int w_dtype, const float* bias, void* y_bf16, int B, int Cin, int H,
                                    int W, int Cout, uint32_t* counters, int ncounters, void* stream) {
  GILL_REQUIRE(x_f32 && w_oihw && y_bf16 && B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0 && ncounters >= 0, "conv_in: bad argument");
  GILL_REQUIRE(Cin <= CONV_IN_MAX_CIN, "conv_in: in_channels must be 1 .. 14 (9 * in_channels fits two 64-wide K steps)");
  return op_conv_in(x_f32, w_oihw, w_dtype, bias, y_bf16, B, Cin, H, W, Cout, counters, ncounters, (hipStream_t)stream);
}

extern "C" int gill_op_timestep_embed(const float* t, int n, int dim, void* out_bf16, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(t && out_bf16 && n > 0 && dim > 0, "timestep_embed: bad argument");
  GILL_TRY(timestep_embed_launch(t, n, dim, (bf16_t*)out_bf16, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_reduce_ln(const float* ws, int sk, int M, int D, const float* bias, float* h, const float* g, const float* b, void* nb_bf16,
                                 float eps, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(ws && bias && h && g && b && nb_bf16 && M > 0 && D > 0, "reduce_ln: bad argument");
  GILL_TRY(opt_reduce_ln_launch(ws, sk, M, D, bias, h, g, b, (bf16_t*)nb_bf16, eps, s));      // (h is updated in place: no repeat loop)
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// The two ways TfmRun::linear runs an in-place residual GEMM into the fp32 stream with the LayerNorm behind it, `splitk` ways on row-major weights:
// fuse = 1: partials + opt_reduce_ln_kernel; fuse = 0: the GEMM with its own reducer + layernorm_launch.  eps is the block's 1e-5.
extern "C" int gill_op_linear_reduce_ln(const void* A_bf16, const void* W_bf16, const float* bias, float* h, const float* g, const float* b,
                                        void* nb_bf16, int M, int N, int K, int splitk, int fuse, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(A_bf16 && W_bf16 && bias && h && g && b && nb_bf16 && M > 0, "linear_reduce_ln: bad argument");
  GILL_REQUIRE(splitk > 1 && N % 4 == 0 && N <= 8192, "linear_reduce_ln: splitk > 1, N a multiple of 4, at most 8192");
  float* ws = op_splitk_ws((size_t)splitk * M * N);
  GILL_REQUIRE(ws != nullptr, "split-K workspace allocation failed");
  GILL_TRY(tfm_linear_launch((const bf16_t*)A_bf16, M, (const bf16_t*)W_bf16, 0, bias, N, K, h, ACT_NONE, h, true, splitk, ws, fuse != 0, g, b,
                             (bf16_t*)nb_bf16, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_skinny_gemm(const void* x_bf16, const void* W_bf16, float* out_f32, int M, int N, int K, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x_bf16 && W_bf16 && out_f32 && N > 0 && K > 0, "skinny_gemm: bad argument");
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(skinny_gemm_launch((const bf16_t*)x_bf16, (const bf16_t*)W_bf16, M, N, K, out_f32, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// The fused LM-head loss on its own (lmloss.hip).  One grow-only workspace, like the split-K one above.
extern "C" int gill_op_lm_head_loss(const void* X_bf16, const void* W_bf16, const int64_t* target, int M, int V, int D, float* lse, float* tgt,
                                    int32_t* rank, float* summary, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(M >= 1 && V >= 1, "lm_head_loss: M, V >= 1");
  static void* ws = nullptr;
  static size_t cap = 0;
  const size_t need = lm_loss_workspace_bytes(M, V);
  if (need > cap) {
    if (ws) { GILL_CHECK_HIP(hipDeviceSynchronize()); (void)hipFree(ws); }
    ws = nullptr; cap = 0;
    GILL_CHECK_HIP(hipMalloc(&ws, need + (need >> 2)));
    cap = need + (need >> 2);
  }
  for (int r = 0; r < op_repeat(); ++r)
    GILL_TRY(lm_loss_launch((const bf16_t*)X_bf16, (const bf16_t*)W_bf16, target, M, V, D, lse, tgt, (int*)rank, summary, ws, s));
  return 0;
}

// The image-block heads and the rerank score (img_heads.hip): no host wait.
extern "C" int gill_op_img_block_heads(const float* hidden_f32, int64_t rows, int D, const int32_t* row_idx, int n, const void* Wr_bf16,
                                       const float* br, int E, const void* Wd_bf16, const float* bd, int C, float* ret_emb, float* probs,
                                       int32_t* choice, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  for (int r = 0; r < op_repeat(); ++r)
    GILL_TRY(img_heads_launch(hidden_f32, rows, D, (const int*)row_idx, n, (const bf16_t*)Wr_bf16, br, E, (const bf16_t*)Wd_bf16, bd, C, ret_emb, probs,
                              (int*)choice, s));
  return 0;
}

extern "C" int gill_op_img_rerank_scores(const float* visual_f32, const float* ret_emb_f32, int n, int g, int E, float* scores, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  for (int r = 0; r < op_repeat(); ++r) GILL_TRY(img_rerank_launch(visual_f32, ret_emb_f32, n, g, E, scores, s));
  return 0;
}

extern "C" int gill_lm_loss_geometry(int M, int V, int D, int* row_tile, int* col_tile, int* n_slabs, int* cols_per_slab) {
  GILL_REQUIRE(M >= 1 && V >= 1 && D >= 32 && D % 32 == 0, "lm_loss_geometry: M, V >= 1 and D a positive multiple of 32");
  lm_loss_geometry(M, V, D, row_tile, col_tile, n_slabs, cols_per_slab);
  return 0;
}

// ---- the GEMM launcher's plan, host only (gemm_plan.h; tests/test_gemm_plan_host.py)
// case descriptor of gill_gemm_plan (include/gill_amd.h GILL_GEMM_PLAN_CASE_INTS): the GemmArgs fields a plan reads, pointers as 0 / 1 flags
static void gemm_args_from_desc(const int32_t* c, GemmArgs* out) {
  GemmArgs a;
  int i = 0;
  a.M = c[i++]; a.N = c[i++]; a.K = c[i++]; a.lda = c[i++]; a.ldc = c[i++]; a.ldr = c[i++]; a.K1 = c[i++]; a.conv = c[i++];
  a.IH = c[i++]; a.IW = c[i++]; a.OH = c[i++]; a.OW = c[i++]; a.Cin = c[i++]; a.stride = c[i++]; a.ups = c[i++]; a.pad_shift = c[i++];
  a.KX = c[i++]; a.KX1 = c[i++]; a.k_chunked = c[i++]; a.alpha = c[i++] ? 1.f : 0.5f; a.rows_per_batch = c[i++]; a.resid_f32 = c[i++];
  a.act = c[i++]; a.out_mode = c[i++]; a.heads = c[i++]; a.dp = c[i++]; a.ntok = c[i++]; a.splitk = c[i++]; a.w_blk64 = c[i++];
  a.partials_only = c[i++]; a.gn_groups = c[i++]; a.gn_cg = c[i++]; a.ln_planes = c[i++]; a.wb_rows = c[i++]; a.fn_cg = c[i++];
  static float dummy[4];      // never dereferenced: a plan reads pointers as present / absent
  auto flag = [&](int v) -> void* { return v ? (void*)dummy : nullptr; };
  a.A = (const bf16_t*)flag(c[i++]); a.A2 = (const bf16_t*)flag(c[i++]); a.X1 = (const bf16_t*)flag(c[i++]); a.X2 = (const bf16_t*)flag(c[i++]);
  a.W = (const bf16_t*)flag(c[i++]); a.bias = (const float*)flag(c[i++]); a.rowvec = (const float*)flag(c[i++]); a.resid = flag(c[i++]);
  a.C = flag(c[i++]); a.ws = (float*)flag(c[i++]); a.gn_stats = (float*)flag(c[i++]); a.row_stats = (float*)flag(c[i++]);
  a.ln_stats = (const float*)flag(c[i++]); a.ln_colsum = (const float*)flag(c[i++]); a.fn_Y = (bf16_t*)flag(c[i++]);
  a.fn_gamma = (const float*)flag(c[i++]); a.fn_beta = (const float*)flag(c[i++]); a.coop_ctr = (unsigned*)flag(c[i++]); a.fn_ss = (float*)flag(c[i++]);
  *out = a;
}

static_assert(GILL_GEMM_PLAN_ROW_INTS == 1 + GEMM_PLAN_INTS, "a row = the return code + the plan");
extern "C" int gill_gemm_plan(const int32_t* cases, int n, int pp, int coop, int cus, int32_t* rows) {
  GILL_REQUIRE(n >= 0 && (n == 0 || (cases != nullptr && rows != nullptr)), "gemm_plan: null case list or output");
  const GemmEnv env = {pp, coop, cus};
  for (int i = 0; i < n; ++i) {
    GemmArgs a;
    gemm_args_from_desc(cases + (size_t)i * GILL_GEMM_PLAN_CASE_INTS, &a);
    GemmPlan p;
    int32_t* r = rows + (size_t)i * GILL_GEMM_PLAN_ROW_INTS;
    r[0] = gemm_plan(a, env, &p);      // (a refusal leaves the zero plan)
    const int* v = reinterpret_cast<const int*>(&p);      // (GemmPlan is GEMM_PLAN_INTS ints, in the row's order)
    for (int k = 0; k < GEMM_PLAN_INTS; ++k) r[1 + k] = v[k];
  }
  return 0;
}
extern "C" int gill_gemm_plan_log(int32_t* rows, int cap, int* launched) {
  GILL_REQUIRE(cap >= 0 && launched != nullptr && (cap == 0 || rows != nullptr), "gemm_plan_log: null output or negative capacity");
  GemmPlan plans[GEMM_PLAN_LOG_CAP];
  const int n = gemm_plan_log_take(plans, cap, launched);
  for (int i = 0; i < n; ++i) {
    int32_t* r = rows + (size_t)i * GILL_GEMM_PLAN_ROW_INTS;
    r[0] = 0;
    const int* v = reinterpret_cast<const int*>(&plans[i]);
    for (int k = 0; k < GEMM_PLAN_INTS; ++k) r[1 + k] = v[k];
  }
  return 0;
}
extern "C" int gill_gemm_query(const int32_t* queries, int n, int pp, int coop, int cus, int32_t* answers) {
  GILL_REQUIRE(n >= 0 && (n == 0 || (queries != nullptr && answers != nullptr)), "gemm_query: null query list or output");
  const GemmEnv env = {pp, coop, cus};
  for (int i = 0; i < n; ++i) {
    const int32_t* q = queries + (size_t)i * 7;
    switch (q[0]) {
      case 0: answers[i] = gemm_pick_splitk_env(env, q[1], q[2], q[3], q[4], q[5] != 0, q[6] != 0); break;
      case 1: answers[i] = gemm_pick_splitk_blk64_env(env, q[1], q[2], q[3]); break;
      case 2: answers[i] = gemm_fused_gn_ok(q[1], q[2]) ? 1 : 0; break;
      case 3: answers[i] = gemm_conv_pingpong_env(env, q[1], q[2]) ? 1 : 0; break;
      case 4: answers[i] = conv_k_chunked_env(env, q[1], q[2], q[3]) ? 1 : 0; break;
      case 5: answers[i] = gemm_stream64_weights(q[1], q[2]) ? 1 : 0; break;
      default: GILL_REQUIRE(false, "gemm_query: unknown question");
    }
  }
  return 0;
}

// ---- which kernels a UNet transformer block runs, host only (xf_plan.h; tests/test_xf_plan_host.py)
static_assert(sizeof(XfForms) + sizeof(XfPlan) == GILL_UNET_XF_PLAN_ROW_INTS * sizeof(int), "a row = the forms + the plan, all int");
extern "C" int gill_unet_xf_plan(const int32_t* cases, int n, int lnproj, int xalg, int ffn_fused, int32_t* rows) {
  GILL_REQUIRE(n >= 0 && (n == 0 || (cases != nullptr && rows != nullptr)), "unet_xf_plan: null case list or output");
  const XfEnv env = {lnproj != 0, xalg != 0, ffn_fused != 0};
  for (int i = 0; i < n; ++i) {
    const int32_t* c = cases + (size_t)i * GILL_UNET_XF_PLAN_CASE_INTS;
    const int C = c[0], heads = c[1], Bx = c[6];
    GILL_REQUIRE(C > 0 && heads > 0 && C % heads == 0 && attn_padded_dim(C / heads) > 0 && c[4] > 0 && Bx > 0 && (c[7] == 0 || Bx % 2 == 0),
                 "unet_xf_plan: heads must divide C into a supported head dim; hw and Bx positive; a shared block has an even Bx");
    const XfGeom g = {C, heads, attn_padded_dim(C / heads), c[2], c[3], c[4], c[5] != 0};
    const XfForms f = xf_forms(g, env);
    GILL_REQUIRE(xf_forms_consistent(f), "internal: transformer block forms that exclude each other");
    const XfPlan p = xf_plan(f, g, Bx, c[4], c[7] != 0);
    int32_t* r = rows + (size_t)i * GILL_UNET_XF_PLAN_ROW_INTS;
    const int nf = sizeof f / sizeof(int), np = sizeof p / sizeof(int);      // (both are rows of ints, in the row's order)
    for (int k = 0; k < nf; ++k) r[k] = reinterpret_cast<const int*>(&f)[k];
    for (int k = 0; k < np; ++k) r[nf + k] = reinterpret_cast<const int*>(&p)[k];
  }
  return 0;
}

// ---- which attention kernel gill_op_attention runs, host only (attention_plan.h; tests/test_attention_inst_host.py)
static_assert(sizeof(AttnPlan) == GILL_ATTENTION_PLAN_INTS * sizeof(int), "a row = the plan, all int");
extern "C" int gill_attention_plan(int B, int H, int nq, int nkv, int d, int causal, int att_dma, int32_t* out) {
  GILL_REQUIRE(out != nullptr, "attention_plan: null output");
  GILL_REQUIRE(B > 0 && H > 0 && nq > 0 && nkv > 0 && d > 0, "attention_plan: empty attention");
  const int dp = attn_padded_dim(d);
  GILL_REQUIRE(dp > 0, "attention_plan: head dim > 160 unsupported");
  AttnArgs a;      // the geometry gill_op_attention gives the launcher; a plan reads no pointer
  a.B = B; a.H = H; a.nq = nq; a.nkv = nkv; a.nq_pad = round_up(nq, 32); a.nkv_pad = round_up(nkv, 32); a.dp = dp; a.dpv = round_up(dp, 32);
  a.ldo = H * dp; a.causal = causal; a.d = d;
  const AttnPlan p = attention_plan(a, att_dma != 0);
  for (int k = 0; k < GILL_ATTENTION_PLAN_INTS; ++k) out[k] = reinterpret_cast<const int*>(&p)[k];
  return 0;
}

// ---- the w8 format and its linear on their own (linear_w8.hip; tests/test_w8_ops_gpu.py)
extern "C" int gill_op_w8_quant(const void* w_bf16, int N, int K, void* w8, float* scale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(w8_quant_launch((const bf16_t*)w_bf16, 0, N, K, (unsigned char*)w8, scale, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_w8_dequant(const void* w8, const float* scale, int N, int K, int blk64, void* out_bf16, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(w8_dequant_launch((const unsigned char*)w8, scale, N, K, blk64 != 0, (bf16_t*)out_bf16, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gill_op_linear_w8(const void* A_bf16, const void* w8, const float* scale, const float* bias, const float* resid_f32, void* out, int M,
                                 int N, int K, int act, int out_f32, int splitk, const float* ln_g, const float* ln_b, void* ln_out_bf16,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(A_bf16 && w8 && scale && out, "linear_w8: null operand");
  GILL_REQUIRE(M >= 1 && M <= W8_MAX_ROWS && N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0 && splitk >= 0 && splitk <= K / 64,
               "linear_w8: 1 <= M <= W8_MAX_ROWS; N and K multiples of 64; at most K / 64 slices");
  const int sk = splitk > 0 ? splitk : w8_pick_splitk(N, K);
  const size_t ws_floats = (size_t)sk * M * N;
  float* ws = op_splitk_ws(ws_floats);
  GILL_REQUIRE(ws != nullptr, "split-K workspace allocation failed");
  const bool in_place = resid_f32 == (const float*)out;      // (out is updated in place: no repeat loop)
  for (int r = 0, rep = in_place ? 1 : op_repeat(); r < rep; ++r)
    GILL_TRY(tfm_linear_w8_launch((const bf16_t*)A_bf16, M, (const unsigned char*)w8, scale, bias, N, K, resid_f32, act, out, out_f32 != 0, splitk, ws,
                                  ws_floats, ln_g, ln_b, (bf16_t*)ln_out_bf16, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
