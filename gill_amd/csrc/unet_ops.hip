// The UNet's operator-level entry points (gill_op_*), for tests and tools; their operands come from the engine's own code: sd_schedule.h, xf_weights.h.
#include "sd_schedule.h"
#include "xf_weights.h"
#include "xf_args.h"

// Operator-level entry for the loop's sampler arithmetic: the schedule, the stage and step kernels and the device-side step counter exactly as
// sd_denoise_on (unet.hip) drives them, the UNet replaced by the caller's model outputs.  For tests/test_samplers_gpu.py; synchronises.
// inpaint 1 / 2 (gill_op_sd_inpaint_run): the blend kernel after every step / the concat stage kernel, and unet_in_out (ncalls,Bx,n_in) holds BOTH
// CFG halves of the UNet input; inpaint 0 is the entry as it was.
static int op_sd_sampler_run(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float guidance, const float* latents0,
                             const float* init_noise, const float* model_out, const float* noise, int B, int64_t n, float* lat_out,
                             float* unet_in_out, void* stream, int inpaint = 0, const float* latent_mask = nullptr,
                             const float* masked_latents = nullptr, int64_t hw = 0) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(sampler && latents0 && model_out && lat_out && unet_in_out, "null argument");
  GILL_REQUIRE(B >= 1 && n >= 1 && (int64_t)B * n <= ((int64_t)1 << 28), "B, n out of range");
  GILL_REQUIRE(inpaint == 0 || (init_noise && latent_mask && hw >= 1 && n % hw == 0), "inpaint: init_noise, latent_mask and hw dividing n required");
  SdSchedule sched;
  GILL_TRY(sd_schedule(sampler, v_prediction != 0, num_steps, sched, start));
  GILL_REQUIRE(!sched.needs_noise || noise != nullptr, "this sampler draws noise in its steps: a [ncalls][B][n] noise table is required");
  const bool linear = sched.kind != SD_PNDM, cfg = guidance > 1.0f;
  const int ncalls = (int)sched.timesteps.size(), Bx = cfg ? 2 * B : B;
  const size_t total = (size_t)B * n;
  const size_t n_in = inpaint == 2 ? (size_t)(2 * n + hw) : (size_t)n;     // the UNet input's floats per sample
  DevBuf rows, ctr, gd, slot, lat, lat2, saved, ring, keepd;
  std::vector<float> keep32;
  if (inpaint == 1) {
    std::vector<double> keep;
    GILL_TRY(sd_inpaint_keep(sampler, v_prediction != 0, num_steps, start, sched, keep));
    keep32.assign(keep.begin(), keep.end());
    GILL_TRY(keepd.alloc(sizeof(float) * keep32.size()));
    GILL_CHECK_HIP(hipMemcpyAsync(keepd.p, keep32.data(), keepd.bytes, hipMemcpyHostToDevice, s));
  }
  GILL_TRY(rows.alloc(linear ? sizeof(SamplerRow) * ncalls : sizeof(PlmsRow) * ncalls));
  GILL_CHECK_HIP(hipMemcpyAsync(rows.p, linear ? (const void*)sched.rows.data() : (const void*)sched.plms.data(), rows.bytes, hipMemcpyHostToDevice, s));
  GILL_TRY(ctr.alloc_zero(sizeof(int) * 2, s));
  GILL_TRY(gd.alloc(sizeof(float)));
  GILL_CHECK_HIP(hipMemcpyAsync(gd.p, &guidance, sizeof(float), hipMemcpyHostToDevice, s));
  GILL_TRY(slot.alloc(sizeof(noise)));
  GILL_CHECK_HIP(hipMemcpyAsync(slot.p, &noise, sizeof(noise), hipMemcpyHostToDevice, s));
  GILL_TRY(lat.alloc(sizeof(float) * total)); GILL_TRY(lat2.alloc(sizeof(float) * (size_t)B * n_in * 2));
  GILL_TRY(saved.alloc(sizeof(float) * total)); GILL_TRY(ring.alloc(sizeof(float) * total * 4));
  GILL_CHECK_HIP(hipStreamSynchronize(s));     // the host-side sources above are locals
  if (init_noise) GILL_TRY(add_noise_f32_launch(latents0, init_noise, (float)sched.add_a, (float)sched.add_b, (int64_t)total, (float*)lat.p, s));
  else GILL_TRY(scale_f32_launch(latents0, (float)sched.init_noise_sigma, (int64_t)total, (float*)lat.p, s));
  SdLoopArgs la;
  la.rows = linear ? nullptr : (const PlmsRow*)rows.p; la.ctr = (int*)ctr.p; la.temb_table = nullptr; la.temb_total = 0; la.temb_cur = nullptr;
  la.lat = (float*)lat.p; la.lat2 = (float*)lat2.p; la.cur_sample = (float*)saved.p; la.ets = (float*)ring.p;
  la.B = B; la.n = n; la.guidance = (const float*)gd.p; la.cfg = cfg ? 1 : 0;
  if (linear) { la.srows = (const SamplerRow*)rows.p; la.noise = (const float* const*)slot.p; }
  SdInpaintArgs ia;
  ia.x0 = latents0; ia.z0 = init_noise; ia.mask = latent_mask; ia.xm = masked_latents; ia.keep = (const float*)keepd.p; ia.hw = hw;
  for (int i = 0; i < ncalls; ++i) {
    ia.l = la;
    GILL_TRY(inpaint == 2 ? sd_stage_concat_launch(ia, s) : sd_stage_launch(la, s));
    const size_t in_floats = inpaint ? (size_t)Bx * n_in : total;      // (the plain entries return the first CFG half only)
    GILL_CHECK_HIP(hipMemcpyAsync(unet_in_out + (size_t)i * in_floats, lat2.p, sizeof(float) * in_floats, hipMemcpyDeviceToDevice, s));
    la.eps = model_out + (size_t)i * Bx * n;
    GILL_TRY(linear ? sampler_step_launch(la, s) : plms_step_launch(la, s));
    if (inpaint == 1) GILL_TRY(sd_blend_launch(ia, s));
    GILL_CHECK_HIP(hipMemcpyAsync(lat_out + (size_t)i * total, lat.p, sizeof(float) * total, hipMemcpyDeviceToDevice, s));
  }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
extern "C" int gill_op_sd_sampler_run(const gill_sd_sampler* sampler, int v_prediction, int num_steps, float guidance, const float* latents0,
                                      const float* model_out, const float* noise, int B, int64_t n, float* lat_out, float* unet_in_out,
                                      void* stream) {
  return op_sd_sampler_run(sampler, v_prediction, num_steps, 0, guidance, latents0, nullptr, model_out, noise, B, n, lat_out, unet_in_out, stream);
}
extern "C" int gill_op_sd_sampler_run_from(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float guidance,
                                           const float* latents0, const float* init_noise, const float* model_out, const float* noise, int B,
                                           int64_t n, float* lat_out, float* unet_in_out, void* stream) {
  GILL_REQUIRE(init_noise != nullptr, "null argument");
  return op_sd_sampler_run(sampler, v_prediction, num_steps, start, guidance, latents0, init_noise, model_out, noise, B, n, lat_out, unet_in_out, stream);
}
extern "C" int gill_op_sd_inpaint_run(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float guidance,
                                      const float* latents0, const float* init_noise, const float* latent_mask, const float* masked_latents,
                                      const float* model_out, const float* noise, int B, int64_t n, int64_t hw, float* lat_out,
                                      float* unet_in_out, void* stream) {
  GILL_REQUIRE(init_noise != nullptr && latent_mask != nullptr, "null argument");
  return op_sd_sampler_run(sampler, v_prediction, num_steps, start, guidance, latents0, init_noise, model_out, noise, B, n, lat_out, unet_in_out,
                           stream, masked_latents ? 2 : 1, latent_mask, masked_latents, hw);
}

// Operator-level entry for the fused feed-forward block (ffn.hip) on NATURAL operands (diffusers parameter layouts): folds norm3 into the
// GEGLU projection, builds [Wp.W2 | Wp] and the kernel's weight layouts with the loader's recipes (xf_weights.h), forms the LayerNorm row sums
// of t, launches the kernel.  out = proj_out(ff2(geglu(ff1(LN(t)))) + t) + resid.  For tests/test_ops_gpu.py and tools; synchronises.
// o2 / Wo / bo2 (optional, all or none): the PRE form — t := t + to_out(o2) first, inside the kernel (o2 [M][320] = the cross-attention
// output, heads x 40; Wo [320][320], bo2 [320]: BasicTransformerBlock.attn2.to_out[0]).
// ln_stats (optional, non-PRE form only): the caller's row-sum planes [ln_planes][R][2] (GemmArgs::row_stats layout, R = ln_rows ? ln_rows : M;
// rows m >= R read the sums of row m - R) in place of the one plane the entry forms itself.
static int op_ffn_fused(const void* t, const float* ln_g, const float* ln_b, const void* W1, const float* b1, const void* W2,
                        const float* b2, const void* Wp, const float* bp, const void* resid, void* out, float* gn_stats,
                        int M, int rows_per_batch, const void* o2, const void* Wo, const float* bo2, const float* ln_stats, int ln_planes,
                        int ln_rows, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const XfHeads hd = xf_heads(8, 40);
  const int C = 320, inner = 4 * C, heads = hd.heads, d = hd.d, dp = hd.dp, hdp = hd.hdp;
  GILL_REQUIRE(t && ln_g && ln_b && W1 && b1 && W2 && b2 && Wp && bp && resid && out, "null argument");
  GILL_REQUIRE((o2 != nullptr) == (Wo != nullptr) && (o2 != nullptr) == (bo2 != nullptr), "o2 / Wo / bo2: all or none");
  GILL_REQUIRE(ffn_fused_supported(C, M), "ffn_fused: M must be a multiple of 128");
  GILL_REQUIRE(ln_stats || (ln_planes == 0 && ln_rows == 0), "ffn_fused: ln_planes / ln_rows describe the caller's ln_stats");
  GILL_REQUIRE(!ln_stats || !o2, "ffn_fused: row-sum planes belong to the form without attn2.to_out in front (that one forms its own statistics)");
  GILL_REQUIRE(!ln_stats || (ln_planes >= 1 && ln_rows >= 0 && ln_rows <= M && (ln_rows == 0 || M <= 2 * ln_rows)),
               "ffn_fused: ln_planes >= 1, and rows m >= ln_rows read row m - ln_rows: M <= 2 ln_rows");
  DevBuf idx, wff1, bff1, sff1, wfo, bfo, w1c, b1c, w2p, st, wpp, o2p, wop;
  if (o2) {
    GILL_TRY(wpp.alloc(sizeof(bf16_t) * (size_t)C * C));
    GILL_TRY(o2p.alloc_zero(sizeof(bf16_t) * (size_t)M * hdp, s));
    GILL_TRY(wop.alloc_zero(sizeof(bf16_t) * (size_t)C * hdp, s));
    GILL_TRY(pad_head_cols_launch(o2, 0, M, heads, d, dp, (bf16_t*)o2p.p, s));
    GILL_TRY(pad_head_cols_launch(Wo, 0, C, heads, d, dp, (bf16_t*)wop.p, s));
  }
  GILL_TRY(idx.alloc(sizeof(int32_t) * 2 * inner));
  GILL_TRY(wff1.alloc(sizeof(bf16_t) * (size_t)2 * inner * C)); GILL_TRY(bff1.alloc(sizeof(float) * 2 * inner)); GILL_TRY(sff1.alloc(sizeof(float) * 2 * inner));
  GILL_TRY(xf_geglu_weights((const bf16_t*)W1, b1, inner, C, ln_g, ln_b, (int32_t*)idx.p, (bf16_t*)wff1.p, (float*)bff1.p, (float*)sff1.p, s));
  GILL_TRY(wfo.alloc(sizeof(bf16_t) * (size_t)C * 5 * C)); GILL_TRY(bfo.alloc(sizeof(float) * C));
  GILL_TRY(xf_ffo_weights(Wp, 0, W2, 0, b2, 1, bp, 1, C, (bf16_t*)wfo.p, (float*)bfo.p, s));
  GILL_TRY(w1c.alloc(sizeof(bf16_t) * (size_t)8 * C * C)); GILL_TRY(b1c.alloc(sizeof(float) * 8 * C)); GILL_TRY(w2p.alloc(sizeof(bf16_t) * (size_t)4 * C * C));
  GILL_TRY(ffn_relayout_launch((const bf16_t*)wff1.p, (const float*)bff1.p, (const bf16_t*)wfo.p, (bf16_t*)w1c.p, (float*)b1c.p,
                               (bf16_t*)w2p.p, o2 ? (bf16_t*)wpp.p : nullptr, s));
  FfnArgs fa;
  fa.M = M; fa.T = (const bf16_t*)t;
  if (ln_stats) {
    fa.ln_stats = ln_stats; fa.ln_planes = ln_planes; fa.ln_rows = ln_rows;
  } else {
    GILL_TRY(st.alloc(sizeof(float) * (size_t)M * 2));
    GILL_TRY(row_sums_launch((const bf16_t*)t, M, C, (float*)st.p, s));
    fa.ln_stats = (const float*)st.p; fa.ln_planes = 1;
  }
  fa.W1c = (const bf16_t*)w1c.p; fa.b1c = (const float*)b1c.p; fa.W2p = (const bf16_t*)w2p.p;
  fa.Wfo = (const bf16_t*)wfo.p; fa.bo = (const float*)bfo.p; fa.resid = (const bf16_t*)resid; fa.out = (bf16_t*)out;
  fa.gn_stats = gn_stats; fa.rows_per_batch = rows_per_batch;
  if (o2) { fa.X = (const bf16_t*)o2p.p; fa.Wo = (const bf16_t*)wop.p; fa.bo2 = bo2; fa.Wpp = (const bf16_t*)wpp.p; }
  for (int r = 0, rep = op_repeat(); r < rep; ++r) GILL_TRY(ffn_fused_launch(fa, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
extern "C" int gill_op_ffn_fused(const void* t, const float* ln_g, const float* ln_b, const void* W1, const float* b1, const void* W2,
                                 const float* b2, const void* Wp, const float* bp, const void* resid, void* out, float* gn_stats,
                                 int M, int rows_per_batch, const void* o2, const void* Wo, const float* bo2, void* stream) {
  return op_ffn_fused(t, ln_g, ln_b, W1, b1, W2, b2, Wp, bp, resid, out, gn_stats, M, rows_per_batch, o2, Wo, bo2, nullptr, 0, 0, stream);
}
extern "C" int gill_op_ffn_fused_ex(const void* t, const float* ln_g, const float* ln_b, const void* W1, const float* b1, const void* W2,
                                    const float* b2, const void* Wp, const float* bp, const void* resid, void* out, float* gn_stats,
                                    int M, int rows_per_batch, const void* o2, const void* Wo, const float* bo2, const float* ln_stats,
                                    int ln_planes, int ln_rows, void* stream) {
  return op_ffn_fused(t, ln_g, ln_b, W1, b1, W2, b2, Wp, bp, resid, out, gn_stats, M, rows_per_batch, o2, Wo, bo2, ln_stats, ln_planes, ln_rows,
                      stream);
}

// Operator-level entry for the fp8 GEGLU projection (linear_fp8.hip) on NATURAL operands (diffusers parameter layouts): the loader's GEGLU recipe
// (value / gate interleave, norm3 folded in), then rows and LayerNorm-ed activations quantised to e4m3 as the engine's fp8 mode does, then
// the kernel.  out [M][inner] = h * gelu(g), [h | g] = LN(t) W^T + b (W [2 inner][C], diffusers order [value rows | gate rows]).  C % 128 == 0.
// For tests/test_fp8_gpu.py and tools; synchronises.
extern "C" int gill_op_geglu_fp8(const void* t, const float* ln_g, const float* ln_b, const void* W, const float* b, void* out, int M, int inner, int C,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(t && ln_g && ln_b && W && b && out && M > 0 && inner % 16 == 0 && C % 128 == 0, "geglu_fp8: null argument / inner % 16 / C % 128");
  DevBuf idx, wperm, bperm, cs, w8, sc, st, t8;
  GILL_TRY(idx.alloc(sizeof(int32_t) * 2 * inner));
  GILL_TRY(wperm.alloc(sizeof(bf16_t) * (size_t)2 * inner * C)); GILL_TRY(bperm.alloc(sizeof(float) * 2 * inner)); GILL_TRY(cs.alloc(sizeof(float) * 2 * inner));
  GILL_TRY(xf_geglu_weights((const bf16_t*)W, b, inner, C, ln_g, ln_b, (int32_t*)idx.p, (bf16_t*)wperm.p, (float*)bperm.p, (float*)cs.p, s));
  GILL_TRY(w8.alloc((size_t)2 * inner * C)); GILL_TRY(sc.alloc(sizeof(float) * 2 * inner));
  GILL_TRY(linear_weight_quant_fp8_launch((const bf16_t*)wperm.p, 2 * inner, C, F8_LIN_ACT_SCALE, (unsigned char*)w8.p, (float*)sc.p, s));
  GILL_TRY(st.alloc(sizeof(float) * (size_t)M * 2));
  GILL_TRY(row_sums_launch((const bf16_t*)t, M, C, (float*)st.p, s));
  GILL_TRY(t8.alloc((size_t)M * C));
  LinF8Args a;
  a.M = M; a.N = 2 * inner; a.K = C; a.A8 = (const unsigned char*)t8.p; a.W8 = (const unsigned char*)w8.p; a.colscale = (const float*)sc.p;
  a.bias = (const float*)bperm.p; a.C = (bf16_t*)out;
  for (int r = 0, rep = op_repeat(); r < rep; ++r) {
    GILL_TRY(ln_quant_fp8_launch((const bf16_t*)t, M, C, (const float*)st.p, 1, 0, 1e-5f, F8_LIN_ACT_SCALE, (unsigned char*)t8.p, s));
    GILL_TRY(geglu_fp8_launch(a, s));
  }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// The fp8 GEGLU's three launchers one by one on caller operands (tests/test_fp8_ops_gpu.py; the convolution's are in capi.hip): what goes in and
// comes out is what the engine's kernels read and write, quantised bytes included.  Each synchronises.
extern "C" int gill_op_linear_weight_quant_fp8(const void* w_bf16, int N, int K, float act_scale, void* w8, float* colscale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(w_bf16 && w8 && colscale && N > 0 && K > 0 && act_scale > 0.f, "linear_weight_quant_fp8: bad argument");
  GILL_TRY(linear_weight_quant_fp8_launch((const bf16_t*)w_bf16, N, K, act_scale, (unsigned char*)w8, colscale, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
// stats [planes][R][2] fp32 {sum, sum of squares}, R = ln_rows ? ln_rows : M (GemmArgs::row_stats layout)
extern "C" int gill_op_ln_quant_fp8(const void* t_bf16, int M, int C, const float* stats, int planes, int ln_rows, float eps, float act_scale,
                                    void* y8, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(t_bf16 && stats && y8 && M > 0 && C > 0 && ln_rows >= 0 && ln_rows <= M && (ln_rows == 0 || M <= 2 * ln_rows) && act_scale > 0.f,
               "ln_quant_fp8: bad argument (rows m >= ln_rows read row m - ln_rows: M <= 2 ln_rows)");
  GILL_TRY(ln_quant_fp8_launch((const bf16_t*)t_bf16, M, C, stats, planes, ln_rows, eps, act_scale, (unsigned char*)y8, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
// x8 [M][K], w8 [N][K] in the PHYSICAL row order ([16 value | 16 gate] per 16 outputs), colscale / bias [N] in that order -> out [M][N / 2] bf16
extern "C" int gill_op_geglu_fp8_q(const void* x8, const void* w8, const float* colscale, const float* bias, void* out_bf16, int M, int N, int K,
                                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(x8 && w8 && colscale && out_bf16, "geglu_fp8_q: null argument");
  LinF8Args a;
  a.M = M; a.N = N; a.K = K; a.A8 = (const unsigned char*)x8; a.W8 = (const unsigned char*)w8; a.colscale = colscale; a.bias = bias;
  a.C = (bf16_t*)out_bf16;
  for (int r = 0, rep = op_repeat(); r < rep; ++r) GILL_TRY(geglu_fp8_launch(a, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// Operator-level entry for the fused projection pairs around norm1 / norm2 of a level-0 block (lnproj.hip) on NATURAL operands
// (unpadded heads, plain LayerNorm parameters): the loader's QKV recipe pads / folds / permutes them, then the kernel.
//   mode 0: t = W1 . x + b1;  [q | k | v] = W2 . LN(t)            x [M][320], W2 [3 * 320][320] = to_q | to_k | to_v rows
//   mode 1: t = W1 . x + b1 + t;  q = W2 . LN(t)                  x [M][320] = the attention output (heads x 40), W2 [320][320]
// q, k: [B][8][hw_pad][48] (q scaled by log2(e) / sqrt(40)); vt: [B][8][64][hw_pad] with row 48 = 1.  For tests and tools; synchronises.
// gn_ss (optional, mode 0 with HW % 128 == 0): [B][2][320] GroupNorm scale | shift the kernel applies to the rows of x as it loads them.
static int op_lnproj(int mode, const void* x, void* t, const void* W1, const float* b1, const float* ln_g, const float* ln_b,
                     const void* W2, void* q, void* k, void* vt, int B, int HW, const float* gn_ss, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const XfHeads hd = xf_heads(8, 40);
  const int C = 320, heads = hd.heads, d = hd.d, dp = hd.dp, dpv = hd.dpv, hdp = hd.hdp, M = B * HW;
  const int nseg = mode == 0 ? 3 : 1;
  GILL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 or 1");
  GILL_REQUIRE(x && t && W1 && b1 && ln_g && ln_b && W2 && q && (mode == 1 || (k && vt)), "null argument");
  GILL_REQUIRE(lnproj_supported(C, M, heads, dp), "lnproj: B * HW must be a multiple of 128");
  DevBuf xp, w1p, w2, w2p, cs, cb;
  GILL_TRY(w2.alloc_zero(sizeof(bf16_t) * (size_t)nseg * hdp * C, s));
  GILL_TRY(w2p.alloc(sizeof(bf16_t) * (size_t)nseg * hdp * C));
  GILL_TRY(cs.alloc_zero(sizeof(float) * (size_t)nseg * hdp, s)); GILL_TRY(cb.alloc_zero(sizeof(float) * (size_t)nseg * hdp, s));
  HeadRows seg[3];
  for (int sg = 0; sg < nseg; ++sg) seg[sg] = HeadRows{(const bf16_t*)W2 + (size_t)sg * C * C, 0};
  GILL_TRY(xf_qkv_weights(seg, nseg, nullptr, heads, d, dp, C, ln_g, ln_b, (bf16_t*)w2.p, (float*)cs.p, (float*)cb.p, (bf16_t*)w2p.p, s));
  LnProjArgs a;
  a.mode = mode; a.M = M; a.T = (bf16_t*)t; a.b1 = b1; a.W2p = (const bf16_t*)w2p.p; a.c2 = (const float*)cb.p;
  a.Cq = (bf16_t*)q; a.Ck = (bf16_t*)k; a.Cvt = (bf16_t*)vt; a.heads = heads; a.dp = dp; a.dpv = dpv; a.ntok = HW; a.ntok_pad = round_up(HW, 32);
  a.qscale = hd.qscale; a.gn_ss = gn_ss;
  if (mode == 0) {
    a.X = (const bf16_t*)x; a.W1 = (const bf16_t*)W1;
  } else {
    GILL_TRY(xp.alloc_zero(sizeof(bf16_t) * (size_t)M * hdp, s));
    GILL_TRY(w1p.alloc_zero(sizeof(bf16_t) * (size_t)C * hdp, s));
    GILL_TRY(pad_head_cols_launch(x, 0, M, heads, d, dp, (bf16_t*)xp.p, s));
    GILL_TRY(pad_head_cols_launch(W1, 0, C, heads, d, dp, (bf16_t*)w1p.p, s));
    a.X = (const bf16_t*)xp.p; a.W1 = (const bf16_t*)w1p.p;
  }
  for (int r = 0, rep = op_repeat(); r < rep; ++r) GILL_TRY(lnproj_launch(a, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
extern "C" int gill_op_lnproj(int mode, const void* x, void* t, const void* W1, const float* b1, const float* ln_g, const float* ln_b,
                              const void* W2, void* q, void* k, void* vt, int B, int HW, void* stream) {
  return op_lnproj(mode, x, t, W1, b1, ln_g, ln_b, W2, q, k, vt, B, HW, nullptr, stream);
}
extern "C" int gill_op_lnproj_ex(int mode, const void* x, void* t, const void* W1, const float* b1, const float* ln_g, const float* ln_b,
                                 const void* W2, void* q, void* k, void* vt, int B, int HW, const float* gn_ss, void* stream) {
  return op_lnproj(mode, x, t, W1, b1, ln_g, ln_b, W2, q, k, vt, B, HW, gn_ss, stream);
}

// Op-level entry of the two-GEMM cross-attention ("XALG", xf_weights.hip) on a torch-layout attn2 (to_q / to_out [C][C], to_k / to_v [C][E], heads
// of d = C / H >= 80 features, unpadded, norm2's gain and bias): the loader's recipes fold the weights, xalg_operands_launch builds the per-sample
// operands from `ctx` [B][ctx_len][E] as unet_ctx_cache does, then out = t + softmax(LN(t) Wq^T K^T / sqrt(d)) V Wo^T + bo on t [B * HW][C].
// `P` (optional) receives the softmax weights [B * HW][80 H] (key slot j of head h at column 80 h + j).  For tests and tools; synchronises.
extern "C" int gill_op_cross_attention_folded(const void* t, const float* ln_g, const float* ln_b, const void* Wq, const void* Wk, const void* Wv,
                                              const void* Wo, const float* bo, const void* ctx, void* out, void* P, int B, int HW, int C, int H,
                                              int ctx_len, int E, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(t && ln_g && ln_b && Wq && Wk && Wv && Wo && bo && ctx && out, "null argument");
  GILL_REQUIRE(H > 0 && H % 2 == 0 && C % H == 0, "cross_attention_folded: an even number of heads dividing C");
  const int d = C / H, M = B * HW, n80 = 80 * H;
  GILL_REQUIRE(d % 16 == 0 && d >= 80 && d <= 160 && C % 64 == 0 && E % 64 == 0 && ctx_len >= 1 && ctx_len <= 80 && HW % 64 == 0,
               "cross_attention_folded: head dim 80..160 (multiple of 16), C and E multiples of 64, at most 80 context tokens, HW a multiple of 64");
  DevBuf wq, wkv, cs, cq, xg, xgb, T, mq, mcs, mb, wo, st, p;
  GILL_TRY(wq.alloc(sizeof(bf16_t) * (size_t)C * C)); GILL_TRY(wkv.alloc(sizeof(bf16_t) * (size_t)2 * C * E));      // (dp = d below: this entry takes unpadded heads, every row is written)
  GILL_TRY(cs.alloc(sizeof(float) * C)); GILL_TRY(cq.alloc_zero(sizeof(float) * C, s));
  const HeadRows sq = {Wq, 0}, skv[2] = {{Wk, 0}, {Wv, 0}};
  GILL_TRY(xf_qkv_weights(&sq, 1, nullptr, H, d, d, C, ln_g, ln_b, (bf16_t*)wq.p, (float*)cs.p, (float*)cq.p, nullptr, s));
  GILL_TRY(xf_qkv_weights(skv, 2, nullptr, H, d, d, E, nullptr, nullptr, (bf16_t*)wkv.p, nullptr, nullptr, nullptr, s));
  GILL_TRY(xg.alloc(sizeof(bf16_t) * (size_t)2 * H * C * E)); GILL_TRY(xgb.alloc(sizeof(float) * (size_t)H * E));
  GILL_TRY(xalg_fold_launch((const bf16_t*)wq.p, (const float*)cq.p, (const bf16_t*)wkv.p, (const bf16_t*)Wo, H, C, d, d, E, (bf16_t*)xg.p, (float*)xgb.p, s));
  GILL_TRY(T.alloc(sizeof(bf16_t) * (size_t)B * ctx_len * 2 * H * C));
  GILL_TRY(mq.alloc(sizeof(bf16_t) * (size_t)B * n80 * C)); GILL_TRY(wo.alloc(sizeof(bf16_t) * (size_t)B * n80 * C));
  GILL_TRY(mcs.alloc(sizeof(float) * (size_t)B * n80)); GILL_TRY(mb.alloc(sizeof(float) * (size_t)B * n80));
  GILL_TRY(xalg_operands_launch((const bf16_t*)ctx, (const bf16_t*)xg.p, (const float*)xgb.p, B, H, C, E, ctx_len, (bf16_t*)T.p, (bf16_t*)mq.p,
                                (float*)mcs.p, (float*)mb.p, (bf16_t*)wo.p, s));
  GILL_TRY(st.alloc(sizeof(float) * (size_t)M * 2));
  GILL_TRY(row_sums_launch((const bf16_t*)t, M, C, (float*)st.p, s));
  void* pp = P;
  if (!pp) { GILL_TRY(p.alloc(sizeof(bf16_t) * (size_t)M * n80)); pp = p.p; }
  GemmArgs g, g2;
  xf_xalg_args((const bf16_t*)t, M, HW, C, H, {(const float*)st.p, 1, 0}, (const bf16_t*)mq.p, (const float*)mcs.p, (const float*)mb.p, (const bf16_t*)wo.p,
               bo, pp, t, out, &g, &g2);
  for (int r = 0, rep = op_repeat(); r < rep; ++r) { GILL_TRY(gemm_launch(g, s)); GILL_TRY(gemm_launch(g2, s)); }
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// Operator-level entries for the folded-LayerNorm chain of UNet levels 1-3 (unet.hip xf()): the GEMM that writes the residual stream and files
// its row-sum planes (GemmArgs::row_stats), and the GEMM that reads them back (GemmArgs::ln_stats) in its GEGLU / QKV epilogue or its split-K
// reducer.  The producer builds its GemmArgs as UNetRun::linear() does, the consumer with xf()'s own builders (xf_args.h); both synchronise.  For
// tests/test_ln_gemm_gpu.py and tools.
// splitk: 0 = the engine's heuristic (UNetRun::pick_sk), 1 = unsplit, n > 1 = forced.
static int op_ln_splitk(GemmArgs& g, int splitk, DevBuf& ws) {
  g.splitk = splitk > 0 ? splitk : gemm_pick_splitk(g.M, g.N, g.K, g.act, true, false);
  if (g.splitk > 1) {
    GILL_TRY(ws.alloc(sizeof(float) * (size_t)g.splitk * g.M * g.N));
    g.ws = (float*)ws.p;
  }
  return 0;
}
// Producer.  T [M][N] bf16 = (A [M][K1] ++ A2 [M][K - K1]) . W [N][K]^T + bias + resid (resid may alias T: attn1 / attn2.to_out run in place),
// planes [*nplanes][M][2] fp32 = {sum, sum of squares} of the stored row m over the columns of each plane; *nplanes = gemm_row_planes() of the
// launch (an error when it exceeds planes_cap, the planes the caller's buffer holds).
extern "C" int gill_op_linear_rowstats(const void* A, const void* A2, int K1, const void* W, const float* bias, const void* resid, void* T,
                                       float* planes, int planes_cap, int* nplanes, int M, int N, int K, int splitk, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(A && W && T && planes && nplanes && M > 0 && N > 0 && K > 0, "linear_rowstats: null argument");
  GILL_REQUIRE((A2 != nullptr) == (K1 < K) && K1 > 0 && K1 <= K, "linear_rowstats: A2 if and only if K1 < K");
  DevBuf ws;
  GemmArgs g;
  g.M = M; g.N = N; g.K = K; g.K1 = K1; g.A = (const bf16_t*)A; g.lda = K1; g.A2 = (const bf16_t*)A2; g.lda2 = K - K1;
  g.W = (const bf16_t*)W; g.bias = bias; g.resid = resid; g.ldr = N; g.act = ACT_NONE; g.C = T; g.ldc = N;
  GILL_TRY(op_ln_splitk(g, splitk, ws));
  g.row_stats = planes;
  *nplanes = gemm_row_planes(g);
  GILL_REQUIRE(*nplanes <= planes_cap, "linear_rowstats: the planes buffer is too small for this launch");
  for (int r = 0, rep = resid == T ? 1 : op_repeat(); r < rep; ++r) GILL_TRY(gemm_launch(g, s));      // (in place: a second launch would add the residual twice)
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// Consumer.  LN(T; ln_g, ln_b) W^T + b on T [M][C] bf16 and the caller's row-sum planes [P][R][2] (R = ln_rows, or M when ln_rows == 0; rows
// m >= R read the sums of row m - R), W / b in diffusers layout, permuted / padded and folded by the loader's recipes (xf_weights.h).
//   mode 0 (GEGLU): W [2 inner][C] = [value rows | gate rows], b [2 inner] -> out [M][inner] bf16 = value * gelu(gate).
//   mode 1 (QKV):   W [nseg C][C] = to_q (| to_k | to_v), nseg = 1 | 3, heads * d == C, b [nseg C] or null, M = B * ntok ->
//                   q, k [B][heads][ntok_pad][dp], vt [B][heads][dpv][ntok_pad] (dp = attn_padded_dim(d), dpv = dp rounded up to 32, ntok_pad = ntok
//                   rounded up to 32, q scaled by log2(e) / sqrt(d), row dp of vt = 1 where dpv > dp): what xf() passes.  k, vt unused for nseg = 1.
extern "C" int gill_op_ln_gemm(int mode, const void* T, const float* planes, int P, int ln_rows, const float* ln_g, const float* ln_b, const void* W,
                               const float* b, void* out, void* q, void* k, void* vt, int M, int C, int inner, int nseg, int heads, int d, int ntok,
                               int splitk, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GILL_REQUIRE(mode == 0 || mode == 1, "ln_gemm: mode must be 0 (GEGLU) or 1 (QKV)");
  // no_ln (mode 1 only): the head-major scatter without a folded LayerNorm, as the OPT / CLIP engines' QKV GEMM runs — on a 64 x 64-blocked copy of
  // the padded matrix where the engines block it (gemm_stream64_weights): the one way an operator call reaches the STREAM64 tile's scatter epilogue
  const bool no_ln = mode == 1 && !planes && !ln_g && !ln_b;
  GILL_REQUIRE(T && W && M > 0 && C > 0 && (no_ln || (planes && ln_g && ln_b && P >= 1)), "ln_gemm: null argument");
  GILL_REQUIRE(ln_rows >= 0 && ln_rows <= M && (ln_rows == 0 || 2 * ln_rows >= M), "ln_gemm: ln_rows must cover at least half the rows");
  DevBuf idx, wf, cs, cb, ws, wblk;
  GemmArgs g;
  const XfLnRows ln = {planes, no_ln ? 1 : P, ln_rows};
  if (mode == 0) {
    GILL_REQUIRE(out && b && inner > 0 && inner % 64 == 0, "ln_gemm (GEGLU): output / bias missing, or inner not a multiple of 64");
    const int N = 2 * inner;
    GILL_TRY(idx.alloc(sizeof(int32_t) * N));
    GILL_TRY(wf.alloc(sizeof(bf16_t) * (size_t)N * C)); GILL_TRY(cb.alloc(sizeof(float) * N)); GILL_TRY(cs.alloc(sizeof(float) * N));
    GILL_TRY(xf_geglu_weights((const bf16_t*)W, b, inner, C, ln_g, ln_b, (int32_t*)idx.p, (bf16_t*)wf.p, (float*)cb.p, (float*)cs.p, s));
    g = xf_geglu_args((const bf16_t*)T, M, C, inner, ln, (const bf16_t*)wf.p, (const float*)cs.p, (const float*)cb.p, out);
  } else {
    GILL_REQUIRE((nseg == 1 || nseg == 3) && heads > 0 && d > 0 && heads * d == C && ntok > 0 && M % ntok == 0,
                 "ln_gemm (QKV): nseg 1 or 3, heads * d == C, M a multiple of ntok");
    GILL_REQUIRE(q && (nseg == 1 || (k && vt)), "ln_gemm (QKV): output missing");
    const XfHeads hd = xf_heads(heads, d);
    GILL_REQUIRE(hd.dp > 0, "ln_gemm (QKV): unsupported head dim");
    const int dp = hd.dp, N = nseg * hd.hdp;
    GILL_TRY(wf.alloc_zero(sizeof(bf16_t) * (size_t)N * C, s));
    GILL_TRY(cs.alloc_zero(sizeof(float) * N, s)); GILL_TRY(cb.alloc_zero(sizeof(float) * N, s));
    HeadRows seg[3];
    for (int sg = 0; sg < nseg; ++sg) seg[sg] = HeadRows{(const bf16_t*)W + (size_t)sg * C * C, 0};
    GILL_TRY(xf_qkv_weights(seg, nseg, b, heads, d, dp, C, ln_g, ln_b, (bf16_t*)wf.p, (float*)cs.p, (float*)cb.p, nullptr, s));
    g = xf_qkv_args((const bf16_t*)T, M, C, ln, (const bf16_t*)wf.p, no_ln ? nullptr : (const float*)cs.p, (const float*)cb.p, nseg, hd, ntok, (bf16_t*)q,
                    (bf16_t*)k, (bf16_t*)vt);
    if (no_ln && gemm_stream64_weights(N, C)) {
      GILL_TRY(wblk.alloc(sizeof(bf16_t) * (size_t)N * C));
      GILL_TRY(convert_to_bf16_blk64_launch(wf.p, GILL_DTYPE_BF16, N, C, (bf16_t*)wblk.p, s));
      g.W = (const bf16_t*)wblk.p; g.w_blk64 = 1;
      if (splitk <= 0) splitk = gemm_pick_splitk_blk64(M, N, C);
    }
  }
  GILL_TRY(op_ln_splitk(g, splitk, ws));
  for (int r = 0, rep = op_repeat(); r < rep; ++r) GILL_TRY(gemm_launch(g, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}
