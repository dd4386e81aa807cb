// Which kernels a UNet transformer block runs: decided here and nowhere else.  Loader::xf asks xf_forms() once per layer for the weight layouts to
// build, UNetRun::xf() and forward() ask xf_plan() once per call for what to launch; the host-only entry gill_unet_xf_plan
// (tests/test_xf_plan_host.py) asks both.  Plain C++: no kernel, no HIP call and no HIP header behind this file (tools/xf_plan_check.cpp compiles it alone).
#pragma once
#include <stdlib.h>

bool ffn_fused_supported(int C, int M);                     // ffn.hip: C = 320, M a positive multiple of its 128-row tile
bool lnproj_supported(int C, int M, int heads, int dp);     // lnproj.hip: C = 320, 8 heads of padded dim 48, M a positive multiple of 128

// The three switches, each default on, '0' = off.  xf_env_default() reads the environment once per process; everything else takes an XfEnv.
//   GILL_UNET_LNPROJ=0     proj_in / QKV and attn1.to_out / attn2.to_q of the level-0 blocks as separate GEMMs, not the fused pairs (lnproj.hip)
//   GILL_UNET_XALG=0       attn2 of levels 1-3 as to_q + attention kernel + to_out, not the two per-sample GEMMs ("XALG": xf_weights.hip)
//   GILL_UNET_FFN_FUSED=0  the level-0 feed-forward as GEGLU + the two-source ffo GEMM, not one kernel (ffn.hip: loop 528.9 -> 522.8 ms)
struct XfEnv { bool lnproj, xalg, ffn_fused; };
inline const XfEnv& xf_env_default() {
  static const XfEnv env = [] {
    auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
    return XfEnv{on("GILL_UNET_LNPROJ"), on("GILL_UNET_XALG"), on("GILL_UNET_FFN_FUSED")};
  }();
  return env;
}

// One layer.  dp: the padded head dim, attn_padded_dim(C / heads); hw: tokens per sample at the layer's level; fp8: gill_unet_config.fp8_convs == 1
struct XfGeom { int C, heads, dp, ctx_len, ctx_dim, hw, fp8; };

// Load time: the weight layouts a layer gets besides the GEMM ones (all int: a row of gill_unet_xf_plan)
struct XfForms {
  int lnproj;      // wqkv1p / wq2p: the K order of the fused projection pairs
  int xalg;        // xg / xgb, and per-sample operands instead of K / V caches
  int ffn_fused;   // w1c / b1c / w2p: the fused feed-forward kernel's layouts
  int ffn_pre;     // ... with wpp, and w1c in the permuted k order: the kernel also runs attn2.to_out (ffn.hip PRE)
  int geglu_fp8;   // wff1_8 / cs_ff1: the GEGLU projection's rows in e4m3
};
inline XfForms xf_forms(const XfGeom& g, const XfEnv& env) {
  const int H = g.heads, hdp = H * g.dp;
  XfForms f;
  f.lnproj = env.lnproj && lnproj_supported(g.C, 128, H, g.dp);
  // cross-attention as two GEMMs: where the 80 key slots per head are no wider than the head itself (d >= 80: SD-1.5 levels 1-3) and a sample is
  // whole 64-row tiles (per-sample weights: a tile must not straddle samples — sample_size 32 / 96 have 16- / 144-token mid blocks)
  f.xalg = env.xalg && H % 2 == 0 && g.ctx_len <= 80 && 80 * H <= hdp && g.dp <= 160 && g.C % 64 == 0 && g.ctx_dim % 64 == 0 && g.hw % 64 == 0;
  f.ffn_fused = env.ffn_fused && ffn_fused_supported(g.C, 128);
  f.ffn_pre = f.ffn_fused && hdp == 384;
  // fp8 mode (BASELINE configs[4]): the GEGLU projection of the blocks that run it as a GEMM (levels 1-3; level 0 has the fused kernel)
  f.geglu_fp8 = g.fp8 && g.C % 128 == 0 && !f.ffn_fused;
  return f;
}
// What xf_plan() relies on; Loader::xf checks it once per layer.  Both fused level-0 forms keep the attention kernel for attn2 — they need 8 heads of
// padded dim 48 (H * dp = 384), XALG needs 80 H <= H * dp — so no geometry gets XALG together with either.
inline bool xf_forms_consistent(const XfForms& f) { return !(f.xalg && (f.lnproj || f.ffn_pre)) && (f.ffn_fused || !f.ffn_pre) && !(f.geglu_fp8 && f.ffn_fused); }

enum { XF_CROSS_ATTN = 0, XF_CROSS_XALG = 1 };
enum { XF_FFN_GEMM = 0, XF_FFN_GEMM_FP8 = 1, XF_FFN_FUSED = 2, XF_FFN_FUSED_PRE = 3 };

// Run time: one call of the block on Bx_full samples of HW tokens (all int, as above)
struct XfPlan {
  int lnproj;      // proj_in + norm1 + QKV, and attn1.to_out + residual + norm2 + attn2.to_q, as one kernel each
  int gn_table;    // ... which takes the block's GroupNorm as a per-(sample, channel) scale | shift table, not as a normalised copy
  int cross;       // XF_CROSS_*
  int ffn;         // XF_FFN_*
  int M, M1;       // rows of the full batch; rows up to the end of the self-attention (half of M on the shared prefix of a CFG pair)
};
// shared: the block's input covers the first half of a CFG pair; it runs at that half batch up to the end of the self-attention
inline XfPlan xf_plan(const XfForms& f, const XfGeom& g, int Bx_full, int HW, bool shared) {
  XfPlan p;
  p.M = Bx_full * HW;
  p.M1 = shared ? p.M / 2 : p.M;
  // Not on the shared-prefix block: its M1 = M / 2 rows are 128 tiles for 256 CUs — one tile per CU takes as long as at full size, the two GEMMs take half.
  p.lnproj = f.lnproj && !shared && lnproj_supported(g.C, p.M, g.heads, g.dp) && HW % 32 == 0;
  p.gn_table = p.lnproj && HW % 128 == 0;
  p.cross = f.xalg ? XF_CROSS_XALG : XF_CROSS_ATTN;
  if (f.ffn_fused && ffn_fused_supported(g.C, p.M) && HW % 128 == 0) p.ffn = f.ffn_pre ? XF_FFN_FUSED_PRE : XF_FFN_FUSED;
  else p.ffn = f.geglu_fp8 ? XF_FFN_GEMM_FP8 : XF_FFN_GEMM;
  return p;
}
