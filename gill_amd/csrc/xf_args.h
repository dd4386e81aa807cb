// The GemmArgs of a transformer block's folded-LayerNorm GEMMs, one builder per form: UNetRun::xf() (unet.hip) and the operator entries
// (unet_ops.hip) launch what these return, so an operator test runs the engine's arguments and not a copy of them.
#pragma once
#include "ops.h"
#include <math.h>

// padded head geometry of the attention operands, and the scale the Q segment carries (attention.hip works in the log2 domain)
struct XfHeads { int heads, d, dp, dpv, hdp; float qscale; };
static inline XfHeads xf_heads(int heads, int d) {
  const int dp = attn_padded_dim(d);
  return XfHeads{heads, d, dp, round_up(dp, 32), heads * dp, 1.4426950408889634f / sqrtf((float)d)};
}

// the row-sum planes a folded LayerNorm reads (GemmArgs::ln_stats / ln_planes / ln_rows)
struct XfLnRows { const float* stats; int planes; int rows; };

// LN(T) W^T + bias on T [M][C], scattered into the OUT_QKV layouts: nseg = 3 -> q | k | v, 1 -> q alone; M = B * ntok
static inline GemmArgs xf_qkv_args(const bf16_t* T, int M, int C, XfLnRows ln, const bf16_t* W, const float* colsum, const float* bias, int nseg,
                                   const XfHeads& h, int ntok, bf16_t* q, bf16_t* k, bf16_t* vt) {
  GemmArgs g;
  g.M = M; g.N = nseg * h.hdp; g.K = C; g.K1 = C; g.A = T; g.lda = C; g.W = W;
  g.ln_stats = ln.stats; g.ln_planes = ln.planes; g.ln_rows = ln.rows; g.ln_colsum = colsum; g.bias = bias;
  g.out_mode = OUT_QKV; g.Cq = q; g.Ck = k; g.Cvt = vt; g.heads = h.heads; g.dp = h.dp; g.dpv = h.dpv;
  g.ntok = ntok; g.ntok_pad_q = g.ntok_pad_kv = round_up(ntok, 32); g.seg_base = 0;      // kv tiles are 32 wide; pad rows hold finite stale data and are masked
  g.qscale = h.qscale;
  return g;
}

// XALG, on the per-sample operands of xalg_operands_launch (Wq_b, cs_b, b_b [B][80 H]...; Wo_b [B][C][80 H]):
//   scores: P [M][80 H] = softmax80(LN(T) Wq_b^T)      values: out = P Wo_b^T + bo + resid (resid may alias out)
static inline void xf_xalg_args(const bf16_t* T, int M, int HW, int C, int heads, XfLnRows ln, const bf16_t* Wq_b, const float* cs_b, const float* b_b,
                                const bf16_t* Wo_b, const float* bo, void* P, const void* resid, void* out, GemmArgs* scores, GemmArgs* values) {
  const int n80 = 80 * heads;
  GemmArgs g;
  g.M = M; g.N = n80; g.K = C; g.K1 = C; g.A = T; g.lda = C; g.W = Wq_b;
  g.wb_rows = HW; g.wb_stride = (int64_t)n80 * C; g.vb_stride = n80;
  g.ln_stats = ln.stats; g.ln_planes = ln.planes; g.ln_rows = ln.rows; g.ln_colsum = cs_b; g.bias = b_b;
  g.out_mode = OUT_SOFTMAX80; g.C = P; g.ldc = n80;
  *scores = g;
  GemmArgs g2;
  g2.M = M; g2.N = C; g2.K = n80; g2.K1 = n80; g2.A = (const bf16_t*)P; g2.lda = n80; g2.W = Wo_b; g2.bias = bo;
  g2.wb_rows = HW; g2.wb_stride = (int64_t)n80 * C;
  g2.resid = resid; g2.ldr = C; g2.C = out; g2.ldc = C;
  *values = g2;
}

// out [M][inner] = value * gelu(gate), [value | gate] = LN(T) W^T + bias on the GEGLU-permuted rows W [2 inner][C]
static inline GemmArgs xf_geglu_args(const bf16_t* T, int M, int C, int inner, XfLnRows ln, const bf16_t* W, const float* colsum, const float* bias, void* out) {
  GemmArgs g;
  g.M = M; g.N = 2 * inner; g.K = C; g.K1 = C; g.A = T; g.lda = C; g.W = W; g.bias = bias;
  g.ln_stats = ln.stats; g.ln_planes = ln.planes; g.ln_rows = ln.rows; g.ln_colsum = colsum;
  g.act = ACT_GEGLU; g.C = out; g.ldc = inner;
  return g;
}
