// Load-time weight recipes of the UNet's transformer block, written once: the engine (unet.hip Loader::xf, unet_ctx_cache) and the operator entries
// (unet_ops.hip, capi.hip) both build their operands here, so an operator test checks the layout the engine runs.  A recipe writes buffers its CALLER allocated.
#pragma once
#include "engine_util.h"

// dst[r][h*dp + dd] = src[r][h*d + dd] (dd < d): the head columns of an attention output / a to_out weight padded d -> dp.  dst pre-zeroed.
int pad_head_cols_launch(const void* src, int dtype, int rows, int H, int d, int dp, bf16_t* dst, hipStream_t s);
// stats[m] = {sum, sum of squares} of row m of t [M][C]: one plane of a folded LayerNorm's row sums (in the engine the producing GEMM files them)
int row_sums_launch(const bf16_t* t, int M, int C, float* stats, hipStream_t s);
enum { XF_LAYOUT = 1, XF_FOLD = 2, XF_KPERM = 4, XF_ALL = 7 };   // steps of the two projection recipes: the entries run all in one call, the loader one at a time in its own launch order
struct HeadRows { const void* w; int dtype; };   // one projection weight [H*d][cols] in the checkpoint's dtype (gill_tensor::dtype)
// QKV-style projection: seg[0 .. nseg) stacked, head rows padded d -> dp, into w [nseg*H*dp][cols], `bias` (optional, [nseg*H*d]) likewise into cbias;
// ln_g != nullptr: LayerNorm(ln_g, ln_b) folded in (ln_fold_rows_launch: w scaled in place, colsum written, beta . W^T ADDED to cbias);
// wperm != nullptr: the k-permuted copy of w for lnproj.hip.  w and cbias pre-zeroed (the pad rows stay zero).
int xf_qkv_weights(const HeadRows* seg, int nseg, const float* bias, int H, int d, int dp, int cols, const float* ln_g, const float* ln_b,
                   bf16_t* w, float* colsum, float* cbias, bf16_t* wperm, hipStream_t s, int steps = XF_ALL);
// GEGLU projection: rows of W [2 inner][K] ([value rows | gate rows]) and of b (optional) into the value / gate interleave (geglu_row_permutation;
// idx: [2 inner] device scratch); ln_g != nullptr: the LayerNorm folded in (beta . W^T ADDED to the permuted bias).  The caller's next steps where
// it takes them: the fp8 row quantisation (linear_weight_quant_fp8_launch), the fused kernel's layouts (ffn_relayout_launch).
int xf_geglu_weights(const bf16_t* W, const float* b, int inner, int K, const float* ln_g, const float* ln_b, int32_t* idx, bf16_t* w,
                     float* bias, float* colsum, hipStream_t s, int steps = XF_ALL);
// ff2 + proj_out as one map: w_out [C][5C] = [Wp W2 | Wp], b_out [C] = Wp b2 + bp (ffo_fuse_kernel), every source in its own dtype
int xf_ffo_weights(const void* wp, int dt_p, const void* w2, int dt_2, const void* b2, int dt_b2, const void* bp, int dt_bp, int C,
                   bf16_t* w_out, float* b_out, hipStream_t s);
// Cross-attention as two GEMMs ("XALG", xf_weights.hip), the fold: wq [H*dp][C] (norm2 folded, cq its constant part), wkv [2*H*dp][E], wo [C][H*dp]
// -> xg [2 H C][E] = G | G2, xgb [H][E].
int xalg_fold_launch(const bf16_t* wq, const float* cq, const bf16_t* wkv, const bf16_t* wo, int H, int C, int d, int dp, int E, bf16_t* xg,
                     float* xgb, hipStream_t s);
// Once per prompt: T [B ctx_len][2 H C] = ctx [G | G2]^T (scratch), dealt into the scores operand Mq [B][80 H][C] with its column sums cs and
// constants cb [B][80 H], and the values operand Wo [B][C][80 H].
int xalg_operands_launch(const bf16_t* ctx, const bf16_t* xg, const float* xgb, int B, int H, int C, int E, int ctx_len, bf16_t* T, bf16_t* Mq,
                         float* cs, float* cb, bf16_t* Wo, hipStream_t s);
