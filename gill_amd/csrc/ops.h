// Internal C++ operator layer of libgill_amd: every hot op of the generate_images path as a
// stream-ordered launcher.  The engines (opt.hip / mapper.hip / unet.hip) are sequences of
// these launches; capi.hip re-exports a subset 1:1 for the operator-level parity tests.
#pragma once
#include "common.h"

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_SILU = 3, ACT_GEGLU = 4, ACT_QUICK_GELU = 5 /* x*sigmoid(1.702x): CLIP */ };
enum { OUT_BF16 = 0, OUT_F32 = 1, OUT_QKV = 2, OUT_SOFTMAX80 = 3 };

// C[M,N] = epilogue( alpha * A[M,K] . W[N,K]^T )       (bf16 operands, fp32 MFMA accumulate)
//  A is either a plain row-major matrix (optionally the K-concatenation of two matrices) or the
//  implicit im2col view of an NHWC tensor for a 3x3 / pad 1 convolution (stride 1|2, optional
//  fused nearest-2x upsample, optional channel-concatenation of two NHWC tensors).
struct GemmArgs {
  int M = 0, N = 0, K = 0;
  const bf16_t* A = nullptr;  int lda = 0;
  const bf16_t* A2 = nullptr; int lda2 = 0;
  int K1 = 0;                 // plain: columns taken from A (K1 == K when single source); conv: channels of A
  int conv = 0;               // 0 plain GEMM, 1 conv3x3 pad 1 over NHWC
  int IH = 0, IW = 0, OH = 0, OW = 0, Cin = 0, stride = 1, ups = 0;
  // conv, stride 2 only: the window's origin moves one pixel down and right — output (oy, ox) reads rows 2 oy .. 2 oy + 2 and columns
  // 2 ox .. 2 ox + 2, indices >= IH / IW read zero: diffusers' Downsample2D with padding 0, F.pad(x, (0, 1, 0, 1)) + conv(stride 2, pad 0)
  // (the VAE encoder's downsamplers).  0: the symmetric pad-1 window.  IH, IW even; no upsample, no fused 1x1 segment.
  int pad_shift = 0;
  // conv only: extra plain K segment appended after the 9 taps (a fused 1x1 conv of the tensor X1 ++ X2 at the same
  // pixel, i.e. ResnetBlock2D's conv_shortcut): KX channels in total, the first KX1 from X1
  const bf16_t* X1 = nullptr; const bf16_t* X2 = nullptr; int KX = 0, KX1 = 0;
  const bf16_t* W = nullptr;  // [N][K], K contiguous.  conv: k = tap*Cin + c (conv_weight_relayout_launch), or with k_chunked
                              // k = (c / 64) * 576 + tap * 64 + c % 64 — 64-channel chunks, the 9 taps inside a chunk
                              // (conv_weight_relayout_chunked_launch) — then the KX shortcut channels
  int k_chunked = 0;          // conv: the chunk-major K order.  The 9 shifted reads of a chunk's input patch are then 9
                              // consecutive K steps and hit L2; worth it (conv_k_chunked()) once a sample's input no longer
                              // fits the 4 MiB L2 next to the weights: tap-major re-streams it from the fabric 9 times
                              // (398 MB fetched for a 42 MB input at 64x64x640), but pays one address set-up per K step
  float alpha = 1.f;
  const float* bias = nullptr;
  const float* rowvec = nullptr; int rows_per_batch = 1; int rowvec_bstride = 0;  // + rowvec[(m/rows_per_batch)*bstride + n]
  const void* resid = nullptr; int ldr = 0; int resid_f32 = 0;
  int act = ACT_NONE;
  int out_mode = OUT_BF16;
  void* C = nullptr; int ldc = 0;
  // OUT_QKV: scatter into head-major attention operands.
  //   segment = seg_base + n / (heads*dp): 0 -> Q[b][h][t][dp], 1 -> K[b][h][t][dp], 2 -> Vt[b][h][dd][t]
  bf16_t* Cq = nullptr; bf16_t* Ck = nullptr; bf16_t* Cvt = nullptr;
  int heads = 0, dp = 0, dpv = 0, ntok = 0, ntok_pad_q = 0, ntok_pad_kv = 0, seg_base = 0;
  float qscale = 1.f;   // multiplies the Q segment: softmax scale * log2(e) (attention.hip works in the log2 domain)
  int kv_tok_offset = 0;  // K / Vt rows land at token t + kv_tok_offset (appending to a KV cache); Q rows stay at t
  // split-K (0/1 = off).  ws must hold splitk*M*N floats.
  int splitk = 1; float* ws = nullptr;
  int w_blk64 = 0;         // W is stored as [N / 64][K / 64][64][64] (convert_to_bf16_blk64_launch): the STREAM64 kernel up to GEMM_STREAM64_MAX_ROWS rows, the general tiles above
  int partials_only = 0;   // split-K: write the fp32 partials and stop — the caller runs its own reducer (tfm.hip: reduce + residual + LayerNorm)
  // Both kinds of fused statistics are FIXED-ORDER: a producer writes each partial sum exactly once (no atomics, nothing to
  // zero), the consumer adds the partials in index order, so two runs of the same launch sequence are bit-identical.
  // fused GroupNorm statistics of the output: gn_stats[(b * nslab + slab) * gn_groups + g][2] = {sum, sum of squares} of the
  // STORED (bf16-rounded) values of the gn_cg channels of bin g over the output rows of slab `slab` of sample b = m / rows_per_batch; rows per slab =
  // gemm_gn_slab_rows() (64, or 16 when a split-K reducer with small blocks produces them), nslab = rows_per_batch / that
  // (row-major epilogue only; the tile width must be a multiple of gn_cg: gemm_fused_gn_ok())
  // Statistics source: the in-kernel epilogue and the plain split-K reducer sum the values as stored.  Two producers of this layout still sum the fp32
  // values BEFORE their rounding to bf16 (~1e-4 of a sum away): the fused-norm reducer (gemm_reduce.hip splitk_finish_unit, one slab
  // per sample) and the fp8 convolution's epilogue (conv_fp8.hip); a two-source consumer may therefore read one block of each kind.
  float* gn_stats = nullptr; int gn_groups = 0; int gn_cg = 0;
  // LayerNorm folded into the NEXT GEMM: LN(x) W^T + b = rstd (x (g*W)^T - mean * colsum(g*W)) + (beta W^T + b).
  //  producer: row_stats[(plane * M + m)][2] = {sum, sum of squares} of the bf16-rounded outputs of row m in the columns of
  //            plane `plane` (row-major bf16 epilogue); gemm_row_planes() tells how many planes this launch writes;
  //  consumer: ln_stats = the producer's row_stats of A over ln_planes planes, ln_colsum[n] = sum_k W'[n,k] (W' = g*W is what
  //            `W` holds, and `bias` holds beta W^T + b); mean/rstd over K with eps ln_eps.  GEGLU and QKV epilogues
  //            (+ split-K reducer).
  float* row_stats = nullptr;
  //            ln_rows (0 = M): rows per plane; rows m >= ln_rows read the sums of row m - ln_rows (a batch whose second half
  //            repeats the first: the shared classifier-free-guidance prefix).
  const float* ln_stats = nullptr; int ln_planes = 1; int ln_rows = 0; const float* ln_colsum = nullptr; float ln_eps = 1e-5f;
  // Per-sample operands (the cross-attention of UNet levels 1-3 as two GEMMs, xf_weights.hip "XALG"): rows [b * wb_rows, (b + 1) * wb_rows)
  // multiply W + b * wb_stride (elements); OUT_SOFTMAX80 also reads bias / ln_colsum at + b * vb_stride.  Tiles must not straddle
  // samples (wb_rows % tile rows == 0).  0 = one weight matrix for all rows.
  int wb_rows = 0; int64_t wb_stride = 0; int vb_stride = 0;
  // OUT_SOFTMAX80 (folded-LayerNorm consumer, like OUT_QKV): C[m][80 h .. 80 h + 79] = softmax over the 80 columns of group h of
  // exp2-domain scores rstd (A W^T - mean colsum) + bias; N % 160 == 0; no split-K.  Columns that must not take part carry bias -1e30.
  // split-K only: the GroupNorm (+ SiLU) that consumes this output, run by the reducer itself (gemm_reduce.hip "REDUCE + GROUPNORM"):
  // fn_Y [M][N] bf16 = [silu]((C - mean) * rstd * fn_gamma + fn_beta) with mean / rstd over (rows_per_batch rows, fn_cg channels).
  // C may then be null (the raw tensor has no other reader).  gemm_fused_norm_ok() says which geometries the reducer takes.
  bf16_t* fn_Y = nullptr; const float* fn_gamma = nullptr; const float* fn_beta = nullptr; float fn_eps = 1e-5f; int fn_silu = 0; int fn_cg = 0;
  // COOP (gemm.hip "COOP"): the GroupNorm finish that used to be a second launch, done by the producing kernel's own workgroups, which wait for each other
  // on an arrival counter — legal because the grid is at most one workgroup per CU (gemm_coop_ok() checks it against the device), i.e. co-resident.
  //   splitk == 1 only (3x3 convolutions on the ping-pong tiles): the epilogue publishes its per-slab GroupNorm partials (gn_stats), waits for the other
  //     M tiles of its (sample, N tile), totals them in the consumer's order and writes fn_Y = [silu](GroupNorm(C)) straight from the accumulators
  //     (C itself only when non-null), and / or the per-(sample, channel) scale | shift table fn_ss [B][2][N] (what lnproj.hip applies on load).
  //   (The same hand-off for the split-K reduction measured slower than the reducer launch — profiles/r06_coop_finish.md — and is not in the product.)
  // coop_ctr: one zeroed 32-bit counter per (sample group, N tile) of THIS launch (gemm_coop_counters() says how many).
  unsigned* coop_ctr = nullptr; float* fn_ss = nullptr;
  // Unused word (the flag of the removed in-kernel split-K finish lived here).  GemmArgs travels by value in every GEMM kernel's argument block:
  // without it the struct is 8 bytes shorter, the argument offsets of all 63 gemm_kernel instantiations move and two of them change beyond the offsets
  // (profiles/gemm_prune_isa.md).  The next field added takes its place.
  int spare_word = 0;
};
// gemm_coop_ok(), gemm_coop_counters(), gemm_gn_slab_rows() and gemm_row_planes() read the launch's plan (gemm_plan.h: the host-side decisions of
// gemm_launch(), made in one place) for callers that need the answer before the launch.
// can this launch finish in-kernel (GemmArgs::coop_ctr)?  splitk == 1, geometry of the ping-pong tiles, whole samples per counter group, grid <= CUs of the device.
bool gemm_coop_ok(const GemmArgs& a);
int gemm_coop_counters(const GemmArgs& a);
int gemm_coop_giveups(unsigned* count);      // read + clear the device-side give-up counter of the bounded waits (synchronous)
int gemm_coop_mode();      // GILL_GEMM_COOP: 0 = every finish a launch of its own, anything else (default 1) = GroupNorm finish in the conv epilogue
bool gemm_fused_norm_ok(const GemmArgs& a);
int gemm_launch(const GemmArgs& a, hipStream_t s);
#define GN_SLAB_ROWS 64        // rows per fused GroupNorm-statistics partial of the in-kernel epilogue
#define GN_SLAB_ROWS_MIN 16    // ... of the smallest producer (size statistics buffers for rows / GN_SLAB_ROWS_MIN partials)
int gemm_gn_slab_rows(const GemmArgs& a);
#define GEMM_MAX_ROW_PLANES(N) (((N) + 63) / 64 > 2 * (((N) + 127) / 128) ? ((N) + 63) / 64 : 2 * (((N) + 127) / 128))
// planes of row_stats this launch writes (depends on the tile width and on split-K, both fixed by the arguments)
int gemm_row_planes(const GemmArgs& a);
// can a GEMM with N output columns produce fused GroupNorm statistics for bins of cg channels?
bool gemm_fused_gn_ok(int N, int cg);
// heuristic split-K factor for under-filled grids.  plain: not a conv (64-row tiles available); generic: 128-row 4-wave tiles only (the fp8 conv
// kernel): neither the 64-row nor the ping-pong rules
int gemm_pick_splitk(int M, int N, int K, int act, bool plain = false, bool generic = false);
// STREAM64 (gemm.hip): which weight matrices are stored 64 x 64-blocked, and the split-K factor of a GEMM on one.  Up to GEMM_STREAM64_MAX_ROWS rows
// such a GEMM runs on the 128 x 64 streaming tile, above on the general tiles, which read the blocked layout as well
#ifndef GEMM_STREAM64_MAX_ROWS
#define GEMM_STREAM64_MAX_ROWS 256
#endif
bool gemm_stream64_weights(int N, int K);
int gemm_pick_splitk_blk64(int M, int N, int K);

// split-K reducer of gemm_launch on its own (partials a.ws [splitk][M][N] fp32 written by another kernel: conv_fp8.hip)
int gemm_splitk_reduce_launch(const GemmArgs& a, hipStream_t s);

// 3x3 / pad 1 / stride 1 convolution with fp8 (OCP e4m3) activations and weights on v_mfma_scale_f32_16x16x128_f8f6f4
// (conv_fp8.hip): C[M, N] bf16 = colscale[n] * (A8 (*) W8) + bias + rowvec + resid, M = B*H*W, N = Cout
#define F8_ACT_SCALE 8.0f     // activations are stored as fp8(8 * x): SiLU(GroupNorm) lives in [-0.28, ~8]
struct ConvF8Args {
  int B = 0, H = 0, W = 0, Cin = 0, M = 0, N = 0, Kpad = 0;
  const unsigned char* A8 = nullptr;       // [B][H][W][Cin] fp8
  const unsigned char* W8 = nullptr;       // [N][Kpad] fp8, K order of conv_weight_quant_fp8_launch
  const float* colscale = nullptr;         // [N]: weight scale / activation scale
  const float* bias = nullptr;
  const float* rowvec = nullptr; int rows_per_batch = 1; int rowvec_bstride = 0;
  const bf16_t* resid = nullptr;           // [M][N] bf16
  bf16_t* C = nullptr;                     // [M][N] bf16
  float* gn_stats = nullptr; int gn_groups = 0; int gn_cg = 0;   // fused GroupNorm partials (GemmArgs::gn_stats layout; splitk == 1)
  int splitk = 1; float* ws = nullptr;     // fp32 partials [splitk][M][N]; finish with gemm_splitk_reduce_launch
};
int conv3x3_fp8_launch(const ConvF8Args& a, hipStream_t s);

// GEGLU projection with fp8 (e4m3) activations and weights (linear_fp8.hip): C[M][N / 2] bf16 = (A8 . Wv8^T * sv + bv) * gelu(A8 . Wg8^T * sg + bg),
// W8 [N][K] in the engine's value / gate-interleaved row order (16 value rows | 16 gate rows per 16 outputs), K % 128 == 0
#define F8_LIN_ACT_SCALE 16.0f     // LayerNorm-ed activations are stored as fp8(16 * x): |x| up to 28 sigma in range, the bulk in e4m3's normal range
struct LinF8Args {
  int M = 0, N = 0, K = 0;
  const unsigned char* A8 = nullptr;       // [M][K] fp8: ln_quant_fp8_launch
  const unsigned char* W8 = nullptr;       // [N][K] fp8: linear_weight_quant_fp8_launch
  const float* colscale = nullptr;         // [N]: weight scale / activation scale
  const float* bias = nullptr;             // [N]
  bf16_t* C = nullptr;                     // [M][N / 2] bf16
};
int geglu_fp8_launch(const LinF8Args& a, hipStream_t s);
int linear_weight_quant_fp8_launch(const bf16_t* w, int N, int K, float act_scale, unsigned char* w8, float* colscale, hipStream_t s);
int ln_quant_fp8_launch(const bf16_t* t, int M, int C, const float* ln_stats, int planes, int ln_rows, float eps, float act_scale, unsigned char* y,
                        hipStream_t s);
int conv_fp8_kpad(int Cin);
int quant_bf16_fp8_launch(const bf16_t* x, float scale, int64_t n, unsigned char* y, hipStream_t s);
int conv_weight_quant_fp8_launch(const void* w_oihw, int dtype, int Cout, int Cin, float act_scale, unsigned char* w8, float* colscale,
                                 hipStream_t s);

// Flash-style attention over head-major operands (see GemmArgs OUT_QKV):
//   Q [B][H][nq_pad][dp], K [B][H][nkv_pad][dp], Vt [B][H][dpv][nkv_pad]  ->  O [B*nq][H*dp] (token-major)
struct AttnArgs {
  const bf16_t* Q = nullptr; const bf16_t* K = nullptr; const bf16_t* Vt = nullptr; bf16_t* O = nullptr;
  int B = 0, H = 0, nq = 0, nkv = 0, nq_pad = 0, nkv_pad = 0, dp = 0, dpv = 0;
  int ldo = 0;          // row stride of O in elements (>= H*dp)
  float scale = 1.f;    // informative only: Q must arrive pre-multiplied by scale * log2(e) (GemmArgs::qscale)
  int d = 0;            // the real head dim when known (0: not stated).  dp = 48 with d = 40: the kernel uses padding dim 40 (see QF)
  int causal = 0;
  int kv_bstride_zero = 0;  // 1: K/Vt have a single batch entry shared by every b (learned queries etc.)
  int xcd_map = 1;          // 1: all query tiles of a (sample, head) on one XCD (set by the launcher)
};
int attention_launch(const AttnArgs& a, hipStream_t s);

// Decode attention with append (attention_decode.hip): ONE new token per sequence against that sequence's own cache length.  For (b, h) with
// n = lens[b] read on the device (clamped into [0, pitch - 1]; a clamp sets flags[b] = 1 when flags is given):
//   K[b][h][n][:] = k[b][h dp ..], Vt[b][h][:][n] = v[b][h dp ..] (row dp := 1.0 where dpv > dp, as the QKV epilogue writes it), and
//   O[b][h dp ..] = softmax(qscale * q . [K[0 .. n - 1] ; k]) . [V[0 .. n - 1] ; v]   — the new key and value from the input rows, slots > n never read as data.
// q / k / v: rows of ld elements, head h at column h * dp (the three thirds of a plain (B, 3 D) projection).  dp 64 | 80 | 128.
struct AttnDecodeArgs {
  const bf16_t* q = nullptr; const bf16_t* k = nullptr; const bf16_t* v = nullptr; int ld = 0;
  bf16_t* K = nullptr; bf16_t* Vt = nullptr;     // [B][H][pitch][dp], [B][H][dpv][pitch]
  const int32_t* lens = nullptr;                 // [B] device
  bf16_t* O = nullptr; int ldo = 0;              // [B][ldo], token-major
  int32_t* flags = nullptr;                      // [B] device, nullable
  int B = 0, H = 0, dp = 0, dpv = 0, pitch = 0;
  float qscale = 1.f;                            // log2(e) / sqrt(head dim): the kernel works in the log2 domain
};
int attention_decode_launch(const AttnDecodeArgs& a, hipStream_t s);

// Decode attention with a multi-token append (attention_append.hip): row b brings nq consecutive new tokens, 1 <= nq <= 16, at its own cache length
// n = lens[b] (clamped into [0, pitch - nq]; a clamp sets flags[b]).  q / k / v / O hold B * nq rows, row b * nq + i the token n + i of sequence b.
// Token i is stored at slot n + i and attends to K[0 .. n - 1] and the tokens 0 .. i of its block; slots beyond are never read as data.  A row's O and
// cache are, bit for bit, those of nq successive attention_decode_launch calls with lens = n + i; nq == 1 is that launch.
struct AttnAppendArgs : AttnDecodeArgs {
  int nq = 1;
};
int attention_append_launch(const AttnAppendArgs& a, hipStream_t s);

// Ragged multi-token attention with append (attention_extend.hip): row b brings cu_new[b + 1] - cu_new[b] consecutive new tokens (zero is legal:
// the row is left untouched) at its own cache length n = lens[b], clamped into [0, pitch - count] (a clamp sets flags[b]).  q / k / v / O hold
// total_new packed rows, row cu_new[b] + i the token n + i of sequence b; B in AttnDecodeArgs counts sequences.  Token i is stored at slot n + i
// and attends to the slots 0 .. n + i; slots beyond are excluded by selection.  max_new / total_new: host bounds of the per-row count and of
// cu_new[B] (they size the grid; a row whose device values exceed them is treated as empty and flagged).  Flash pattern on bf16 MFMA; the
// accuracy bar of the decode kernels, not their bits.
struct AttnExtendArgs : AttnDecodeArgs {
  const int32_t* cu_new = nullptr;               // [B + 1] device
  int total_new = 0, max_new = 0;
};
int attention_extend_launch(const AttnExtendArgs& a, hipStream_t s);

// The same two operators on an e4m3 cache (attention_decode_kv8.hip, attention_extend_kv8.hip; the format: attention_kv8_dev.h).  Every key row
// and value row of a (token, head) is dp e4m3 bytes and one int8 exponent e (scale 2^e): K8 [B][H][pitch][dp], Vt8 [B][H][dpv][pitch] bytes (rows
// dp .. dpv - 1 are never read as data and never written: no ones-row), Kexp / Vexp [B][H][pitch].  Every key and value, the new tokens' own
// included, is rounded to its e4m3 row before any query uses it, so the result is a function of the token sequence, not of how it was fed.
// Lengths, clamps, flags, q / k / v and O as in AttnDecodeArgs / AttnExtendArgs.
struct AttnDecodeKv8Args {
  const bf16_t* q = nullptr; const bf16_t* k = nullptr; const bf16_t* v = nullptr; int ld = 0;
  uint8_t* K8 = nullptr; uint8_t* Vt8 = nullptr; int8_t* Kexp = nullptr; int8_t* Vexp = nullptr;
  const int32_t* lens = nullptr;
  bf16_t* O = nullptr; int ldo = 0;
  int32_t* flags = nullptr;
  int B = 0, H = 0, dp = 0, dpv = 0, pitch = 0;
  float qscale = 1.f;
};
int attention_decode_kv8_launch(const AttnDecodeKv8Args& a, hipStream_t s);
struct AttnExtendKv8Args : AttnDecodeKv8Args {
  const int32_t* cu_new = nullptr;
  int total_new = 0, max_new = 0;
};
int attention_extend_kv8_launch(const AttnExtendKv8Args& a, hipStream_t s);

// Fork attention (attention_fork.hip): C packed candidate continuations against the read-only prefixes of a bf16 cache.  Candidate c brings
// cu_new[c + 1] - cu_new[c] packed rows (zero is legal: nothing is stored for it), names its cache row parent[c] in [0, Bc) and sees that row's
// slots 0 .. plen[c] - 1 (zero is legal: it attends to itself only); token i attends to [K[p][0 .. n - 1] ; k_0 .. k_i].  K / Vt are never
// written.  n outside [0, pitch] is clamped (flags[c] = 1); a parent outside [0, Bc), a count outside [0, max_new] or a packed range outside
// [0, total_new) make the candidate empty and flagged.  A candidate's output bits depend on its own packed operands, its prefix and n only.
// ws / ws_bytes: the caller's workspace of at least attention_fork_ws_bytes(C, H, dp, max_new) bytes (0 today: ws may then be null).
struct AttnForkArgs {
  const bf16_t* q = nullptr; const bf16_t* k = nullptr; const bf16_t* v = nullptr; int ld = 0;
  const bf16_t* K = nullptr; const bf16_t* Vt = nullptr;      // [Bc][H][pitch][dp], [Bc][H][dpv][pitch]
  const int32_t* parent = nullptr; const int32_t* plen = nullptr; const int32_t* cu_new = nullptr;   // [C], [C], [C + 1] device
  bf16_t* O = nullptr; int ldo = 0;
  int32_t* flags = nullptr;                                   // [C] device, nullable
  int C = 0, Bc = 0, H = 0, dp = 0, dpv = 0, pitch = 0, total_new = 0, max_new = 0;
  float qscale = 1.f;                                         // log2(e) / sqrt(head dim)
  void* ws = nullptr; size_t ws_bytes = 0;
};
size_t attention_fork_ws_bytes(int C, int H, int d, int max_new);   // host only
int attention_fork_launch(const AttnForkArgs& a, hipStream_t s);

// Branch decode attention (attention_branch.hip): S branches, ONE new token each, packed in G groups of at most 32 siblings.  Group g holds the
// branches gstart[g] .. gstart[g + 1] - 1; all of them attend to the slots 0 .. gplen[g] - 1 of main-cache row gparent[g] (K / Vt: const, read
// once per (group, head)) and each to its own branch-cache row: branch s has m = lens[s] - gplen[g] own cached tokens in Kb[s] / Vtb[s] and
// stores its new key / value at slot m there.  O[s] = softmax(qscale * q_s . [K[p][0 .. n - 1] ; Kb[s][0 .. m - 1] ; k_s]) . [V.. ; Vb.. ; v_s].
// n outside [0, pitch] or m outside [0, bpitch - 1] is clamped (flags[s] = 1); a parent outside [0, Bc) or a group of more than 32 / a range
// outside [0, S] empties the group (flagged, no read through it).  A branch's bits depend on its own operands, its prefix, n, its row and m only.
struct AttnBranchArgs {
  const bf16_t* q = nullptr; const bf16_t* k = nullptr; const bf16_t* v = nullptr; int ld = 0;       // S rows
  const bf16_t* K = nullptr; const bf16_t* Vt = nullptr;      // [Bc][H][pitch][dp], [Bc][H][dpv][pitch]
  bf16_t* Kb = nullptr; bf16_t* Vtb = nullptr;                // [Sb][H][bpitch][dp], [Sb][H][dpv][bpitch]
  const int32_t* gstart = nullptr; const int32_t* gparent = nullptr; const int32_t* gplen = nullptr;   // [G + 1], [G], [G] device
  const int32_t* lens = nullptr;                              // [S] device: the branch's total position
  bf16_t* O = nullptr; int ldo = 0;
  int32_t* flags = nullptr;                                   // [S] device, nullable
  int S = 0, G = 0, Sb = 0, Bc = 0, H = 0, dp = 0, dpv = 0, pitch = 0, bpitch = 0;
  float qscale = 1.f;                                         // log2(e) / sqrt(head dim)
};
int attention_branch_launch(const AttnBranchArgs& a, hipStream_t s);

// Adopt a branch into its dialogue (attention_branch.hip): Kb[s][h][0 .. count - 1] -> K[r][h][plen .. plen + count - 1], the matching columns of
// Vtb[s] -> Vt[r], and the ones-row entry Vt[r][h][dp][slot] = 1 where dpv > dp (as attention_append writes it).  Host values; errors that
// launch nothing: plen + count > pitch - 1, count > bpitch, s outside [0, Sb), r outside [0, Bc).  count == 0 is legal (nothing is launched).
struct KvBranchAdoptArgs {
  const bf16_t* Kb = nullptr; const bf16_t* Vtb = nullptr; bf16_t* K = nullptr; bf16_t* Vt = nullptr;
  int Sb = 0, Bc = 0, H = 0, dp = 0, dpv = 0, pitch = 0, bpitch = 0;
  int s = 0, r = 0, plen = 0, count = 0;
};
int kv_branch_adopt_launch(const KvBranchAdoptArgs& a, hipStream_t s);


// The feed-forward sub-block + proj_out + outer residual of a level-0 transformer block (C = 320) as one kernel (ffn.hip):
//   out = [Wp.W2 | Wp] . [ value * gelu(gate) | t ] + bo + resid,  [value | gate] = W1' . LN(t) + b1'  (LN from the row-sum planes).
// W1c / b1c / W2p: ffn_relayout_launch() of the engine's wff1 / bff1 (LayerNorm-folded GEGLU rows) and wfo ([Wp.W2 | Wp], [C][5C]).
struct FfnArgs {
  int M = 0;
  const bf16_t* T = nullptr;                                           // [M][320] residual stream (raw)
  const float* ln_stats = nullptr; int ln_planes = 0, ln_rows = 0; float ln_eps = 1e-5f;
  const bf16_t* W1c = nullptr; const float* b1c = nullptr;             // [20][128][320], [20][128]
  const bf16_t* W2p = nullptr;                                         // [320][1280], hidden order permuted within every 16
  const bf16_t* Wfo = nullptr; const float* bo = nullptr;              // [320][1600] (its last 320 columns = Wp), [320]
  const bf16_t* resid = nullptr; bf16_t* out = nullptr;                // [M][320]
  float* gn_stats = nullptr; int rows_per_batch = 0;                   // optional: GroupNorm partials of the output, bins of 5 channels,
                                                                       // [(b * rows_per_batch / 64 + slab) * 64 + bin][2] (GemmArgs::gn_stats layout)  // X != nullptr: the block's attn2.to_out + residual run in front, inside the kernel: t = Wo . X + bo2 + T (T = the stream BEFORE
  // attn2.to_out; t is never stored, its LayerNorm statistics are formed in registers: ln_stats unused).  W1c then in the permuted k
  // order and Wpp = Wp with it (ffn_relayout_launch with Wpp != nullptr).
  const bf16_t* X = nullptr;                                           // [M][384] cross-attention output (8 heads x padded 48)
  const bf16_t* Wo = nullptr; const float* bo2 = nullptr;              // [320][384], [320]
  const bf16_t* Wpp = nullptr;                                         // [320][320]
};
bool ffn_fused_supported(int C, int M);
int ffn_relayout_launch(const bf16_t* wff1, const float* bff1, const bf16_t* wfo, bf16_t* W1c, float* b1c, bf16_t* W2p, bf16_t* Wpp,
                        hipStream_t s);
int ffn_fused_launch(const FfnArgs& a, hipStream_t s);

// Two GEMMs of a level-0 transformer block around a LayerNorm as one kernel (lnproj.hip):
//   mode 0: T = W1 . X + b1 (proj_in, K1 = 320);  [q | k | v] = W2p . LN(T) + c2 scattered head-major (three segments of 384 columns)
//   mode 1: T = W1 . X + b1 + T (attn1.to_out, K1 = 384, in place);  q = W2p . LN(T) + c2 (one segment)
// W2p: lnproj_kperm_launch() of the engine's LayerNorm-folded wqkv1 / wq2; c2 their folded bias (ln_fold_rows_launch).
struct LnProjArgs {
  int mode = 0;
  int M = 0;
  const bf16_t* X = nullptr;       // [M][K1]
  bf16_t* T = nullptr;             // [M][320] residual stream (written; mode 1: read as the residual first)
  const bf16_t* W1 = nullptr;      // [320][K1]
  const float* b1 = nullptr;       // [320]
  const bf16_t* W2p = nullptr;     // [nseg * 384][320], K order permuted
  const float* c2 = nullptr;       // [nseg * 384]
  float ln_eps = 1e-5f;
  bf16_t *Cq = nullptr, *Ck = nullptr, *Cvt = nullptr;       // GemmArgs' OUT_QKV layout
  int heads = 0, dp = 0, dpv = 0, ntok = 0, ntok_pad = 0, seg_base = 0;
  float qscale = 1.f;
  // mode 0: X is the RAW block input and gn_ss [B][2][320] its GroupNorm scale / shift (groupnorm_apply_launch(..., ss_out)): the kernel
  // normalises the rows it has just loaded, y = bf16(x * scale + shift) as the stand-alone pass rounds it (ntok % 128 == 0)
  const float* gn_ss = nullptr;
};
bool lnproj_supported(int C, int M, int heads, int dp);
int lnproj_kperm_launch(const bf16_t* src, int N, bf16_t* dst, hipStream_t s);
int lnproj_launch(const LnProjArgs& a, hipStream_t s);

// LayerNorm over the last dim (eps inside sqrt), fp32 or bf16 rows in, bf16 rows out.
int layernorm_launch(const void* x, int x_f32, const float* gamma, const float* beta, bf16_t* y,
                     int rows, int C, float eps, hipStream_t s);
// same but fp32 output (used for the final norms whose result is returned to the caller)
int layernorm_f32out_launch(const void* x, int x_f32, const float* gamma, const float* beta, float* y,
                            int rows, int C, float eps, hipStream_t s);

// GroupNorm (+ optional SiLU) over NHWC bf16, input = channel-concat of up to two tensors.
//   stats: fp32 scratch of groupnorm_stats_floats(B, HW, groups) floats (per-slab partial sums, written here).
#define GN_STATS_ROWS 32       // pixels per partial of the stand-alone statistics pass
static inline size_t groupnorm_stats_floats(int B, int HW, int groups) {
  return (size_t)B * ((HW + GN_STATS_ROWS - 1) / GN_STATS_ROWS) * groups * 2 + (size_t)B * groups * 2;   // partials + totals scratch
}
// floats of the totals scratch groupnorm_apply_launch needs when a statistics block holds more than 64 partials per bin
static inline size_t groupnorm_totals_floats(int B, int nbins1, int nbins2) { return (size_t)B * (nbins1 + nbins2) * 2; }
int groupnorm_launch(const bf16_t* x1, int C1, const bf16_t* x2, int C2, int B, int HW, int groups,
                     const float* gamma, const float* beta, float eps, int silu, bf16_t* y,
                     float* stats, hipStream_t s, float out8_scale = 0.f);
// normalise from per-slab partial sums written in bins by producer epilogues (GemmArgs::gn_stats layout: nslab1 / nslab2
// partials per (sample, bin)); groupnorm_bins_align() tells whether a (channels per group, split point, bin sizes)
// combination is usable
int groupnorm_apply_launch(const bf16_t* x1, int C1, const bf16_t* x2, int C2, int B, int HW, int groups, const float* gamma,
                           const float* beta, float eps, int silu, bf16_t* y, const float* stats1, int bin1, int sc1, int nslab1,
                           const float* stats2, int bin2, int nslab2, hipStream_t s, float out8_scale = 0.f,
                           float* tot_scratch = nullptr, float* ss_out = nullptr);
// ss_out != nullptr: nothing is normalised — the per-(sample, channel) scale and shift are written as [B][2][C] floats for a consumer
// that applies y = bf16(x * scale + shift) itself (lnproj.hip mode 0: the transformer block's GroupNorm on its way into proj_in)
// out8_scale > 0: y is an fp8 (e4m3) tensor [B][HW][C] holding fp8(out8_scale * value) — the A operand of conv3x3_fp8_launch
bool groupnorm_bins_align(int cg, int sc1, int bin1, int bin2);

// ---- small elementwise / gather kernels ----
int embed_rows_bf16_launch(const int64_t* ids, const bf16_t* table, int vocab, int n, int D, bf16_t* out, hipStream_t s);
int embed_tokens_launch(const int64_t* ids, const bf16_t* table, int vocab, const bf16_t* extra, int n_extra, const bf16_t* pos_table,
                        int pos_offset, int B, int T, int D, float* out_f32, hipStream_t s);   // id < 0: row -(id + 1) of extra (n_extra > 0)
int gather_rows_launch(const void* src, int src_f32, const int32_t* row_idx, int nrows, int D, void* dst, int dst_f32,
                       hipStream_t s);
int add_cast_launch(const void* a, int a_f32, const void* b, int b_f32, int64_t n, int64_t b_period, bf16_t* out,
                    hipStream_t s);  // out = bf16(a + b[i % b_period])
int cast_f32_to_bf16_launch(const float* x, bf16_t* y, int64_t n, hipStream_t s);
int cast_bf16_to_f32_launch(const bf16_t* x, float* y, int64_t n, hipStream_t s);
int timestep_embed_launch(const float* t, int n, int dim, bf16_t* out, hipStream_t s);  // [n][dim] = [cos | sin]
int silu_bf16_launch(const bf16_t* x, bf16_t* y, int64_t n, hipStream_t s);
// im2col of a tiny-Cin NCHW fp32 tensor for conv_in: out [B*H*W][kpad] bf16, k = tap*Cin + c (zero beyond 9*Cin)
int im2col_nchw_launch(const float* x, int B, int Cin, int H, int W, int kpad, bf16_t* out, hipStream_t s, unsigned* zero = nullptr, int nzero = 0);
// conv_out: NHWC bf16 (B,H,W,Cin) -> NCHW fp32 (B,Cout,H,W), 3x3 pad 1, direct (Cout tiny)
int conv_out_launch(const bf16_t* x, const bf16_t* w /*[Cout][9][Cin]*/, const float* bias, int B, int Cin, int H, int W,
                    int Cout, float* y, hipStream_t s, int force_general = 0, int* path = nullptr);
// skinny GEMV-ish: out[M][N] (f32) = x[M][K] (bf16) . W[N][K]^T ; M <= 8, any N (lm_head)
int skinny_gemm_launch(const bf16_t* x, const bf16_t* W, int M, int N, int K, float* out, hipStream_t s);
// ---- LM-head loss without a logits tensor (lmloss.hip; HF CrossEntropyLoss over lm_head(hidden_states[-1]) + utils.accuracy's topk) ----
// Per row of X (M, D) bf16 against W (V, D) bf16 row-major and target (M) int64 (-100: ignored; other values clamped into [0, V)):
// lse = log sum_c exp(logit[c]), tgt = logit[target], rank = #{c != target: logit[c] > tgt or (logit[c] == tgt and c < target)}; an ignored row
// gets rank -1 and lse = tgt = 0.  summary (nullable) [4] = {mean of lse - tgt over valid rows (NaN when none), n_valid, #rank < 1, #rank < 5}.
// workspace: lm_loss_workspace_bytes(M, V) bytes of device memory (partials; nothing to zero).  D % 32 == 0.  No (M, V) buffer anywhere.
void lm_loss_geometry(int M, int V, int D, int* row_tile, int* col_tile, int* n_slabs, int* cols_per_slab);   // host only; any output may be null
size_t lm_loss_workspace_bytes(int M, int V);
int lm_loss_launch(const bf16_t* X, const bf16_t* W, const int64_t* target, int M, int V, int D, float* lse, float* tgt, int* rank, float* summary,
                   void* workspace, hipStream_t s);
// ---- the image-block heads and the rerank score (img_heads.hip; models.py:671-676, :698-704, :733-751) ----
// n blocks in one launch, one workgroup each; Wr / br and Wd / bd nullable as pairs (not both).  Arguments are checked before anything is enqueued.
int img_heads_launch(const float* hidden, int64_t rows, int D, const int* row_idx, int n, const bf16_t* Wr, const float* br, int E, const bf16_t* Wd,
                     const float* bd, int C, float* ret_emb, float* probs, int* choice, hipStream_t s);
// scores (n, g) = cos(visual[b g + j], ret_emb[b]); zero rows give 0
int img_rerank_launch(const float* visual, const float* ret_emb, int n, int g, int E, float* scores, hipStream_t s);
// ---- decode decision of the generate loop (decode.hip; models.py:471-520) ----
constexpr int kDecodeMaxIds = 16;
struct DecodeRuleDev {          // gill_decode_rule resolved on the host: ids in [0, vocab), conditions evaluated
  int vocab;
  int n_ret, n_gen;
  int ret[kDecodeMaxIds], gen[kDecodeMaxIds];       // normalised like a torch index (negative counts from the end)
  int64_t ret_raw[kDecodeMaxIds];                   // as given: what the forced step emits (:520)
  int64_t ret0_raw;
  int special;                  // ids present and ret[0] != -1 and gen[0] != -1 (:478)
  int suppress;                 // step < min_word_tokens (:479)
  int do_ret_scale, do_gen_scale;
  float ret_scale, gen_scale, filter_value;
  int ret_eq_gen;
};
// rule + torch.argmax per row (in place), then the [IMG] forcing of B == 1, the emitted ids into tokens[b][col ..], their count
// (-1: forced [IMG0] with ret != gen) into *n_out and their bf16 embedding rows into next_embeds row b + j
int decode_rule_pick_launch(float* logits, int B, int V, const DecodeRuleDev& r, const bf16_t* table, int D, int64_t* tokens,
                            int ld, int col, int32_t* n_out, bf16_t* next_embeds, hipStream_t s);
int decode_rule_launch(float* logits, int B, int V, const DecodeRuleDev& r, hipStream_t s);   // the rule only, in place
// The seeded draw in the place of the argmax (gill_decode_sampler, checked by the launcher): rule in place, then per row the token
// argmax_c exp(y_c - max) / -log(u_c) over the top-p filter's kept set, y = x / temperature, u_c the Philox4x32-10 uniform of
// (seed; c >> 2, row0 + b, draw, 0) word c & 3 (philox.h); rows with no finite maximum take torch.argmax's pick.  The rest as
// decode_rule_pick_launch.  vocab <= 65536.
struct DecodeSampler {
  uint64_t seed;
  int draw, row0;
  double temperature, top_p;
};
int decode_sample_check(int B, int V, const DecodeRuleDev& r, const DecodeSampler& sm, int D, int ld, int col);   // host: arguments only
int decode_sample_launch(float* logits, int B, int V, const DecodeRuleDev& r, const DecodeSampler& sm, const bf16_t* table, int D,
                         int64_t* tokens, int ld, int col, int32_t* n_out, bf16_t* next_embeds, hipStream_t s);
// Ragged decision (one launch per iteration; include/gill_amd.h "ragged decode state"): state int32 [DEC_FIELDS][B] then the active-row count.
enum { DEC_LEN = 0, DEC_STEP = 1, DEC_FORCED = 2, DEC_NTOK = 3, DEC_ROW_ID = 4, DEC_FLAGS = 5, DEC_FIELDS = 6 };
enum { DEC_FLAG_ASSERT = 1, DEC_FLAG_CLAMP = 2, DEC_FLAG_FULL = 4 };
// sm == nullptr: greedy; else the seeded draw keyed (seed, row_id, draw = the row's step); sm->draw / sm->row0 are not read.
// clamp_flags (nullable): [B] words set by attention_decode_launch, folded into the rows' flags and cleared
int decode_ragged_launch(float* logits, int B, int V, const DecodeRuleDev& r, int min_word_tokens, int max_steps, const DecodeSampler* sm,
                         int32_t* state, int32_t* clamp_flags, const bf16_t* table, int D, int64_t* tokens, int ld, bf16_t* next_embeds,
                         hipStream_t s);
// out = in / temperature (reciprocal: in * fp32(1 / temperature)), then the top-p filter when top_p < 1
int decode_filter_launch(const float* in, float* out, int B, int V, double temperature, int reciprocal, double top_p,
                         double filter_value, hipStream_t s);
// classifier-free guidance + PLMS update on fp32 NCHW latents (see sd_schedule.hip for the coefficient layout)
// One row per UNet call of a denoise loop, computed on the host once per call of gill_sd_denoise and read by the
// device: the loop's only per-step inputs.  The step index itself lives on the device (SdLoopArgs::ctr), so replaying one
// captured UNet step N times needs no host-side per-step argument and no copy between replays.
struct PlmsRow {
  int mode;              // 0: first step, 1: repeated step, 2..4: multistep orders
  int slot_new;          // ring slot to write the new guided eps into (-1: don't store)
  int s1, s2, s3;        // ring slots of ets[-2], ets[-3], ets[-4] where needed (ets[-1] = new / slot of last)
  float sample_coeff, eps_coeff;   // x_prev = sample_coeff * sample - eps_coeff * eps'
};
// The same for every sampler that is a linear update in (sample, model output, one step of history, noise): DDIM, DPM-Solver++(2M), Euler,
// Euler ancestral (sd_schedule.hip builds the rows in double and rounds them to fp32 once).  With e the guided model output and x the latents:
//   m = p_x * x + p_e * e ;  if slot_new >= 0: ring[slot_new] = m ;  x_next = c_x * x + c_0 * m + c_1 * ring[s1] + c_n * z[step]
// ring[s1] is read only where c_1 != 0 and the noise only where c_n != 0.  in_scale is scale_model_input, applied by the stage kernel.
struct SamplerRow {
  int slot_new, s1;
  float in_scale;
  float p_x, p_e;
  float c_x, c_0, c_1, c_n;
};
struct SdLoopArgs {
  const PlmsRow* rows;   // [ncalls] on device (PNDM loops)
  const SamplerRow* srows = nullptr;        // [ncalls] on device (every other sampler; nullptr in a PNDM loop)
  const float* const* noise = nullptr;      // device slot holding the [ncalls][B][n] noise table's address (or null): not a kernel argument, so
                                            // one captured step serves every call's table
  int* ctr;              // ctr[0]: next step (written by the PLMS kernel only), ctr[1]: current step (written by the stage kernel only)
  const float* temb_table; int temb_total;   // [ncalls][temb_total] -> temb_cur
  float* temb_cur;
  const float* eps;      // [2B][n] : uncond rows then cond rows
  float* lat;            // [B][n] in/out
  float* lat2;           // [2B][n] (or [B][n]): the UNet input = cat([latents] * 2)
  float* cur_sample;     // [B][n] saved sample (PLMS warm-up)
  float* ets;            // [4][B][n] ring of past eps'
  int B; int64_t n;      // n = C*H*W per sample
  const float* guidance; // device scalar (not a kernel argument: one captured step graph serves every guidance value)
  int cfg;               // 1: eps holds [uncond | cond] halves and guidance is applied; 0: eps is [B][n]
};
// plain device-side fill / copy kernels for use INSIDE a captured forward: hipMemsetAsync / hipMemcpyAsync become memset /
// memcpy graph nodes, whose replay was not reliable (profiles/r02_soak_bisect.md).  16-byte aligned pointers and sizes.
int zero_bytes_launch(void* dst, size_t bytes, hipStream_t s);
int copy_bytes_launch(void* dst, const void* src, size_t bytes, hipStream_t s);
int dup_pair_launch(void* a, const void* b, void* b2, size_t bytes, hipStream_t s);   // a[bytes..] := a[0..bytes); b2[0..bytes) = b2[bytes..] := b[0..bytes)
// first kernel of a step: latents -> UNet input (both CFG halves), time-embedding row of the current step -> temb_cur
int sd_stage_launch(const SdLoopArgs& a, hipStream_t s);
// last kernel of a step: CFG combine + PLMS update of the latents (custom_sd.py:641-646), then step counter + 1
int plms_step_launch(const SdLoopArgs& a, hipStream_t s);
// the same for a SamplerRow loop (a.srows)
int sampler_step_launch(const SdLoopArgs& a, hipStream_t s);
// dst = scale * src over n floats (latents * init_noise_sigma, custom_sd.py:472)
int scale_f32_launch(const float* src, float scale, int64_t n, float* dst, hipStream_t s);
// dst = a * x + b * z over n floats (the schedulers' add_noise: the first kernel of an image-to-image loop)
int add_noise_f32_launch(const float* x, const float* z, float a, float b, int64_t n, float* dst, hipStream_t s);
// Inpainting (include/gill_amd.h gill_sd_inpaint).  The loop's arguments plus the inpaint fields, as a struct of its own: SdLoopArgs, and with it
// the argument block of the three loop kernels above, stays what it was.
struct SdInpaintArgs {
  SdLoopArgs l;          // l.n = C * hw: the LATENTS' floats per sample (the UNet input of concat mode has (2 C + 1) * hw)
  const float* x0 = nullptr;     // [B][n] scaled VAE latents of the image (blend)
  const float* z0 = nullptr;     // [B][n] the add-noise draw that formed the start (blend)
  const float* mask = nullptr;   // [B][hw] latent mask, 1 = repaint
  const float* xm = nullptr;     // [B][n] scaled VAE latents of the masked image (concat)
  const float* keep = nullptr;   // [ncalls][2] on device: add_noise pair at the noise level the latents have after each call (blend)
  int64_t hw = 0;
};
// image (B,3,H,W), mask (Bm,1,H,W), Bm 1 or B -> masked image (B,3,H,W) = image * (mask < 0.5), latent mask (B,1,H/8,W/8) = mask[8y][8x] >= 0.5
int inpaint_prepare_launch(const float* image, const float* mask, int B, int Bm, int H, int W, float* masked, float* lmask, hipStream_t s);
// blend mode, after the step kernel: lat = m * lat + (1 - m) * (ka * x0 + kb * z0), (ka, kb) = keep[ctr[1]]
int sd_blend_launch(const SdInpaintArgs& a, hipStream_t s);
// concat mode, in place of sd_stage_launch: lat2 = [in_scale * lat | mask | xm] per sample, both CFG halves; the rest as sd_stage_launch
int sd_stage_concat_launch(const SdInpaintArgs& a, hipStream_t s);

// weight re-layout helpers (run once at engine creation)
int conv_weight_relayout_launch(const void* w, int dtype, int Cout, int Cin, bf16_t* out /*[Cout][9][Cin]*/, hipStream_t s);   // conv_in / conv_out
// measured (tools/one_op.py, 8 samples): 64x64x640 -> 320: 150.9 -> 145.4 us, 64x64x960: 207.6 -> 193.7 us; but 64x64x320: 75.9 ->
// 77.8 us and the split-K level-1 convs lose 14-18 % (32x32x1280 -> 640: 166.8 -> 193.2 us)
// (not for convolutions that run on the ping-pong 256 x 160 tile — gemm_conv_pingpong(): there a new (tap, chunk) segment every K
// step lengthens the memory phase, measured 155 us chunk-major against 126 us tap-major for 64 x 64 x 640 -> 320)
bool gemm_conv_pingpong(int rows_multiple_of, int Cout);     // true: gemm_launch runs this conv's 3x3 GEMM on the ping-pong kernel
bool conv_k_chunked(int HW, int Cin, int Cout);   // chunk-major K order for this conv?  Decided by the shape alone: a large input (>= 4096 pixels, > 4 MiB per sample) off the ping-pong tile
int conv_weight_relayout_ups4_launch(const void* w, int dtype, int Cout, int Cin, bf16_t* out /*[4][Cout][4][Cin]*/, hipStream_t s);   // GemmArgs::ups == 2
int conv_weight_relayout_chunked_launch(const void* w, int dtype, int Cout, int Cin, bf16_t* out /*[Cout][Cin/64][9][64]*/, hipStream_t s);   // GemmArgs::conv
int convert_to_bf16_launch(const void* src, int dtype, int64_t n, bf16_t* dst, hipStream_t s);
int convert_to_bf16_blk64_launch(const void* src, int dtype, int N, int K, bf16_t* dst, hipStream_t s);   // -> [N / 64][K / 64][64][64] (STREAM64)
int convert_to_f32_launch(const void* src, int dtype, int64_t n, float* dst, hipStream_t s);
// copy rows of a [rows][cols] matrix into a (possibly wider/padded/permuted) destination:
//   dst[dst_row_of(r)][0..cols) = src[r][0..cols)   with dst_row index list on device
int scatter_rows_bf16_launch(const bf16_t* src, int rows, int cols, const int32_t* dst_rows, bf16_t* dst, int dst_ld,
                             hipStream_t s);

int permute_f32_launch(const float* src, const int32_t* idx, int n, float* dst, hipStream_t s);
// fold LayerNorm(g, beta) into the Linear that follows it: W <- bf16(W*g) in place, colsum[n] = sum_k W', bias[n] += beta.W[n]
int ln_fold_rows_launch(bf16_t* W, int N, int K, const float* g, const float* beta, float* colsum, float* bias, hipStream_t s);
int pack_heads_launch(const bf16_t* src, int B, int n, int H, int d, int n_pad, int dp, int dpv, int mode, bf16_t* dst,
                      hipStream_t s, float mul = 1.f);
int unpad_heads_launch(const bf16_t* src, int64_t rows, int H, int d, int dp, bf16_t* dst, hipStream_t s);

// padded head dim used by the attention kernel for a true head dim d (0 = unsupported)
static inline int attn_padded_dim(int d) {
  if (d <= 48) return 48;
  if (d <= 64) return 64;
  if (d <= 80) return 80;
  if (d <= 128) return 128;
  if (d <= 160) return 160;
  return 0;
}

const bf16_t* gill_zero_page();   // >= 256 B of device zeros

// ---- weight-only fp8 linear of the decode step (linear_w8.hip) ----
#define W8_MAX_ROWS 16      // activation rows of one launch: the 16 columns of the MFMA's second operand
struct W8Args {
  const bf16_t* A = nullptr;               // [M][K]
  int M = 0, N = 0, K = 0;                 // 1 <= M <= W8_MAX_ROWS; N, K multiples of 64
  const unsigned char* W8 = nullptr;       // e4m3 bytes in the kernel's order [N / 16][K / 64][64][16] (w8_quant_launch)
  const float* scale = nullptr;            // [N] powers of two
  const float* bias = nullptr;             // [N] or null
  const float* resid = nullptr;            // [M][N] fp32 or null, added after the activation; may be C
  int act = ACT_NONE;                      // ACT_NONE or ACT_RELU
  int out_f32 = 0;
  void* C = nullptr;                       // [M][N] bf16 or fp32
  int splitk = 0;                          // 0: w8_pick_splitk(N, K); 1: unsplit; k > 1: k slices
  float* ws = nullptr;                     // [sk][M][N] fp32 partials of a split (or partials_only) launch
  size_t ws_floats = 0;
  int partials_only = 0;                   // stop at the partials (scale applied; bias, act, resid, C unused): the caller's reducer finishes
};
int w8_pick_splitk(int N, int K);          // a function of the matrix alone: no row's bits depend on M
int linear_w8_splitk(const W8Args& a);     // the slices linear_w8_launch(a) writes
int linear_w8_launch(const W8Args& a, hipStream_t s);
// bf16 [N][K] (row-major, or blk: 64 x 64-blocked) -> e4m3 bytes in the kernel's order + scale[N]; and back (w8 * s, exact)
int w8_quant_launch(const bf16_t* w, int blk, int N, int K, unsigned char* w8, float* scale, hipStream_t s);
int w8_dequant_launch(const unsigned char* w8, const float* scale, int N, int K, int blk, bf16_t* out, hipStream_t s);
