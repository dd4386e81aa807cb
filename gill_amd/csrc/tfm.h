// The pre-LayerNorm transformer block the OPT, CLIP vision, CLIP text and mapper engines share:
//   h += out_proj(attn(q, k, v = qkv(LN1(h))))       q scaled by head_dim^-0.5
//   h += fc2(act(fc1(LN2(h))))
// fp32 residual stream, bf16 GEMM operands, fp32 accumulation; attention is the shared flash kernel.  One matrix struct, one layer
// struct, one weight loader, one workspace and one runner with the only layer loop (TfmRun::layers); an engine keeps what is particular
// to it (embeddings, caches, final norms) and sets the switches of struct Tfm.  OPT's ragged decode step, and its cached forward on the e4m3
// bytes, are that loop with a TfmDecode argument (decode attention with append in place of the flash kernel), the fp8-weight mode the same loop
// with TfmRun::use_w8; the extend pass of a dialogue session (packed new tokens at per-row lengths) is the same argument with cu_new set.
// Nothing here allocates or builds strings per launch.
#pragma once
#include "engine_util.h"

// One matrix of the block, y = x . W^T + b: the bf16 weights [N][K], row-major or 64 x 64-blocked (blk: gemm_stream64_weights, the STREAM64
// layout), the bias (may be null) and, in the OPT engine's w8 mode only, the same matrix as e4m3 bytes in linear_w8.hip's order with one
// power-of-two scale per row (tfm_quantize_layer_w8; w then holds bytes * scale).  TfmRun::linear picks the kernel.
struct TfmMat {
  bf16_t* w = nullptr; int blk = 0; float* b = nullptr;
  int N = 0, K = 0;
  unsigned char* w8 = nullptr; float* scale = nullptr;
};

struct TfmLayer {
  TfmMat qkv, o, fc1, fc2;   // qkv: [3D][D] rows q | k | v
  float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
};

// Tensor names under a layer's prefix, each up to and including the separator in front of "weight" / "bias".
struct TfmNames {
  const char* qkv[3];   // q, k, v projections; qkv[1] == nullptr: qkv[0] is one packed [3D][D] in_proj
  const char *o, *fc1, *fc2, *ln1, *ln2;
};
// stream64: store the matrices gemm_stream64_weights() names in the STREAM64 layout (convert_to_bf16_blk64_launch)
int tfm_load_layer(const WeightTable& wt, DevPool& pool, const std::string& prefix, const TfmNames& names, int D, int F, bool stream64,
                   TfmLayer* L, hipStream_t s);

// A loaded layer's four matrices -> e4m3 bytes + scales (TfmMat::w8 / scale), and the bf16 matrices replaced, in their own layouts, by the
// dequantised values: the quantised model is an exact bf16 model and every bf16 kernel runs on it unchanged.  q | k | v are quantised as the stacked
// [3D][D] matrix (a row's scale is its own either way).  About 1.5 x the layer's bf16 bytes afterwards.
int tfm_quantize_layer_w8(DevPool& pool, TfmLayer* L, hipStream_t s);
// tfm_linear_launch on the e4m3 bytes (M <= W8_MAX_ROWS).  ln_out: an in-place residual GEMM into the fp32 stream (out == resid, fp32, no act, a bias)
// leaves partials [sk][M][N] and ends in opt_reduce_ln_launch, at any sk; without it the kernel's own epilogue (sk == 1) or its finishing pass.
// splitk as W8Args::splitk.
int tfm_linear_w8_launch(const bf16_t* A, int M, const unsigned char* W8, const float* scale, const float* b, int N, int K, const float* resid,
                         int act, void* out, bool out_f32, int splitk, float* ws, size_t ws_floats, const float* ln_g, const float* ln_b,
                         bf16_t* ln_out, hipStream_t s);

// Geometry, per-engine switches and workspace of the block (the fp32 stream itself stays with the engine).
struct Tfm {
  int D = 0, F = 0, H = 0, dp = 0, dpv = 0;
  bool fuse_ln = false;     // split-K out_proj / fc2 hand the LayerNorm that follows them to their reducer (opt_reduce_ln_kernel)
  bool split_qkv = true;    // the QKV GEMM takes the split factor of gemm_pick_splitk*(); false: always 1
  bf16_t* nbuf = nullptr;   // [rows][D] normalised stream: the operand of the next GEMM
  bf16_t* ff = nullptr;     // [rows][F]
  bf16_t *q = nullptr, *k = nullptr, *vt = nullptr, *o = nullptr;
  float* splitk_ws = nullptr; size_t splitk_ws_floats = 0;
  // buffers for max_batch sequences of up to max_tok tokens; ws_cap_floats != 0 caps the split-K partials
  int alloc(DevPool& pool, int max_batch, int max_tok, int D, int F, int H, int dp, int dpv, size_t ws_cap_floats = 0);
};

// a K / Vt cache of one layer: K [B][H][pad][dp], Vt [B][H][dpv][pad].  fmt GILL_KV_E4M3: the four e4m3 buffers of AttnDecodeKv8Args (ops.h) in
// their place (k / vt stay null): only the two `dec` branches of self_attn can run on it, the flash kernel writes and reads a bf16 cache
struct TfmKv {
  bf16_t* k = nullptr; bf16_t* vt = nullptr; int pad = 0;
  int fmt = 0;
  uint8_t* k8 = nullptr; uint8_t* vt8 = nullptr; int8_t* kexp = nullptr; int8_t* vexp = nullptr;
};

// split-K reducer + bias + fp32 residual (h, updated in place) + LayerNorm -> nb (opt_reduce_ln_kernel): ws [sk][M][D] fp32, D % 4 == 0, D <= 8192
int opt_reduce_ln_launch(const float* ws, int sk, int M, int D, const float* bias, float* h, const float* g, const float* b, bf16_t* nb,
                         float eps, hipStream_t s);
// TfmRun::linear's bf16 launch with the split factor, its workspace and the fuse_ln switch stated (the operator tests force them): fuse_ln and a
// split-K in-place residual GEMM into the fp32 stream -> partials + opt_reduce_ln_launch, every other launch -> the GEMM (its own reducer) +
// layernorm_launch.  This and tfm_linear_w8_launch have two callers each: TfmRun::linear and the operator entries of capi.hip.
int tfm_linear_launch(const bf16_t* A, int M, const bf16_t* W, int blk, const float* b, int N, int K, const float* resid, int act, void* out,
                      bool out_f32, int splitk, float* ws, bool fuse_ln, const float* ln_g, const float* ln_b, bf16_t* ln_out, hipStream_t s);

// The decode step as a mode of self_attn / layers (a cache): the T rows of sequence b are its tokens at positions lens[b] .. lens[b] + T - 1.
// Self-attention is then a plain QKV linear into Tfm::q as [B * T][3D] -> attention_decode_launch (T == 1: the ragged step) or
// attention_append_launch (T > 1, at most 16: the cached forward on the e4m3 bytes), which append the rows' K / V at lens[b] .., clamp a length
// beyond the cache and raise flags[b] (nullable) -> the out-projection.
// With cu_new (the extend pass, gill_opt_extend): the stream holds T = total_new PACKED rows (layers is called with B = 1), rows
// cu_new[b] .. cu_new[b + 1] - 1 the new tokens of sequence b < nseq at positions lens[b] ..; the projection goes to qkv ([total_new][3D], the
// caller's: Tfm::q is sized for 16 rows of it) and attention is attention_extend_launch with the host bound max_new of a row's count.
// Fork mode (the scoring pass, gill_opt_score_candidates): cu_new set and fork_parent set.  The packed rows are nseq CANDIDATES; candidate c reads
// the slots 0 .. fork_plen[c] - 1 of cache row fork_parent[c] < fork_rows and its own tokens (attention_fork_launch); the cache is not written
// and lens is not read.  fork_ws / fork_ws_bytes: the operator's workspace, reused by every layer.
// Branch mode (gill_opt_decode_step_branch): br set, cu_new null, T == 1.  The B rows are BRANCHES packed in br_groups groups (br_gstart /
// br_gparent / br_gplen on the device, AttnBranchArgs); row s at position lens[s] reads the slots 0 .. br_gplen[g] - 1 of main-cache row
// br_gparent[g] < br_main_rows and appends to row s < br_rows of the layer's branch cache br[layer] (pad = the branch pitch), layer = kv - br_main:
// attention_branch_launch.  The main cache is not written.
struct TfmDecode {
  const int32_t* lens = nullptr; int32_t* flags = nullptr;
  const int32_t* cu_new = nullptr; int nseq = 0, max_new = 0; bf16_t* qkv = nullptr;
  const int32_t* fork_parent = nullptr; const int32_t* fork_plen = nullptr; int fork_rows = 0;
  void* fork_ws = nullptr; size_t fork_ws_bytes = 0;
  const TfmKv* br = nullptr; const TfmKv* br_main = nullptr;
  const int32_t* br_gstart = nullptr; const int32_t* br_gparent = nullptr; const int32_t* br_gplen = nullptr;
  int br_groups = 0, br_rows = 0, br_main_rows = 0;
};

struct TfmRun {
  const Tfm& t;
  hipStream_t s;
  bool use_w8 = false;      // linear() runs a matrix that has e4m3 bytes on them (the caller has checked M <= W8_MAX_ROWS)
  int splitk(int M, int N, int K, int act, int blk) const;
  // y = act(A . W^T + b [+ resid_f32]); out fp32 or bf16.  ln_g / ln_b / ln_out: the LayerNorm that consumes the result (in-place
  // residual GEMMs into the fp32 stream: out == resid).  bf16 weights: with Tfm::fuse_ln a split-K launch hands it to the reducer
  // (opt_reduce_ln_kernel); every other launch is followed by the stand-alone pass.  e4m3 bytes (use_w8): unsplit without a residual, the
  // launcher's own split factor with one, and the LayerNorm always through the reducer.
  int linear(const bf16_t* A, int M, const TfmMat& m, const float* resid, int act, void* out, bool out_f32, const float* ln_g = nullptr,
             const float* ln_b = nullptr, bf16_t* ln_out = nullptr) const;
  // scatter the segments seg_base .. seg_base + nseg - 1 of the packed projection m (q | k | v row blocks of D) into the head-major attention operands
  int qkv(const bf16_t* A, int B, int ntok, const TfmMat& m, int nseg, int seg_base, int npad_q, int npad_kv, bf16_t* K, bf16_t* Vt,
          int kv_tok_offset) const;
  int attend(int B, int nq, int nkv, int npad_q, int npad_kv, const bf16_t* K, const bf16_t* Vt, bool causal) const;
  // the two sub-blocks over the stream h (B * T rows); nbuf holds their LayerNorm of h on entry and, with next_g, that of next_g / next_b on exit.
  // kv: the T rows are the tokens past .. past + T - 1 of each sequence; their K / Vt are appended to the cache and they attend to it.
  // dec (needs kv, T <= 16): every row at its own length instead of `past`
  int self_attn(float* h, int B, int T, const TfmLayer& L, bool causal, const float* next_g, const float* next_b, const TfmKv* kv = nullptr,
                int past = 0, const TfmDecode* dec = nullptr) const;
  int ffn(float* h, int rows, const TfmLayer& L, int act, const float* next_g = nullptr, const float* next_b = nullptr) const;
  // n layers: LN1 stand-alone for the first, every later LayerNorm rides on the GEMM in front of it (see linear).
  // kv: one cache per layer holding `past` tokens (OPT's cached decode); nullptr: plain forward over T tokens
  int layers(float* h, const TfmLayer* L, int n, int B, int T, int act, bool causal, const TfmKv* kv = nullptr, int past = 0,
             const TfmDecode* dec = nullptr) const;
};
