// The convolutional stack the UNet and the VAE decoder share: NHWC bf16 activations out of a bump arena, 3x3 convs as implicit GEMMs
// (nearest-2x upsample and the ResnetBlock2D 1x1 shortcut folded in), GroupNorm statistics filed by the producing GEMM's epilogue.
// One set of weight / activation types, one set of weight loaders, one set of GemmArgs builders and one GroupNorm dispatch; an engine
// keeps its own gemm() wrapper (split-K rule, workspace size, COOP), its K order, its statistics bin width and its GroupNorm eps,
// and passes each of them in (DESIGN.md "convnet.h").  Host side only: nothing here changes a launch.
#pragma once
#include "engine_util.h"

struct ConvW {
  bf16_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0; int chunked = 0; /* K order: GemmArgs::k_chunked */ int ups4 = 0; /* w = the 4-tap parity-class form (GemmArgs::ups == 2) */
  // gill_unet_config.fp8_convs: e4m3 weights [cout][kpad] in conv_fp8.hip's K order + per-output-channel de-quantisation scale
  unsigned char* w8 = nullptr; float* cs = nullptr; int kpad = 0;
};
struct NormW { float* g = nullptr; float* b = nullptr; int c = 0; };
struct ResW {   // ResnetBlock2D
  NormW n1, n2;
  ConvW c1, c2;
  bool has_sc = false;
  // conv2 with the 1x1 conv_shortcut fused as extra K channels: weights [cout][9*cout + cin], bias b2 + b_sc
  bf16_t* c2f_w = nullptr; float* c2f_b = nullptr;
  int cin = 0, cout = 0;
};

// stats: optional slot [Bx][H*W/64][C/sbin][2] that the PRODUCING GEMM epilogue fills with this tensor's per-slab GroupNorm
// partial sums (GemmArgs::gn_stats: written once each, added in slab order by the consumer)
// sbin: channels per statistics bin — the engine's choice (ConvRun::tensor), and part of the bits: it fixes the summation order
// nslab: partials per (sample, bin) the producer actually wrote (set when the producing GEMM is launched)
struct Tensor { bf16_t* p = nullptr; int H = 0, W = 0, C = 0; float* stats = nullptr; int sbin = 0; int nslab = 1; };

struct Arena {
  unsigned char* base = nullptr;
  size_t cap = 0, off = 0, high = 0;
  bool dry = false;
  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    void* p = dry ? (void*)(uintptr_t)(0x1000 + off) : (void*)(base + off);
    off += bytes;
    if (off > high) high = off;
    return p;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

// The per-handle workspace of a conv stack (an engine handle derives from it).
struct ConvWorkspace {
  Arena arena;
  unsigned char* arena_mem = nullptr;
  float* gn_stats = nullptr;      // per-forward pool of GroupNorm partial-sum slots (bump-allocated; the dry run sizes it)
  size_t gn_floats = 0, gn_next = 0;
  float* splitk_ws = nullptr; size_t splitk_ws_floats = 0;
};

// ---- load time (convnet.hip).  p: the tensor-name prefix in front of ".weight" / ".bias" ----
bool conv_ups4_enabled();   // GILL_CONV_UPS4 (default on), read once per process
int load_norm(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int c, NormW* n);
// hw: pixels per sample of the conv's INPUT — decides the K order (GemmArgs::k_chunked, conv_k_chunked()); 0: always tap-major
// f8: e4m3 weights for conv_fp8.hip instead
// ups4: the conv follows a nearest-2x upsample — store the four pre-summed 2x2-tap kernels instead (gemm.hip "UPS4";
// GILL_CONV_UPS4 = 0 keeps the 9-tap gather over the upsampled grid)
int load_conv3(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int cin, int cout, int hw, ConvW* c,
               bool f8 = false, bool ups4 = false);
// conv_in as im2col + the MFMA GEMM: weights [cout][tap*cin + c], K = 9 cin zero-padded to whole 64-wide K steps: 64 up to 7 input channels (the
// UNet's 4, the VAE's 3 and 4), 128 up to 14 (the 9-channel inpainting UNet)
constexpr int CONV_IN_MAX_CIN = 14;
static inline int conv_in_kpad(int cin) { return (9 * cin + 63) / 64 * 64; }
// the part behind the weight lookup: OIHW of any loader dtype -> tmp [cout][9][cin] -> the first 9 cin columns of w64 [cout][64] (zeroed by the caller)
int conv_in_im2col_weight(const void* w_oihw, int dtype, int cin, int cout, bf16_t* tmp, bf16_t* w64, hipStream_t s);
int load_conv_in_im2col(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int cin, int cout, bf16_t** w, float** b);
int load_conv_out(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int cin, int cout, bf16_t** w, float** b);   // [cout][9][cin] for conv_out_launch
// r->c2f_w rows = [conv2 taps (9*cout, r->c2's K order) | shortcut (cin)], r->c2f_b = conv2 bias + shortcut bias
int fuse_shortcut_into_conv2(DevPool& pool, hipStream_t s, const bf16_t* sc_w /*[cout][cin]*/, const float* sc_b, ResW* r);
// dst[r][0 .. cols) = src[r][0 .. cols): a dense [rows][cols] matrix into rows of pitch dst_ld elements (dst may point at a column offset)
int copy_rows_bf16(const bf16_t* src, int rows, int cols, bf16_t* dst, int dst_ld, hipStream_t s);

// ---- run time: what a forward of either engine carries.  The dry run (sizing the arena and the statistics pool at create) and every real
// run must make the same sequence of tensor() / stats_slot() / arena.alloc() calls ----
struct ConvRun {
  ConvWorkspace* ws;
  int groups;       // GroupNorm groups (config norm_num_groups)
  hipStream_t s;
  int Bx;
  bool dry;

  float* stats_slot(size_t floats) {   // next slot of the per-forward GroupNorm partial-sum pool
    float* p = dry ? (float*)(uintptr_t)16 : ws->gn_stats + ws->gn_next;
    ws->gn_next += (floats + 3) & ~(size_t)3;
    return p;
  }
  // sbin != 0: the producer files GroupNorm partial sums in bins of sbin channels (where the map is whole slabs and the epilogue can)
  Tensor tensor(int H, int W, int C, int sbin = 0) {
    Tensor t; t.H = H; t.W = W; t.C = C;
    t.p = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)Bx * H * W * C);
    if (sbin && (H * W) % GN_SLAB_ROWS == 0 && gemm_fused_gn_ok(C, sbin)) {
      t.sbin = sbin;
      t.stats = stats_slot((size_t)Bx * (H * W / GN_SLAB_ROWS_MIN) * (C / sbin) * 2);
    }
    return t;
  }
  void fuse_stats(GemmArgs& g, const Tensor& y) const {
    if (!y.stats) return;
    g.gn_stats = y.stats; g.gn_groups = y.C / y.sbin; g.gn_cg = y.sbin;
    g.rows_per_batch = y.H * y.W;
  }
  // 3x3 conv (pad 1) over x1 (++ x2): stride 1|2, optional fused nearest-2x upsample; y = conv + bias + rowvec + resid
  // pad_shift = 1 (stride 2): the window of Downsample2D(padding = 0), F.pad(x, (0, 1, 0, 1)) + conv(pad 0) — GemmArgs::pad_shift
  GemmArgs conv_args(const Tensor& x1, const Tensor* x2, const ConvW& w, int stride, int ups, const float* rowvec, int rv_bstride,
                     const bf16_t* resid, const Tensor& y, int pad_shift = 0) const {
    GemmArgs g;
    g.conv = 1; g.IH = x1.H; g.IW = x1.W; g.OH = y.H; g.OW = y.W; g.Cin = w.cin; g.stride = stride; g.ups = ups; g.pad_shift = pad_shift;
    g.M = Bx * y.H * y.W; g.N = w.cout; g.K = 9 * w.cin;
    g.A = x1.p; g.A2 = x2 ? x2->p : nullptr; g.K1 = x1.C;
    g.W = w.w; g.bias = w.b; g.k_chunked = w.chunked;
    if (ups && w.ups4) { g.ups = 2; g.K = 4 * w.cin; }
    g.rowvec = rowvec; g.rows_per_batch = y.H * y.W; g.rowvec_bstride = rv_bstride;
    g.resid = resid; g.ldr = w.cout;
    g.C = y.p; g.ldc = w.cout;
    fuse_stats(g, y);
    return g;
  }
  // out = conv2(n2) + conv_shortcut(x1 ++ x2): ONE implicit GEMM whose K runs over the 9 taps of n2 and then over
  // the raw input channels (no separate 1x1 GEMM, no shortcut tensor written and re-read as a residual)
  GemmArgs conv2_shortcut_args(const Tensor& n2, const Tensor& x1, const Tensor* x2, const ResW& w, const Tensor& out) const {
    GemmArgs g;
    g.conv = 1; g.IH = n2.H; g.IW = n2.W; g.OH = n2.H; g.OW = n2.W; g.Cin = w.cout; g.stride = 1; g.ups = 0;
    g.M = Bx * n2.H * n2.W; g.N = w.cout; g.K = 9 * w.cout + w.cin;
    g.A = n2.p; g.K1 = w.cout;
    g.X1 = x1.p; g.X2 = x2 ? x2->p : nullptr; g.KX = w.cin; g.KX1 = x1.C;
    g.W = w.c2f_w; g.bias = w.c2f_b; g.k_chunked = w.c2.chunked;
    g.rows_per_batch = n2.H * n2.W;
    g.C = out.p; g.ldc = w.cout;
    fuse_stats(g, out);
    return g;
  }
  // GroupNorm (+ SiLU) of x1 (++ x2) into y.  Inputs whose producers filed the sums (in bins the groups are made of) skip the statistics pass.
  // y8_scale > 0: y holds fp8(y8_scale * value) instead of bf16 (same shape; the A operand of the fp8 convs)
  // ss_out: write the per-(sample, channel) scale / shift table instead of normalising (single-source inputs whose producer filed the
  // statistics; *folded says whether that was possible — if not, y is normalised as usual)
  int gnorm(const Tensor& x1, const Tensor* x2, const NormW& n, float eps, int silu, const Tensor& y, float y8_scale = 0.f,
            float* ss_out = nullptr, bool* folded = nullptr) {
    const int C = x1.C + (x2 ? x2->C : 0);
    const bool ready = x1.stats != nullptr && (x2 == nullptr || x2->stats != nullptr) &&
                       groupnorm_bins_align(C / groups, x1.C, x1.sbin, x2 ? x2->sbin : 0);
    const int HW = x1.H * x1.W;
    // (slot order: statistics, then totals)
    float* stats = ready ? nullptr : stats_slot(groupnorm_stats_floats(Bx, HW, groups));
    // out-of-place totals for producers that wrote more than 64 partials per bin (SD-2.1-768: 96x96 maps); a skip tensor's
    // partials are read again by the up block's concatenated norm1 and must stay as their producer wrote them
    float* tot = ready ? stats_slot(groupnorm_totals_floats(Bx, x1.C / x1.sbin, x2 ? x2->C / x2->sbin : 0)) : nullptr;
    if (dry) return 0;
    GILL_REQUIRE(ws->gn_next <= ws->gn_floats, "internal: GroupNorm stats pool exhausted");
    if (ready) {
      const bool fold = ss_out != nullptr && x2 == nullptr;
      if (folded) *folded = fold;
      return groupnorm_apply_launch(x1.p, x1.C, x2 ? x2->p : nullptr, x2 ? x2->C : 0, Bx, HW, groups, n.g, n.b, eps, silu, y.p,
                                    x1.stats, x1.sbin, x1.C, x1.nslab, x2 ? x2->stats : nullptr, x2 ? x2->sbin : 0,
                                    x2 ? x2->nslab : 0, s, y8_scale, tot, fold ? ss_out : nullptr);
    }
    return groupnorm_launch(x1.p, x1.C, x2 ? x2->p : nullptr, x2 ? x2->C : 0, Bx, HW, groups, n.g, n.b, eps, silu, y.p, stats, s,
                            y8_scale);
  }
};

// ---- the VAE mid block's single-head attention behind its GroupNorm (vae.hip), shared by the engine (VRun::attention) and gill_op_vae_attention:
// one OUT_QKV GEMM (heads = 1, dp = dpv = C, qscale = 1 / sqrt(C): the natural-exponent domain; V stored transposed [B][C][HW]), then per image
// S = Q K^T (bf16, ldc = HW), vae_row_softmax_kernel in place, O = P V, and to_out over all B * HW rows.
struct VaeAttnArgs {
  const bf16_t* n = nullptr;                                   // [B * HW][C]: the normalised input
  const bf16_t* wqkv = nullptr; const float* bqkv = nullptr;   // [3C][C] = to_q | to_k | to_v, [3C]
  const bf16_t* wo = nullptr; const float* bo = nullptr;       // [C][C], [C]
  bf16_t *q = nullptr, *k = nullptr, *vt = nullptr, *o = nullptr;   // B * HW * C elements each
  bf16_t* sc = nullptr;      // scores, then probabilities, of image b at sc + b * sc_bstride ([HW][HW])
  size_t sc_bstride = 0;     // 0: one buffer reused by every image (the engine); HW * HW: every image's P is kept
  float* ws = nullptr; size_t ws_floats = 0;                   // split-K partials and how many floats they may take
  int B = 0, HW = 0, C = 0;
  // to_out: the caller fills C / ldc, the residual (resid / ldr) and the fused GroupNorm statistics hookup; the chain fills the rest and,
  // as for every GEMM, the split (read back for gemm_gn_slab_rows())
  GemmArgs out;
  int splits[3] = {0, 0, 0};   // the split factors used: QKV, S, PV (of the last image; they depend on the shape alone)
};
int vae_gemm_launch(GemmArgs& g, float* ws, size_t ws_floats, hipStream_t s);   // gemm_pick_splitk(), capped by ws_floats, then gemm_launch()
int vae_row_softmax_launch(bf16_t* sc, int rows, int n, hipStream_t s);         // in place over [rows][n] bf16; n % 8 == 0 or an error
int vae_attention_chain(VaeAttnArgs& a, hipStream_t s);
