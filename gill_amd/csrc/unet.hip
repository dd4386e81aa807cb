// Stage 3 — Stable Diffusion UNet + PNDM/PLMS classifier-free-guidance loop.
//
// Replaces self.sd_pipe(prompt_embeds=..., guidance_scale=..., num_inference_steps=...)
// (gill/models.py:730-731); the loop is the one restated in-tree at gill/custom_sd.py:607-651:
//   latent_model_input = cat([latents]*2)            custom_sd.py:630
//   noise_pred = unet(latent_model_input, t, encoder_hidden_states=prompt_embeds).sample      :633-638
//   noise_pred = uncond + g * (text - uncond)        :641-643
//   latents = scheduler.step(noise_pred, t, latents) :646          (PNDMScheduler, skip_prk_steps)
// The UNet itself (diffusers UNet2DConditionModel, SD-1.5 config) is not in the reference tree; its
// structure here follows the public architecture (state-dict key names are diffusers').
//
// MI355X design: activations are NHWC bf16 so that
//   * every 3x3 conv is an implicit GEMM whose K steps are contiguous 128-B channel runs (gemm.hip),
//   * (B, HW, C) attention tokens ARE the NHWC tensor: no transposes anywhere,
//   * skip-connection concats are never materialised (two-source GroupNorm / conv / shortcut GEMM),
//   * nearest-2x upsampling is folded into the following conv's gather.
// Step-invariant work is hoisted out of the 51-call loop: the cross-attention K/V of all 16 layers
// (they depend only on the prompt embedding) and the whole time-embedding MLP + the 22 resnet
// time projections for every timestep (one batched GEMM chain -> a [steps][sum Cout] table that the
// conv epilogues add as a per-channel row vector).
#include "convnet.h"
#include "sd_schedule.h"
#include "xf_weights.h"
#include "xf_plan.h"
#include "xf_args.h"
#include <math.h>
#include <map>
#include <set>

namespace {

struct LinW { bf16_t* w = nullptr; float* b = nullptr; int out = 0, in = 0; };

struct ResnetW : ResW {
  LinW sc;             // conv_shortcut as a GEMM of its own (fp8 mode)
  int temb_off = 0;    // this block's columns of the time-embedding table
};

struct XfW {  // Transformer2DModel with one BasicTransformerBlock
  int C = 0, heads = 0, d = 0, dp = 0, dpv = 0, layer_id = 0;
  XfGeom geom{};              // what the forms and every call's plan are decided from (xf_plan.h)
  XfForms forms{};            // the layouts this layer was loaded with: the optional weights below exist exactly where their form is set
  NormW gn;
  LinW proj_in, proj_out;
  NormW ln1, ln2, ln3;
  bf16_t* wqkv1 = nullptr;    // [3*H*dp][C]
  LinW out1;                  // [C][H*dp]
  bf16_t* wq2 = nullptr;      // [H*dp][C]
  bf16_t* wkv2 = nullptr;     // [2*H*dp][ctx_dim]
  LinW out2;
  bf16_t* wff1 = nullptr; float* bff1 = nullptr;   // GEGLU-permuted [8C][C]
  unsigned char* wff1_8 = nullptr; float* cs_ff1 = nullptr;   // gill_unet_config.fp8_convs: the same (LayerNorm-folded) rows in e4m3 + per-row de-quantisation scale (linear_fp8.hip)
  bf16_t* w1c = nullptr; float* b1c = nullptr; bf16_t* w2p = nullptr;   // the same weights as the fused feed-forward kernel reads them (ffn.hip; C = 320 only)
  bf16_t* wpp = nullptr;        // proj_out's weight in the permuted k order, and w1c written in that order: the fused feed-forward kernel also runs attn2.to_out (ffn.hip PRE)
  bf16_t *wqkv1p = nullptr, *wq2p = nullptr;   // wqkv1 / wq2 (LayerNorm-folded) with the K order of the fused projection pairs (lnproj.hip; C = 320 only)
  // norm1/2/3 are folded into wqkv1 / wq2 / wff1 at load (GemmArgs::ln_stats): column sums of g*W and beta.W^T (+ bias)
  float *s_qkv1 = nullptr, *c_qkv1 = nullptr, *s_q2 = nullptr, *c_q2 = nullptr, *s_ff1 = nullptr;
  bf16_t* xg = nullptr; float* xgb = nullptr;   // XALG (xf_weights.hip): [2 H C][ctx_dim] = G | G2, and gb [H][ctx_dim]
  LinW ff2;                   // [C][4C]
  bf16_t* wfo = nullptr; float* bfo = nullptr;   // ff2 and proj_out as one map: [C][4C + C] = [Wp W2 | Wp], bias Wp b2 + bp
};

// row sums feeding a folded LayerNorm: [planes][rows][2], planes fixed by the producing GEMM's tiling (gemm_row_planes)
struct RowStats { float* p = nullptr; int planes = 1; };

}  // namespace

struct GraphKey {     // (the guidance scale and the noise table's address are device-side scalars, not part of the captured step)
  int Bx, cfg;
  int linear;         // which step kernel the step ends with: 0 plms_step_kernel, 1 sampler_step_kernel (and the stage kernel's row table)
  int inpaint;        // 0: none (text-to-image, image-to-image), 1: sd_blend_kernel after the step kernel, 2: sd_stage_concat_kernel stages
  bool operator<(const GraphKey& o) const {
    if (Bx != o.Bx) return Bx < o.Bx;
    if (cfg != o.cfg) return cfg < o.cfg;
    if (linear != o.linear) return linear < o.linear;
    return inpaint < o.inpaint;
  }
};

struct gill_unet : ConvWorkspace {
  gill_unet_config cfg;
  DevPool pool;
  // weights
  bf16_t* conv_in_w = nullptr; float* conv_in_b = nullptr;
  bf16_t* conv_out_w = nullptr; float* conv_out_b = nullptr;
  NormW norm_out;
  LinW te1, te2;
  bf16_t* temb_proj_w = nullptr; float* temb_proj_b = nullptr; int temb_total = 0;   // [sum Cout][1280]
  std::vector<ResnetW> down_res[4], up_res[4];
  std::vector<XfW> down_xf[4], up_xf[4];
  ConvW down_ds[3], up_us[3];
  ResnetW mid_res[2];
  XfW mid_xf;
  int n_xf = 0;
  int temb_dim = 0;
  // workspace (+ ConvWorkspace)
  float* ln_stats = nullptr;      // per-forward pool of the row-sum planes feeding the folded LayerNorms
  size_t ln_floats = 0, ln_next = 0;
  // COOP arrival counters (GemmArgs::coop_ctr): one slot range per GEMM launch of a forward, bump-allocated in launch order (the dry run sizes the
  // pool), all zeroed by the forward's first kernel (im2col_nchw_launch)
  unsigned* coop_ctr = nullptr; size_t coop_n = 0, coop_next = 0;
  std::vector<bf16_t*> kcache, vcache;   // per transformer layer: [Bx][H][ctx_pad][dp] / [Bx][H][dpv][ctx_pad]
  int ctx_pad = 0;
  // XALG layers (XfW::xg): per-sample operands of the two cross-attention GEMMs — scores [Bx][80 H][C] + its folded-LayerNorm
  // column sums and constants [Bx][80 H], values [Bx][C][80 H]
  std::vector<bf16_t*> xq_w, xo_w; std::vector<float*> xq_cs, xq_b;
  // time embedding scratch
  float* t_dev = nullptr;       // [rows]
  bf16_t* t_sin = nullptr;      // [rows][320]
  bf16_t* t_h1 = nullptr;       // [rows][1280]
  bf16_t* t_h2 = nullptr;       // [rows][1280]
  float* temb_table = nullptr;  // [rows][temb_total]
  int temb_rows_cap = 0;
  // loop state
  float* lat = nullptr;         // [B][4*L*L]
  float* lat2 = nullptr;        // [2B][in_channels*L*L]: the UNet input (9 channels on an inpainting UNet; everything else here has out_channels)
  float* eps = nullptr;         // [2B][4*L*L]
  float* cur_sample = nullptr;
  float* ets = nullptr;         // [4][B][4*L*L]
  bf16_t* ctx_full = nullptr;   // [2B][77][768]
  float* temb_cur = nullptr;    // [temb_total]: time-embedding row of the step being replayed
  PlmsRow* plms_rows = nullptr; // [temb_rows_cap]: per-step PLMS coefficients of the running loop
  SamplerRow* sampler_rows = nullptr;   // [temb_rows_cap]: the same for the linear samplers (SdLoopArgs::srows)
  const float** noise_slot = nullptr;   // [1]: address of the running loop's noise table (SdLoopArgs::noise)
  int* step_ctr = nullptr;      // [2]: next / current step of the running loop (SdLoopArgs::ctr)
  float* guidance_dev = nullptr; // [1]: guidance scale of the running loop (SdLoopArgs::guidance)
  // inpainting (gill_sd_inpaint): the running loop's operands, copied here so that the captured step holds the handle's addresses
  float* inp_x0 = nullptr;      // [B][4*L*L] image latents
  float* inp_z0 = nullptr;      // [B][4*L*L] add-noise draw
  float* inp_xm = nullptr;      // [B][4*L*L] masked-image latents (concat mode)
  float* inp_mask = nullptr;    // [B][L*L]
  float* keep_rows = nullptr;   // [temb_rows_cap][2] (SdInpaintArgs::keep)
  // hipGraph of one UNet forward per UNet batch size (captured after the first eager forward of that size)
  std::map<GraphKey, hipGraphExec_t> graphs;
  std::set<GraphKey> warmed;
  bool use_graph = true;
  // The denoise loop runs on the handle's private stream, fenced to the caller's stream by events (capture needs a
  // non-NULL stream anyway; see DESIGN.md "hipGraph replay and the NULL stream").
  StreamFence fence;
  ~gill_unet() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
  }
};

namespace {

struct Loader {
  const WeightTable& wt;
  DevPool& pool;
  hipStream_t s;
  int ctx_len = 0;
  int norm(const std::string& p, int c, NormW* n) { return load_norm(wt, pool, s, p, c, n); }
  // hw: pixels per sample of the conv's INPUT (decides the K order, see load_conv3)
  int conv3(const std::string& p, int cin, int cout, int hw, ConvW* c, bool f8 = false, bool ups4 = false) {
    return load_conv3(wt, pool, s, p, cin, cout, hw, c, f8, ups4);
  }
  int lin(const std::string& p, int out, int in, LinW* l, bool bias = true) {
    l->out = out; l->in = in;
    GILL_TRY(load_bf16(wt, pool, p + ".weight", (int64_t)out * in, &l->w, s));
    if (bias) return load_f32(wt, pool, p + ".bias", out, &l->b, s);
    return 0;
  }
  int resnet(const std::string& p, int cin, int cout, int hw, int temb_dim, int* temb_off, bf16_t* temb_w, float* temb_b,
             ResnetW* r, bool f8) {
    r->cin = cin; r->cout = cout;
    f8 = f8 && cin % 64 == 0 && cout % 64 == 0;
    GILL_TRY(norm(p + ".norm1", cin, &r->n1));
    GILL_TRY(conv3(p + ".conv1", cin, cout, hw, &r->c1, f8));
    GILL_TRY(norm(p + ".norm2", cout, &r->n2));
    GILL_TRY(conv3(p + ".conv2", cout, cout, hw, &r->c2, f8));
    r->has_sc = (cin != cout);
    if (r->has_sc) GILL_TRY(lin(p + ".conv_shortcut", cout, cin, &r->sc));
    // (fp8 mode: the 1x1 shortcut stays a bf16 GEMM of its own whose output is conv2's residual)
    if (r->has_sc && !f8) GILL_TRY(fuse_shortcut_into_conv2(pool, s, r->sc.w, r->sc.b, r));
    // time_emb_proj rows go into the shared [sum Cout][temb_dim] matrix
    r->temb_off = *temb_off;
    const gill_tensor* t;
    GILL_TRY(wt.get(p + ".time_emb_proj.weight", (int64_t)cout * temb_dim, &t));
    GILL_TRY(convert_to_bf16_launch(t->data, t->dtype, (int64_t)cout * temb_dim, temb_w + (size_t)r->temb_off * temb_dim, s));
    GILL_TRY(wt.get(p + ".time_emb_proj.bias", cout, &t));
    GILL_TRY(convert_to_f32_launch(t->data, t->dtype, cout, temb_b + r->temb_off, s));
    *temb_off += cout;
    return 0;
  }
  // hw: tokens per sample at this layer (the softmax GEMM of the two-GEMM cross-attention runs on 64-row tiles of ONE sample)
  int xf(const std::string& p, int C, int H, int ctx_dim, int layer_id, int hw, XfW* x, bool f8 = false) {
    x->C = C; x->heads = H; x->d = C / H; x->dp = attn_padded_dim(x->d); x->dpv = round_up(x->dp, 32); x->layer_id = layer_id;
    GILL_REQUIRE(x->dp > 0, "unsupported attention head dim");
    const int hdp = H * x->dp;
    GILL_REQUIRE(hdp % 64 == 0, "padded attention width must be a multiple of 64");
    x->geom = XfGeom{C, H, x->dp, ctx_len, ctx_dim, hw, f8};
    const XfForms forms = x->forms = xf_forms(x->geom, xf_env_default());
    GILL_REQUIRE(xf_forms_consistent(forms), "internal: transformer block forms that exclude each other");
    GILL_TRY(norm(p + ".norm", C, &x->gn));
    GILL_TRY(lin(p + ".proj_in", C, C, &x->proj_in));
    GILL_TRY(lin(p + ".proj_out", C, C, &x->proj_out));
    const std::string b = p + ".transformer_blocks.0";
    GILL_TRY(norm(b + ".norm1", C, &x->ln1));
    GILL_TRY(norm(b + ".norm2", C, &x->ln2));
    GILL_TRY(norm(b + ".norm3", C, &x->ln3));
    const char* proj[6] = {".attn1.to_q", ".attn1.to_k", ".attn1.to_v", ".attn2.to_q", ".attn2.to_k", ".attn2.to_v"};
    HeadRows hr[6];   // attn1's q | k | v, attn2's q, attn2's k | v (over the context): segments of the xf_weights.h recipes, which the operator entries run too (here step by step: the launches keep this loader's order)
    for (int i = 0; i < 6; ++i) {
      const gill_tensor* t;
      GILL_TRY(wt.get(b + proj[i] + ".weight", (int64_t)C * (i < 4 ? C : ctx_dim), &t));
      hr[i] = HeadRows{t->data, t->dtype};
    }
    GILL_TRY(pool.alloc(&x->wqkv1, (size_t)3 * hdp * C, true));
    GILL_TRY(pool.alloc(&x->wq2, (size_t)hdp * C, true));
    GILL_TRY(pool.alloc(&x->wkv2, (size_t)2 * hdp * ctx_dim, true));
    GILL_TRY(xf_qkv_weights(hr, 3, nullptr, H, x->d, x->dp, C, x->ln1.g, x->ln1.b, x->wqkv1, x->s_qkv1, x->c_qkv1, x->wqkv1p, s, XF_LAYOUT));
    GILL_TRY(xf_qkv_weights(hr + 3, 1, nullptr, H, x->d, x->dp, C, x->ln2.g, x->ln2.b, x->wq2, x->s_q2, x->c_q2, x->wq2p, s, XF_LAYOUT));
    GILL_TRY(xf_qkv_weights(hr + 4, 2, nullptr, H, x->d, x->dp, ctx_dim, nullptr, nullptr, x->wkv2, nullptr, nullptr, nullptr, s));   // (no LayerNorm in front of to_k / to_v)
    for (int a = 1; a <= 2; ++a) {
      LinW* o = (a == 1) ? &x->out1 : &x->out2;
      const std::string on = b + ".attn" + std::to_string(a) + ".to_out.0";
      o->out = C; o->in = hdp;
      const gill_tensor* t;
      GILL_TRY(wt.get(on + ".weight", (int64_t)C * C, &t));
      GILL_TRY(pool.alloc(&o->w, (size_t)C * hdp, true));
      GILL_TRY(pad_head_cols_launch(t->data, t->dtype, C, H, x->d, x->dp, o->w, s));
      GILL_TRY(load_f32(wt, pool, on + ".bias", C, &o->b, s));
    }
    // GEGLU projection: its rows in the value / gate 16-row interleave
    const int inner = 4 * C; bf16_t* tmpw; float* tmpb; int32_t* idx;
    GILL_TRY(load_bf16(wt, pool, b + ".ff.net.0.proj.weight", (int64_t)2 * inner * C, &tmpw, s));
    GILL_TRY(load_f32(wt, pool, b + ".ff.net.0.proj.bias", 2 * inner, &tmpb, s));
    GILL_TRY(pool.alloc(&idx, (size_t)2 * inner, false));
    GILL_TRY(pool.alloc(&x->wff1, (size_t)2 * inner * C, false));
    GILL_TRY(pool.alloc(&x->bff1, (size_t)2 * inner, false));
    GILL_TRY(xf_geglu_weights(tmpw, tmpb, inner, C, x->ln3.g, x->ln3.b, idx, x->wff1, x->bff1, x->s_ff1, s, XF_LAYOUT));
    GILL_TRY(lin(b + ".ff.net.2", C, 4 * C, &x->ff2));
    const gill_tensor *tp, *t2, *tb2, *tbp;      // ff2 and proj_out once more, as one map
    GILL_TRY(wt.get(p + ".proj_out.weight", (int64_t)C * C, &tp));
    GILL_TRY(wt.get(b + ".ff.net.2.weight", (int64_t)C * 4 * C, &t2));
    GILL_TRY(wt.get(b + ".ff.net.2.bias", C, &tb2));
    GILL_TRY(wt.get(p + ".proj_out.bias", C, &tbp));
    GILL_TRY(pool.alloc(&x->wfo, (size_t)C * 5 * C, false)); GILL_TRY(pool.alloc(&x->bfo, (size_t)C, false));
    GILL_TRY(xf_ffo_weights(tp->data, tp->dtype, t2->data, t2->dtype, tb2->data, tb2->dtype, tbp->data, tbp->dtype, C, x->wfo, x->bfo, s));
    // the three LayerNorms are folded into the projections that consume them (zeroed: the fold ADDS its constant part to the bias it is given)
    GILL_TRY(pool.alloc(&x->s_qkv1, (size_t)3 * hdp)); GILL_TRY(pool.alloc(&x->c_qkv1, (size_t)3 * hdp));
    GILL_TRY(pool.alloc(&x->s_q2, (size_t)hdp)); GILL_TRY(pool.alloc(&x->c_q2, (size_t)hdp));
    GILL_TRY(pool.alloc(&x->s_ff1, (size_t)8 * C));
    GILL_TRY(xf_qkv_weights(hr, 3, nullptr, H, x->d, x->dp, C, x->ln1.g, x->ln1.b, x->wqkv1, x->s_qkv1, x->c_qkv1, x->wqkv1p, s, XF_FOLD));
    GILL_TRY(xf_qkv_weights(hr + 3, 1, nullptr, H, x->d, x->dp, C, x->ln2.g, x->ln2.b, x->wq2, x->s_q2, x->c_q2, x->wq2p, s, XF_FOLD));
    GILL_TRY(xf_geglu_weights(tmpw, tmpb, inner, C, x->ln3.g, x->ln3.b, idx, x->wff1, x->bff1, x->s_ff1, s, XF_FOLD));
    // the optional layouts (xf_plan.h has the rules).  fp8 GEGLU: the folded rows quantised per output row
    if (forms.geglu_fp8) {
      GILL_TRY(pool.alloc(&x->wff1_8, (size_t)8 * C * C, false));
      GILL_TRY(pool.alloc(&x->cs_ff1, (size_t)8 * C, false));
      GILL_TRY(linear_weight_quant_fp8_launch(x->wff1, 8 * C, C, F8_LIN_ACT_SCALE, x->wff1_8, x->cs_ff1, s));
    }
    // cross-attention as two GEMMs; otherwise the layer keeps its K / V caches and the attention-kernel form
    if (forms.xalg) {
      GILL_TRY(pool.alloc(&x->xg, (size_t)2 * H * C * ctx_dim, false));
      GILL_TRY(pool.alloc(&x->xgb, (size_t)H * ctx_dim));
      GILL_TRY(xalg_fold_launch(x->wq2, x->c_q2, x->wkv2, x->out2.w, H, C, x->d, x->dp, ctx_dim, x->xg, x->xgb, s));
    }
    if (forms.ffn_fused) {
      GILL_TRY(pool.alloc(&x->w1c, (size_t)8 * C * C, false));
      GILL_TRY(pool.alloc(&x->b1c, (size_t)8 * C, false));
      GILL_TRY(pool.alloc(&x->w2p, (size_t)4 * C * C, false));
      if (forms.ffn_pre) GILL_TRY(pool.alloc(&x->wpp, (size_t)C * C, false));
      GILL_TRY(ffn_relayout_launch(x->wff1, x->bff1, x->wfo, x->w1c, x->b1c, x->w2p, x->wpp, s));
    }
    if (forms.lnproj) {
      GILL_TRY(pool.alloc(&x->wqkv1p, (size_t)3 * hdp * C, false));
      GILL_TRY(pool.alloc(&x->wq2p, (size_t)hdp * C, false));
      GILL_TRY(xf_qkv_weights(hr, 3, nullptr, H, x->d, x->dp, C, x->ln1.g, x->ln1.b, x->wqkv1, x->s_qkv1, x->c_qkv1, x->wqkv1p, s, XF_KPERM));
      GILL_TRY(xf_qkv_weights(hr + 3, 1, nullptr, H, x->d, x->dp, C, x->ln2.g, x->ln2.b, x->wq2, x->s_q2, x->c_q2, x->wq2p, s, XF_KPERM));
    }
    return 0;
  }
};

}  // namespace

static int unet_plan_and_alloc(gill_unet* m);

extern "C" int gill_unet_create(gill_unet** out, const gill_unet_config* cfg, const gill_tensor* weights, int n_weights) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  GILL_REQUIRE(cfg->layers_per_block == 2, "only layers_per_block == 2 (SD-1.x/2.x) is supported");
  GILL_REQUIRE(cfg->max_batch >= 1, "max_batch must be >= 1");
  for (int i = 0; i < 4; ++i)
    GILL_REQUIRE(cfg->block_out_channels[i] % 64 == 0, "block_out_channels must be multiples of 64");
  GILL_REQUIRE(cfg->cross_attention_dim % 64 == 0, "cross_attention_dim must be a multiple of 64");
  GILL_REQUIRE(cfg->sample_size % 8 == 0, "sample_size must be a multiple of 8");
  gill_unet* m = new gill_unet();
  m->cfg = *cfg;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  Loader L{wt, m->pool, s, cfg->ctx_len};
  const int* ch = cfg->block_out_channels;
  const int ctxd = cfg->cross_attention_dim;
  // heads per resolution level: SD-1.x uses num_heads everywhere, SD-2.x a fixed head dim of 64 (5, 10, 20, 20 heads)
  int Hl[4];
  for (int i = 0; i < 4; ++i) {
    Hl[i] = cfg->heads_per_level[i] > 0 ? cfg->heads_per_level[i] : cfg->num_heads;
    GILL_REQUIRE(Hl[i] > 0 && ch[i] % Hl[i] == 0, "heads must divide the channel count of their level");
  }
  const int temb_dim = ch[0] * 4;
  m->temb_dim = temb_dim;

  // total width of the per-resnet time projections
  int temb_total = 0;
  for (int i = 0; i < 4; ++i) temb_total += 2 * ch[i];
  temb_total += 2 * ch[3];
  for (int i = 0; i < 4; ++i) temb_total += 3 * ch[3 - i];
  m->temb_total = temb_total;
  if ((rc = m->pool.alloc(&m->temb_proj_w, (size_t)temb_total * temb_dim, false))) return fail(rc);
  if ((rc = m->pool.alloc(&m->temb_proj_b, (size_t)temb_total, false))) return fail(rc);
  int temb_off = 0;

  // conv_in runs as im2col (K = 36 zero-padded to 64) + the MFMA GEMM, conv_out as a direct kernel
  if ((rc = load_conv_in_im2col(wt, m->pool, s, "conv_in", cfg->in_channels, ch[0], &m->conv_in_w, &m->conv_in_b))) return fail(rc);
  if ((rc = load_conv_out(wt, m->pool, s, "conv_out", ch[0], cfg->out_channels, &m->conv_out_w, &m->conv_out_b))) return fail(rc);
  if ((rc = L.norm("conv_norm_out", ch[0], &m->norm_out))) return fail(rc);
  if ((rc = L.lin("time_embedding.linear_1", temb_dim, ch[0], &m->te1))) return fail(rc);
  if ((rc = L.lin("time_embedding.linear_2", temb_dim, temb_dim, &m->te2))) return fail(rc);

  int layer_id = 0;
  const bool f8 = cfg->fp8_convs != 0;   // ResnetBlock2D convolutions on the fp8 matrix instruction (conv_fp8.hip)
  const bool f8lin = cfg->fp8_convs == 1; // ... and the GEGLU projections of levels 1-3 (linear_fp8.hip); fp8_convs = 2: the convolutions only (round-5 mode, for A/B)
  auto hw_of = [&](int level) { const int side = cfg->sample_size >> level; return side * side; };   // pixels per sample
  // down blocks: CrossAttnDownBlock2D x3, DownBlock2D
  for (int i = 0; i < 4; ++i) {
    const int cin = (i == 0) ? ch[0] : ch[i - 1];
    const std::string p = "down_blocks." + std::to_string(i);
    m->down_res[i].resize(2);
    for (int j = 0; j < 2; ++j)
      if ((rc = L.resnet(p + ".resnets." + std::to_string(j), j == 0 ? cin : ch[i], ch[i], hw_of(i), temb_dim, &temb_off,
                         m->temb_proj_w, m->temb_proj_b, &m->down_res[i][j], f8))) return fail(rc);
    if (i < 3) {
      m->down_xf[i].resize(2);
      for (int j = 0; j < 2; ++j)
        if ((rc = L.xf(p + ".attentions." + std::to_string(j), ch[i], Hl[i], ctxd, layer_id++, hw_of(i), &m->down_xf[i][j], f8lin))) return fail(rc);
      if ((rc = L.conv3(p + ".downsamplers.0.conv", ch[i], ch[i], hw_of(i), &m->down_ds[i]))) return fail(rc);
    }
  }
  // mid
  if ((rc = L.resnet("mid_block.resnets.0", ch[3], ch[3], hw_of(3), temb_dim, &temb_off, m->temb_proj_w, m->temb_proj_b, &m->mid_res[0], f8)))
    return fail(rc);
  if ((rc = L.xf("mid_block.attentions.0", ch[3], Hl[3], ctxd, layer_id++, hw_of(3), &m->mid_xf, f8lin))) return fail(rc);
  if ((rc = L.resnet("mid_block.resnets.1", ch[3], ch[3], hw_of(3), temb_dim, &temb_off, m->temb_proj_w, m->temb_proj_b, &m->mid_res[1], f8)))
    return fail(rc);
  // up blocks: UpBlock2D, CrossAttnUpBlock2D x3
  const int rev[4] = {ch[3], ch[2], ch[1], ch[0]};
  for (int i = 0; i < 4; ++i) {
    const int outc = rev[i];
    const int prev = (i == 0) ? rev[0] : rev[i - 1];
    const int inc = rev[i + 1 < 4 ? i + 1 : 3];
    const std::string p = "up_blocks." + std::to_string(i);
    m->up_res[i].resize(3);
    for (int j = 0; j < 3; ++j) {
      const int skip = (j == 2) ? inc : outc;
      const int rin = (j == 0) ? prev : outc;
      if ((rc = L.resnet(p + ".resnets." + std::to_string(j), rin + skip, outc, hw_of(3 - i), temb_dim, &temb_off, m->temb_proj_w,
                         m->temb_proj_b, &m->up_res[i][j], f8))) return fail(rc);
    }
    if (i > 0) {
      m->up_xf[i].resize(3);
      for (int j = 0; j < 3; ++j)
        if ((rc = L.xf(p + ".attentions." + std::to_string(j), outc, Hl[3 - i], ctxd, layer_id++, hw_of(3 - i), &m->up_xf[i][j], f8lin))) return fail(rc);
    }
    if (i < 3)
      if ((rc = L.conv3(p + ".upsamplers.0.conv", outc, outc, hw_of(3 - i), &m->up_us[i], false, true))) return fail(rc);
  }
  m->n_xf = layer_id;
  if (temb_off != temb_total) { gill_set_error("internal: temb table width mismatch"); return fail(-4); }

  if ((rc = unet_plan_and_alloc(m))) return fail(rc);
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("unet create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_unet_destroy(gill_unet* h) { delete h; }

// ------------------------------------------------------------------------------------------------------------------
namespace {

struct UNetRun : ConvRun {
  gill_unet* m;
  const float* temb_rows;   // row for sample 0
  int temb_bstride;         // 0: every sample uses the same row
  UNetRun(gill_unet* m, hipStream_t s, int Bx, const float* temb_rows, int temb_bstride, bool dry)
      : ConvRun{m, m->cfg.norm_num_groups, s, Bx, dry}, m(m), temb_rows(temb_rows), temb_bstride(temb_bstride) {}
  // classifier-free-guidance pair: samples b and b + Bx/2 carry the same latents and timestep and differ only in the prompt,
  // so everything before the first cross-attention runs once on the first half (gill_sd_denoise sets this)
  bool cfg_pair = false;
  // GILL_DEBUG_SYNC=1 (tools): synchronise after every launch of the forward and say which one it was, to attribute a device fault
  int dbg_sync(const char* what, int a = 0, int b = 0, int c = 0) {
    static const bool on = getenv("GILL_DEBUG_SYNC") != nullptr;
    if (!on || dry) return 0;
    GILL_CHECK_HIP(hipStreamSynchronize(s));
    fprintf(stderr, "[unet] ok: %s %d %d %d\n", what, a, b, c);
    return 0;
  }
  RowStats ln_slot(int rows, int C) {   // row-sum planes of a [rows][C] residual stream (sized for any tiling of C columns)
    RowStats r;
    r.p = dry ? (float*)(uintptr_t)16 : m->ln_stats + m->ln_next;
    m->ln_next += (size_t)rows * 2 * GEMM_MAX_ROW_PLANES(C);
    return r;
  }
  // want_stats: the producer files this tensor's GroupNorm partial sums, in bins of C / 64 channels (finer than a group, so the sums also
  // serve the wider groups of a skip concat) where there are at least two of them, else per group
  Tensor talloc(int H, int W, int C, bool want_stats = false) {
    if (!want_stats || C % groups != 0) return tensor(H, W, C);
    return tensor(H, W, C, (C % 64 == 0 && C / 64 >= 2) ? C / 64 : C / groups);
  }
  Tensor talloc8(int H, int W, int C) {   // fp8 activation tensor (one byte per element)
    Tensor t; t.H = H; t.W = W; t.C = C;
    t.p = (bf16_t*)m->arena.alloc((size_t)Bx * H * W * C);
    return t;
  }
  int pick_sk(GemmArgs& g, bool generic = false) {
    g.splitk = gemm_pick_splitk(g.M, g.N, g.K, g.act, !g.conv, generic);
    while (g.splitk > 1 && (size_t)g.splitk * g.M * g.N > m->splitk_ws_floats) --g.splitk;
    g.ws = m->splitk_ws;
    return 0;
  }
  // The GroupNorm (+ SiLU) that consumes a GEMM's output, offered to the producer: a split-K launch of a supported geometry runs it in
  // its reducer (gemm_reduce.hip "REDUCE + GROUPNORM") and sets `done`; otherwise the consumer runs its GroupNorm-apply as before.
  // raw_needed = false: nobody else reads the raw output (conv1 -> norm2 inside a ResnetBlock2D): it is not even written.
  // ss: (optional) the consumer wants the per-(sample, channel) scale | shift table [Bx][2][C] instead of a normalised copy (the level-0 transformer
  // blocks: lnproj.hip applies it to the rows it loads) — only the in-kernel finish (COOP) writes it; y is then unused.
  struct FusedNorm { const NormW* n; float eps; int silu; Tensor y; bool raw_needed; bool done; float* ss = nullptr; };
  // One such offer on its way from the producing block to the consuming one (forward() keeps a single one in flight): offer() names the
  // consumer's GroupNorm, the producer sets `done` if it ran it, take() hands the result to the consumer — once: a second take() finds nothing.
  // The normalised copy (or, table = true, the scale | shift table) is allocated whether or not the offer is taken: same arena layout in the
  // dry run and in every real run.
  struct Handoff {
    UNetRun& r;
    FusedNorm fn{nullptr, 0.f, 0, Tensor(), true, false};
    struct Taken {   // by value: the next offer() overwrites fn while the consumer still reads what it took
      Tensor y; bool has_y = false; const float* ss = nullptr;
      const Tensor* copy() const { return has_y ? &y : nullptr; }
    };
    FusedNorm* offer(const NormW& n, float eps, int silu, int H, int W, int C, bool table = false) {
      Tensor y; y.H = H; y.W = W; y.C = C;
      if (!table) y = r.talloc(H, W, C);
      fn = FusedNorm{&n, eps, silu, y, true, false};
      if (table) fn.ss = (float*)r.m->arena.alloc(sizeof(float) * (size_t)r.Bx * 2 * C);
      return &fn;
    }
    Taken take() {
      Taken t;
      if (fn.done && fn.ss) t.ss = fn.ss;
      else if (fn.done) { t.y = fn.y; t.has_y = true; }
      fn.done = false;
      return t;
    }
  };
  int gemm(GemmArgs& g, RowStats* rs = nullptr, Tensor* ys = nullptr, FusedNorm* fn = nullptr) {
    // COOP counters of this launch: the same slot range in the dry run and in every real run (whether or not the launch ends up using them)
    unsigned* ctr = dry ? nullptr : m->coop_ctr + m->coop_next;
    m->coop_next += (size_t)gemm_coop_counters(g);
    if (dry) return 0;
    GILL_REQUIRE(m->coop_next <= m->coop_n, "internal: COOP counter pool exhausted");
    pick_sk(g);
    // (split-K partials come from 128-row tiles: not where a sample's rows are fewer — the 8 x 8 maps of the mid block)
    if (g.out_mode == OUT_SOFTMAX80 || (g.wb_rows && g.wb_rows % 128 != 0)) g.splitk = 1;
    g.coop_ctr = ctr;
    if (fn) {
      g.rows_per_batch = fn->y.H * fn->y.W;
      g.fn_Y = fn->ss ? nullptr : fn->y.p; g.fn_ss = fn->ss;
      g.fn_gamma = fn->n->g; g.fn_beta = fn->n->b; g.fn_eps = fn->eps; g.fn_silu = fn->silu;
      g.fn_cg = g.N / m->cfg.norm_num_groups;
      // the finish inside the producing launch (gemm.hip "COOP"), else — split-K only — the reducer launch that also normalises
      if (gemm_coop_ok(g) || (g.splitk > 1 && !fn->ss && gemm_fused_norm_ok(g))) {
        fn->done = true;
        if (!fn->raw_needed) {
          g.C = nullptr;
          if (g.splitk > 1) { g.gn_stats = nullptr; if (ys) ys->stats = nullptr; }      // (splitk == 1: the partials ARE the hand-off between the workgroups)
        }
      } else {
        g.fn_Y = nullptr; g.fn_ss = nullptr;
      }
    }
    if (rs) { g.row_stats = rs->p; rs->planes = gemm_row_planes(g); }
    if (ys && ys->stats) ys->nslab = ys->H * ys->W / gemm_gn_slab_rows(g);
    // (round 4: touching every GEMM's weights right before it is worth 3.4 % of a forward's kernel time, and a side-stream prefetcher costs 4.5-15 %:
    // profiles/r04_weight_touch.md, r04_weight_prefetch.md; the probe switch is gone)
    GILL_TRY(gemm_launch(g, s));
    return dbg_sync(g.conv ? "conv" : (g.act == ACT_GEGLU ? "geglu" : (g.out_mode == OUT_QKV ? "qkv" : (g.out_mode == OUT_SOFTMAX80 ? "scores+softmax" : "gemm"))), g.M, g.N, g.K);
  }
  // ConvRun::gnorm, named on stderr under GILL_DEBUG_SYNC
  int gnorm(const Tensor& x1, const Tensor* x2, const NormW& n, float eps, int silu, const Tensor& y, float y8_scale = 0.f,
            float* ss_out = nullptr, bool* folded = nullptr) {
    GILL_TRY(dbg_sync("before groupnorm", x1.C, x2 ? x2->C : 0, x1.H * x1.W));
    return ConvRun::gnorm(x1, x2, n, eps, silu, y, y8_scale, ss_out, folded);
  }
  // 3x3 conv (pad 1, stride 1) of an fp8 activation tensor x8 (gnorm(..., F8_ACT_SCALE)) with fp8 weights:
  // y = conv + bias + rowvec + resid (resid may alias y.p), GroupNorm partials of y fused like conv()
  int conv8(const Tensor& x8, const ConvW& w, const float* rowvec, int rv_bstride, const bf16_t* resid, Tensor& y) {
    if (dry) return 0;
    ConvF8Args a;
    a.B = Bx; a.H = x8.H; a.W = x8.W; a.Cin = w.cin; a.M = Bx * x8.H * x8.W; a.N = w.cout; a.Kpad = w.kpad;
    a.A8 = reinterpret_cast<const unsigned char*>(x8.p); a.W8 = w.w8; a.colscale = w.cs; a.C = y.p;
    a.rows_per_batch = x8.H * x8.W;
    GemmArgs g;      // split-K geometry + the reducer's epilogue
    g.M = a.M; g.N = a.N; g.K = 9 * w.cin;
    pick_sk(g, true);     // (the fp8 kernel has neither 64-row tiles nor a ping-pong variant: generic split rule)
    a.splitk = g.splitk;
    if (a.splitk > 1) {
      a.ws = g.ws;
      GILL_TRY(conv3x3_fp8_launch(a, s));
      g.bias = w.b; g.rowvec = rowvec; g.rows_per_batch = a.rows_per_batch; g.rowvec_bstride = rv_bstride;
      g.resid = resid; g.ldr = w.cout; g.C = y.p; g.ldc = w.cout;
      fuse_stats(g, y);
      if (y.stats) y.nslab = y.H * y.W / gemm_gn_slab_rows(g);
      return gemm_splitk_reduce_launch(g, s);
    }
    a.bias = w.b; a.rowvec = rowvec; a.rowvec_bstride = rv_bstride; a.resid = resid;
    if (y.stats) { a.gn_stats = y.stats; a.gn_groups = y.C / y.sbin; a.gn_cg = y.sbin; y.nslab = y.H * y.W / GN_SLAB_ROWS; }
    return conv3x3_fp8_launch(a, s);
  }
  // 3x3 conv (pad 1) over x1 (++ x2): stride 1|2, optional fused nearest-2x upsample
  int conv(const Tensor& x1, const Tensor* x2, const ConvW& w, int stride, int ups, const float* rowvec, int rv_bstride,
           const bf16_t* resid, Tensor& y, FusedNorm* fn = nullptr) {
    GemmArgs g = conv_args(x1, x2, w, stride, ups, rowvec, rv_bstride, resid, y);
    return gemm(g, nullptr, &y, fn);
  }
  int linear(const bf16_t* A, int lda, const bf16_t* A2, int lda2, int K1, int M, const bf16_t* W, const float* b, int N,
             int K, const bf16_t* resid, int act, bf16_t* out, int ldc, Tensor* ystats = nullptr,
             RowStats* row_stats = nullptr, FusedNorm* fn = nullptr) {
    GemmArgs g;
    g.M = M; g.N = N; g.K = K; g.K1 = K1; g.A = A; g.lda = lda; g.A2 = A2; g.lda2 = lda2; g.W = W; g.bias = b;
    g.resid = resid; g.ldr = N; g.act = act; g.C = out; g.ldc = ldc;
    if (ystats) fuse_stats(g, *ystats);
    return gemm(g, row_stats, ystats, fn);
  }

  // out_stats: the output feeds a single-source GroupNorm next (accumulate its sums in conv2's epilogue)
  // pre: x1 already normalised by its producer's reducer (norm1 + SiLU of THIS block: single-source input only);
  // next: the GroupNorm that consumes this block's output, offered to conv2's reducer
  int resnet(const Tensor& x1, const Tensor* x2, const ResnetW& w, Tensor* out, bool out_stats, const Tensor* pre = nullptr,
             FusedNorm* next = nullptr) {
    const int H = x1.H, Wd = x1.W;
    *out = talloc(H, Wd, w.cout, out_stats);
    const size_t mk = m->arena.mark();
    if (w.c1.w8) {
      // fp8 mode: both GroupNorm-apply passes write e4m3 (half the bytes of the bf16 tensors they replace) and both convs run on
      // the fp8 matrix instruction; the 1x1 shortcut (bf16 GEMM over the raw input) lands in `out` first and conv2 adds onto it
      Tensor n1 = talloc8(H, Wd, w.cin);
      GILL_TRY(gnorm(x1, x2, w.n1, 1e-5f, 1, n1, F8_ACT_SCALE));
      Tensor h = talloc(H, Wd, w.cout, true);   // -> norm2
      GILL_TRY(conv8(n1, w.c1, temb_rows ? temb_rows + w.temb_off : nullptr, temb_bstride, nullptr, h));
      Tensor n2 = talloc8(H, Wd, w.cout);
      GILL_TRY(gnorm(h, nullptr, w.n2, 1e-5f, 1, n2, F8_ACT_SCALE));
      const bf16_t* resid = x1.p;
      if (w.has_sc) {
        GILL_TRY(linear(x1.p, x1.C, x2 ? x2->p : nullptr, x2 ? x2->C : 0, x1.C, Bx * H * Wd, w.sc.w, w.sc.b, w.cout, w.cin, nullptr, 0,
                        out->p, w.cout));
        resid = out->p;
      }
      GILL_TRY(conv8(n2, w.c2, nullptr, 0, resid, *out));
      m->arena.release(mk);
      return 0;
    }
    Tensor n1 = talloc(H, Wd, w.cin);
    if (pre && !x2) n1 = *pre;
    else GILL_TRY(gnorm(x1, x2, w.n1, 1e-5f, 1, n1));
    Tensor h = talloc(H, Wd, w.cout, true);   // -> norm2
    Tensor n2 = talloc(H, Wd, w.cout);
    FusedNorm f2{&w.n2, 1e-5f, 1, n2, false, false};      // norm2 + SiLU in conv1's split-K reducer where there is one
    GILL_TRY(conv(n1, nullptr, w.c1, 1, 0, temb_rows ? temb_rows + w.temb_off : nullptr, temb_bstride, nullptr, h, &f2));
    if (!f2.done) GILL_TRY(gnorm(h, nullptr, w.n2, 1e-5f, 1, n2));
    if (w.has_sc) {
      GemmArgs g = conv2_shortcut_args(n2, x1, x2, w, *out);
      GILL_TRY(gemm(g, nullptr, out, next));
    } else {
      GILL_TRY(conv(n2, nullptr, w.c2, 1, 0, nullptr, 0, x1.p, *out, next));
    }
    m->arena.release(mk);
    return 0;
  }

  int attend(const bf16_t* q, const bf16_t* k, const bf16_t* vt, bf16_t* o, int nq, int nkv, int nq_pad, int nkv_pad,
             const XfW& w) {
    if (dry) return 0;
    AttnArgs a;
    a.Q = q; a.K = k; a.Vt = vt; a.O = o;
    a.B = Bx; a.H = w.heads; a.nq = nq; a.nkv = nkv; a.nq_pad = nq_pad; a.nkv_pad = nkv_pad;
    a.dp = w.dp; a.dpv = w.dpv; a.ldo = w.heads * w.dp; a.d = w.d;
    a.scale = 1.0f / sqrtf((float)w.d);
    return attention_launch(a, s);
  }

  // Bx for a scope: xf() sizes its buffers for the full batch of a CFG pair and runs its GroupNorm and self-attention kernel at the half batch
  struct BatchScope {
    int& Bx; const int saved;
    BatchScope(int& Bx, int b) : Bx(Bx), saved(Bx) { Bx = b; }
    ~BatchScope() { Bx = saved; }
  };
  // what one call of the block runs (xf_plan.h); Bx is the batch of the block's input: half of a CFG pair where `shared`
  XfPlan xf_plan_of(const XfW& w, int HW, bool shared) const { return xf_plan(w.forms, w.geom, shared ? 2 * Bx : Bx, HW, shared); }
  // one block's tensors on their way through the three stages of xf()
  struct XfBlock {
    const XfW& w; const XfPlan p; const int HW, hw_pad, Bpre; const bool shared;
    Tensor t;                            // transformer residual stream
    Tensor xd;                           // the outer residual at full batch
    bf16_t *q, *k, *vt, *o;              // attention operands (attn1's, then attn2's query) and output
    // norm1/2/3 never materialise: the GEMM that writes the residual stream also accumulates each row's sum and sum of
    // squares, and the projection that follows applies mean / rstd in its epilogue on weights pre-multiplied by the LN gain
    RowStats st1, st2, st3;
    XfHeads heads() const { return xf_heads(w.heads, w.d); }
    // proj_in + norm1 + QKV, and attn1.to_out + residual + norm2 + attn2.to_q, as one kernel each (lnproj.hip): what both modes share
    LnProjArgs lnproj_args() const {
      LnProjArgs lp;
      lp.M = p.M; lp.T = t.p; lp.heads = w.heads; lp.dp = w.dp; lp.dpv = w.dpv; lp.ntok = HW; lp.ntok_pad = hw_pad;
      lp.Cq = q; lp.Ck = k; lp.Cvt = vt; lp.qscale = heads().qscale;
      return lp;
    }
  };

  // n: the block's input after its GroupNorm; or (gn_ss) x itself and the scale | shift table the projection kernel applies to the rows it loads
  int xf_self_attention(XfBlock& b, const bf16_t* n, const float* gn_ss) {
    const XfW& w = b.w; const int C = w.C;
    if (b.p.lnproj) {
      LnProjArgs lp = b.lnproj_args();
      lp.mode = 0; lp.X = n; lp.gn_ss = gn_ss; lp.W1 = w.proj_in.w; lp.b1 = w.proj_in.b; lp.W2p = w.wqkv1p; lp.c2 = w.c_qkv1;
      if (!dry) GILL_TRY(lnproj_launch(lp, s));
    } else {
      GILL_TRY(linear(n, C, nullptr, 0, C, b.p.M1, w.proj_in.w, w.proj_in.b, C, C, nullptr, ACT_NONE, b.t.p, C, nullptr, &b.st1));
      GemmArgs g = xf_qkv_args(b.t.p, b.p.M1, C, {b.st1.p, b.st1.planes, 0}, w.wqkv1, w.s_qkv1, w.c_qkv1, 3, b.heads(), b.HW, b.q, b.k, b.vt);
      GILL_TRY(gemm(g));
    }
    BatchScope half(Bx, b.Bpre);
    return attend(b.q, b.k, b.vt, b.o, b.HW, b.HW, b.hw_pad, b.hw_pad, w);
  }

  // x: the block's input (the shared prefix's half batch is duplicated into b.xd here, with the residual stream)
  int xf_cross_attention(XfBlock& b, const Tensor& x) {
    const XfW& w = b.w; const XfPlan& p = b.p; const int C = w.C, hdp = w.heads * w.dp;
    if (p.lnproj) {
      LnProjArgs lp = b.lnproj_args();
      lp.mode = 1; lp.X = b.o; lp.W1 = w.out1.w; lp.b1 = w.out1.b; lp.W2p = w.wq2p; lp.c2 = w.c_q2;
      if (!dry) GILL_TRY(lnproj_launch(lp, s));
    } else {
      GILL_TRY(linear(b.o, hdp, nullptr, 0, hdp, p.M1, w.out1.w, w.out1.b, C, hdp, b.t.p, ACT_NONE, b.t.p, C, nullptr, &b.st2));
      // second half of the pair := first half (residual stream, its LayerNorm row sums, the block input)
      // (out1 ran on M1 rows: its row-sum planes are [planes][M1][2]; the consumers below wrap rows >= M1 onto them)
      if (b.shared && !dry) GILL_TRY(dup_pair_launch(b.t.p, x.p, b.xd.p, sizeof(bf16_t) * (size_t)p.M1 * C, s));
      const XfLnRows ln2 = {b.st2.p, b.st2.planes, p.M1};
      if (p.cross == XF_CROSS_XALG) {
        // P = softmax80(LN(t) Mq_b^T), t += P Wo_b^T + bias on per-sample weights (xf_weights.hip)
        const int id = w.layer_id;
        GemmArgs g, g2;
        xf_xalg_args(b.t.p, p.M, b.HW, C, w.heads, ln2, m->xq_w[id], m->xq_cs[id], m->xq_b[id], m->xo_w[id], w.out2.b, b.o, b.t.p, b.t.p, &g, &g2);
        GILL_TRY(gemm(g));
        return gemm(g2, &b.st3);
      }
      GemmArgs g = xf_qkv_args(b.t.p, p.M, C, ln2, w.wq2, w.s_q2, w.c_q2, 1, b.heads(), b.HW, b.q, b.k, b.vt);
      GILL_TRY(gemm(g));
    }
    // the attention kernel over the K / V cached per prompt
    GILL_REQUIRE(m->kcache[w.layer_id] != nullptr || dry, "internal: cross-attention K/V cache missing");
    GILL_TRY(attend(b.q, m->kcache[w.layer_id], m->vcache[w.layer_id], b.o, b.HW, m->cfg.ctx_len, b.hw_pad, m->ctx_pad, w));
    // (with the fused feed-forward kernel's PRE form, attn2.to_out + residual run inside it: ffn.hip)
    if (p.ffn == XF_FFN_FUSED_PRE) return 0;
    return linear(b.o, hdp, nullptr, 0, hdp, p.M, w.out2.w, w.out2.b, C, hdp, b.t.p, ACT_NONE, b.t.p, C, nullptr, &b.st3);
  }

  int xf_feed_forward(XfBlock& b, Tensor* out, FusedNorm* next) {
    const XfW& w = b.w; const XfPlan& p = b.p; const int C = w.C, M = p.M;
    if (p.ffn == XF_FFN_FUSED || p.ffn == XF_FFN_FUSED_PRE) {
      // GEGLU feed-forward, its residual, proj_out and the outer residual as ONE kernel (ffn.hip)
      if (dry) return 0;
      FfnArgs fa;
      fa.M = M; fa.T = b.t.p; fa.ln_stats = b.st3.p; fa.ln_planes = b.st3.planes;
      fa.W1c = w.w1c; fa.b1c = w.b1c; fa.W2p = w.w2p; fa.Wfo = w.wfo; fa.bo = w.bfo; fa.resid = b.xd.p; fa.out = out->p;
      if (p.ffn == XF_FFN_FUSED_PRE) { fa.X = b.o; fa.Wo = w.out2.w; fa.bo2 = w.out2.b; fa.Wpp = w.wpp; }
      if (out->stats && out->sbin == 5) { fa.gn_stats = out->stats; fa.rows_per_batch = b.HW; out->nslab = b.HW / GN_SLAB_ROWS; }
      else out->stats = nullptr;        // (no partials from this producer: the consumer runs its own statistics pass)
      return ffn_fused_launch(fa, s);
    }
    bf16_t* ffh = (bf16_t*)m->arena.alloc(sizeof(bf16_t) * (size_t)M * 4 * C);
    if (p.ffn == XF_FFN_GEMM_FP8) {
      // fp8 mode: norm3 applied explicitly into an e4m3 copy of t (one pass: 3 bytes per element), then the GEGLU GEMM on the fp8 matrix instruction
      unsigned char* t8 = (unsigned char*)m->arena.alloc((size_t)M * C);
      if (!dry) {
        GILL_TRY(ln_quant_fp8_launch(b.t.p, M, C, b.st3.p, b.st3.planes, 0, 1e-5f, F8_LIN_ACT_SCALE, t8, s));
        LinF8Args a;
        a.M = M; a.N = 8 * C; a.K = C; a.A8 = t8; a.W8 = w.wff1_8; a.colscale = w.cs_ff1; a.bias = w.bff1; a.C = ffh;
        GILL_TRY(geglu_fp8_launch(a, s));
        GILL_TRY(dbg_sync("geglu fp8", M, 8 * C, C));
      }
    } else {
      GemmArgs g = xf_geglu_args(b.t.p, M, C, 4 * C, {b.st3.p, b.st3.planes, 0}, w.wff1, w.s_ff1, w.bff1, ffh);
      GILL_TRY(gemm(g));
    }
    // feed-forward output, its residual, proj_out and the outer residual: one GEMM over K = [h | t] (see ffo_fuse_kernel in xf_weights.hip; the
    // reference graph's two GEMMs measured 604.3 -> 588.9 ms against it, profiles/HISTORY.md)
    return linear(ffh, 4 * C, b.t.p, C, 4 * C, M, w.wfo, w.bfo, C, 5 * C, b.xd.p, ACT_NONE, out->p, C, out, nullptr, next);
  }

  // shared: `x` (and Bx) cover only the first half of a CFG pair; the block runs at that half batch up to the end of the self-attention, then
  // the residual stream is duplicated and the rest runs on the full pair
  // pre: x already normalised (this block's GroupNorm, no SiLU) by its producer's reducer; next: see resnet()
  // pre_ss: this block's GroupNorm as a scale | shift table already written by its producer's in-kernel finish (FusedNorm::ss; only where
  // the plan has gn_table)
  int xf(const Tensor& x, const XfW& w, Tensor* out, bool out_stats, bool shared = false, const Tensor* pre = nullptr,
         FusedNorm* next = nullptr, const float* pre_ss = nullptr) {
    const int H = x.H, Wd = x.W, C = w.C, HW = H * Wd;
    XfBlock b{w, xf_plan_of(w, HW, shared), HW, round_up(HW, 32), Bx, shared};
    BatchScope full(Bx, shared ? 2 * Bx : Bx);     // every buffer is sized for the full batch
    *out = talloc(H, Wd, C, out_stats);
    const size_t mk = m->arena.mark();
    Tensor n = talloc(H, Wd, C);
    b.xd = shared ? talloc(H, Wd, C) : x;
    // the fused projection kernel applies this GroupNorm itself to the rows it loads (lnproj.hip: gn_ss) where the producer filed the
    // statistics: the stand-alone pass (13 us, 21 MB read + 21 MB written per level-0 block) becomes a 640-float table per sample
    float* gn_ss = nullptr;
    bool gn_folded = false;
    {
      BatchScope half(Bx, b.Bpre);
      if (b.p.gn_table) gn_ss = (float*)m->arena.alloc(sizeof(float) * (size_t)Bx * 2 * C);
      if (pre_ss && gn_ss) { gn_ss = const_cast<float*>(pre_ss); gn_folded = true; }
      else if (pre) n = *pre;
      else GILL_TRY(gnorm(x, nullptr, w.gn, 1e-6f, 0, n, 0.f, gn_ss, &gn_folded));
    }
    b.t = talloc(H, Wd, C);
    b.st1 = ln_slot(b.p.M, C); b.st2 = ln_slot(b.p.M, C); b.st3 = ln_slot(b.p.M, C);
    b.q = (bf16_t*)m->arena.alloc(sizeof(bf16_t) * (size_t)Bx * w.heads * b.hw_pad * w.dp);      // (kv tiles are 32 wide; pad rows hold finite stale data and are masked)
    b.k = (bf16_t*)m->arena.alloc(sizeof(bf16_t) * (size_t)Bx * w.heads * b.hw_pad * w.dp);
    b.vt = (bf16_t*)m->arena.alloc(sizeof(bf16_t) * (size_t)Bx * w.heads * w.dpv * b.hw_pad);
    b.o = (bf16_t*)m->arena.alloc(sizeof(bf16_t) * (size_t)b.p.M * w.heads * w.dp);
    GILL_TRY(xf_self_attention(b, gn_folded ? x.p : n.p, gn_folded ? gn_ss : nullptr));
    GILL_TRY(xf_cross_attention(b, x));
    GILL_TRY(xf_feed_forward(b, out, next));
    m->arena.release(mk);
    return 0;
  }

  // sample: (Bx, in_ch, L, L) fp32 NCHW -> eps (Bx, out_ch, L, L) fp32 NCHW
  int forward(const float* sample, float* eps_out) {
    const gill_unet_config& c = m->cfg;
    const int* ch = c.block_out_channels;
    const int L = c.sample_size;
    m->arena.off = 0;
    m->gn_next = 0;
    m->ln_next = 0;
    m->coop_next = 0;
    // (the statistics pools need no zeroing: every partial sum is written exactly once by its producer; the COOP arrival counters are zeroed
    // by the forward's first kernel, below)
    std::vector<Tensor> skips;
    Tensor x = talloc(L, L, ch[0], true);
    {
      // conv_in: im2col (K = 9*Cin padded to whole 64-wide steps: 64 for 4 channels, 128 for the inpainting UNet's 9) + MFMA GEMM
      const size_t mk = m->arena.mark();
      const int kpad = conv_in_kpad(c.in_channels);
      bf16_t* col = (bf16_t*)m->arena.alloc(sizeof(bf16_t) * (size_t)Bx * L * L * kpad);
      if (!dry) GILL_TRY(im2col_nchw_launch(sample, Bx, c.in_channels, L, L, kpad, col, s, m->coop_ctr, (int)m->coop_n));
      GILL_TRY(linear(col, kpad, nullptr, 0, kpad, Bx * L * L, m->conv_in_w, m->conv_in_b, ch[0], kpad, nullptr, ACT_NONE, x.p, ch[0], &x));
      m->arena.release(mk);
    }
    skips.push_back(x);
    // Where a block's last GEMM is a split-K launch (levels 2-3 at the 8-sample batch) and the next consumer's first op is a
    // single-source GroupNorm, that norm is offered to the producer's reducer (FusedNorm): `pn` carries the normalised copy forward.
    // Round 6: the same offer goes to non-split producers too — the 3x3 convolutions of levels 0-1 finish the norm in their own epilogue
    // (gemm.hip "COOP": the workgroups of a sample wait for each other's partials) — as a normalised copy, or (table) as the scale | shift table
    // the level-0 projection kernel applies on load.
    Handoff pn{*this};
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 2; ++j) {
        Tensor y;
        // CFG pair: the first resnet and the first transformer block up to its self-attention see identical inputs in
        // both halves of the batch -> run them on the first half only (xf() widens to the full pair inside)
        const bool share = cfg_pair && i == 0 && j == 0 && Bx % 2 == 0 && temb_bstride == 0;
        BatchScope prefix(Bx, share ? Bx / 2 : Bx);     // (to the end of this iteration)
        const Handoff::Taken pre = pn.take();
        // this resnet's consumer: the transformer block's GroupNorm (i < 3), else the next resnet's / the mid block's norm1
        FusedNorm* nx = nullptr;
        if (i < 3) nx = pn.offer(m->down_xf[i][j].gn, 1e-6f, 0, x.H, x.W, ch[i], xf_plan_of(m->down_xf[i][j], x.H * x.W, share).gn_table);
        else nx = pn.offer(j == 0 ? m->down_res[3][1].n1 : m->mid_res[0].n1, 1e-5f, 1, x.H, x.W, ch[i]);
        GILL_TRY(resnet(x, nullptr, m->down_res[i][j], &y, true, pre.copy(), nx));
        x = y;
        // next consumer: resnet norm1 (j == 0) / the downsample conv or the mid block's norm1 (j == 1)
        if (i < 3) {
          const Handoff::Taken pre2 = pn.take();
          FusedNorm* nx2 = (i >= 2 && j == 0) ? pn.offer(m->down_res[i][1].n1, 1e-5f, 1, x.H, x.W, ch[i]) : nullptr;
          Tensor z; GILL_TRY(xf(x, m->down_xf[i][j], &z, true, share, pre2.copy(), nx2, pre2.ss)); x = z;   // next GroupNorm and / or a skip
        }
        skips.push_back(x);
      }
      if (i < 3) {
        Tensor y = talloc(x.H / 2, x.W / 2, ch[i], true);
        FusedNorm* nx = pn.offer(m->down_res[i + 1][0].n1, 1e-5f, 1, y.H, y.W, ch[i]);
        GILL_TRY(conv(x, nullptr, m->down_ds[i], 2, 0, nullptr, 0, nullptr, y, nx));
        x = y;
        skips.push_back(x);
      }
    }
    {
      const Handoff::Taken pre = pn.take();
      FusedNorm* nx = pn.offer(m->mid_xf.gn, 1e-6f, 0, x.H, x.W, ch[3]);
      Tensor y; GILL_TRY(resnet(x, nullptr, m->mid_res[0], &y, true, pre.copy(), nx)); x = y;
      const Handoff::Taken pre2 = pn.take();
      FusedNorm* nx2 = pn.offer(m->mid_res[1].n1, 1e-5f, 1, x.H, x.W, ch[3]);
      Tensor z; GILL_TRY(xf(x, m->mid_xf, &z, true, false, pre2.copy(), nx2)); x = z;
      const Handoff::Taken pre3 = pn.take();
      Tensor u; GILL_TRY(resnet(x, nullptr, m->mid_res[1], &u, true, pre3.copy(), nullptr)); x = u;   // -> two-source norm1 of up block 0
    }
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 3; ++j) {
        Tensor skip = skips.back(); skips.pop_back();
        Tensor y;
        // (norm1 of an up-block resnet is two-source: never offered; its conv2 feeds the transformer block's GroupNorm)
        FusedNorm* nx = (i >= 1) ? pn.offer(m->up_xf[i][j].gn, 1e-6f, 0, x.H, x.W, ch[3 - i], xf_plan_of(m->up_xf[i][j], x.H * x.W, false).gn_table) : nullptr;
        GILL_TRY(resnet(x, &skip, m->up_res[i][j], &y, true, nullptr, nx));
        x = y;
        if (i > 0) {
          const Handoff::Taken pre = pn.take();
          Tensor z; GILL_TRY(xf(x, m->up_xf[i][j], &z, true, false, pre.copy(), nullptr, pre.ss)); x = z;
        }
      }
      if (i < 3) {
        // (4-tap form: the epilogue's GroupNorm slabs are 64 SOURCE rows of one parity class — tiny grids leave the sums to the consumer)
        Tensor y = talloc(x.H * 2, x.W * 2, x.C, !m->up_us[i].ups4 || (x.H * x.W) % GN_SLAB_ROWS == 0);
        GILL_TRY(conv(x, nullptr, m->up_us[i], 1, 1, nullptr, 0, nullptr, y));
        x = y;
      }
    }
    Tensor n = talloc(L, L, ch[0]);
    GILL_TRY(gnorm(x, nullptr, m->norm_out, 1e-5f, 1, n));
    GILL_TRY(dbg_sync("last groupnorm"));
    if (!dry) GILL_TRY(conv_out_launch(n.p, m->conv_out_w, m->conv_out_b, Bx, ch[0], L, L, c.out_channels, eps_out, s));
    GILL_TRY(dbg_sync("conv_out"));
    // (a real run must never need more than the dry run of unet_plan_and_alloc() counted)
    GILL_REQUIRE(dry || m->arena.high <= m->arena.cap, "internal: activation arena overflow (the dry run and the real run allocate differently)");
    return 0;
  }
};

}  // namespace

static int unet_plan_and_alloc(gill_unet* m) {
  const gill_unet_config& c = m->cfg;
  const int Bx = c.max_batch;
  const int L = c.sample_size;
  const size_t n_lat = (size_t)c.out_channels * L * L, n_in = (size_t)c.in_channels * L * L;
  m->ctx_pad = round_up(c.ctx_len, 64);     // whole 64-key tiles: the LDS-DMA attention kernel streams them unclamped (attention.hip)
  // dry run to size the activation arena
  m->arena.dry = true; m->arena.off = 0; m->arena.high = 0;
  m->kcache.assign(m->n_xf, nullptr); m->vcache.assign(m->n_xf, nullptr);
  m->xq_w.assign(m->n_xf, nullptr); m->xo_w.assign(m->n_xf, nullptr); m->xq_cs.assign(m->n_xf, nullptr); m->xq_b.assign(m->n_xf, nullptr);
  UNetRun r{m, nullptr, Bx, nullptr, 0, true};
  GILL_TRY(r.forward(nullptr, nullptr));
  if (Bx % 2 == 0) {               // the CFG shared-prefix path allocates differently: size for the larger of the two
    const size_t gn1 = m->gn_next; const size_t ln1 = m->ln_next; const size_t co1 = m->coop_next;
    r.cfg_pair = true;
    GILL_TRY(r.forward(nullptr, nullptr));   // (arena.high is a running maximum)
    if (gn1 > m->gn_next) m->gn_next = gn1;
    if (ln1 > m->ln_next) m->ln_next = ln1;
    if (co1 > m->coop_next) m->coop_next = co1;
  }
  // (unet_ctx_cache stages the XALG layers' T = ctx [G | G2]^T here: at most ctx_len x 2 x 8 x 1280 bf16 per sample)
  const size_t t_stage = sizeof(bf16_t) * (size_t)Bx * c.ctx_len * 2 * 8 * c.block_out_channels[3];
  const size_t need = (m->arena.high > t_stage ? m->arena.high : t_stage) + (1 << 20);
  GILL_TRY(m->pool.alloc(&m->arena_mem, need, true));
  m->arena.base = m->arena_mem; m->arena.cap = need; m->arena.dry = false; m->arena.off = 0;
  m->gn_floats = m->gn_next + 64;           // counted by the dry run
  GILL_TRY(m->pool.alloc(&m->gn_stats, m->gn_floats));
  m->ln_floats = m->ln_next + 64;           // counted by the dry run (max batch)
  GILL_TRY(m->pool.alloc(&m->ln_stats, m->ln_floats));
  m->coop_n = m->coop_next + 64;            // COOP arrival counters: counted by the dry run
  GILL_TRY(m->pool.alloc(&m->coop_ctr, m->coop_n));
  m->splitk_ws_floats = (size_t)48 << 20;   // 192 MiB of fp32 partials
  GILL_TRY(m->pool.alloc(&m->splitk_ws, m->splitk_ws_floats, false));
  // cross-attention K/V caches
  auto alloc_cache = [&](const XfW& w) -> int {
    if (w.forms.xalg) {
      const size_t n80 = (size_t)80 * w.heads;
      GILL_TRY(m->pool.alloc(&m->xq_w[w.layer_id], (size_t)Bx * n80 * w.C, false));
      GILL_TRY(m->pool.alloc(&m->xo_w[w.layer_id], (size_t)Bx * n80 * w.C, false));
      GILL_TRY(m->pool.alloc(&m->xq_cs[w.layer_id], (size_t)Bx * n80));
      GILL_TRY(m->pool.alloc(&m->xq_b[w.layer_id], (size_t)Bx * n80));
      // (unet_ctx_cache stages T = ctx [G | G2]^T in the activation arena, which is idle between forwards)
      GILL_REQUIRE(m->arena.cap >= sizeof(bf16_t) * (size_t)Bx * c.ctx_len * 2 * w.heads * w.C, "internal: arena smaller than the cross-attention staging tensor");
      return 0;
    }
    GILL_TRY(m->pool.alloc(&m->kcache[w.layer_id], (size_t)Bx * w.heads * m->ctx_pad * w.dp, true));
    GILL_TRY(m->pool.alloc(&m->vcache[w.layer_id], (size_t)Bx * w.heads * w.dpv * m->ctx_pad, true));
    return 0;
  };
  for (int i = 0; i < 3; ++i) for (const XfW& w : m->down_xf[i]) GILL_TRY(alloc_cache(w));
  GILL_TRY(alloc_cache(m->mid_xf));
  for (int i = 1; i < 4; ++i) for (const XfW& w : m->up_xf[i]) GILL_TRY(alloc_cache(w));
  // time embedding scratch: up to 1024 rows (timesteps of a schedule, or per-sample timesteps)
  m->temb_rows_cap = 1024 > Bx ? 1024 : Bx;
  GILL_TRY(m->pool.alloc(&m->t_dev, (size_t)m->temb_rows_cap));
  GILL_TRY(m->pool.alloc(&m->t_sin, (size_t)m->temb_rows_cap * c.block_out_channels[0]));
  GILL_TRY(m->pool.alloc(&m->t_h1, (size_t)m->temb_rows_cap * m->temb_dim));
  GILL_TRY(m->pool.alloc(&m->t_h2, (size_t)m->temb_rows_cap * m->temb_dim));
  GILL_TRY(m->pool.alloc(&m->temb_table, (size_t)m->temb_rows_cap * m->temb_total));
  // loop state
  GILL_TRY(m->pool.alloc(&m->lat, (size_t)Bx * n_lat));
  GILL_TRY(m->pool.alloc(&m->lat2, (size_t)Bx * n_in));
  GILL_TRY(m->pool.alloc(&m->eps, (size_t)Bx * n_lat));
  GILL_TRY(m->pool.alloc(&m->cur_sample, (size_t)Bx * n_lat));
  GILL_TRY(m->pool.alloc(&m->ets, (size_t)4 * Bx * n_lat));
  GILL_TRY(m->pool.alloc(&m->ctx_full, (size_t)Bx * c.ctx_len * c.cross_attention_dim));
  GILL_TRY(m->pool.alloc(&m->temb_cur, (size_t)m->temb_total));
  GILL_TRY(m->pool.alloc(&m->plms_rows, (size_t)m->temb_rows_cap));
  GILL_TRY(m->pool.alloc(&m->sampler_rows, (size_t)m->temb_rows_cap));
  GILL_TRY(m->pool.alloc(&m->noise_slot, (size_t)1));
  GILL_TRY(m->pool.alloc(&m->step_ctr, (size_t)2));
  GILL_TRY(m->pool.alloc(&m->guidance_dev, (size_t)4));
  // inpainting operands, by the mode this handle can run (a loop without CFG holds max_batch samples)
  GILL_TRY(m->pool.alloc(&m->inp_mask, (size_t)Bx * L * L));
  if (c.in_channels == c.out_channels) {      // blend
    GILL_TRY(m->pool.alloc(&m->inp_x0, (size_t)Bx * n_lat));
    GILL_TRY(m->pool.alloc(&m->inp_z0, (size_t)Bx * n_lat));
    GILL_TRY(m->pool.alloc(&m->keep_rows, (size_t)m->temb_rows_cap * 2));
  } else {                                    // concat
    GILL_TRY(m->pool.alloc(&m->inp_xm, (size_t)Bx * n_lat));
  }
  { const char* e = getenv("GILL_NO_GRAPH"); m->use_graph = !(e && e[0] == '1'); }
  if (getenv("GILL_DEBUG_SYNC")) m->use_graph = false;   // dbg_sync() synchronises the stream after every launch: illegal inside a capture
  return 0;
}

// time-embedding MLP + all resnet time projections for `rows` timesteps -> m->temb_table [rows][temb_total]
static int unet_time_table(gill_unet* m, const float* t_host, int rows, hipStream_t s) {
  GILL_REQUIRE(rows >= 1 && rows <= m->temb_rows_cap, "too many timesteps for the time-embedding scratch");
  const int c0 = m->cfg.block_out_channels[0], td = m->temb_dim;
  GILL_CHECK_HIP(hipMemcpyAsync(m->t_dev, t_host, sizeof(float) * rows, hipMemcpyHostToDevice, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));   // t_host may be a transient host buffer
  GILL_TRY(timestep_embed_launch(m->t_dev, rows, c0, m->t_sin, s));
  GemmArgs g;
  g.M = rows; g.N = td; g.K = c0; g.K1 = c0; g.A = m->t_sin; g.lda = c0; g.W = m->te1.w; g.bias = m->te1.b;
  g.act = ACT_SILU; g.C = m->t_h1; g.ldc = td;
  GILL_TRY(gemm_launch(g, s));
  GemmArgs g2;
  g2.M = rows; g2.N = td; g2.K = td; g2.K1 = td; g2.A = m->t_h1; g2.lda = td; g2.W = m->te2.w; g2.bias = m->te2.b;
  g2.act = ACT_SILU;   // every resnet applies SiLU to emb before its time_emb_proj
  g2.C = m->t_h2; g2.ldc = td;
  GILL_TRY(gemm_launch(g2, s));
  GemmArgs g3;
  g3.M = rows; g3.N = m->temb_total; g3.K = td; g3.K1 = td; g3.A = m->t_h2; g3.lda = td; g3.W = m->temb_proj_w;
  g3.bias = m->temb_proj_b; g3.out_mode = OUT_F32; g3.C = m->temb_table; g3.ldc = m->temb_total;
  return gemm_launch(g3, s);
}

// cross-attention K/V of every transformer layer for ctx (Bx,77,ctx_dim)
static int unet_ctx_cache(gill_unet* m, const bf16_t* ctx, int Bx, hipStream_t s) {
  const gill_unet_config& c = m->cfg;
  auto one = [&](const XfW& w) -> int {
    if (w.forms.xalg) {
      const int H = w.heads, C = w.C, E = c.cross_attention_dim, id = w.layer_id;
      return xalg_operands_launch(ctx, w.xg, w.xgb, Bx, H, C, E, c.ctx_len, (bf16_t*)m->arena.base, m->xq_w[id], m->xq_cs[id], m->xq_b[id], m->xo_w[id], s);
    }
    GemmArgs g;
    g.M = Bx * c.ctx_len; g.N = 2 * w.heads * w.dp; g.K = c.cross_attention_dim; g.K1 = g.K;
    g.A = ctx; g.lda = c.cross_attention_dim; g.W = w.wkv2;
    g.out_mode = OUT_QKV; g.Ck = m->kcache[w.layer_id]; g.Cvt = m->vcache[w.layer_id];
    g.heads = w.heads; g.dp = w.dp; g.dpv = w.dpv; g.ntok = c.ctx_len; g.ntok_pad_q = m->ctx_pad;
    g.ntok_pad_kv = m->ctx_pad; g.seg_base = 1;
    return gemm_launch(g, s);
  };
  for (int i = 0; i < 3; ++i) for (const XfW& w : m->down_xf[i]) GILL_TRY(one(w));
  GILL_TRY(one(m->mid_xf));
  for (int i = 1; i < 4; ++i) for (const XfW& w : m->up_xf[i]) GILL_TRY(one(w));
  return 0;
}

// The in-kernel GroupNorm finishes (gemm.hip "COOP") wait for each other inside a launch: legal only while this handle's stream has the device's CUs
// to itself.  A bounded wait that ran out NaN-poisons its outputs and counts itself on the device; every entry point looks at that count first
// (its own time-table upload synchronises with the stream anyway) and refuses to go on silently.
static int unet_coop_check() {
  unsigned n = 0;
  GILL_TRY(gemm_coop_giveups(&n));
  if (n) {
    gill_set_error("an earlier call's in-kernel GroupNorm finish timed out " + std::to_string(n) + " time(s) and NaN-poisoned its outputs: the GPU is shared with "
                   "another stream or process that also runs waiting workgroups.  Give the handle the device to itself, or set GILL_GEMM_COOP=0");
    return -5;
  }
  return 0;
}
extern "C" int gill_coop_timeouts(void) {
  unsigned n = 0;
  if (gemm_coop_giveups(&n) != 0) return -1;
  return (int)n;
}

extern "C" int gill_unet_forward(gill_unet* m, const float* sample, const float* timesteps_host, const void* ctx_bf16,
                                 int Bx, float* eps_out, void* stream) {
  GILL_REQUIRE(m && sample && timesteps_host && ctx_bf16 && eps_out, "null argument");
  GILL_TRY(unet_coop_check());
  GILL_REQUIRE(Bx >= 1 && Bx <= m->cfg.max_batch, "batch exceeds the UNet handle's max_batch");
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(unet_time_table(m, timesteps_host, Bx, s));
  GILL_TRY(unet_ctx_cache(m, (const bf16_t*)ctx_bf16, Bx, s));
  UNetRun r{m, s, Bx, m->temb_table, m->temb_total, false};
  return r.forward(sample, eps_out);
}

// init_noise != nullptr: image-to-image — the loop starts at step `start` from add_noise(latents0, init_noise) instead of latents0 * init_noise_sigma
// inpaint (needs init_noise): 1 blend — latent_mask given, the handle's UNet takes the latents alone; 2 concat — latent_mask and masked_latents
// given, the handle's UNet takes [latents | mask | masked-image latents]
static int sd_denoise_on(gill_unet* m, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond,
                         const float* latents0, int B, int num_steps, float guidance, float* latents_out, const float* noise, hipStream_t s,
                         int start = 0, const float* init_noise = nullptr, int inpaint = 0, const float* latent_mask = nullptr,
                         const float* masked_latents = nullptr) {
  const bool cfg = guidance > 1.0f;     // do_classifier_free_guidance (custom_sd.py:588)
  const int Bx = cfg ? 2 * B : B;
  GILL_REQUIRE(B >= 1 && Bx <= m->cfg.max_batch, "batch exceeds the UNet handle's max_batch");
  GILL_REQUIRE(!cfg || uncond_bf16 != nullptr, "uncond embedding required when guidance > 1");
  const gill_unet_config& c = m->cfg;
  const int L = c.sample_size;
  const int64_t n_lat = (int64_t)c.out_channels * L * L;     // the latents; the UNet input of a concat-mode handle has in_channels
  GILL_REQUIRE(inpaint == 2 || c.in_channels == c.out_channels,
               "this handle's UNet takes [latents | mask | masked-image latents] (in_channels != out_channels): use gill_sd_inpaint with masked_latents");
  GILL_REQUIRE(inpaint == 0 || (init_noise && latent_mask && (inpaint == 1 || masked_latents)), "inpaint: null argument");
  const size_t ctx_elems = (size_t)c.ctx_len * c.cross_attention_dim;

  SdSchedule sched;
  GILL_TRY(sd_schedule(sampler, c.v_prediction != 0, num_steps, sched, start));
  const bool linear = sched.kind != SD_PNDM;
  const int ncalls = (int)sched.timesteps.size();
  GILL_REQUIRE(ncalls <= m->temb_rows_cap, "too many steps for the time-embedding scratch");
  GILL_REQUIRE(!sched.needs_noise || noise != nullptr, "this sampler draws noise in its steps: a [ncalls][B][n] noise table is required");

  if (linear) {
    GILL_CHECK_HIP(hipMemcpyAsync(m->sampler_rows, sched.rows.data(), sizeof(SamplerRow) * ncalls, hipMemcpyHostToDevice, s));
    GILL_CHECK_HIP(hipMemcpyAsync(m->noise_slot, &noise, sizeof(noise), hipMemcpyHostToDevice, s));   // (synchronised below)
  } else
  GILL_CHECK_HIP(hipMemcpyAsync(m->plms_rows, sched.plms.data(), sizeof(PlmsRow) * ncalls, hipMemcpyHostToDevice, s));
  GILL_CHECK_HIP(hipMemsetAsync(m->step_ctr, 0, sizeof(int) * 2, s));
  GILL_CHECK_HIP(hipMemcpyAsync(m->guidance_dev, &guidance, sizeof(float), hipMemcpyHostToDevice, s));   // (synchronised below)
  std::vector<float> keep32;
  if (inpaint) {
    // the loop's operands into the handle's buffers, as ctx_full: the captured step then holds the handle's addresses and serves every call
    GILL_CHECK_HIP(hipMemcpyAsync(m->inp_mask, latent_mask, sizeof(float) * (size_t)B * L * L, hipMemcpyDeviceToDevice, s));
    if (inpaint == 1) {
      std::vector<double> keep;
      GILL_TRY(sd_inpaint_keep(sampler, c.v_prediction != 0, num_steps, start, sched, keep));
      keep32.assign(keep.begin(), keep.end());
      GILL_CHECK_HIP(hipMemcpyAsync(m->keep_rows, keep32.data(), sizeof(float) * keep32.size(), hipMemcpyHostToDevice, s));   // (synchronised below)
      GILL_CHECK_HIP(hipMemcpyAsync(m->inp_x0, latents0, sizeof(float) * n_lat * B, hipMemcpyDeviceToDevice, s));
      GILL_CHECK_HIP(hipMemcpyAsync(m->inp_z0, init_noise, sizeof(float) * n_lat * B, hipMemcpyDeviceToDevice, s));
    } else {
      GILL_CHECK_HIP(hipMemcpyAsync(m->inp_xm, masked_latents, sizeof(float) * n_lat * B, hipMemcpyDeviceToDevice, s));
    }
  }
  // hoisted: time-embedding table for every call (its stream sync also covers the host `rows` buffer), prompt K/V caches
  GILL_TRY(unet_time_table(m, sched.timesteps.data(), ncalls, s));
  // prompt_embeds = cat([negative_prompt_embeds.repeat(B), prompt_embeds])  (custom_sd.py:365-371)
  if (cfg) {
    for (int b = 0; b < B; ++b)
      GILL_CHECK_HIP(hipMemcpyAsync(m->ctx_full + (size_t)b * ctx_elems,
                                    (const bf16_t*)uncond_bf16 + (n_uncond == B ? (size_t)b * ctx_elems : 0),
                                    sizeof(bf16_t) * ctx_elems, hipMemcpyDeviceToDevice, s));
    GILL_CHECK_HIP(hipMemcpyAsync(m->ctx_full + (size_t)B * ctx_elems, cond_bf16, sizeof(bf16_t) * ctx_elems * B,
                                  hipMemcpyDeviceToDevice, s));
  } else {
    GILL_CHECK_HIP(hipMemcpyAsync(m->ctx_full, cond_bf16, sizeof(bf16_t) * ctx_elems * B, hipMemcpyDeviceToDevice, s));
  }
  GILL_TRY(unet_ctx_cache(m, m->ctx_full, Bx, s));
  if (init_noise) GILL_TRY(add_noise_f32_launch(latents0, init_noise, (float)sched.add_a, (float)sched.add_b, n_lat * B, m->lat, s));
  else GILL_TRY(scale_f32_launch(latents0, (float)sched.init_noise_sigma, n_lat * B, m->lat, s));    // custom_sd.py:472

  // One loop step = stage kernel (latents -> UNet input, time-embedding row of the device-side step counter) + UNet forward
  // (~390 launches at ~10+ us of host time each: at small batch the GPU outruns the host) + CFG/PLMS kernel (reads its
  // coefficients from the device-side table, bumps the counter).  The step is captured ONCE per batch size into a hipGraph
  // and replayed ncalls times back to back: nothing but graph launches sits between two steps.
  SdLoopArgs la;
  la.rows = m->plms_rows; la.ctr = m->step_ctr; la.temb_table = m->temb_table; la.temb_total = m->temb_total;
  la.temb_cur = m->temb_cur; la.eps = m->eps; la.lat = m->lat; la.lat2 = m->lat2; la.cur_sample = m->cur_sample; la.ets = m->ets;
  la.B = B; la.n = n_lat; la.guidance = m->guidance_dev; la.cfg = cfg ? 1 : 0;
  if (linear) { la.srows = m->sampler_rows; la.noise = m->noise_slot; }
  SdInpaintArgs ia;
  ia.l = la; ia.x0 = m->inp_x0; ia.z0 = m->inp_z0; ia.mask = m->inp_mask; ia.xm = m->inp_xm; ia.keep = m->keep_rows; ia.hw = (int64_t)L * L;
  // the graph bakes in B, the CFG flag and the step's loop kernels (with their row table) besides the buffer addresses
  const GraphKey gkey{Bx, cfg ? 1 : 0, linear ? 1 : 0, inpaint};
  auto one_step = [&](hipStream_t st) -> int {
    GILL_TRY(inpaint == 2 ? sd_stage_concat_launch(ia, st) : sd_stage_launch(la, st));
    UNetRun r{m, st, Bx, m->temb_cur, 0, false};
    r.cfg_pair = cfg;
    GILL_TRY(r.forward(m->lat2, m->eps));
    GILL_TRY(linear ? sampler_step_launch(la, st) : plms_step_launch(la, st));
    return inpaint == 1 ? sd_blend_launch(ia, st) : 0;      // (a kernel, not a memcpy node: ops.h)
  };
  for (int i = 0; i < ncalls; ++i) {
    auto git = m->graphs.find(gkey);
    if (git == m->graphs.end() && m->use_graph && m->warmed.count(gkey)) {
      hipGraph_t graph = nullptr;
      hipGraphExec_t exec = nullptr;
      // s is the handle's private stream (never the legacy NULL stream, which cannot be captured)
      GILL_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
      const int rc_status = one_step(s);
      const hipError_t ec = hipStreamEndCapture(s, &graph);
      if (rc_status != 0) { if (graph) (void)hipGraphDestroy(graph); return rc_status; }
      GILL_CHECK_HIP(ec);
      GILL_CHECK_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      (void)hipGraphDestroy(graph);
      git = m->graphs.emplace(gkey, exec).first;
    }
    if (git != m->graphs.end()) {
      GILL_CHECK_HIP(hipGraphLaunch(git->second, s));
    } else {
      // first step of this batch size runs eagerly: it also performs every one-time kernel attribute set-up,
      // which must not happen inside a stream capture
      GILL_TRY(one_step(s));
      m->warmed.insert(gkey);
    }
  }
  GILL_CHECK_HIP(hipMemcpyAsync(latents_out, m->lat, sizeof(float) * n_lat * B, hipMemcpyDeviceToDevice, s));
  return 0;
}

// every public loop, its arguments checked: sd_denoise_on on the handle's private stream, between two fences to the caller's
static int sd_denoise_fenced(gill_unet* m, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond, const float* latents0,
                             int B, int num_steps, float guidance, float* latents_out, const float* noise, void* stream, int start = 0,
                             const float* init_noise = nullptr, int inpaint = 0, const float* latent_mask = nullptr, const float* masked_latents = nullptr) {
  GILL_TRY(unet_coop_check());
  hipStream_t caller = (hipStream_t)stream;
  GILL_TRY(m->fence.enter(caller));
  const int rc = sd_denoise_on(m, sampler, cond_bf16, uncond_bf16, n_uncond, latents0, B, num_steps, guidance, latents_out, noise, m->fence.stream, start,
                               init_noise, inpaint, latent_mask, masked_latents);
  GILL_TRY(m->fence.leave(caller));
  return rc;
}
extern "C" int gill_sd_denoise_ex(gill_unet* m, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond,
                                  const float* latents0, int B, int num_steps, float guidance, float* latents_out, const float* noise,
                                  void* stream) {
  GILL_REQUIRE(m && sampler && cond_bf16 && latents0 && latents_out, "null argument");
  GILL_REQUIRE(guidance <= 1.0f || uncond_bf16 == nullptr || n_uncond == 1 || n_uncond == B, "negative embeddings: batch must be 1 or B");
  return sd_denoise_fenced(m, sampler, cond_bf16, uncond_bf16, n_uncond, latents0, B, num_steps, guidance, latents_out, noise, stream);
}
extern "C" int gill_sd_denoise_from(gill_unet* m, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond,
                                    int start, const float* init_latents, const float* init_noise, int B, int num_steps, float guidance,
                                    float* latents_out, const float* noise, void* stream) {
  GILL_REQUIRE(m && sampler && cond_bf16 && init_latents && init_noise && latents_out, "null argument");
  GILL_REQUIRE(guidance <= 1.0f || uncond_bf16 == nullptr || n_uncond == 1 || n_uncond == B, "negative embeddings: batch must be 1 or B");
  return sd_denoise_fenced(m, sampler, cond_bf16, uncond_bf16, n_uncond, init_latents, B, num_steps, guidance, latents_out, noise, stream, start, init_noise);
}
extern "C" int gill_sd_inpaint(gill_unet* m, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond,
                               int start, const float* init_latents, const float* init_noise, const float* latent_mask,
                               const float* masked_latents, int B, int num_steps, float guidance, float* latents_out, const float* noise,
                               void* stream) {
  GILL_REQUIRE(m && sampler && cond_bf16 && init_latents && init_noise && latent_mask && latents_out, "null argument");
  GILL_REQUIRE(guidance <= 1.0f || uncond_bf16 == nullptr || n_uncond == 1 || n_uncond == B, "negative embeddings: batch must be 1 or B");
  const gill_unet_config& c = m->cfg;
  if (masked_latents)
    GILL_REQUIRE(c.in_channels == 2 * c.out_channels + 1,
                 "inpaint: masked_latents given (concat mode), but this handle's UNet does not take [latents | mask | masked-image latents] "
                 "(in_channels != 2 * out_channels + 1): pass NULL to blend with the mask instead");
  else
    GILL_REQUIRE(c.in_channels == c.out_channels,
                 "inpaint: masked_latents is NULL (blend mode), but this handle's UNet takes more than the latents "
                 "(in_channels != out_channels): an inpainting UNet needs the masked image's latents");
  return sd_denoise_fenced(m, sampler, cond_bf16, uncond_bf16, n_uncond, init_latents, B, num_steps, guidance, latents_out, noise, stream, start, init_noise,
                           masked_latents ? 2 : 1, latent_mask, masked_latents);
}
extern "C" int gill_sd_denoise(gill_unet* m, const void* cond_bf16, const void* uncond_bf16, int n_uncond, const float* latents0,
                               int B, int num_steps, float guidance, float* latents_out, void* stream) {
  const gill_sd_sampler pndm = {SD_PNDM, 1, 0, 0.f};
  return gill_sd_denoise_ex(m, &pndm, cond_bf16, uncond_bf16, n_uncond, latents0, B, num_steps, guidance, latents_out, nullptr, stream);
}
extern "C" int gill_sd_inpaint_prepare(const float* image, const float* mask, int B, int Bm, int H, int W, float* masked_image_out,
                                       float* latent_mask_out, void* stream) {
  GILL_REQUIRE(image && mask && masked_image_out && latent_mask_out, "null argument");
  return inpaint_prepare_launch(image, mask, B, Bm, H, W, masked_image_out, latent_mask_out, (hipStream_t)stream);
}
