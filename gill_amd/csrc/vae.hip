// Stage 3b — Stable Diffusion VAE decoder: final latents -> 512x512 RGB.
//
// Replaces StableDiffusionPipeline.decode_latents (gill/custom_sd.py:385-392):
//     latents = 1 / 0.18215 * latents
//     image = self.vae.decode(latents).sample
//     image = (image / 2 + 0.5).clamp(0, 1)
// The decoder itself is diffusers' AutoencoderKL (SD-1.5 vae/config.json: block_out_channels 128/256/512/512,
// layers_per_block 2, GroupNorm(32, eps 1e-6), SiLU, one single-head 512-d attention in the mid block) — not in the
// reference tree; structure restated from the published model, state-dict names are diffusers'
// ("decoder.up_blocks.2.resnets.0.conv_shortcut.weight", "post_quant_conv.weight", ...).
//
// Built from the same kernels as the UNet: NHWC bf16 activations, implicit-GEMM 3x3 convs with the 1x1 shortcut and
// the nearest-2x upsample folded in, GroupNorm statistics accumulated by the producing conv's epilogue.  The single
// 512-wide attention head does not fit the flash kernel's register budget, so it runs as two MFMA GEMMs per image
// (S = Q K^T, O = P V) around a row-softmax kernel: 68 GFLOP per image, once per image — not a hot spot.
//
// The encoder half (image-to-image: AutoencoderKL.encode(image).latent_dist.sample() * scaling_factor) is the mirror image on the same
// pieces: conv_in 3 -> ch[0] as im2col (K = 27 padded to 64) + GEMM from fp32 NCHW pixels, four down blocks of two resnets
// ("encoder.down_blocks.{i}.resnets.{j}", the 1x1 shortcut fused into conv2) with, below the last, "downsamplers.0.conv": diffusers'
// Downsample2D(padding = 0), F.pad(x, (0, 1, 0, 1)) + conv(stride 2, pad 0), run as the stride-2 gather with its origin shifted
// (GemmArgs::pad_shift); the mid block (resnet, the same single-head attention, resnet); conv_norm_out + SiLU; conv_out to
// 2 * latent_channels fp32 NCHW; and one finishing kernel for quant_conv, the mean | logvar split, the clamp and the sample.
// It lives INSIDE gill_vae (VaeEncoder, built only when the weight table holds "encoder.conv_in.weight") with an arena and a
// statistics pool of its own, sized by its own dry run: see DESIGN.md "VAE encoder".
#include "convnet.h"
#include <math.h>
#include <memory>

struct AttnW {      // the mid block's single-head attention
  NormW gn;
  bf16_t* wqkv = nullptr; float* bqkv = nullptr;   // [3C][C]
  bf16_t* wo = nullptr; float* bo = nullptr;
};

// the encoder half: its weights and its own workspace (arena + GroupNorm statistics pool); the split-K workspace is the handle's
struct VaeEncoder : ConvWorkspace {
  bf16_t* conv_in_w = nullptr; float* conv_in_b = nullptr;   // [ch0][64] (im2col K = 27 padded to 64)
  ResW down_res[4][2];
  ConvW down_ds[3];
  ResW mid_res[2];
  AttnW attn;
  NormW norm_out;
  bf16_t* conv_out_w = nullptr; float* conv_out_b = nullptr; // [2 lc][9][ch3]
  float* q_w = nullptr; float* q_b = nullptr;                // quant_conv ((2 lc) x (2 lc) + 2 lc), fp32
  float* h_f32 = nullptr;                                    // [B][2 lc][L][L]: conv_out's output, quant_conv's input
};

struct gill_vae : ConvWorkspace {
  gill_vae_config cfg;
  DevPool pool;
  float* pq_w = nullptr; float* pq_b = nullptr;        // post_quant_conv (4x4 + 4), fp32
  bf16_t* conv_in_w = nullptr; float* conv_in_b = nullptr;   // [C][64] (im2col K = 36 padded to 64)
  ResW mid_res[2];
  AttnW attn;
  std::vector<ResW> up_res[4];
  std::unique_ptr<VaeEncoder> enc;                     // null: decoder-only weights
  ConvW up_us[3];
  NormW norm_out;
  bf16_t* conv_out_w = nullptr; float* conv_out_b = nullptr;
  // workspace (+ ConvWorkspace)
  float* lat_prep = nullptr;   // [B][4][L][L] after scaling + post_quant_conv
  float* img_f32 = nullptr;    // [B][3][8L][8L]
};

// z' = post_quant_conv(z / scaling_factor): per-pixel CxC matrix on NCHW fp32 (C = 4)
__global__ __launch_bounds__(256) void vae_latent_prep_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                              const float* __restrict__ b, float inv_scale, int C, int HW,
                                                              int64_t total, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const int c = (int)((i / HW) % C);
    const int64_t bb = i / ((int64_t)HW * C);
    float acc = b[c];
    for (int k = 0; k < C; ++k) acc += w[c * C + k] * (z[(bb * C + k) * HW + p] * inv_scale);
    out[i] = acc;
  }
}

// Encoder finish on fp32 NCHW: moments = quant_conv(h) (per-pixel (2C)x(2C) matrix), mean | logvar = split, logvar clamped to [-30, 20],
// z = scale * (mean + exp(0.5 logvar) * noise) — noise == nullptr: the posterior mode, z = scale * mean.  One thread per (sample, latent
// channel, pixel) forms its mean and its logvar row.  moments (optional): [B][2C][HW] = mean | clamped logvar.
__global__ __launch_bounds__(256) void vae_encode_finish_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b,
                                                                const float* __restrict__ noise, float scale, int C, int HW, int64_t total,
                                                                float* __restrict__ z, float* __restrict__ moments) {
  const int C2 = 2 * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const int c = (int)((i / HW) % C);
    const int64_t bb = i / ((int64_t)HW * C);
    float mean = b[c], logvar = b[C + c];
    for (int k = 0; k < C2; ++k) {
      const float v = h[(bb * C2 + k) * HW + p];
      mean += w[c * C2 + k] * v;
      logvar += w[(C + c) * C2 + k] * v;
    }
    logvar = fminf(fmaxf(logvar, -30.f), 20.f);
    z[i] = noise ? scale * (mean + __expf(0.5f * logvar) * noise[i]) : scale * mean;
    if (moments) {
      moments[(bb * C2 + c) * HW + p] = mean;
      moments[(bb * C2 + C + c) * HW + p] = logvar;
    }
  }
}

// in-place softmax over rows of a bf16 matrix [rows][n] (n % 512 == 0 not required; n % 8 == 0): one wave per row
__global__ __launch_bounds__(256) void vae_row_softmax_kernel(bf16_t* __restrict__ s, int rows, int n) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  bf16_t* r = s + (size_t)row * n;
  float mx = -INFINITY;
  for (int c = lane * 8; c < n; c += 512) {
    const uint4 u = *reinterpret_cast<const uint4*>(r + c);
    const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmaxf(mx, fmaxf(bf2f((bf16_t)(uu[i] & 0xffff)), bf2f((bf16_t)(uu[i] >> 16))));
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane * 8; c < n; c += 512) {
    const uint4 u = *reinterpret_cast<const uint4*>(r + c);
    const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sum += __expf(bf2f((bf16_t)(uu[i] & 0xffff)) - mx) + __expf(bf2f((bf16_t)(uu[i] >> 16)) - mx);
  }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int c = lane * 8; c < n; c += 512) {
    const uint4 u = *reinterpret_cast<const uint4*>(r + c);
    const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
    uint4 o;
    uint32_t oo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      oo[i] = pack_bf2(__expf(bf2f((bf16_t)(uu[i] & 0xffff)) - mx) * inv, __expf(bf2f((bf16_t)(uu[i] >> 16)) - mx) * inv);
    o.x = oo[0]; o.y = oo[1]; o.z = oo[2]; o.w = oo[3];
    *reinterpret_cast<uint4*>(r + c) = o;
  }
}

int vae_row_softmax_launch(bf16_t* sc, int rows, int n, hipStream_t s) {
  GILL_REQUIRE(sc && rows > 0 && n > 0 && n % 8 == 0, "row softmax: the row length must be a multiple of 8 (the kernel reads 8 elements at a time)");
  hipLaunchKernelGGL(vae_row_softmax_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, sc, rows, n);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

// every GEMM of the VAE, the attention's included: the conv split rule, capped by the partials the workspace holds
int vae_gemm_launch(GemmArgs& g, float* ws, size_t ws_floats, hipStream_t s) {
  g.splitk = gemm_pick_splitk(g.M, g.N, g.K, g.act);
  while (g.splitk > 1 && (size_t)g.splitk * g.M * g.N > ws_floats) --g.splitk;
  g.ws = ws;
  return gemm_launch(g, s);
}

// The single-head attention behind its GroupNorm (convnet.h VaeAttnArgs): the engine's VRun::attention and gill_op_vae_attention both run this.
int vae_attention_chain(VaeAttnArgs& a, hipStream_t s) {
  const int B = a.B, HW = a.HW, C = a.C, M = B * HW;
  GILL_REQUIRE(B >= 1 && HW > 0 && C > 0 && HW % 64 == 0 && C % 64 == 0, "vae attention: HW and C must be multiples of 64");
  GILL_REQUIRE(a.n && a.wqkv && a.bqkv && a.wo && a.bo && a.q && a.k && a.vt && a.sc && a.o && a.out.C, "vae attention: null argument");
  {
    // heads = 1, dp = C: Q and K come out plain row-major [B*HW][C], V transposed [B][C][HW]
    GemmArgs g;
    g.M = M; g.N = 3 * C; g.K = C; g.K1 = C; g.A = a.n; g.lda = C; g.W = a.wqkv; g.bias = a.bqkv;
    g.out_mode = OUT_QKV; g.Cq = a.q; g.Ck = a.k; g.Cvt = a.vt; g.heads = 1; g.dp = C; g.dpv = C; g.ntok = HW;
    g.ntok_pad_q = HW; g.ntok_pad_kv = HW; g.seg_base = 0;
    g.qscale = 1.0f / sqrtf((float)C);   // the natural-exponent domain: vae_row_softmax_kernel takes __expf of the stored scores
    GILL_TRY(vae_gemm_launch(g, a.ws, a.ws_floats, s));
    a.splits[0] = g.splitk;
  }
  for (int b = 0; b < B; ++b) {
    bf16_t* sc = a.sc + (size_t)b * a.sc_bstride;
    GemmArgs g1;   // S = Q K^T
    g1.M = HW; g1.N = HW; g1.K = C; g1.K1 = C; g1.A = a.q + (size_t)b * HW * C; g1.lda = C; g1.W = a.k + (size_t)b * HW * C;
    g1.C = sc; g1.ldc = HW;
    GILL_TRY(vae_gemm_launch(g1, a.ws, a.ws_floats, s));
    GILL_TRY(vae_row_softmax_launch(sc, HW, HW, s));
    GemmArgs g2;   // O = P V
    g2.M = HW; g2.N = C; g2.K = HW; g2.K1 = HW; g2.A = sc; g2.lda = HW; g2.W = a.vt + (size_t)b * C * HW;
    g2.C = a.o + (size_t)b * HW * C; g2.ldc = C;
    GILL_TRY(vae_gemm_launch(g2, a.ws, a.ws_floats, s));
    a.splits[1] = g1.splitk; a.splits[2] = g2.splitk;
  }
  GemmArgs& g3 = a.out;   // to_out (+ the caller's residual and GroupNorm statistics hookup)
  g3.M = M; g3.N = C; g3.K = C; g3.K1 = C; g3.A = a.o; g3.lda = C; g3.W = a.wo; g3.bias = a.bo;
  return vae_gemm_launch(g3, a.ws, a.ws_floats, s);
}

// image = (x / 2 + 0.5).clamp(0, 1): NCHW fp32 -> NHWC uint8 (round(x * 255), what numpy_to_pil produces)
__global__ __launch_bounds__(256) void vae_to_uint8_kernel(const float* __restrict__ x, int C, int HW, int64_t total,
                                                           uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int p = (int)((i / C) % HW);
    const int64_t bb = i / ((int64_t)C * HW);
    float v = x[(bb * C + c) * HW + p] * 0.5f + 0.5f;
    v = fminf(fmaxf(v, 0.f), 1.f);
    out[i] = (uint8_t)__float2int_rn(v * 255.f);
  }
}

namespace {

struct Loader {
  const WeightTable& wt;
  DevPool& pool;
  hipStream_t s;
  // (every conv in the tap-major K order: hw = 0, see load_conv3)
  int resnet(const std::string& p, int cin, int cout, ResW* r) {
    r->cin = cin; r->cout = cout;
    GILL_TRY(load_norm(wt, pool, s, p + ".norm1", cin, &r->n1));
    GILL_TRY(load_conv3(wt, pool, s, p + ".conv1", cin, cout, 0, &r->c1));
    GILL_TRY(load_norm(wt, pool, s, p + ".norm2", cout, &r->n2));
    GILL_TRY(load_conv3(wt, pool, s, p + ".conv2", cout, cout, 0, &r->c2));
    r->has_sc = (cin != cout);
    if (r->has_sc) {
      bf16_t* scw; float* scb;
      GILL_TRY(load_bf16(wt, pool, p + ".conv_shortcut.weight", (int64_t)cout * cin, &scw, s));
      GILL_TRY(load_f32(wt, pool, p + ".conv_shortcut.bias", cout, &scb, s));
      GILL_TRY(fuse_shortcut_into_conv2(pool, s, scw, scb, r));
    }
    return 0;
  }
  // attention projection weight under either naming (diffusers >= 0.16 "to_q" / legacy "query")
  int attn_lin(const std::string& base, const char* modern, const char* legacy, int C, bf16_t* wdst, float* bdst) {
    std::string n = base + "." + modern;
    if (!wt.find(n + ".weight")) n = base + "." + legacy;
    const gill_tensor* t;
    GILL_TRY(wt.get(n + ".weight", (int64_t)C * C, &t));
    GILL_TRY(convert_to_bf16_launch(t->data, t->dtype, (int64_t)C * C, wdst, s));
    GILL_TRY(wt.get(n + ".bias", C, &t));
    return convert_to_f32_launch(t->data, t->dtype, C, bdst, s);
  }
};

// One forward of either half: `ws` (ConvRun) is that half's workspace — the handle itself for the decoder, m->enc for the encoder
struct VRun : ConvRun {
  gill_vae* m;
  VRun(gill_vae* m, ConvWorkspace* w, hipStream_t s, int B, bool dry) : ConvRun{w, m->cfg.norm_num_groups, s, B, dry}, m(m) {}

  // want_stats: the producer files this tensor's GroupNorm partial sums, one bin per group
  Tensor talloc(int H, int W, int C, bool want_stats) { return tensor(H, W, C, want_stats && C % groups == 0 ? C / groups : 0); }
  // every GEMM, the attention's included: the conv split rule, 16 Mi floats of partials
  int gemm(GemmArgs& g, Tensor* ys = nullptr) {
    if (dry) return 0;
    GILL_TRY(vae_gemm_launch(g, ws->splitk_ws, ws->splitk_ws_floats, s));
    if (ys && ys->stats) ys->nslab = ys->H * ys->W / gemm_gn_slab_rows(g);
    return 0;
  }
  int gnorm(const Tensor& x, const NormW& n, int silu, const Tensor& y) { return ConvRun::gnorm(x, nullptr, n, 1e-6f, silu, y); }
  int conv(const Tensor& x, const ConvW& w, int ups, const bf16_t* resid, Tensor& y) {
    GemmArgs g = conv_args(x, nullptr, w, 1, ups, nullptr, 0, resid, y);
    return gemm(g, &y);
  }
  // Downsample2D(padding = 0): the stride-2 window with its origin shifted (GemmArgs::pad_shift)
  int down(const Tensor& x, const ConvW& w, Tensor& y) {
    GemmArgs g = conv_args(x, nullptr, w, 2, 0, nullptr, 0, nullptr, y, 1);
    return gemm(g, &y);
  }
  int resnet(const Tensor& x, const ResW& w, Tensor* out, bool out_stats) {
    const int H = x.H, Wd = x.W;
    *out = talloc(H, Wd, w.cout, out_stats);
    const size_t mk = ws->arena.mark();
    Tensor n1 = talloc(H, Wd, w.cin, false);
    GILL_TRY(gnorm(x, w.n1, 1, n1));
    Tensor h = talloc(H, Wd, w.cout, true);
    GILL_TRY(conv(n1, w.c1, 0, nullptr, h));
    Tensor n2 = talloc(H, Wd, w.cout, false);
    GILL_TRY(gnorm(h, w.n2, 1, n2));
    if (w.has_sc) {
      GemmArgs g = conv2_shortcut_args(n2, x, nullptr, w, *out);
      GILL_TRY(gemm(g, out));
    } else {
      GILL_TRY(conv(n2, w.c2, 0, x.p, *out));
    }
    ws->arena.release(mk);
    return 0;
  }
  // single-head attention over the HW tokens of a C-channel map (+ residual)
  int attention(const Tensor& x, const AttnW& a, Tensor* out, bool out_stats) {
    const int C = x.C, HW = x.H * x.W, M = Bx * HW;
    *out = talloc(x.H, x.W, C, out_stats);
    const size_t mk = ws->arena.mark();
    Tensor n = talloc(x.H, x.W, C, false);
    GILL_TRY(gnorm(x, a.gn, 0, n));
    bf16_t* q = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)M * C);
    bf16_t* k = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)M * C);
    bf16_t* vt = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)M * C);
    bf16_t* sc = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)HW * HW);   // scores of ONE image at a time
    bf16_t* o = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)M * C);
    if (!dry) {
      VaeAttnArgs v;
      v.n = n.p; v.wqkv = a.wqkv; v.bqkv = a.bqkv; v.wo = a.wo; v.bo = a.bo;
      v.q = q; v.k = k; v.vt = vt; v.sc = sc; v.sc_bstride = 0; v.o = o;
      v.ws = ws->splitk_ws; v.ws_floats = ws->splitk_ws_floats; v.B = Bx; v.HW = HW; v.C = C;
      v.out.resid = x.p; v.out.ldr = C; v.out.C = out->p; v.out.ldc = C;
      fuse_stats(v.out, *out);
      GILL_TRY(vae_attention_chain(v, s));
      if (out->stats) out->nslab = HW / gemm_gn_slab_rows(v.out);
    }
    ws->arena.release(mk);
    return 0;
  }

  int decode(const float* latents, float* img_out_f32) {
    const gill_vae_config& c = m->cfg;
    const int* ch = c.block_out_channels;
    const int L = c.latent_size;
    const int ctop = ch[3];
    ws->arena.off = 0;
    ws->gn_next = 0;
    if (!dry) {
      const int64_t total = (int64_t)Bx * c.latent_channels * L * L;
      int blocks = (int)((total + 255) / 256);
      hipLaunchKernelGGL(vae_latent_prep_kernel, dim3(blocks), dim3(256), 0, s, latents, m->pq_w, m->pq_b,
                         1.0f / c.scaling_factor, c.latent_channels, L * L, total, m->lat_prep);
      GILL_CHECK_HIP(hipGetLastError());
    }
    Tensor x = talloc(L, L, ctop, true);
    {
      bf16_t* col = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)Bx * L * L * 64);
      if (!dry) GILL_TRY(im2col_nchw_launch(m->lat_prep, Bx, c.latent_channels, L, L, 64, col, s));
      GemmArgs g;
      g.M = Bx * L * L; g.N = ctop; g.K = 64; g.K1 = 64; g.A = col; g.lda = 64; g.W = m->conv_in_w; g.bias = m->conv_in_b;
      g.C = x.p; g.ldc = ctop;
      fuse_stats(g, x);
      GILL_TRY(gemm(g, &x));
    }
    { Tensor y; GILL_TRY(resnet(x, m->mid_res[0], &y, true)); x = y; }
    { Tensor y; GILL_TRY(attention(x, m->attn, &y, true)); x = y; }
    { Tensor y; GILL_TRY(resnet(x, m->mid_res[1], &y, true)); x = y; }
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 3; ++j) {
        Tensor y;
        // the output feeds the next resnet's norm1 / conv_norm_out, except before an upsampling conv
        GILL_TRY(resnet(x, m->up_res[i][j], &y, !(j == 2 && i < 3)));
        x = y;
      }
      if (i < 3) {
        // (4-tap form: the epilogue's GroupNorm slabs are 64 SOURCE rows of one parity class — tiny grids leave the sums to the consumer)
        Tensor y = talloc(x.H * 2, x.W * 2, x.C, !m->up_us[i].ups4 || (x.H * x.W) % GN_SLAB_ROWS == 0);
        GILL_TRY(conv(x, m->up_us[i], 1, nullptr, y));
        x = y;
      }
    }
    Tensor n = talloc(x.H, x.W, x.C, false);
    GILL_TRY(gnorm(x, m->norm_out, 1, n));
    if (!dry) GILL_TRY(conv_out_launch(n.p, m->conv_out_w, m->conv_out_b, Bx, x.C, x.H, x.W, c.out_channels, img_out_f32, s));
    return 0;
  }

  // image (B,3,8L,8L) fp32 -> e->h_f32 (B,2 lc,L,L): everything in front of quant_conv
  int encode(const float* image) {
    VaeEncoder* e = m->enc.get();
    const gill_vae_config& c = m->cfg;
    const int* ch = c.block_out_channels;
    const int side = 8 * c.latent_size;
    ws->arena.off = 0;
    ws->gn_next = 0;
    Tensor x = talloc(side, side, ch[0], true);
    {
      const size_t mk = ws->arena.mark();
      bf16_t* col = (bf16_t*)ws->arena.alloc(sizeof(bf16_t) * (size_t)Bx * side * side * 64);
      if (!dry) GILL_TRY(im2col_nchw_launch(image, Bx, c.out_channels, side, side, 64, col, s));
      GemmArgs g;
      g.M = Bx * side * side; g.N = ch[0]; g.K = 64; g.K1 = 64; g.A = col; g.lda = 64; g.W = e->conv_in_w; g.bias = e->conv_in_b;
      g.C = x.p; g.ldc = ch[0];
      fuse_stats(g, x);
      GILL_TRY(gemm(g, &x));
      ws->arena.release(mk);
    }
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 2; ++j) {
        Tensor y;
        // the output feeds the next resnet's norm1 (or the mid block's), except in front of a downsampling conv
        GILL_TRY(resnet(x, e->down_res[i][j], &y, !(j == 1 && i < 3)));
        x = y;
      }
      if (i < 3) {
        Tensor y = talloc(x.H / 2, x.W / 2, x.C, true);
        GILL_TRY(down(x, e->down_ds[i], y));
        x = y;
      }
    }
    { Tensor y; GILL_TRY(resnet(x, e->mid_res[0], &y, true)); x = y; }
    { Tensor y; GILL_TRY(attention(x, e->attn, &y, true)); x = y; }
    { Tensor y; GILL_TRY(resnet(x, e->mid_res[1], &y, true)); x = y; }
    Tensor n = talloc(x.H, x.W, x.C, false);
    GILL_TRY(gnorm(x, e->norm_out, 1, n));
    if (!dry) GILL_TRY(conv_out_launch(n.p, e->conv_out_w, e->conv_out_b, Bx, x.C, x.H, x.W, 2 * c.latent_channels, e->h_f32, s));
    return 0;
  }
};

int load_attn(Loader& L, DevPool& pool, const std::string& a, int C, AttnW* w) {
  GILL_TRY(load_norm(L.wt, pool, L.s, a + ".group_norm", C, &w->gn));
  GILL_TRY(pool.alloc(&w->wqkv, (size_t)3 * C * C, false));
  GILL_TRY(pool.alloc(&w->bqkv, (size_t)3 * C, false));
  GILL_TRY(pool.alloc(&w->wo, (size_t)C * C, false));
  GILL_TRY(pool.alloc(&w->bo, (size_t)C, false));
  GILL_TRY(L.attn_lin(a, "to_q", "query", C, w->wqkv, w->bqkv));
  GILL_TRY(L.attn_lin(a, "to_k", "key", C, w->wqkv + (size_t)C * C, w->bqkv + C));
  GILL_TRY(L.attn_lin(a, "to_v", "value", C, w->wqkv + (size_t)2 * C * C, w->bqkv + 2 * C));
  return L.attn_lin(a, "to_out.0", "proj_attn", C, w->wo, w->bo);
}

// the encoder half of a handle whose decoder half (and split-K workspace) is already built
int build_encoder(gill_vae* m, Loader& L) {
  const gill_vae_config& c = m->cfg;
  const int* ch = c.block_out_channels;
  const int lc = c.latent_channels;
  GILL_REQUIRE(c.out_channels * 9 <= 64 && 2 * lc <= 8, "vae encoder: image / latent channel counts too large");
  GILL_REQUIRE(c.latent_size % 8 == 0, "vae encoder: latent_size must be a multiple of 8");
  m->enc.reset(new VaeEncoder());
  VaeEncoder* e = m->enc.get();
  DevPool& pool = m->pool;
  GILL_TRY(load_conv_in_im2col(L.wt, pool, L.s, "encoder.conv_in", c.out_channels, ch[0], &e->conv_in_w, &e->conv_in_b));
  for (int i = 0; i < 4; ++i) {
    const std::string b = "encoder.down_blocks." + std::to_string(i);
    for (int j = 0; j < 2; ++j)
      GILL_TRY(L.resnet(b + ".resnets." + std::to_string(j), (j == 0 && i > 0) ? ch[i - 1] : ch[i], ch[i], &e->down_res[i][j]));
    if (i < 3) GILL_TRY(load_conv3(L.wt, pool, L.s, b + ".downsamplers.0.conv", ch[i], ch[i], 0, &e->down_ds[i]));
  }
  GILL_TRY(L.resnet("encoder.mid_block.resnets.0", ch[3], ch[3], &e->mid_res[0]));
  GILL_TRY(L.resnet("encoder.mid_block.resnets.1", ch[3], ch[3], &e->mid_res[1]));
  GILL_TRY(load_attn(L, pool, "encoder.mid_block.attentions.0", ch[3], &e->attn));
  GILL_TRY(load_norm(L.wt, pool, L.s, "encoder.conv_norm_out", ch[3], &e->norm_out));
  GILL_TRY(load_conv_out(L.wt, pool, L.s, "encoder.conv_out", ch[3], 2 * lc, &e->conv_out_w, &e->conv_out_b));
  GILL_TRY(load_f32(L.wt, pool, "quant_conv.weight", (int64_t)4 * lc * lc, &e->q_w, L.s));
  GILL_TRY(load_f32(L.wt, pool, "quant_conv.bias", 2 * lc, &e->q_b, L.s));
  // its own arena and statistics pool, sized by its own dry run; the split-K workspace is shared with the decoder half (one call at a time)
  e->splitk_ws = m->splitk_ws; e->splitk_ws_floats = m->splitk_ws_floats;
  e->arena.dry = true; e->arena.off = 0; e->arena.high = 0;
  VRun r{m, e, nullptr, c.max_batch, true};
  GILL_TRY(r.encode(nullptr));
  GILL_TRY(pool.alloc(&e->arena_mem, e->arena.high + (1 << 20), true));
  e->arena.base = e->arena_mem; e->arena.cap = e->arena.high + (1 << 20); e->arena.dry = false;
  e->gn_floats = e->gn_next + 64;
  GILL_TRY(pool.alloc(&e->gn_stats, e->gn_floats));
  return pool.alloc(&e->h_f32, (size_t)c.max_batch * 2 * lc * c.latent_size * c.latent_size);
}

}  // namespace

extern "C" int gill_vae_create(gill_vae** out, const gill_vae_config* cfg, const gill_tensor* weights, int n_weights) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  GILL_REQUIRE(cfg->layers_per_block == 2 && cfg->max_batch >= 1, "only layers_per_block == 2 is supported");
  GILL_REQUIRE(cfg->latent_channels * 9 <= 64 && cfg->out_channels <= 8, "latent/out channel counts too large");
  for (int i = 0; i < 4; ++i) GILL_REQUIRE(cfg->block_out_channels[i] % 64 == 0, "block_out_channels must be multiples of 64");
  GILL_REQUIRE((cfg->latent_size * cfg->latent_size) % 64 == 0, "latent_size^2 must be a multiple of 64");
  gill_vae* m = new gill_vae();
  m->cfg = *cfg;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  Loader L{wt, m->pool, s};
  const int* ch = cfg->block_out_channels;
  const int ctop = ch[3], lc = cfg->latent_channels;
  if ((rc = load_f32(wt, m->pool, "post_quant_conv.weight", (int64_t)lc * lc, &m->pq_w, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, "post_quant_conv.bias", lc, &m->pq_b, s))) return fail(rc);
  if ((rc = load_conv_in_im2col(wt, m->pool, s, "decoder.conv_in", lc, ctop, &m->conv_in_w, &m->conv_in_b))) return fail(rc);
  if ((rc = L.resnet("decoder.mid_block.resnets.0", ctop, ctop, &m->mid_res[0]))) return fail(rc);
  if ((rc = L.resnet("decoder.mid_block.resnets.1", ctop, ctop, &m->mid_res[1]))) return fail(rc);
  if ((rc = load_attn(L, m->pool, "decoder.mid_block.attentions.0", ctop, &m->attn))) return fail(rc);
  // up blocks walk the channel list backwards: [512, 512, 256, 128]
  int prev = ctop;
  for (int i = 0; i < 4; ++i) {
    const int outc = ch[3 - i];
    m->up_res[i].resize(3);
    for (int j = 0; j < 3; ++j) {
      const std::string p = "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
      if ((rc = L.resnet(p, j == 0 ? prev : outc, outc, &m->up_res[i][j]))) return fail(rc);
    }
    if (i < 3)
      if ((rc = load_conv3(wt, m->pool, s, "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", outc, outc, 0, &m->up_us[i], false, true)))
        return fail(rc);
    prev = outc;
  }
  if ((rc = load_norm(wt, m->pool, s, "decoder.conv_norm_out", ch[0], &m->norm_out))) return fail(rc);
  if ((rc = load_conv_out(wt, m->pool, s, "decoder.conv_out", ch[0], cfg->out_channels, &m->conv_out_w, &m->conv_out_b))) return fail(rc);
  // workspace: dry run sizes the arena and counts the GroupNorm slots
  const int B = cfg->max_batch, Lz = cfg->latent_size;
  m->arena.dry = true; m->arena.off = 0; m->arena.high = 0;
  VRun r{m, m, nullptr, B, true};
  if ((rc = r.decode(nullptr, nullptr))) return fail(rc);
  if ((rc = m->pool.alloc(&m->arena_mem, m->arena.high + (1 << 20), true))) return fail(rc);
  m->arena.base = m->arena_mem; m->arena.cap = m->arena.high + (1 << 20); m->arena.dry = false;
  m->gn_floats = m->gn_next + 64;
  if ((rc = m->pool.alloc(&m->gn_stats, m->gn_floats))) return fail(rc);
  m->splitk_ws_floats = (size_t)16 << 20;
  if ((rc = m->pool.alloc(&m->splitk_ws, m->splitk_ws_floats, false))) return fail(rc);
  if ((rc = m->pool.alloc(&m->lat_prep, (size_t)B * cfg->latent_channels * Lz * Lz))) return fail(rc);
  if ((rc = m->pool.alloc(&m->img_f32, (size_t)B * cfg->out_channels * 64 * Lz * Lz))) return fail(rc);
  if (wt.find("encoder.conv_in.weight"))
    if ((rc = build_encoder(m, L))) return fail(rc);
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("vae create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_vae_destroy(gill_vae* h) { delete h; }

extern "C" int gill_vae_decode(gill_vae* m, const float* latents, int B, float* image_f32, uint8_t* image_u8, void* stream) {
  GILL_REQUIRE(m && latents && (image_f32 || image_u8), "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "batch exceeds the VAE handle's max_batch");
  hipStream_t s = (hipStream_t)stream;
  float* img = image_f32 ? image_f32 : m->img_f32;
  VRun r{m, m, s, B, false};
  GILL_TRY(r.decode(latents, img));
  if (image_u8) {
    const int side = 8 * m->cfg.latent_size;
    const int64_t total = (int64_t)B * side * side * m->cfg.out_channels;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(vae_to_uint8_kernel, dim3(blocks), dim3(256), 0, s, img, m->cfg.out_channels, side * side, total, image_u8);
    GILL_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int gill_vae_encode(gill_vae* m, const float* image, int B, const float* noise, float* latents_out, float* moments_out, void* stream) {
  GILL_REQUIRE(m && image && latents_out, "null argument");
  GILL_REQUIRE(m->enc != nullptr, "this VAE handle was built without encoder weights (encoder.* / quant_conv.*)");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "batch exceeds the VAE handle's max_batch");
  hipStream_t s = (hipStream_t)stream;
  VRun r{m, m->enc.get(), s, B, false};
  GILL_TRY(r.encode(image));
  const gill_vae_config& c = m->cfg;
  const int hw = c.latent_size * c.latent_size;
  const int64_t total = (int64_t)B * c.latent_channels * hw;
  hipLaunchKernelGGL(vae_encode_finish_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, s, m->enc->h_f32, m->enc->q_w, m->enc->q_b, noise,
                     c.scaling_factor, c.latent_channels, hw, total, latents_out, moments_out);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
