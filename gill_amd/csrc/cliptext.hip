// CLIP text tower (transformers CLIPTextModel as the Stable Diffusion pipeline calls it: gill/custom_sd.py:305-309 and :353-357
// read `text_encoder(input_ids)[0]`, last_hidden_state after final_layer_norm) on gfx950, through the same GEMM / attention /
// LayerNorm kernels as the vision tower (clip.hip) and the OPT engine.
//   ids (B,T) int32 -> token_embedding[ids] + position_embedding[0..T) -> L x { LN1, QKV (bias), causal softmax(QK^T/sqrt(d)) V,
//   out_proj, +res, LN2, fc1, quick_gelu | gelu, fc2, +res } -> final_layer_norm -> (B,T,D) bf16 and / or fp32.
// fp32 residual stream, bf16 GEMM operands, fp32 accumulation (as clip.hip / opt.hip).  No attention mask: the reference passes
// none (neither SD-1.5's nor SD-2.1's text_encoder config sets use_attention_mask), so padding positions attend causally like
// any other.  Two kernels live here, the two ends of the tower; everything between them is a launch of ops.h.
// Launches per forward: 1 + 7 L + 1 without split-K (86 at L = 12, 163 at L = 23); a GEMM that gemm_pick_splitk() splits
// (few rows) adds its reducer.
#include "ops.h"
#include "engine_util.h"
#include <string>
#include <vector>

namespace {
struct TextLayer {
  bf16_t* wqkv = nullptr; float* bqkv = nullptr;   // [3D][D] rows: q | k | v
  bf16_t* wo = nullptr; float* bo = nullptr;
  bf16_t* w1 = nullptr; float* b1 = nullptr;
  bf16_t* w2 = nullptr; float* b2 = nullptr;
  float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
};
constexpr int kFinalLnMaxOctets = 4;    // final LayerNorm keeps a row in registers: D <= 8 * 64 * 4 = 2048
}  // namespace

struct gill_clip_text {
  gill_clip_text_config cfg;
  DevPool pool;
  int dp = 0, dpv = 0;
  float* tok = nullptr;       // [vocab][D] fp32: the rows enter the fp32 stream unrounded
  float* pos = nullptr;       // [max_positions][D]
  float *fing = nullptr, *finb = nullptr;
  std::vector<TextLayer> layers;
  // workspace
  float* h = nullptr;         // [B*T][D]
  bf16_t* nbuf = nullptr;     // [B*T][D]
  bf16_t* ff = nullptr;       // [B*T][F]
  bf16_t *q = nullptr, *k = nullptr, *vt = nullptr, *o = nullptr;
  float* splitk_ws = nullptr; size_t splitk_ws_floats = 0;
};

// h[b*T + t][:] = token_embedding[ids[b*T + t]][:] + position_embedding[t][:]       (CLIPTextEmbeddings.forward)
// One wave per row, 16-byte loads and stores; the id is wave-uniform, read once from device memory.  Memory-bound: 2 reads + 1
// write of D floats per row.  The caller validates the ids; the clamp keeps a bad one inside the table instead of faulting.
__global__ __launch_bounds__(256) void clip_text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                              const float* __restrict__ pos, int rows, int T, int D, int vocab,
                                                              float* __restrict__ h) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* e = reinterpret_cast<const float4*>(tok + (size_t)id * D);
  const float4* p = reinterpret_cast<const float4*>(pos + (size_t)(row % T) * D);
  float4* o = reinterpret_cast<float4*>(h + (size_t)row * D);
  for (int c = lane; c < D / 4; c += 64) {
    const float4 a = e[c], b = p[c];
    o[c] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
}

// final_layer_norm over the fp32 stream: y = (x - mean) * rstd * g + b, written as bf16 (the context gill_sd_denoise consumes)
// and / or fp32 (what return_prompts_only hands back) in one pass.  One wave per row; lane l owns the octets l, l + 64, ... of the
// row, which is read once and stays in registers; exact two-pass mean / variance on the registers.  The bf16 value is the
// rounding of the fp32 value that is stored, so the two outputs can never disagree.
template <int MAXV>
__global__ __launch_bounds__(256) void clip_text_final_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, bf16_t* __restrict__ y16,
                                                                 float* __restrict__ y32, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = D >> 3;
  const float* xr = x + (size_t)row * D;
  float v[MAXV][8];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int o = lane + k * 64;
    if (o < nv) {
      const float4 a = *reinterpret_cast<const float4*>(xr + o * 8), b = *reinterpret_cast<const float4*>(xr + o * 8 + 4);
      v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; v[k][3] = a.w; v[k][4] = b.x; v[k][5] = b.y; v[k][6] = b.z; v[k][7] = b.w;
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[k][i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[k][i] = 0.f;
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k)
    if (lane + k * 64 < nv) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float dlt = v[k][i] - mean; ss += dlt * dlt; }
    }
  const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int o = lane + k * 64;
    if (o < nv) {
      const float4 g0 = *reinterpret_cast<const float4*>(gamma + o * 8), g1 = *reinterpret_cast<const float4*>(gamma + o * 8 + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(beta + o * 8), b1 = *reinterpret_cast<const float4*>(beta + o * 8 + 4);
      const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float r[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = (v[k][i] - mean) * rstd * g[i] + bb[i];
      if (y32) {
        float* yr = y32 + (size_t)row * D + o * 8;
        *reinterpret_cast<float4*>(yr) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(yr + 4) = make_float4(r[4], r[5], r[6], r[7]);
      }
      if (y16) {
        uint4 u;
        u.x = pack_bf2(r[0], r[1]); u.y = pack_bf2(r[2], r[3]); u.z = pack_bf2(r[4], r[5]); u.w = pack_bf2(r[6], r[7]);
        *reinterpret_cast<uint4*>(y16 + (size_t)row * D + o * 8) = u;
      }
    }
  }
}

extern "C" int gill_clip_text_create(gill_clip_text** out, const gill_clip_text_config* cfg, const gill_tensor* weights, int n_weights) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  const int D = cfg->hidden_size, F = cfg->intermediate_size, H = cfg->num_heads, V = cfg->vocab_size, P = cfg->max_positions;
  GILL_REQUIRE(D > 0 && F > 0 && D % 64 == 0 && F % 64 == 0 && H > 0 && D % H == 0, "CLIP text dims must be multiples of 64");
  GILL_REQUIRE(D <= 8 * 64 * kFinalLnMaxOctets, "CLIP text hidden size above 2048");
  GILL_REQUIRE(V >= 1 && P >= 1 && cfg->max_batch >= 1 && cfg->num_layers >= 1, "bad CLIP text geometry");
  GILL_REQUIRE(cfg->hidden_act == GILL_CLIP_TEXT_ACT_QUICK_GELU || cfg->hidden_act == GILL_CLIP_TEXT_ACT_GELU,
               "CLIP text hidden_act must be quick_gelu (0) or gelu (1)");
  const int hd = D / H;
  GILL_REQUIRE(attn_padded_dim(hd) == hd, "CLIP text head dim must be one of 48/64/80/128/160");
  gill_clip_text* m = new gill_clip_text();
  m->cfg = *cfg;
  m->dp = hd; m->dpv = round_up(hd, 32);
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  const std::string tm = "text_model.";
  if ((rc = load_f32(wt, m->pool, tm + "embeddings.token_embedding.weight", (int64_t)V * D, &m->tok, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, tm + "embeddings.position_embedding.weight", (int64_t)P * D, &m->pos, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, tm + "final_layer_norm.weight", D, &m->fing, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, tm + "final_layer_norm.bias", D, &m->finb, s))) return fail(rc);
  m->layers.resize(cfg->num_layers);
  for (int i = 0; i < cfg->num_layers; ++i) {
    TextLayer& L = m->layers[i];
    const std::string p = tm + "encoder.layers." + std::to_string(i) + ".";
    if ((rc = m->pool.alloc(&L.wqkv, (size_t)3 * D * D, false))) return fail(rc);
    if ((rc = m->pool.alloc(&L.bqkv, (size_t)3 * D, false))) return fail(rc);
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      const gill_tensor* t;
      if ((rc = wt.get(p + "self_attn." + names[j] + ".weight", (int64_t)D * D, &t))) return fail(rc);
      if ((rc = convert_to_bf16_launch(t->data, t->dtype, (int64_t)D * D, L.wqkv + (size_t)j * D * D, s))) return fail(rc);
      if ((rc = wt.get(p + "self_attn." + names[j] + ".bias", D, &t))) return fail(rc);
      if ((rc = convert_to_f32_launch(t->data, t->dtype, D, L.bqkv + (size_t)j * D, s))) return fail(rc);
    }
    if ((rc = load_bf16(wt, m->pool, p + "self_attn.out_proj.weight", (int64_t)D * D, &L.wo, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "self_attn.out_proj.bias", D, &L.bo, s))) return fail(rc);
    if ((rc = load_bf16(wt, m->pool, p + "mlp.fc1.weight", (int64_t)F * D, &L.w1, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "mlp.fc1.bias", F, &L.b1, s))) return fail(rc);
    if ((rc = load_bf16(wt, m->pool, p + "mlp.fc2.weight", (int64_t)D * F, &L.w2, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "mlp.fc2.bias", D, &L.b2, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "layer_norm1.weight", D, &L.ln1g, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "layer_norm1.bias", D, &L.ln1b, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "layer_norm2.weight", D, &L.ln2g, s))) return fail(rc);
    if ((rc = load_f32(wt, m->pool, p + "layer_norm2.bias", D, &L.ln2b, s))) return fail(rc);
  }
  const size_t R = (size_t)cfg->max_batch * P;
  const size_t Tpad = round_up(P, 32);
  if ((rc = m->pool.alloc(&m->h, R * D))) return fail(rc);
  if ((rc = m->pool.alloc(&m->nbuf, R * D))) return fail(rc);
  if ((rc = m->pool.alloc(&m->ff, R * F))) return fail(rc);
  if ((rc = m->pool.alloc(&m->q, (size_t)cfg->max_batch * H * Tpad * m->dp))) return fail(rc);
  if ((rc = m->pool.alloc(&m->k, (size_t)cfg->max_batch * H * Tpad * m->dp))) return fail(rc);
  if ((rc = m->pool.alloc(&m->vt, (size_t)cfg->max_batch * H * m->dpv * Tpad))) return fail(rc);
  if ((rc = m->pool.alloc(&m->o, R * D))) return fail(rc);
  // split-K partials: gemm_pick_splitk() splits only under-filled grids (< 384 tiles of 128 x 128, at most 16 ways aiming at 512
  // workgroups), so splitk * M * N stays near 512 * 128 * 128 floats whatever max_batch is; a launch that would not fit runs unsplit
  m->splitk_ws_floats = (size_t)16 * R * (size_t)(F > 3 * D ? F : 3 * D);
  if (m->splitk_ws_floats > ((size_t)16 << 20)) m->splitk_ws_floats = (size_t)16 << 20;
  if ((rc = m->pool.alloc(&m->splitk_ws, m->splitk_ws_floats, false))) return fail(rc);
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("clip text create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_clip_text_destroy(gill_clip_text* h) { delete h; }

namespace {
struct TextRun {
  gill_clip_text* m;
  hipStream_t s;
  int splitk(int M, int N, int K, int act) const {
    const int sk = gemm_pick_splitk(M, N, K, act);
    return (size_t)sk * M * N > m->splitk_ws_floats ? 1 : sk;
  }
  int linear(const bf16_t* A, int M, const bf16_t* W, const float* b, int N, int K, const float* resid, int act, void* out,
             bool out_f32) {
    GemmArgs g;
    g.M = M; g.N = N; g.K = K; g.K1 = K; g.A = A; g.lda = K; g.W = W; g.bias = b;
    g.resid = resid; g.ldr = N; g.resid_f32 = 1;
    g.act = act; g.out_mode = out_f32 ? OUT_F32 : OUT_BF16; g.C = out; g.ldc = N;
    g.splitk = splitk(M, N, K, act);
    g.ws = m->splitk_ws;
    return gemm_launch(g, s);
  }
};
}  // namespace

extern "C" int gill_clip_text_forward(gill_clip_text* m, const int32_t* ids, int B, int T, void* out_bf16, float* out_f32,
                                      void* stream) {
  GILL_REQUIRE(m && ids, "null argument");
  GILL_REQUIRE(out_bf16 || out_f32, "no output buffer");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "batch exceeds the CLIP text handle's max_batch");
  GILL_REQUIRE(T >= 1 && T <= m->cfg.max_positions, "sequence length exceeds the CLIP text handle's max_positions");
  hipStream_t s = (hipStream_t)stream;
  const gill_clip_text_config& c = m->cfg;
  const int D = c.hidden_size, F = c.intermediate_size, R = B * T;
  const int Tpad = round_up(T, 32);
  const int act = c.hidden_act == GILL_CLIP_TEXT_ACT_GELU ? ACT_GELU : ACT_QUICK_GELU;
  TextRun r{m, s};
  hipLaunchKernelGGL(clip_text_embed_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, ids, m->tok, m->pos, R, T, D, c.vocab_size, m->h);
  GILL_CHECK_HIP(hipGetLastError());
  for (const TextLayer& L : m->layers) {
    GILL_TRY(layernorm_launch(m->h, 1, L.ln1g, L.ln1b, m->nbuf, R, D, 1e-5f, s));
    {
      GemmArgs g;
      g.M = R; g.N = 3 * D; g.K = D; g.K1 = D; g.A = m->nbuf; g.lda = D; g.W = L.wqkv; g.bias = L.bqkv;
      g.out_mode = OUT_QKV; g.Cq = m->q; g.Ck = m->k; g.Cvt = m->vt;
      g.heads = c.num_heads; g.dp = m->dp; g.dpv = m->dpv; g.ntok = T; g.ntok_pad_q = Tpad; g.ntok_pad_kv = Tpad;
      g.seg_base = 0;
      g.qscale = 1.4426950408889634f / sqrtf((float)m->dp);
      g.splitk = r.splitk(R, 3 * D, D, 0);
      g.ws = m->splitk_ws;
      GILL_TRY(gemm_launch(g, s));
    }
    {
      AttnArgs a;
      a.Q = m->q; a.K = m->k; a.Vt = m->vt; a.O = m->o;
      a.B = B; a.H = c.num_heads; a.nq = T; a.nkv = T; a.nq_pad = Tpad; a.nkv_pad = Tpad;
      a.dp = m->dp; a.dpv = m->dpv; a.ldo = D; a.scale = 1.0f / sqrtf((float)m->dp); a.causal = 1;
      GILL_TRY(attention_launch(a, s));
    }
    GILL_TRY(r.linear(m->o, R, L.wo, L.bo, D, D, m->h, ACT_NONE, m->h, true));
    GILL_TRY(layernorm_launch(m->h, 1, L.ln2g, L.ln2b, m->nbuf, R, D, 1e-5f, s));
    GILL_TRY(r.linear(m->nbuf, R, L.w1, L.b1, F, D, nullptr, act, m->ff, false));
    GILL_TRY(r.linear(m->ff, R, L.w2, L.b2, D, F, m->h, ACT_NONE, m->h, true));
  }
  hipLaunchKernelGGL((clip_text_final_ln_kernel<kFinalLnMaxOctets>), dim3(cdiv(R, 4)), dim3(256), 0, s, m->h, m->fing, m->finb,
                     (bf16_t*)out_bf16, out_f32, R, D, 1e-5f);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
